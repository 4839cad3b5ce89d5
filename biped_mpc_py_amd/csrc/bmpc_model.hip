// bmpc_model.hip -- parts of the model and of the ADMM row rules that every kernel family states through ONE function
// (gfx950 / CDNA4): the body axes and the general rows of a foot block, and the relaxation / projection / dual step of a row.
// Included by the dense solve kernels (bmpc_kernels.hip), the stage-structured ones (bmpc_stage.hip) and the evaluation
// (bmpc_evaluate.hip), which keep what is a property of a family: which lane does what, masks, LDS stores, debug views.
//
// Leaf functions only: forced inline, values and references to statically indexed register arrays in, values out; no LDS,
// no state.  Same expressions in the same order as the kernels had them; the dressings placed by measurement -- widen(),
// BMPC_OPAQUE -- stay with the callers, which hand the dressed values in.  What else of the model was tried here and why it
// is still stated per family (references, step geometry, bounds, class rules, stopping tests): docs/history_r09.md.
//
// Compiles as plain C++ for tests/emu (BMPC_EMU) like the files that include it.
#ifndef BMPC_MODEL_HIP
#define BMPC_MODEL_HIP

#ifndef BMPC_EMU
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace bmpc {

typedef double RT;                       // iterate / residual / block-algebra arithmetic; the evaluation's type

// ---------------------------------------------------------------------------------------------------- the model of a step

// Body axes of the line-foot rows: columns y and z of R = eul2rotm(x_fb[0:3]) = Rz(e2) Ry(e1) Rx(e0) from the sines and cosines
// of e0, e1, e2 (REF:124-138, 193, 259-262).  The solve kernels round them to f32 at the call, the evaluation keeps them.
__device__ __forceinline__ void body_axes(const RT s0, const RT c0, const RT s1, const RT c1, const RT s2, const RT c2,
                                          RT (&ey)[3], RT (&ez)[3]) {
  ey[0] = c2 * s1 * s0 - s2 * c0; ey[1] = s2 * s1 * s0 + c2 * c0; ey[2] = c1 * s0;
  ez[0] = c2 * s1 * c0 + s2 * s0; ez[1] = s2 * s1 * c0 - c2 * s0; ez[2] = c1 * c0;
}

// General (non-box) rows of one foot block over v = [f(3), m(3)]:
// rows 0..3 friction (+x, +y, -x, -y; REF:220-229), rows 4, 5 line foot (REF:259-262).
__device__ __forceinline__ void general_rows(float mu, const float* ey, const float* ez, float lh,
                                             float lt, float (&G)[6][6]) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int b = 0; b < 6; ++b) G[r][b] = 0.f;
  G[0][0] = 1.f;  G[0][2] = -mu;
  G[1][1] = 1.f;  G[1][2] = -mu;
  G[2][0] = -1.f; G[2][2] = -mu;
  G[3][1] = -1.f; G[3][2] = -mu;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    G[4][b] = -lh * ez[b];  G[4][3 + b] = ey[b];
    G[5][b] = -lt * ez[b];  G[5][3 + b] = -ey[b];
  }
}

// One horizontal coordinate of the foothold a swing leg is steered to (REF:428-434, without the lateral 0.04 side): position p,
// velocity v and command cmd of that coordinate.  The swing controller's `des` (bmpc_lowlevel.hip) and the landing rule of the
// closed-loop simulation (bmpc_plant.hip).
__device__ __forceinline__ double foothold_target(const double p, const double v, const double h, const double dt, const double kv,
                                                  const double cmd) {
  return p + v * 0.5 * h / 2 * dt + kv * (p - cmd);
}

// Leg in stance at schedule step `step` (REF:52-55 generalised): ((step + offset) mod period) < duty, with a non-negative
// remainder.  The gait scheduler (bmpc_lowlevel.hip) and the landing rule of the closed-loop simulation (bmpc_plant.hip).
__device__ __forceinline__ bool in_stance(const int step, const int offset, const int period, const int duty) {
  int m = (step + offset) % period;
  if (m < 0) m += period;
  return m < duty;
}

// ---------------------------------------------------------------------------------------------------- the ADMM row rules
//   One row with iterate z, dual y, penalty rho (irv = 1 / rho) and the row's value zt = (A x~) of this
// iteration: relaxation, projection onto the row's set, and the dual step dy = rho (z_relaxed - z_new), which the caller
// adds to y; res = z~ - z_new is the row's primal residual.
// (The dense family keeps dy -- its secant extrapolation reuses it -- and then adds it, the stage family adds it in the
//  expression of the call.  Whether the compiler contracts the two alike is not known; each family's form is as it was.)
// box row: lb <= z <= ub
__device__ __forceinline__ void project_box(const RT alpha, const RT zt, const RT z, const RT y, const RT irv,
                                            const RT lb, const RT ub, const RT rho, RT& zn, RT& dy, RT& res) {
  const RT zr = alpha * zt + (1 - alpha) * z;
  const RT cand = zr + y * irv;
  zn = fmin(fmax(cand, lb), ub);
  dy = rho * (zr - zn);
  res = zt - zn;
}
// general row: l = -inf, u = 0
__device__ __forceinline__ void project_general(const RT alpha, const RT zt, const RT z, const RT y, const RT irv,
                                                const RT rho, RT& zn, RT& dy, RT& res) {
  const RT zr = alpha * zt + (1 - alpha) * z;
  const RT cand = zr + y * irv;
  zn = fmin(cand, (RT)0);
  dy = rho * (zr - zn);
  res = zt - zn;
}

}  // namespace bmpc
#endif
