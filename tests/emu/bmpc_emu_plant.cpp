// tests/emu/bmpc_emu_plant.cpp -- TEST INFRASTRUCTURE: the entries of libbmpc_emu_plant.so, the per-instance functions of
// csrc/bmpc_plant.hip (plant_step, plant_land) executed on the CPU as plain C++ (BMPC_EMU), one instance after the other.
#include <cmath>
#include <cstdint>

#define BMPC_EMU 1
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__

#include "../../biped_mpc_py_amd/csrc/bmpc_plant.hip"
#include "bmpc.h"

// inverse of a 3x3 by cofactors (what the library's parameter mapping does for I_b^-1); false if singular
static bool inv3(const double* a, double* o) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0)) return false;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  return true;
}

static bool plant_params(const bmpc_params* p, bmpc::PlantParams* q) {
  q->h = p->h; q->dt = p->dt; q->kv = p->kv; q->m = p->m; q->g = p->g;
  q->cmd_x = p->x_cmd[3]; q->cmd_y = p->x_cmd[4];
  for (int i = 0; i < 9; ++i) q->Ib[i] = p->I[i];
  return inv3(p->I, q->Ibinv);
}

// bmpc_plant_step of include/bmpc.h on the CPU.  Returns 0, or -1 where the library would refuse the arguments.
extern "C" int bmpc_emu_plant_step(const bmpc_params* p, int B, int integrator, int substeps, const float* x_fb, const float* u0,
                                   const float* foot, const uint8_t* contact0, const float* wrench, float* x_next) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P) || substeps < 1 || substeps > bmpc::PLANT_MAX_SUBSTEPS || integrator < 0 || integrator > 1) return -1;
  const bmpc::PlantScheme S = bmpc::plant_scheme(p->dt, integrator, substeps);
  for (int b = 0; b < B; ++b) {
    float x[12], u[12], r[6], w[6];
    double xn[12];
    for (int i = 0; i < 12; ++i) { x[i] = x_fb[b * 12 + i]; u[i] = u0[b * 12 + i]; }
    for (int i = 0; i < 6; ++i) { r[i] = foot[b * 6 + i]; w[i] = wrench ? wrench[b * 6 + i] : 0.f; }
    bmpc::plant_step(P, S, x, u, r, contact0[b * 2] ? 1.0 : 0.0, contact0[b * 2 + 1] ? 1.0 : 0.0, w, xn);
    for (int i = 0; i < 12; ++i) x_next[b * 12 + i] = (float)xn[i];
  }
  return 0;
}

// The landing rule as simulate_feedback_kernel applies it: schedule steps k0[b] (this period) and k1[b] (the next), the new state
// x_new [B][12] fp32, foot [B][6] in/out, x_cmd [B][12] or null; lands [B][2] out.
extern "C" int bmpc_emu_plant_landing(const bmpc_params* p, const bmpc_gait* gait, int B, const int32_t* k0, const int32_t* k1,
                                      const float* x_new, const float* x_cmd, float* foot, uint8_t* lands) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P)) return -1;
  for (int b = 0; b < B; ++b) {
    double xs[12];
    for (int i = 0; i < 12; ++i) xs[i] = x_new[b * 12 + i];
    const double cx = x_cmd ? (double)x_cmd[b * 12 + 3] : P.cmd_x, cy = x_cmd ? (double)x_cmd[b * 12 + 4] : P.cmd_y;
    for (int g = 0; g < 2; ++g) {
      double rg[3];
      const bool l = bmpc::plant_land(P, k0[b], k1[b], gait->offset[g], gait->period, gait->duty[g], g == 0 ? 1.0 : -1.0, xs, cx, cy, rg);
      lands[b * 2 + g] = l ? 1 : 0;
      if (l) for (int i = 0; i < 3; ++i) foot[b * 6 + 3 * g + i] = (float)rg[i];
    }
  }
  return 0;
}
