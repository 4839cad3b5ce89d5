// tests/emu/bmpc_emu_plant_body.cpp -- TEST INFRASTRUCTURE: the entries of libbmpc_emu_plant_body.so, the per-instance body and
// the fall outcome of csrc/bmpc_plant.hip (plant_body, plant_step_body, plant_outcome) executed on the CPU as plain C++ (BMPC_EMU),
// one instance after the other.
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

// the handle's block as the library maps it: I_b^-1 by cofactors; false if singular
static bool plant_params(const bmpc_params* p, bmpc::PlantParams* q) {
  q->h = p->h; q->dt = p->dt; q->kv = p->kv; q->m = p->m; q->g = p->g;
  q->cmd_x = p->x_cmd[3]; q->cmd_y = p->x_cmd[4];
  const double* a = p->I;
  double* o = q->Ibinv;
  for (int i = 0; i < 9; ++i) q->Ib[i] = a[i];
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0)) return false;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  return true;
}

// bmpc_plant_step_body of include/bmpc.h on the CPU: m [B], I [B][9], g [B], each null for the handle's.  ok [B] (or null):
// what plant_step_body returned.  Returns 0, or -1 where the library would refuse the arguments.
extern "C" int bmpc_emu_plant_step_body(const bmpc_params* p, int B, int integrator, int substeps, const double* m, const double* I,
                                        const double* g, const float* x_fb, const float* u0, const float* foot,
                                        const uint8_t* contact0, const float* wrench, float* x_next, uint8_t* ok) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P) || substeps < 1 || substeps > bmpc::PLANT_MAX_SUBSTEPS || integrator < 0 || integrator > 1) return -1;
  const bmpc::PlantScheme S = bmpc::plant_scheme(p->dt, integrator, substeps);
  for (int b = 0; b < B; ++b) {
    float x[12], u[12], r[6], w[6];
    double xn[12];
    for (int i = 0; i < 12; ++i) { x[i] = x_fb[b * 12 + i]; u[i] = u0[b * 12 + i]; }
    for (int i = 0; i < 6; ++i) { r[i] = foot[b * 6 + i]; w[i] = wrench ? wrench[b * 6 + i] : 0.f; }
    const bool good = bmpc::plant_step_body(P, m ? m + b : nullptr, I ? I + b * 9 : nullptr, g ? g + b : nullptr, S, x, u, r,
                                            contact0[b * 2] ? 1.0 : 0.0, contact0[b * 2 + 1] ? 1.0 : 0.0, w, xn);
    if (ok) ok[b] = good ? 1 : 0;
    for (int i = 0; i < 12; ++i) x_next[b * 12 + i] = (float)xn[i];
  }
  return 0;
}

// plant_body alone: the handle's I_b^-1 [9] and the instance's Pb.m, Pb.g, Pb.Ib [9], Pb.Ibinv [9] out (21 doubles), the return value
extern "C" int bmpc_emu_plant_body(const bmpc_params* p, const double* m, const double* I9, const double* g, double* handle_inv,
                                   double* out) {
  bmpc::PlantParams P, Pb;
  if (!plant_params(p, &P)) return -1;
  const bool good = bmpc::plant_body(P, m, I9, g, Pb);
  for (int i = 0; i < 9; ++i) { handle_inv[i] = P.Ibinv[i]; out[2 + i] = Pb.Ib[i]; out[11 + i] = Pb.Ibinv[i]; }
  out[0] = Pb.m; out[1] = Pb.g;
  return good ? 1 : 0;
}

// The outcome of a recorded trajectory x_traj [steps][B][12] as bmpc_simulate_body_device reduces it: the arrays initialised as
// the entry does (-1, NaN, NaN), then plant_outcome period by period.
extern "C" void bmpc_emu_plant_outcome(int steps, int B, const float* x_traj, double tilt_max, double z_min, int32_t* first_fall,
                                       float* max_tilt, float* min_z) {
  for (int b = 0; b < B; ++b) { first_fall[b] = -1; max_tilt[b] = std::nanf(""); min_z[b] = std::nanf(""); }
  for (int s = 0; s < steps; ++s)
    for (int b = 0; b < B; ++b) {
      float x[12];
      for (int i = 0; i < 12; ++i) x[i] = x_traj[((size_t)s * B + b) * 12 + i];
      bmpc::plant_outcome(tilt_max, z_min, x, s, first_fall[b], max_tilt[b], min_z[b]);
    }
}
