// tests/emu/bmpc_emu_plant_ground.cpp -- TEST INFRASTRUCTURE: the entries of libbmpc_emu_plant_ground.so, the ground under the plant
// of csrc/bmpc_plant.hip (plant_ground, plant_step_ground, plant_ground_reduce) executed on the CPU as plain C++ (BMPC_EMU), one
// instance after the other.
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

// plant_ground alone: u0 [B][12], contact0 [B][2], mu [B][2] (null: mu_h for both legs) -> u_applied [B][12], flags [B],
// demand [B], ok [B]
extern "C" void bmpc_emu_plant_ground(int B, const float* u0, const uint8_t* contact0, const double* mu, double mu_h, double fz_floor,
                                      float* u_applied, uint8_t* flags, float* demand, uint8_t* ok) {
  for (int b = 0; b < B; ++b) {
    float u[12], ua[12];
    for (int i = 0; i < 12; ++i) u[i] = u0[b * 12 + i];
    const bool good = bmpc::plant_ground(u, contact0[b * 2] != 0, contact0[b * 2 + 1] != 0, mu ? mu[b * 2] : mu_h, mu ? mu[b * 2 + 1] : mu_h,
                                         fz_floor, ua, flags[b], demand[b]);
    ok[b] = good ? 1 : 0;
    for (int i = 0; i < 12; ++i) u_applied[b * 12 + i] = ua[i];
  }
}

// bmpc_plant_step_ground of include/bmpc.h on the CPU: the body m [B], I [B][9], g [B] and mu [B][2], each null for the handle's.
// Returns 0, or -1 where the library would refuse the arguments.
extern "C" int bmpc_emu_plant_step_ground(const bmpc_params* p, int B, int integrator, int substeps, const double* m, const double* I,
                                          const double* g, const double* mu, const float* x_fb, const float* u0, const float* foot,
                                          const uint8_t* contact0, const float* wrench, float* x_next, float* u_applied,
                                          uint8_t* flags, uint8_t* ok) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P) || substeps < 1 || substeps > bmpc::PLANT_MAX_SUBSTEPS || integrator < 0 || integrator > 1) return -1;
  const bmpc::PlantScheme S = bmpc::plant_scheme(p->dt, integrator, substeps);
  for (int b = 0; b < B; ++b) {
    float x[12], u[12], ua[12], r[6], w[6], demand;
    double xn[12];
    for (int i = 0; i < 12; ++i) { x[i] = x_fb[b * 12 + i]; u[i] = u0[b * 12 + i]; }
    for (int i = 0; i < 6; ++i) { r[i] = foot[b * 6 + i]; w[i] = wrench ? wrench[b * 6 + i] : 0.f; }
    const bool good = bmpc::plant_step_ground(P, m ? m + b : nullptr, I ? I + b * 9 : nullptr, g ? g + b : nullptr, mu ? mu[b * 2] : p->mu,
                                              mu ? mu[b * 2 + 1] : p->mu, 0.0, S, x, u, r, contact0[b * 2] != 0, contact0[b * 2 + 1] != 0,
                                              w, xn, ua, flags[b], demand);
    ok[b] = good ? 1 : 0;
    for (int i = 0; i < 12; ++i) { x_next[b * 12 + i] = (float)xn[i]; u_applied[b * 12 + i] = ua[i]; }
  }
  return 0;
}

// The reduced outputs of flags [steps][B] and demand [steps][B] as bmpc_simulate_ground_device reduces them: the arrays
// initialised as the entry does (-1, 0, 0, NaN), then plant_ground_reduce period by period.
extern "C" void bmpc_emu_ground_reduce(int steps, int B, const uint8_t* flags, const float* demand, int32_t* first_slip,
                                       int32_t* slip_periods, int32_t* unloaded_periods, float* mu_demand) {
  for (int b = 0; b < B; ++b) {
    first_slip[b] = -1; mu_demand[b] = std::nanf("");
    for (int g = 0; g < 2; ++g) slip_periods[b * 2 + g] = unloaded_periods[b * 2 + g] = 0;
  }
  for (int s = 0; s < steps; ++s)
    for (int b = 0; b < B; ++b) {
      int32_t sl[2] = {slip_periods[b * 2], slip_periods[b * 2 + 1]}, un[2] = {unloaded_periods[b * 2], unloaded_periods[b * 2 + 1]};
      bmpc::plant_ground_reduce(flags[(size_t)s * B + b], demand[(size_t)s * B + b], s, first_slip[b], sl, un, mu_demand[b]);
      for (int g = 0; g < 2; ++g) { slip_periods[b * 2 + g] = sl[g]; unloaded_periods[b * 2 + g] = un[g]; }
    }
}
