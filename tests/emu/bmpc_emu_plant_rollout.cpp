// tests/emu/bmpc_emu_plant_rollout.cpp -- TEST INFRASTRUCTURE: the entry of libbmpc_emu_plant_rollout.so, rollout_sample of
// csrc/bmpc_plant_rollout.hip (the body of plant_rollout_samples_kernel) executed on the CPU as plain C++ (BMPC_EMU), one plan
// after the other in the order of the kernel's flat index.
#include <cmath>
#include <cstdint>

#define BMPC_EMU 1
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__

#include "../../biped_mpc_py_amd/csrc/bmpc_plant_rollout.hip"
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

// The per-sample part of bmpc_plant_rollout_samples of include/bmpc.h on the CPU: `in` and `out` as the kernel takes them (host
// pointers here), the plant block and the price as the library takes them.  Returns 0, or -1 where the library would refuse.
extern "C" int bmpc_emu_plant_rollout(const bmpc_params* p, int B, const bmpc_plant* plant, const bmpc_rollout_price* price,
                                      const bmpc::RolloutIn* in, const bmpc::RolloutOut* out) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P) || plant->substeps < 1 || plant->substeps > bmpc::PLANT_MAX_SUBSTEPS || plant->integrator < 0 ||
      plant->integrator > 1 || price->S < 1)
    return -1;
  const bmpc::PlantScheme Sc = bmpc::plant_scheme(p->dt, plant->integrator, plant->substeps);
  bmpc::RolloutCost C;
  for (int i = 0; i < 12; ++i) { C.Q[i] = p->Q[i]; C.R[i] = p->R[i]; C.x_cmd[i] = p->x_cmd[i]; }
  bmpc::RolloutIn I = *in;
  I.mu_h = p->mu; I.move_feet = plant->move_feet != 0; I.push_from = plant->push_from; I.push_steps = plant->push_steps;
  const bmpc::RolloutPrice pr = {price->tilt_max, price->z_min, price->fz_floor, price->w_fall, price->w_slip, price->w_unloaded};
  const size_t S = (size_t)price->S;
  for (size_t plan = 0; plan < (size_t)B * S; ++plan) bmpc::rollout_sample(P, Sc, C, I, pr, *out, plan / S, plan);
  return 0;
}

extern "C" int bmpc_emu_plant_rollout_sizes(int* in_bytes, int* out_bytes) {
  *in_bytes = (int)sizeof(bmpc::RolloutIn); *out_bytes = (int)sizeof(bmpc::RolloutOut);
  return 0;
}
