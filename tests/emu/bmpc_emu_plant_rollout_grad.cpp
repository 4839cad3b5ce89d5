// tests/emu/bmpc_emu_plant_rollout_grad.cpp -- TEST INFRASTRUCTURE: the entry of libbmpc_emu_plant_rollout_grad.so,
// rollout_grad_plan of csrc/bmpc_plant_rollout_grad.hip (the body of plant_rollout_grad_kernel) executed on the CPU as plain C++
// (BMPC_EMU), one plan after the other in the order of the kernel's flat index.  The scratch is the caller's arrays; the lane's
// slab, LDS on the device, is an array of this function's.
#include <cmath>
#include <cstdint>

#define BMPC_EMU 1
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
#define __shared__

#include "../../biped_mpc_py_amd/csrc/bmpc_plant_rollout_grad.hip"
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

// bmpc_plant_rollout_grad of include/bmpc.h on the CPU: `in`, `out` and the scratch `W` as the kernel takes them (host pointers
// here), the plant block as the library takes it.  Returns 0, or -1 where the library would refuse.
extern "C" int bmpc_emu_plant_rollout_grad(const bmpc_params* p, int B, int S, const bmpc_plant* plant, const bmpc::RolloutIn* in,
                                           const bmpc::RolloutGradOut* out, const bmpc::RolloutGradScratch* W) {
  bmpc::PlantParams P;
  if (!plant_params(p, &P) || plant->substeps < 1 || plant->substeps > bmpc::PLANT_MAX_SUBSTEPS || plant->integrator < 0 ||
      plant->integrator > 1 || S < 1 || W->plans != (size_t)B * (size_t)S || (!out->x_traj && !W->x_rec))
    return -1;
  const bmpc::PlantScheme Sc = bmpc::plant_scheme(p->dt, plant->integrator, plant->substeps);
  bmpc::RolloutCost C;
  for (int i = 0; i < 12; ++i) { C.Q[i] = p->Q[i]; C.R[i] = p->R[i]; C.x_cmd[i] = p->x_cmd[i]; }
  bmpc::RolloutIn I = *in;
  I.mu_h = p->mu; I.move_feet = plant->move_feet != 0; I.push_from = plant->push_from; I.push_steps = plant->push_steps;
  double slab[bmpc::RGRAD_SLAB];
  const bmpc::LaneSlab L = {slab, 1};
  for (size_t plan = 0; plan < W->plans; ++plan) bmpc::rollout_grad_plan(P, Sc, C, I, *out, *W, L, plan / (size_t)S, plan);
  return 0;
}

extern "C" int bmpc_emu_plant_rollout_grad_sizes(int* in_bytes, int* out_bytes, int* scratch_bytes) {
  *in_bytes = (int)sizeof(bmpc::RolloutIn); *out_bytes = (int)sizeof(bmpc::RolloutGradOut);
  *scratch_bytes = (int)sizeof(bmpc::RolloutGradScratch);
  return 0;
}
