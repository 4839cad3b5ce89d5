// tests/emu/bmpc_emu_samples.cpp -- TEST INFRASTRUCTURE: the entries of libbmpc_emu_samples.so, the two kernels of
// csrc/bmpc_evaluate_samples.hip executed on the CPU (harness: bmpc_emu_harness.hpp, one thread per lane) over the library's grids:
// evaluate_samples_kernel on B ceil(S / C) groups with C from the library's own rule (bmpc::eval_samples_per_group), then -- where
// a reduced output is wanted -- sample_reduce_kernel on one workgroup per instance, scores and weights in scratch arrays where the
// caller asks for neither, as the library's launch does.
#include "bmpc_emu_harness.hpp"

#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate_samples.hip"
#include "bmpc.h"

// I^-1 of the handle's block as the library forms it (by cofactors); false if singular
static bool inertia_inverse(const double* a, double* o) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0)) return false;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  return true;
}

extern "C" int bmpc_emu_samples_per_group(int B, int S) { return bmpc::eval_samples_per_group(B, S); }

// bmpc_evaluate_samples of include/bmpc.h on the CPU: host pointers.  -1 if the inertia is singular.
extern "C" int bmpc_emu_evaluate_samples(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls,
                                         const bmpc_samples* smp, const bmpc_samples_out* out) {
  double Iinv[9];
  if (!inertia_inverse(p->I, Iinv)) return -1;
  const bmpc::EvalParams P = bmpc::eval_params(*p, Iinv);
  const int S = smp->S;
  const size_t n = (size_t)B * (size_t)S;
  const bool reduce = out->best || out->n_valid || out->weights || out->u_mean || out->ess;
  std::vector<double> scratch((out->score ? 0 : n) + (reduce && !out->weights ? n : 0));
  double* score = out->score ? out->score : scratch.data();
  double* weights = out->weights ? out->weights : scratch.data() + (scratch.size() - (reduce ? n : 0));
  const int C = bmpc::eval_samples_per_group(B, S);
  const long long groups = (long long)B * (((long long)S + C - 1) / C);
  const long long lanes = groups * bmpc::eval_lanes(p->h);
  bmpc::SamplesPrice price;
  for (int c = 0; c < 4; ++c) price.w[c] = smp->w_viol[c];
  const bmpc::SamplesOut so = {out->cost, out->violation, score};
  emu_run_grid(bmpc::EVAL_NT, (int)((lanes + bmpc::EVAL_NT - 1) / bmpc::EVAL_NT), [&]() {
    bmpc::evaluate_samples_kernel(P, B, S, C, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref,
                                  controls, price, so);
  });
  if (reduce) {
    const bmpc::ReduceOut ro = {out->best, out->n_valid, weights, out->u_mean, out->ess};
    emu_run_grid(bmpc::REDUCE_NT, B, [&]() { bmpc::sample_reduce_kernel(p->h, S, smp->temperature, score, controls, ro); });
  }
  return 0;
}
