// tests/emu/bmpc_emu_eval.cpp -- TEST INFRASTRUCTURE: the sources of the evaluation family's kernels (csrc/bmpc_evaluate.hip,
// bmpc_evaluate_grad.hip, bmpc_certify.hip) on the CPU, one std::thread per lane of a workgroup, on the harness of bmpc_emu.cpp (which
// stays as it is).  The kernels' one cross-lane primitive, lane_read (a wave-wide permute on the GPU), goes through a shared array
// between two barriers of the lane's wave.
#include "bmpc_emu.cpp"

static double g_lr[1024];
static int g_lri[1024];
namespace bmpc {
static inline double lane_read(double v, int src) {     // value of lane `src` of the own wave; all lanes of the wave call
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_lr[threadIdx.x] = v;
  wb.arrive_and_wait();
  const double r = g_lr[(threadIdx.x & ~63) + src];
  wb.arrive_and_wait();
  return r;
}
static inline int lane_read(int v, int src) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_lri[threadIdx.x] = v;
  wb.arrive_and_wait();
  const int r = g_lri[(threadIdx.x & ~63) + src];
  wb.arrive_and_wait();
  return r;
}
}  // namespace bmpc

#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate_grad.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_certify.hip"

extern "C" int bmpc_emu_eval_lanes(int h) { return bmpc::eval_lanes(h); }

// `kernel(P)` in every lane of the library's launch grid for B instances, block after block: one thread per lane, one barrier per
// wave.  -1 if the inertia is singular.
template <typename Kernel>
static int run_eval_grid(const bmpc_params* p, int B, Kernel kernel) {
  double Iinv[9];
  if (!inv3(p->I, Iinv)) return -1;
  const bmpc::EvalParams P = bmpc::eval_params(*p, Iinv);
  constexpr int NT = bmpc::EVAL_NT;
  const long long lanes = (long long)B * bmpc::eval_lanes(p->h);
  const int blocks = (int)((lanes + NT - 1) / NT);
  for (int b = 0; b < blocks; ++b) {
    std::vector<std::unique_ptr<std::barrier<>>> wb;
    for (int w = 0; w < NT / 64; ++w) { wb.emplace_back(new std::barrier<>(64)); g_wbar[w] = wb.back().get(); }
    std::vector<std::thread> th;
    th.reserve(NT);
    for (int t = 0; t < NT; ++t)
      th.emplace_back([&, t]() {
        threadIdx.x = t;
        blockIdx.x = b;
        kernel(P);
      });
    for (auto& x : th) x.join();
  }
  return 0;
}

// bmpc_evaluate, bmpc_evaluate_grad and bmpc_certify of include/bmpc.h on the CPU: host pointers, the same grid as the library's launch
extern "C" int bmpc_emu_evaluate(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls, const bmpc_eval_out* out) {
  const bmpc::EvalOut o = {out->cost, out->objective, out->states, out->violation};
  return run_eval_grid(p, B, [&](const bmpc::EvalParams& P) {
    bmpc::evaluate_kernel(P, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref, controls, o);
  });
}

extern "C" int bmpc_emu_evaluate_grad(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls, const bmpc_grad_out* out) {
  const bmpc::GradOut o = {out->cost, out->grad_u, out->grad_x0};
  return run_eval_grid(p, B, [&](const bmpc::EvalParams& P) {
    bmpc::evaluate_grad_kernel(P, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref, controls, o);
  });
}

extern "C" int bmpc_emu_certify(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls, double act_tol,
                                const bmpc_cert_out* out) {
  const bmpc::CertOut o = {out->lam, out->resid, out->summary, out->n_active, out->status};
  return run_eval_grid(p, B, [&](const bmpc::EvalParams& P) {
    bmpc::certify_kernel(P, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref, controls, act_tol, o);
  });
}
