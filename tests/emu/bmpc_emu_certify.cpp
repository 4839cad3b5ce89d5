// tests/emu/bmpc_emu_certify.cpp -- TEST INFRASTRUCTURE: the certificate kernel's source (csrc/bmpc_certify.hip) on the CPU, one
// std::thread per lane, on the harness and the lane_read of bmpc_emu_eval.cpp (which stays as it is; bmpc_emu_eval_grad.cpp brings
// the evaluation and gradient kernels along).
#include "bmpc_emu_eval_grad.cpp"

#include "../../biped_mpc_py_amd/csrc/bmpc_certify.hip"

// bmpc_certify of include/bmpc.h on the CPU: host pointers, the same grid as the library's launch
extern "C" int bmpc_emu_certify(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls, double act_tol,
                                const bmpc_cert_out* out) {
  double Iinv[9];
  if (!inv3(p->I, Iinv)) return -1;
  const bmpc::EvalParams P = bmpc::eval_params(*p, Iinv);
  const bmpc::CertOut o = {out->lam, out->resid, out->summary, out->n_active, out->status};
  constexpr int NT = bmpc::EVAL_NT;
  const long long lanes = (long long)B * bmpc_emu_eval_lanes(p->h);
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
        bmpc::certify_kernel(P, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref, controls,
                             act_tol, o);
      });
    for (auto& x : th) x.join();
  }
  return 0;
}
