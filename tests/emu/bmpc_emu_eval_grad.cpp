// tests/emu/bmpc_emu_eval_grad.cpp -- TEST INFRASTRUCTURE: the cost-gradient kernel's source (csrc/bmpc_evaluate_grad.hip) on the CPU,
// on the harness and the lane_read of bmpc_emu_eval.cpp (which stays as it is and brings evaluate_kernel along).
#include "bmpc_emu_eval.cpp"

#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate_grad.hip"

// bmpc_evaluate_grad of include/bmpc.h on the CPU: host pointers, the same grid as the library's launch
extern "C" int bmpc_emu_evaluate_grad(const bmpc_params* p, int B, const bmpc_inputs* in, const float* controls, const bmpc_grad_out* out) {
  double Iinv[9];
  if (!inv3(p->I, Iinv)) return -1;
  const bmpc::EvalParams P = bmpc::eval_params(*p, Iinv);
  const bmpc::GradOut o = {out->cost, out->grad_u, out->grad_x0};
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
        bmpc::evaluate_grad_kernel(P, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, in->x_ref, in->foot_ref, controls, o);
      });
    for (auto& x : th) x.join();
  }
  return 0;
}
