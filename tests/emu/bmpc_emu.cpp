// tests/emu/bmpc_emu.cpp -- TEST INFRASTRUCTURE: the entries of libbmpc_emu.so, the HIP kernels' sources executed on the CPU
// (harness: bmpc_emu_harness.hpp).  Both solve families, with or without supplied references, and the evaluation family
// (evaluate, evaluate_grad, certify).  A parameter block resolves through the library's own make_dev_params and a horizon
// finds its kernel through the library's own variant lists (csrc/bmpc_host_params.hpp): nothing of either is repeated here.
#include "bmpc_emu_harness.hpp"

#include "../../biped_mpc_py_amd/csrc/bmpc_kernels.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_stage.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_evaluate_grad.hip"
#include "../../biped_mpc_py_amd/csrc/bmpc_certify.hip"
#include "bmpc.h"
#define BMPC_DENSE_HORIZONS(X) X(10) X(16) X(20)     // of the library's seven, one per lane map: build time
#include "../../biped_mpc_py_amd/csrc/bmpc_host_params.hpp"

using namespace bmpc_host;

static thread_local char g_err[512] = "";
extern "C" const char* bmpc_emu_last_error() { return g_err; }

extern "C" int bmpc_emu_threads(int h) {
  return dispatch_dense(h, -1, [](auto H) { return bmpc::Dims<decltype(H)::value>::NT; });
}
// The addressing of the warm-start buffers, for the tests that build one by hand.  Stage family: [B][HS][12][6], HS >= h step
// slots (those past h are phantoms).  Dense family: [B][NT][6], variable (row = 6 j + c, foot f) in lane Dims<H>::lane_of.
extern "C" int bmpc_emu_stage_hs(int h) { return stage_step_slots(h); }
extern "C" int bmpc_emu_stage_warm(int h) { return warm_doubles(BMPC_PATH_STAGE, h); }
extern "C" int bmpc_emu_lane_of(int h, int row, int f) {
  if (row < 0 || row >= 6 * h || f < 0 || f > 1) return -1;
  return dispatch_dense(h, -1, [&](auto H) { return bmpc::Dims<decltype(H)::value>::lane_of(row, f); });
}
extern "C" int bmpc_emu_eval_lanes(int h) { return bmpc::eval_lanes(h); }

// What the library's make_dev_params resolves `p` to: the bytes of bmpc::DevParams into out[size] and the five penalties as
// bmpc_effective_penalties reports them into eff5.  Returns the number of bytes, or the library's error code (< 0) with its
// message in bmpc_emu_last_error.
extern "C" int bmpc_emu_dev_params(const bmpc_params* p, void* out, int size, double* eff5) {
  const ErrBuf fail = {g_err, sizeof(g_err)};
  bmpc::DevParams d;
  if (const int rc = make_dev_params(*p, &d, fail); rc != BMPC_OK) return rc;
  if (size < (int)sizeof(d)) return fail(BMPC_ERR_INVALID, "need %d bytes", (int)sizeof(d));
  std::memcpy(out, &d, sizeof(d));
  eff5[0] = d.rho; eff5[1] = d.rho_eq; eff5[2] = d.rho_lo; eff5[3] = d.rho_hi_f; eff5[4] = d.rho_hi_m;
  return (int)sizeof(d);
}

// outputs of a solve (all but controls nullable as in bmpc_solve_batch_device) and the fp64 debug views of bmpc::DebugOut
struct bmpc_emu_out {
  float *controls, *states;
  int32_t* iters;
  float* resid;
  int32_t *status, *nfactor;
  double *dbg_x_ref, *dbg_foot_ref, *dbg_Gt, *dbg_qt;
};
struct bmpc_emu_warm { double* buf; int load, store, shift; double theta; };   // bmpc::WarmArgs; null: cold, nothing stored

// bmpc_solve_batch_device of include/bmpc.h on the CPU: the family resolve_path names, one workgroup after the other
extern "C" int bmpc_emu_solve(const bmpc_params* p, int B, const bmpc_inputs* in, const bmpc_emu_out* out, int assemble_only,
                              const bmpc_emu_warm* w) {
  bmpc::DevParams d;
  if (const int rc = make_dev_params(*p, &d, ErrBuf{g_err, sizeof(g_err)}); rc != BMPC_OK) return rc;
  const bmpc::DebugOut dbg = {out->dbg_x_ref, out->dbg_foot_ref, out->dbg_Gt, out->dbg_qt, nullptr, assemble_only};
  bmpc::WarmArgs warm = {nullptr, 0, 0, 0, 0.5f, p->warm_adapt_start};
  if (w) { warm.buf = w->buf; warm.load = w->load; warm.store = w->store; warm.shift = w->shift; warm.theta = (float)w->theta; }
  warm.x_ref = in->x_ref;
  warm.foot_ref = in->foot_ref;
  if (const char* e = std::getenv("BMPC_EMU_POISON")) g_poison = std::atoi(e);
  const auto run = [&](int NT, auto kernel) {
    emu_run_grid(NT, B, [&]() {
      kernel(d, B, in->x_fb, in->foot, in->contact, in->phase, in->x_cmd, in->mu, out->controls, out->states, out->iters, out->resid,
             out->status, out->nfactor, dbg, warm);
    });
    return (int)BMPC_OK;
  };
  const int rc = resolve_path(p->h, p->path) == BMPC_PATH_STAGE
      ? dispatch_stage(p->h, NO_VARIANT, [&](auto NP, auto NW) {
          return run(64 * decltype(NW)::value, [](auto... a) { bmpc::stage_kernel<decltype(NP)::value, decltype(NW)::value>(a...); });
        })
      : dispatch_dense(p->h, NO_VARIANT, [&](auto H) {
          return run(bmpc::Dims<decltype(H)::value>::NT, [](auto... a) { bmpc::solve_kernel<decltype(H)::value>(a...); });
        });
  return rc == NO_VARIANT ? ErrBuf{g_err, sizeof(g_err)}(BMPC_ERR_INVALID, "no emulated kernel for h=%d", p->h) : rc;
}

// `kernel(P)` in every lane of the library's launch grid of the evaluation family for B instances.  -1 if the inertia is singular.
template <typename Kernel>
static int run_eval_grid(const bmpc_params* p, int B, Kernel kernel) {
  double Iinv[9];
  if (!inv3(p->I, Iinv)) return -1;
  const bmpc::EvalParams P = bmpc::eval_params(*p, Iinv);
  const long long lanes = (long long)B * bmpc::eval_lanes(p->h);
  emu_run_grid(bmpc::EVAL_NT, (int)((lanes + bmpc::EVAL_NT - 1) / bmpc::EVAL_NT), [&]() { kernel(P); });
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
