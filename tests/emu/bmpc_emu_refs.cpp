// Emulation entry with supplied references (include/bmpc.h bmpc_inputs -> bmpc::WarmArgs::x_ref / foot_ref): bmpc_emu_solve of
// bmpc_emu.cpp with the two arrays appended (the same parameter mapping, repeated: the harness file stays as it is).
#include "bmpc_emu.cpp"

extern "C" int bmpc_emu_solve_refs(const bmpc_params* p, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                                   const int32_t* phase, const float* x_cmd, const float* mu, float* controls, float* states,
                                   int32_t* iters, float* resid, int32_t* status, int32_t* nfactor,
                                   double* dbg_x_ref, double* dbg_foot_ref, double* dbg_Gt, double* dbg_qt, int assemble_only,
                                   double* warm_buf, int warm_load, int warm_store, int warm_shift, double warm_theta,
                                   const float* x_ref, const float* foot_ref) {
  bmpc::DevParams d;
  std::memset(&d, 0, sizeof(d));
  d.h = p->h; d.half = p->half; d.max_iter = p->max_iter; d.check_every = p->check_every;
  d.adapt_start = p->adapt_start; d.adapt_every = p->adapt_every; d.max_refactor = p->max_refactor;
  d.adapt_early = p->adapt_early; d.adapt_late = p->adapt_late;
  d.adapt_busy = p->adapt_busy; d.adapt_flips = p->adapt_flips;
  d.confirm_from = p->confirm_from; d.kappa_confirm = (float)p->kappa_confirm;
  d.dt = p->dt; d.kv = p->kv; d.m = p->m; d.g = p->g; d.mu = p->mu;
  d.lt = p->lt - 0.01; d.lh = p->lh - 0.02; d.alpha = p->alpha;
  for (int i = 0; i < 12; ++i) { d.x_cmd[i] = p->x_cmd[i]; d.Q[i] = p->Q[i]; d.R2[i] = 2.0 * p->R[i]; }
  for (int k = 0; k < 3; ++k) { d.sq_e[k] = std::sqrt(2.0 * p->Q[k]); d.sq_w[k] = p->dt * std::sqrt(2.0 * p->Q[6 + k]); }
  d.kpm = p->dt * p->dt / p->m;
  d.kvm = p->dt / p->m;
  {
    double rmin = p->R[0];
    for (int i = 1; i < 12; ++i) rmin = std::fmin(rmin, p->R[i]);
    d.r2min = (float)(2 * rmin);
    d.accel = p->accel ? 1 : 0;
  }
  if (!inv3(p->I, d.Iinv)) return -1;
  for (int i = 0; i < 3; ++i) {
    d.f_max[i] = p->f_max[i]; d.f_min[i] = p->f_min[i]; d.tau_max[i] = p->tau_max[i]; d.tau_min[i] = p->tau_min[i];
  }
  d.rho = (float)p->rho; d.rho_eq = (float)(p->rho * p->rho_eq_scale); d.rho_lo = (float)p->rho_lo;
  d.rho_hi_f = (float)p->rho_hi_f; d.rho_hi_m = (float)p->rho_hi_m;
  d.eps_pri = (float)p->eps_pri; d.eps_dua = (float)p->eps_dua; d.kappa = (float)p->kappa;
  {                                           // (f32 products exactly as the kernels used to form them: SLOW_TOL = 1e-6, U0_TOL = 5)
    const float slow_tol = 1.0e-6f, u0_tol = 5.f;
    d.kappa_sqrt = std::sqrt(d.kappa);
    d.kappa_qrt = std::sqrt(std::sqrt(d.kappa));
    d.slow_tol_r2 = slow_tol * d.r2min;
    d.slow_tol_r2_u0 = u0_tol * slow_tol * d.r2min;
    d.eps_u0 = u0_tol * std::fmax(d.eps_pri, d.eps_dua);
  }
  bmpc::DebugOut dbg = {dbg_x_ref, dbg_foot_ref, dbg_Gt, dbg_qt, nullptr, assemble_only};
  bmpc::WarmArgs warm = {warm_buf, warm_load, warm_store, warm_shift, (float)warm_theta, p->warm_adapt_start};
  warm.x_ref = x_ref;
  warm.foot_ref = foot_ref;
  if (const char* e = std::getenv("BMPC_EMU_POISON")) g_poison = std::atoi(e);
  if (p->path == BMPC_PATH_STAGE) {
    switch (10 * bmpc::stage_waves(p->h) + bmpc::stage_steps_per_lane(p->h)) {
#define EMU_CASE(NN, WW) case 10 * WW + NN: run_stage<NN, WW>(d, B, x_fb, foot, contact, phase, x_cmd, mu, controls, states, iters, resid, status, nfactor, dbg, warm); break;
      EMU_CASE(2, 1) EMU_CASE(3, 1) EMU_CASE(4, 1) EMU_CASE(5, 1) EMU_CASE(3, 2) EMU_CASE(4, 2)
#undef EMU_CASE
      default: return -1;
    }
    return 0;
  }
  switch (p->h) {
    case 10: run_h<10>(d, B, x_fb, foot, contact, phase, x_cmd, mu, controls, states, iters, resid, status, nfactor, dbg, warm); break;
    case 16: run_h<16>(d, B, x_fb, foot, contact, phase, x_cmd, mu, controls, states, iters, resid, status, nfactor, dbg, warm); break;
    case 20: run_h<20>(d, B, x_fb, foot, contact, phase, x_cmd, mu, controls, states, iters, resid, status, nfactor, dbg, warm); break;
    default: return -1;
  }
  return 0;
}
