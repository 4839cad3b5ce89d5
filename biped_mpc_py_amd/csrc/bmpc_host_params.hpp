// bmpc_host_params.hpp -- host only: what a parameter block (include/bmpc.h bmpc_params) resolves to, and which template
// instantiation solves a horizon.  Stated once for libbmpc.so (bmpc_capi.hip) and for the CPU emulation of the kernels
// (tests/emu, plain C++ under BMPC_EMU); include it after the kernel files.  A further DevParams field is a line of
// make_dev_params here and one in the kernels' struct; a further kernel variant a row of one of the two lists below.
#ifndef BMPC_HOST_PARAMS_HPP
#define BMPC_HOST_PARAMS_HPP

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "bmpc.h"

namespace bmpc_host {

// an error message into the caller's buffer; returns `code` (bmpc_capi.hip hands in the buffer of bmpc_last_error)
struct ErrBuf {
  char* msg;
  size_t size;
  int operator()(int code, const char* fmt, ...) const {
    va_list ap;
    va_start(ap, fmt);
    if (msg && size) vsnprintf(msg, size, fmt, ap);
    va_end(ap);
    return code;
  }
};

inline bool inv3(const double* a, double* o) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  if (!(std::fabs(det) > 0)) return false;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  return true;
}

// ---- the kernel variants, each list stated once, and the one dispatcher of each

// Horizons with a dense kernel (explicit 6h x 6h inverse held in registers).  h = 20 sits at 255 VGPRs; h = 22 / 24 were
// built and dropped: a 5-wave workgroup caps a lane at 256 registers whatever the launch bounds say, the row halves no
// longer fit (35 / 30 spilled registers) and 78 / 86 KB of LDS leave one workgroup per CU -- those horizons belong to the
// stage-structured kernels (bmpc_stage.hip).  (The emulation defines the list before it includes this file: it builds fewer.)
#ifndef BMPC_DENSE_HORIZONS
#define BMPC_DENSE_HORIZONS(X) X(8) X(10) X(12) X(14) X(16) X(18) X(20)
#endif
// The stage-structured kernels, compiled per (steps a lane owns, waves per instance): bmpc::stage_steps_per_lane / stage_waves
#define BMPC_STAGE_VARIANTS(X) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(3, 2) X(4, 2)

inline bool dense_horizon(int h) { return h >= 8 && h <= 20 && h % 2 == 0; }
inline bool stage_horizon(int h) { return h >= 1 && h <= 40; }       // (any parity, from ONE step: steps past the horizon are phantoms of the lane map)

template <int N> using Int = std::integral_constant<int, N>;
constexpr int NO_VARIANT = INT_MIN;

// f(Int<H>) for the dense kernel of horizon h, f(Int<NP>, Int<NW>) for the stage kernel of horizon h; `none` if none is built
template <typename F>
int dispatch_dense(int h, int none, F&& f) {
  switch (dense_horizon(h) ? h : 0) {
#define BMPC_CASE(HH) case HH: return f(Int<HH>{});
    BMPC_DENSE_HORIZONS(BMPC_CASE)
#undef BMPC_CASE
    default: return none;
  }
}
template <typename F>
int dispatch_stage(int h, int none, F&& f) {
  switch (stage_horizon(h) ? 10 * bmpc::stage_waves(h) + bmpc::stage_steps_per_lane(h) : 0) {
#define BMPC_CASE(NN, WW) case 10 * WW + NN: return f(Int<NN>{}, Int<WW>{});
    BMPC_STAGE_VARIANTS(BMPC_CASE)
#undef BMPC_CASE
    default: return none;
  }
}

// step slots of the stage family's lane map at horizon h (>= h: those past the horizon are phantoms)
inline int stage_step_slots(int h) { return 5 * bmpc::stage_steps_per_lane(h) * bmpc::stage_waves(h); }
// doubles of solver state per instance in the warm-start buffer (bmpc::WarmArgs::buf) of family `path` at horizon h: dense
// [NT][6], stage [step slots][12][6]; NO_VARIANT if no kernel is built
inline int warm_doubles(int path, int h) {
  if (path == BMPC_PATH_STAGE) return stage_step_slots(h) * 12 * 6;
  return dispatch_dense(h, NO_VARIANT, [](auto H) { return bmpc::Dims<decltype(H)::value>::NT * 6; });
}

// the kernel family that solves horizon h when the caller asks for `path`; 0 if there is none
inline int resolve_path(int h, int path) {
  if (path == BMPC_PATH_DENSE) return dense_horizon(h) ? BMPC_PATH_DENSE : 0;
  if (path == BMPC_PATH_STAGE) return stage_horizon(h) ? BMPC_PATH_STAGE : 0;
  if (path != BMPC_PATH_AUTO) return 0;
  if (dense_horizon(h)) return BMPC_PATH_DENSE;
  return stage_horizon(h) ? BMPC_PATH_STAGE : 0;
}

// ---- the parameter block

// bmpc_default_params of include/bmpc.h
inline void default_params(bmpc_params* p, int h) {
  std::memset(p, 0, sizeof(*p));
  p->h = h;
  p->half = (h == 10) ? 5 : (h > 1 ? h / 2 : 1);                      // REF:101 hard-codes 5 at h = 10
  p->dt = 0.04;                                                       // REF:25
  p->kv = 0.01;                                                       // REF:29
  const double xc[12] = {0, 0, 0, 0, 0, 0.55, 0, 0, 0, 0, 0, 0};       // REF:26
  const double Q[13] = {500, 100, 100, 300, 300, 700, 1, 1, 1, 1, 1, 1, 1};   // REF:27
  for (int i = 0; i < 12; ++i) { p->x_cmd[i] = xc[i]; p->R[i] = 1e-4; }       // REF:28
  for (int i = 0; i < 13; ++i) p->Q[i] = Q[i];
  p->m = 12;                                                          // REF:36
  p->I[0] = 0.932; p->I[4] = 0.9420; p->I[8] = 0.0711;                // REF:37-39
  p->lt = 0.09; p->lh = 0.05; p->g = 9.81; p->mu = 0.5;               // REF:40-44
  for (int i = 0; i < 3; ++i) { p->f_max[i] = 500; p->f_min[i] = 0; } // REF:45-46
  p->tau_max[0] = 0; p->tau_max[1] = 67; p->tau_max[2] = 33.5;        // REF:47
  for (int i = 0; i < 3; ++i) p->tau_min[i] = -p->tau_max[i];         // REF:48
  p->rho = h < 20 ? 0.03 : 0.045;          // (h = 20: -2.5 % kernel time, fewer late re-classifications)
  p->rho_eq_scale = h < 20 ? 1e3 : 1e3 * 0.03 / 0.045;               // rho_eq = 30 for every horizon
  p->rho_lo = 3e-4; p->rho_hi_f = 1.0; p->rho_hi_m = 100.0; p->kappa = 20.0;
  p->alpha = 1.6; p->eps_pri = 1e-7; p->eps_dua = 1e-7;
  // (worst seen in the soaks at the reference's weights: 240 at h = 10, 315 at h = 16 / 20 with the periods below.  The caps
  //  are for the instances that keep re-classifying away from those weights: at R / 100 -- soft end two decades further down
  //  -- 55 of 16384 standing h = 20 instances needed up to 60 factorisations and 995 iterations; capped at 24 / 600 they were
  //  reported unsolved by both families.  The mean is untouched: 131.5 iterations either way.)
  p->max_iter = h <= 12 ? 1000 : 1500;
  p->check_every = 5;
  // (long horizons re-classify every 10 iterations: the 1-in-2000 instances that keep re-classifying need 25-35
  //  factorisations and converge by iteration ~350; capped at 24 they freeze their penalties at iteration 240 and run
  //  into max_iter)
  p->max_refactor = 60;
  // Re-classification period ~ (cost of a factorisation) / (cost of an iteration): 10.6 at h = 10, 15.6 at h = 16,
  // 21.5 at h = 20 (profiles/r02_cfg*_phase_cycles.txt).  Measured on MI355X (build_tmp-style A/B, round 2):
  // h = 16: period 20 from iteration 10 is 8 % faster than 10 / 10 (4.3 instead of 5.6 factorisations, 68 instead of
  // 53 iterations), h = 20: 20 / 20 is 12 % faster (4.8 instead of 6.8, 88 instead of 66); h = 10 is best at 10 / 10.
  // (h > 20 runs on the stage-structured kernels, where a factorisation costs 4-5 iterations instead of 15-20:
  //  period 10 again; measured with tools/stage_probe.py)
  p->adapt_every = (h <= 12 || h > 20) ? 10 : 20;
  p->adapt_start = (h < 20 || h > 20) ? 10 : 20;
  // Two rates at h <= 12 (round 5).  Traces of the model (oracle/ws_model.py, 512 oracle-solved instances): of 240 rows 45 change
  // class between iterations 10 and 20, 18 between 20 and 30, 4.5 between 30 and 40, < 1 after -- the active set is found
  // early, and from iteration 40 on a re-classification mostly walks the rows that flipped late along their ladder.  Early
  // re-classifications 5 apart and late ones 20 apart: 48.9 instead of 53.1 iterations AND 5.05 instead of 5.54 factorisations
  // on the standing set (43.8 / 4.76 instead of 47.7 / 5.02 on the mixed one); tools/schedule_explore.py has the grid.
  p->adapt_flips = 1;
  if (h <= 12) {
    p->adapt_start = 5; p->adapt_every = 5; p->adapt_early = 3; p->adapt_late = 20;
    p->adapt_busy = 10; p->confirm_from = 3; p->kappa_confirm = 400.0;
  } else if (h < 20) {
    // h = 14 .. 18 (a factorisation costs 15 iterations): two early re-classifications 10 apart, then 20, confirmation from the
    // third on.  Model (128 oracle-solved walking instances, h = 16): 57.1 / 4.27 instead of 64.7 / 4.08, worst cost 224 instead
    // of 270; MI355X, config 3: 2.07 instead of 2.13 ms per 4096.  h = 20 (21 iterations per factorisation) gains nothing from
    // any of this (6.09 +- 0.03 ms per 8192 over six schedules) and keeps its single rate.
    p->adapt_start = 10; p->adapt_every = 10; p->adapt_early = 2; p->adapt_late = 20;
    p->confirm_from = 2; p->kappa_confirm = 400.0;
  }
  p->rescue = BMPC_RESCUE_AUTO;
  p->accel = 1;
  p->warm_adapt_start = 5;                                            // (tools/warm_sweep.py)
  p->kp[0] = p->kp[4] = p->kp[8] = 500;                               // REF:30
  p->kd[0] = p->kd[4] = p->kd[8] = 10;                                // REF:31
  p->swingHeight = 0.1;                                               // REF:32
  p->hip_offset[0] = -0.005; p->hip_offset[1] = 0.047; p->hip_offset[2] = -0.126;   // REF:43
}

inline double min_R(const bmpc_params& p) {
  double rmin = p.R[0];
  for (int i = 1; i < 12; ++i) rmin = std::fmin(rmin, p.R[i]);
  return rmin;
}

// Curvature scales of the condensed Hessian (closed forms at step 0 and zero attitude; S2 = sum_{k < h} k^2):
//   torque space  g_tau[a] = 2 (Q_e[a] (dt^2 Iinv_aa)^2 S2 + Q_w[a] (dt Iinv_aa)^2 h)        (REF:165-184, 278-286)
//   force space   g_F[a]   = 2 (Q_p[a] (dt^2 / m)^2 S2 + Q_v[a] (dt / m)^2 h)
// force-like rows see g_F plus the torque curvature through the lever arm of the nominal CoM height, moment-like rows
// g_tau; the soft end of the spectrum is 2 R.  The penalty fields of bmpc_params are the values AT THE REFERENCE PROBLEM
// (REF:22-48 defaults; horizon: the problem's own up to h = 20, else 10) and scale with these ratios, so that weights, step length, mass, inertia and horizon can
// change without re-tuning (at h = 40 the stiff scale is 70 times the one at h = 10, and with
// absolute ceilings the active rows of the early steps converge at 0.97 per iteration).
struct CurvScales { double force, moment, soft; };
inline CurvScales curvature_scales(const bmpc_params& p) {
  double Iinv[9];
  CurvScales c = {1.0, 1.0, 1.0};
  if (!inv3(p.I, Iinv)) return c;
  double s2 = 0;
  for (int k = 1; k < p.h; ++k) s2 += (double)k * k;
  const double dt = p.dt, h = p.h;
  double gt[3], gf = 0;
  for (int a = 0; a < 3; ++a) {
    const double ii = std::fabs(Iinv[4 * a]);
    gt[a] = 2 * (p.Q[a] * (dt * dt * ii) * (dt * dt * ii) * s2 + p.Q[6 + a] * (dt * ii) * (dt * ii) * h);
    gf = std::fmax(gf, 2 * (p.Q[3 + a] * (dt * dt / p.m) * (dt * dt / p.m) * s2 + p.Q[9 + a] * (dt / p.m) * (dt / p.m) * h));
  }
  const double z0 = p.x_cmd[5];
  c.force = gf + z0 * z0 * std::fmax(gt[0], gt[1]);
  c.moment = std::fmax(gt[0], std::fmax(gt[1], gt[2]));
  c.soft = min_R(p);
  return c;
}

// Is a dense solve followed by the rescue pass?  BMPC_RESCUE_AUTO: only away from the reference's model and weights
// (REF:22-48) -- there the dense family has converged on every one of 6 M soaked instances and the extra launch would
// cost the headline configuration ~1 % for nothing; at other weights 1 instance in 10^3..10^4 can stall.
inline bool resolve_rescue(const bmpc_params& p) {
  if (resolve_path(p.h, p.path) != BMPC_PATH_DENSE || !stage_horizon(p.h) || p.rescue == BMPC_RESCUE_OFF) return false;
  if (p.rescue == BMPC_RESCUE_ON) return true;
  bmpc_params ref;
  default_params(&ref, p.h);
  bool same = p.dt == ref.dt && p.m == ref.m && p.g == ref.g && p.lt == ref.lt && p.lh == ref.lh;
  for (int i = 0; i < 12; ++i) same = same && p.Q[i] == ref.Q[i] && p.R[i] == ref.R[i];
  for (int i = 0; i < 9; ++i) same = same && p.I[i] == ref.I[i];
  for (int i = 0; i < 3; ++i)
    same = same && p.f_max[i] == ref.f_max[i] && p.f_min[i] == ref.f_min[i] && p.tau_max[i] == ref.tau_max[i] && p.tau_min[i] == ref.tau_min[i];
  return !same;
}

// What the kernels get for a parameter block.  BMPC_OK, or the error code with its message in `fail`'s buffer.
inline int make_dev_params(const bmpc_params& p, bmpc::DevParams* d, const ErrBuf& fail) {
  if (!resolve_path(p.h, p.path)) return fail(BMPC_ERR_INVALID, "unsupported horizon h=%d for path %d", p.h, p.path);
  if (p.half < 1) return fail(BMPC_ERR_INVALID, "half must be >= 1");
  if (!(p.dt > 0) || !(p.m > 0)) return fail(BMPC_ERR_INVALID, "dt and m must be positive");
  if (!(p.rho > 0) || !(p.rho_lo > 0) || !(p.rho_hi_f > 0) || !(p.rho_hi_m > 0) || !(p.rho_eq_scale > 0))
    return fail(BMPC_ERR_INVALID, "penalties must be positive");
  if (!(p.kappa > 1)) return fail(BMPC_ERR_INVALID, "kappa must be > 1");
  if (p.kappa_confirm != 0 && !(p.kappa_confirm > 1)) return fail(BMPC_ERR_INVALID, "kappa_confirm must be 0 (off) or > 1");
  if (p.adapt_early < 0 || p.adapt_late < 0 || p.adapt_busy < 0 || p.adapt_flips < 0 || p.confirm_from < 0)
    return fail(BMPC_ERR_INVALID, "adapt_early, adapt_late, adapt_busy, adapt_flips, confirm_from must be >= 0");
  if (p.max_iter < 1 || p.check_every < 1) return fail(BMPC_ERR_INVALID, "max_iter, check_every must be >= 1");
  if (p.rescue < BMPC_RESCUE_AUTO || p.rescue > BMPC_RESCUE_ON) return fail(BMPC_ERR_INVALID, "unknown rescue mode %d", p.rescue);
  std::memset(d, 0, sizeof(*d));
  d->h = p.h; d->half = p.half; d->max_iter = p.max_iter; d->check_every = p.check_every;
  d->adapt_start = p.adapt_start; d->adapt_every = p.adapt_every; d->max_refactor = p.max_refactor;
  d->adapt_early = p.adapt_early; d->adapt_late = p.adapt_late;
  d->adapt_busy = p.adapt_busy; d->adapt_flips = p.adapt_flips;
  d->confirm_from = p.confirm_from; d->kappa_confirm = (float)p.kappa_confirm;
  d->dt = p.dt; d->kv = p.kv; d->m = p.m; d->g = p.g; d->mu = p.mu;
  d->lt = p.lt - 0.01;                       // REF:254
  d->lh = p.lh - 0.02;                       // REF:255
  d->alpha = p.alpha;
  d->accel = p.accel ? 1 : 0;
  for (int i = 0; i < 12; ++i) {
    d->x_cmd[i] = p.x_cmd[i];
    d->Q[i] = p.Q[i];
    d->R2[i] = 2.0 * p.R[i];
    if (!(p.R[i] > 0) || !(p.Q[i] >= 0)) return fail(BMPC_ERR_INVALID, "need R > 0, Q >= 0");
  }
  for (int k = 0; k < 3; ++k) { d->sq_e[k] = std::sqrt(2.0 * p.Q[k]); d->sq_w[k] = p.dt * std::sqrt(2.0 * p.Q[6 + k]); }
  d->kpm = p.dt * p.dt / p.m;
  d->kvm = p.dt / p.m;
  if (!inv3(p.I, d->Iinv)) return fail(BMPC_ERR_INVALID, "inertia matrix is singular");
  for (int i = 0; i < 3; ++i) {
    d->f_max[i] = p.f_max[i]; d->f_min[i] = p.f_min[i];
    d->tau_max[i] = p.tau_max[i]; d->tau_min[i] = p.tau_min[i];
    if (p.f_max[i] < p.f_min[i] || p.tau_max[i] < p.tau_min[i]) return fail(BMPC_ERR_INVALID, "upper bound below lower bound");
  }
  double pf = 1, pm = 1, pr = 1;               // curvature of this problem relative to the reference problem
  if (p.penalty_mode == BMPC_PENALTY_SCALED) {
    // Up to h = 20 the reference problem has the horizon of the problem at hand: the absolute values were tuned and soaked
    // at h = 10, 16 and 20 (10.5 M + 3.3 M instances), and the dense kernels' f32 sweep does not hold much larger ones
    // (ceilings 8x higher at h = 20: 2 % of a standing batch lose convergence, some to NaNs, where the stage-structured
    // kernels -- and the absolute values -- converge on every instance).  The long horizons (stage-structured kernels) follow
    // the stiff end, which grows like sum k^2 ~ h^3, relative to h = 10 (h = 40: 72x before the cap below; absolute values
    // there: 0.97 per iteration; relative to h = 20: 20 % more iterations and four times the non-converged instances).
    bmpc_params ref;
    default_params(&ref, p.h <= 20 ? p.h : 10);
    const CurvScales c0 = curvature_scales(ref), c1 = curvature_scales(p);
    if (!(c1.force > 0 && c1.moment > 0 && c1.soft > 0))
      return fail(BMPC_ERR_INVALID, "penalty_mode SCALED needs positive curvature scales (force %g, moment %g, soft %g: some "
                  "tracking weight Q is zero on every state a control acts on); use BMPC_PENALTY_ABSOLUTE", c1.force, c1.moment, c1.soft);
    pf = c1.force / c0.force; pm = c1.moment / c0.moment; pr = c1.soft / c0.soft;
  } else if (p.penalty_mode != BMPC_PENALTY_ABSOLUTE) {
    return fail(BMPC_ERR_INVALID, "unknown penalty_mode %d", p.penalty_mode);
  }
  const double rmin = min_R(p);
  double rho0 = p.rho * std::sqrt(pr * pf);              // between the soft and the stiff end
  double rho_eq = p.rho * p.rho_eq_scale * pf, rho_lo = p.rho_lo * pr, hi_f = p.rho_hi_f * pf, hi_m = p.rho_hi_m * pm;
  if (p.penalty_mode == BMPC_PENALTY_SCALED) {
    // What f32 holds: the stored null-space factor Ka^-1 has entries up to 1 / (2R + rho_lo) with 6e-8 relative error,
    // and that error is multiplied by the stiffest penalty of the block when the step is taken: above
    // eps_f32 x rho_max / (2R + rho_lo) ~ 1 the iteration stops contracting (seen as active-set cycling at R / 100).
    // The ceilings stay six decades above the soft end (error factor 0.06).
    // The dense family holds less: its f32 explicit inverse is the preconditioner of every iteration.  At Q x 10 the moment
    // ceiling resolved to 500 and 2 of 16384 standing h = 20 instances re-classified until the cap, where ceilings of 100 ..
    // 400 converge every instance in <= 490 iterations at the same mean (tools/soak.py options ... rho_hi_m=10..40): 4e5.  The
    // stage family (tuned and soaked at 1e6, h = 40: rho_eq = 500) keeps its cap.  Not binding at the reference's weights.
    const double top = (resolve_path(p.h, p.path) == BMPC_PATH_DENSE ? 4e5 : 1e6) * (2 * rmin + rho_lo);
    rho_eq = std::fmin(rho_eq, top); hi_f = std::fmin(hi_f, top); hi_m = std::fmin(hi_m, top);
    rho0 = std::fmin(rho0, hi_f);
  }
  d->r2min = (float)(2 * rmin);
  d->rho = (float)rho0;
  d->rho_eq = (float)rho_eq;
  d->rho_lo = (float)rho_lo;
  d->rho_hi_f = (float)hi_f; d->rho_hi_m = (float)hi_m;
  d->eps_pri = (float)p.eps_pri; d->eps_dua = (float)p.eps_dua; d->kappa = (float)p.kappa;
  {                                           // (f32 products exactly as the kernels used to form them: SLOW_TOL = 1e-6, U0_TOL = 5)
    const float slow_tol = 1.0e-6f, u0_tol = 5.f;
    d->kappa_sqrt = std::sqrt(d->kappa);
    d->kappa_qrt = std::sqrt(std::sqrt(d->kappa));
    d->slow_tol_r2 = slow_tol * d->r2min;
    d->slow_tol_r2_u0 = u0_tol * slow_tol * d->r2min;
    d->eps_u0 = u0_tol * std::fmax(d->eps_pri, d->eps_dua);
  }
  return BMPC_OK;
}

}  // namespace bmpc_host

#endif
