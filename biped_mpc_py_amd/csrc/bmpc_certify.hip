// bmpc_certify.hip -- KKT certificate of given control sequences (gfx950 / CDNA4): is this plan the constrained optimum, how far
// off is it, and which constraints bind at what price.
//
// Per instance, from the inputs of an evaluation (bmpc_evaluate.hip: bmpc_inputs and controls [h][12]) and an activity tolerance,
// fp64 on the fp32 inputs widened:
//   lam      [h][36]: multipliers of the inequality rows of REF:273-274 in the reference's order per step -- 0..7 friction (leg 0 then
//            leg 1, each +x, +y, -x, -y; REF:220-232), 8..19 upper bounds (+I u <= ub), 20..31 lower bounds (-I u <= -lb)
//            (REF:235-251), 32..35 line foot (REF:254-271).  Rows that are not active are exactly 0.
//   resid    [h][12]: g + C' lam, g = d cost / d controls: the stationarity residual of the condensed problem
//   summary  [4]: stationarity max|resid|, primal_ineq (the largest positive part of C u - b: the maximum of the evaluation's four
//            `violation` entries, same bits), complementarity max|lam_i slack_i|, grad_scale max|g|
//   n_active number of active rows;  status 0 = every NNLS converged, 1 = an iteration cap was reached, 2 = bad instance
//
// Every inequality row touches the controls [f, m] of ONE leg at ONE step.  With g from the adjoint sweep of bmpc_evaluate_grad.hip
// (eval_adjoint below; g has evaluate_grad_kernel's bits), stationarity g + C' lam = 0, lam >= 0 on the active rows splits into 2 h
// independent non-negative least-squares problems per instance: min |C_a' lam + g|, 6 equations, at most 18 candidate rows (4 friction,
// 6 + 6 box, 2 line foot).  A row is active iff slack = b - C u <= act_tol (1 + |b|) (the oracle's rule, oracle/bmpc_oracle.py
// certificate_from_primal).  Lawson-Hanson per (step, leg); the passive set has at most 6 columns and its least squares is a 6 x 6
// Cholesky of the normal equations with a rank guard.
//
// Thread map: the evaluation's -- one lane per (instance, step), the two legs one after the other, groups of L = 16 / 32 / 64 lanes,
// lane_read permutes in the evaluation's fixed order for the sums and maxima, no barrier.  The NNLS loop diverges per lane and holds
// no cross-lane traffic.  It keeps no dynamically indexed private array: the passive set lives in six SLOTS (value, row number) that
// unrolled selects fill, compact and scatter, and a row's coefficients are generated from (mu, body axes) by row class wherever they
// are needed.  LDS: 39 doubles per lane (78 KB per workgroup) in two slabs -- g of both legs (12) and the triangular factor of the
// passive least squares with its right-hand side (27) -- each lane reading only what it wrote, so no barrier.  They are there for the
// register count alone: with g, the factor and six ready-made columns in registers the kernel needs 358 and, capped at 256, goes to
// scratch; with the slabs it has 221 and two waves per SIMD (tests/test_certify_resources.py).
//
// Bad instances (bmpc_evaluate.hip) get NaN in every fp64 output, n_active -1 and status 2; selects keep their values out of every
// other group.  Compiles as plain C++ for tests/emu (BMPC_EMU) like bmpc_evaluate.hip.
#ifndef BMPC_CERTIFY_HIP
#define BMPC_CERTIFY_HIP

#include "bmpc_evaluate_grad.hip"

#ifdef BMPC_EMU
#define BMPC_CERT_OPAQUE(x) do { } while (0)
#else
// The compiler may assume nothing about x from here on.  Used on the lane's read index of the LDS slabs, so that stored values are
// not forwarded to their loads and kept in registers as well.  Without it the slabs save nothing: expect 221 VGPRs with it
// (tests/test_certify_resources.py asserts <= 256 and no scratch); it changes no result.
#define BMPC_CERT_OPAQUE(x) asm volatile("" : "+v"(x))
#endif

namespace bmpc {

struct CertOut {             // all nullable, device pointers
  double* lam;               // [B][h][36]
  double* resid;             // [B][h][12]
  double* summary;           // [B][4]: stationarity, primal_ineq, complementarity, grad_scale
  int32_t* n_active;         // [B]
  int32_t* status;           // [B]
};

constexpr int CERT_ROWS = 18;                  // candidate rows of one leg: 0..3 friction, 4..9 upper bounds of [f, m], 10..15 lower
                                               // bounds, 16, 17 line foot
constexpr int CERT_SLAB = 27;                  // doubles per lane of the least-squares slab in LDS: the triangular factor and y
constexpr int CERT_CAP = 3 * CERT_ROWS;        // least-squares solves per leg (SciPy's nnls: maxiter = 3 n)

// place of a leg's candidate row j in the 36 rows of its step (leg g)
__device__ __forceinline__ constexpr int cert_step_row(const int g, const int j) {
  return j < 4 ? 4 * g + j : (j < 7 ? 8 + 3 * g + (j - 4) : (j < 10 ? 14 + 3 * g + (j - 7) : (j < 13 ? 20 + 3 * g + (j - 10) :
         (j < 16 ? 26 + 3 * g + (j - 13) : 32 + 2 * g + (j - 16)))));
}

struct CertLeg {             // what the general rows of one leg at one step are made of (general_rows of bmpc_model.hip, in fp64)
  double mu, ey[3], ez[3], lh, lt;             // friction coefficient, body axes, line-foot lengths with their margins (REF:254-262)
};

// the 18 candidate rows times v = [f(3), m(3)]: C_leg v
__device__ __forceinline__ void cert_rows_times(const CertLeg& q, const double (&v)[6], double (&o)[CERT_ROWS]) {
  const double mz = q.mu * v[2];
  o[0] = v[0] - mz; o[1] = v[1] - mz; o[2] = -v[0] - mz; o[3] = -v[1] - mz;                    // REF:220-229
#pragma unroll
  for (int a = 0; a < 6; ++a) { o[4 + a] = v[a]; o[10 + a] = -v[a]; }                          // REF:235-251
  const double fz = q.ez[0] * v[0] + q.ez[1] * v[1] + q.ez[2] * v[2], my = q.ey[0] * v[3] + q.ey[1] * v[4] + q.ey[2] * v[5];
  o[16] = my - q.lh * fz; o[17] = -my - q.lt * fz;                                             // REF:259-262
}

// right-hand sides b and slacks b - C v of the 18 candidate rows of a leg with contact flag cg (bounds scaled by contact, REF:239-249)
__device__ __forceinline__ void cert_slacks(const EvalParams& P, const CertLeg& q, const double cg, const double (&v)[6],
                                            double (&slack)[CERT_ROWS], double (&bnd)[CERT_ROWS]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bnd[4 + a] = cg * P.f_max[a]; bnd[7 + a] = cg * P.tau_max[a];
    bnd[10 + a] = -(cg * P.f_min[a]); bnd[13 + a] = -(cg * P.tau_min[a]);
  }
  bnd[0] = bnd[1] = bnd[2] = bnd[3] = bnd[16] = bnd[17] = 0.0;
  cert_rows_times(q, v, slack);
#pragma unroll
  for (int j = 0; j < CERT_ROWS; ++j) slack[j] = bnd[j] - slack[j];
}

// candidate row k (0 .. 17, a run-time value) as a column of C_leg': selects by row class, no indexed array
__device__ __forceinline__ void cert_column(const CertLeg& q, const int k, double (&c)[6]) {
  const bool fric = k >= 0 && k < 4, up = k >= 4 && k < 10, lo = k >= 10 && k < 16, l0 = k == 16;   // (k < 0: an empty slot, zeros)
  const int ax = fric ? (k & 1) : (up ? k - 4 : k - 10);       // the entry a friction / box row puts its +-1 in
  const double one = fric ? (k < 2 ? 1.0 : -1.0) : (up ? 1.0 : -1.0);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double lf;
    if (i < 3) lf = -(l0 ? q.lh : q.lt) * q.ez[i];
    else lf = l0 ? q.ey[i - 3] : -q.ey[i - 3];
    double e = ax == i ? one : 0.0;
    if (i == 2) e = fric ? -q.mu : e;
    c[i] = k < 0 ? 0.0 : ((fric || up || lo) ? e : lf);
  }
}

// least squares over the passive slots (row numbers id[s], -1 = empty): z = argmin |sum_s z_s a(id[s]) - tgt| by the Cholesky factor of
// the normal equations.  The columns are generated from their row numbers as they are needed and never all held.  A slot whose pivot
// is not above 2^-40 of its column's square (an empty slot: 0; a column that depends on the slots before it) gets z = 0; bit s of the
// result says so.
__device__ __forceinline__ int cert_ls(const CertLeg& q, const int (&id)[6], const double (&tgt)[6], double (&z)[6],
                                       double (&F)[CERT_SLAB][EVAL_NT], const int tw, const int tr) {
  // the factor lives in the lane's column of the LDS slab F: row i (i + 1) / 2 + j holds L[i][j] (j < i) or 1 / L[i][i], rows 21 .. 26 hold y.
  // Written through `tw` and read through `tr`, the same number under two names: values forwarded from the store to the load
  // would stay in registers, which is what the slab is there to avoid.
#define LT(i, j) ((i) * ((i) + 1) / 2 + (j))
  int dep = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double ci[6];
    cert_column(q, id[i], ci);
    double b = 0.0, sq = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) { b += ci[e] * tgt[e]; sq += ci[e] * ci[e]; }
    double li[6];
#pragma unroll
    for (int j = 0; j < i; ++j) {              // L[i][j] = (M[i][j] - sum_k L[i][k] L[j][k]) / L[j][j]
      double cj[6];
      cert_column(q, id[j], cj);
      double a = 0.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) a += ci[e] * cj[e];
#pragma unroll
      for (int k = 0; k < j; ++k) a -= li[k] * F[LT(j, k)][tr];
      li[j] = (dep >> j & 1) ? 0.0 : a * F[LT(j, j)][tr];
    }
    double d = sq;
#pragma unroll
    for (int k = 0; k < i; ++k) { d -= li[k] * li[k]; b -= li[k] * F[21 + k][tr]; }
    const bool ok = d > 0x1p-40 * sq;
    dep |= ok ? 0 : (1 << i);
    const double inv = ok ? 1.0 / sqrt(d) : 1.0;
#pragma unroll
    for (int k = 0; k < i; ++k) F[LT(i, k)][tw] = ok ? li[k] : 0.0;
    F[LT(i, i)][tw] = inv;
    F[21 + i][tw] = ok ? b * inv : 0.0;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {               // L' z = y; a guarded slot has y = 0 and an empty row: it stays out of the others
    double a = F[21 + i][tr];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) a -= F[LT(k, i)][tr] * z[k];
    z[i] = (dep >> i & 1) ? 0.0 : a * F[LT(i, i)][tr];
  }
#undef LT
  return dep;
}

// C' x of the passive slots: sum_s xs[s] a(id[s])
__device__ __forceinline__ void cert_combine(const CertLeg& q, const int (&id)[6], const double (&xs)[6], double (&ax)[6]) {
#pragma unroll
  for (int e = 0; e < 6; ++e) ax[e] = 0.0;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    double c[6];
    cert_column(q, id[s], c);
#pragma unroll
    for (int e = 0; e < 6; ++e) ax[e] += xs[s] * c[e];
  }
}

// Lawson-Hanson on the rows `active` (bit j = candidate row j) of one leg: lam >= 0 on them minimising |C' lam - tgt|.  Out: lam per
// candidate row (exactly 0 off the passive set) and ax = C' lam.  Returns 1 if the cap on least-squares solves was reached (lam is
// then still >= 0 and supported on active rows: a valid certificate, not the smallest residual).
__device__ __forceinline__ int cert_nnls(const CertLeg& q, const int active, const double (&tgt)[6], double (&lam)[CERT_ROWS],
                                         double (&ax)[6], double (&F)[CERT_SLAB][EVAL_NT], const int tw, const int tr) {
  double xs[6];                                // the passive set: value and row number of slots 0 .. np - 1; empty slots hold 0 and -1
  int id[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) { xs[s] = 0.0; id[s] = -1; }
  double scale = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) scale = fmax(scale, fabs(tgt[e]));
  const double tolw = 0x1p-46 * scale;         // a dual value below 64 eps of the target's size is rounding, not a descent direction
  int np = 0, in_p = 0, banned = 0, solves = 0, capped = 0;
  bool go = true;
  while (go) {
    // dual w = C (tgt - C' x) of the rows that may still enter: the largest one above the tolerance
    double r[6], w[CERT_ROWS];
    cert_combine(q, id, xs, r);
#pragma unroll
    for (int e = 0; e < 6; ++e) r[e] = tgt[e] - r[e];
    cert_rows_times(q, r, w);
    const int elig = active & ~in_p & ~banned;
    int k = -1;
    double wk = tolw;
#pragma unroll
    for (int j = 0; j < CERT_ROWS; ++j) {
      const bool better = (elig >> j & 1) && w[j] > wk;
      wk = better ? w[j] : wk;
      k = better ? j : k;
    }
    if (k < 0 || np >= 6) break;               // (six independent columns span the leg's space: nothing is left to fit)
#pragma unroll
    for (int s = 0; s < 6; ++s) id[s] = s == np ? k : id[s];
    in_p |= 1 << k;
    ++np;
    bool fresh = true;                         // the first least squares after a row entered: slot np - 1 is that row, its value 0
    for (;;) {
      double z[6];
      const int dep = cert_ls(q, id, tgt, z, F, tw, tr);
      ++solves;
      int rm = 0;                              // slots to take out of the passive set
      double znew = 0.0;
#pragma unroll
      for (int s = 0; s < 6; ++s) znew = s == np - 1 ? z[s] : znew;
      // the row that just entered depends on the passive ones, or its value is not positive (w was rounding): out, and not tried
      // again while the passive set stays as it is (Lawson-Hanson skip it for the iteration); once a slot leaves, it may be needed
      const bool fresh_out = fresh && ((dep >> (np - 1) & 1) || !(znew > 0.0));
      fresh = false;
      if (fresh_out) {
        rm = 1 << (np - 1);
        banned |= 1 << k;
      } else {
        double alpha = 2.0;
        int blk = -1;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          const bool neg = s < np && !(z[s] > 0.0);
          const double a = xs[s] / (xs[s] - z[s]);
          const bool first = neg && a < alpha;
          alpha = first ? a : alpha;
          blk = first ? s : blk;
        }
        if (blk < 0) {                         // the least-squares point is inside the cone: take it
#pragma unroll
          for (int s = 0; s < 6; ++s) xs[s] = z[s];
          break;
        }
        if (solves >= CERT_CAP) { capped = 1; go = false; break; }
#pragma unroll
        for (int s = 0; s < 6; ++s) {          // as far towards it as the cone allows; what reached its face leaves
          xs[s] += alpha * (z[s] - xs[s]);
          rm |= (s < np && (s == blk || !(xs[s] > 0.0))) ? (1 << s) : 0;
        }
        banned = 0;                            // the passive set shrinks: rows set aside against the larger set are candidates again
      }
      // take the slots of `rm` out, highest first; the slots above move down
#pragma unroll
      for (int s = 5; s >= 0; --s) {
        const bool out = rm >> s & 1;
        in_p &= out ? ~(1 << (id[s] & 31)) : ~0;
#pragma unroll
        for (int u = s; u < 6; ++u) {
          if (u == 5) { xs[u] = out ? 0.0 : xs[u]; id[u] = out ? -1 : id[u]; }
          else { xs[u] = out ? xs[u + 1] : xs[u]; id[u] = out ? id[u + 1] : id[u]; }
        }
        np -= out ? 1 : 0;
      }
      if (fresh_out || np == 0) break;         // (x is as it was before the row entered, or empty: back to the dual)
    }
    if (solves >= CERT_CAP) { capped = 1; go = false; }
  }
#pragma unroll
  for (int j = 0; j < CERT_ROWS; ++j) {
    double v = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) v = id[s] == j ? xs[s] : v;
    lam[j] = v;
  }
  cert_combine(q, id, xs, ax);
  return capped;
}

// The backward pass of one (instance, step): evaluate_grad_kernel's (bmpc_evaluate_grad.hip), statement for statement -- from the
// state x after step k, row k of grad_u (`gu`), the euler / p costates `lo`, the omega / v costates `hi` and what A_k' sends down
// (`down`).  It is stated here a second time because calling it from evaluate_grad_kernel was measured to move that kernel's `cost`
// by an ulp on the MI355X (another contraction of the cost sum; grad_u and grad_x0 kept their bits): docs/history_r11.md.  gu has
// evaluate_grad_kernel's bits (tests/test_gpu_certify.py compares them with act_tol = -1).
__device__ __forceinline__ void eval_adjoint(const EvalParams& P, const EvalLane& t, const EvalStep& s, const double (&x)[12],
                                             double (&gu)[12], double (&lo)[6], double (&hi)[6], double (&down)[6]) {
  const int L = t.L, lane = t.lane, gl = t.gl;
  const double dt = P.dt;
  // ---- backward, round 1: lambda_eul, lambda_p = suffix sums of 2 Q e  (lanes past the horizon hold clones: zero by a select)
  double lam[12];                              // lambda_k in the order of the state: euler, p, omega, v
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double ge = 2.0 * P.Q[i] * (x[i] - s.xr[i]);
    lam[i] = t.live ? ge : 0.0;
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) lo[a] = lam[a];
  group_suffix<6>(lo, lane, gl, L);
  // what A_k' sends from (lambda_eul, lambda_p) of THIS lane to (omega, v) of the lane below: dt R_inv,k' lambda_eul, dt lambda_p
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    down[a] = dt * (s.Rv[a] * lo[0] + s.Rv[3 + a] * lo[1] + s.Rv[6 + a] * lo[2]);
    down[3 + a] = dt * lo[3 + a];
  }
  // ---- round 2: lambda_omega, lambda_v = suffix sums of 2 Q e + the lane above's `down`
  {
    const int src = (lane + 1) & 63;
    const bool has_above = gl + 1 < P.h;       // (h <= L: the source is a live lane of this group)
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double o = lane_read(down[a], src);
      hi[a] = lam[6 + a] + (has_above ? o : 0.0);      // (a lane past the horizon: 0 + 0)
    }
  }
  group_suffix<6>(hi, lane, gl, L);

  // ---- row k of grad_u = 2 R u_k + B_k' lambda_k
  {
    double w[3];                               // dt I_w,k' lambda_omega
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = dt * (s.Iw[a] * hi[0] + s.Iw[3 + a] * hi[1] + s.Iw[6 + a] * hi[2]);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const double* r = s.r[g];
      const double wxr[3] = {w[1] * r[2] - w[2] * r[1], w[2] * r[0] - w[0] * r[2], w[0] * r[1] - w[1] * r[0]};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        gu[3 * g + a] = 2.0 * P.R[3 * g + a] * s.u[3 * g + a] + (P.kvm * hi[3 + a] + wxr[a]);
        gu[6 + 3 * g + a] = 2.0 * P.R[6 + 3 * g + a] * s.u[6 + 3 * g + a] + w[a];
      }
    }
  }
}

__global__ void __launch_bounds__(EVAL_NT, 2)   // two waves per SIMD: at most 256 registers, accumulation registers included
certify_kernel(const EvalParams P, const int B,
               const float* __restrict__ x_fb, const float* __restrict__ foot,
               const uint8_t* __restrict__ contact, const int32_t* __restrict__ phase,
               const float* __restrict__ x_cmd, const float* __restrict__ mu_in,
               const float* __restrict__ x_ref, const float* __restrict__ foot_ref,
               const float* __restrict__ controls, const double act_tol, const CertOut out) {
  const EvalLane t = eval_lane(P.h, B);
  const int L = t.L, lane = t.lane;

  // ---- forward and adjoint pass: the evaluation's own functions, the gradient's backward pass
  EvalStep s;
  eval_load(P, t, x_fb, foot, contact, phase, x_cmd, mu_in, x_ref, foot_ref, controls, s);
  const double con[2] = {(double)contact[t.row * 2 + 0], (double)contact[t.row * 2 + 1]};
  double inc[6], x[12];
  eval_step_model(P, s, inc);
  eval_recurrence(P, t, s, inc, x);
  const int bad = eval_bad(t, s, x);
  double g[12], lo[6], hi[6], down[6];
  eval_adjoint(P, t, s, x, g, lo, hi, down);
  double viol[4];
  eval_step_violation(P, s, con, viol);

  // ---- the rows of this step, leg by leg: slacks, activity, NNLS, residual
  double ey[3], ez[3];
  {
    double s0, c0, s1, c1, s2, c2;
    sincos(s.xfb[0], &s0, &c0);
    sincos(s.xfb[1], &s1, &c1);
    sincos(s.xfb[2], &s2, &c2);
    body_axes(s0, c0, s1, c1, s2, c2, ey, ez);
  }
  const double nan = __builtin_nan("");
  const bool store = t.in_batch && t.live;
  {                                            // primal_ineq: reduced and stored now, two registers fewer across the NNLS loop
    double pm[1] = {t.live ? fmax(fmax(viol[0], viol[1]), fmax(viol[2], viol[3])) : 0.0};
    group_max<1>(pm, lane, L);
    if (t.in_batch && t.gl == 0 && out.summary) out.summary[t.inst * 4 + 1] = bad ? nan : pm[0];
  }
  double mx[3] = {0.0, 0.0, 0.0};              // stationarity, complementarity, |g|
  int nact = 0, capped = 0;
  // The leg loop is kept rolled and takes what it needs of its leg by an index that depends on `leg`: g from a slab in LDS (each
  // lane reads only what it wrote: no barrier), the controls, mu and contact from global memory again.  Held in registers across
  // the NNLS loop instead, both legs' values cost 60 registers and the kernel goes to scratch.
  __shared__ double g_slab[12][EVAL_NT];
  __shared__ double ls_slab[CERT_SLAB][EVAL_NT];
  const int tw = threadIdx.x;
  int tr = threadIdx.x;
  BMPC_CERT_OPAQUE(tr);
#pragma unroll
  for (int i = 0; i < 12; ++i) g_slab[i][threadIdx.x] = g[i];
#pragma unroll 1
  for (int leg = 0; leg < 2; ++leg) {
    const bool l1 = leg == 1;
    CertLeg q;
    q.lh = P.lh; q.lt = P.lt;
    q.mu = mu_in ? (double)mu_in[t.row * 2 + leg] : P.mu;
    const double cg = (double)contact[t.row * 2 + leg];
    double v[6], tgt[6], gl6[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      q.ey[a] = ey[a]; q.ez[a] = ez[a];
      v[a] = (double)controls[t.row * 12 + 3 * leg + a];
      v[3 + a] = (double)controls[t.row * 12 + 6 + 3 * leg + a];
      gl6[a] = g_slab[3 * leg + a][threadIdx.x];
      gl6[3 + a] = g_slab[6 + 3 * leg + a][threadIdx.x];
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) tgt[e] = -gl6[e];
    double bnd[CERT_ROWS], slack[CERT_ROWS];
    cert_slacks(P, q, cg, v, slack, bnd);
    int active = 0;
#pragma unroll
    for (int j = 0; j < CERT_ROWS; ++j) active |= slack[j] <= act_tol * (1.0 + fabs(bnd[j])) ? (1 << j) : 0;
    double lam[CERT_ROWS], ax[6];
    capped |= cert_nnls(q, active, tgt, lam, ax, ls_slab, tw, tr);
    nact += __builtin_popcount((unsigned)active);
#pragma unroll
    for (int a = 0; a < 3; ++a) {              // (read and formed again rather than kept across the NNLS loop)
      v[a] = (double)controls[t.row * 12 + 3 * leg + a];
      v[3 + a] = (double)controls[t.row * 12 + 6 + 3 * leg + a];
      gl6[a] = g_slab[3 * leg + a][tr];
      gl6[3 + a] = g_slab[6 + 3 * leg + a][tr];
    }
    cert_slacks(P, q, cg, v, slack, bnd);
#pragma unroll
    for (int j = 0; j < CERT_ROWS; ++j) mx[1] = fmax(mx[1], fabs(lam[j] * slack[j]));
    double res[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      res[e] = gl6[e] + ax[e];
      mx[0] = fmax(mx[0], fabs(res[e]));
      mx[2] = fmax(mx[2], fabs(gl6[e]));
    }
    if (store && out.lam) {
      double* lp = out.lam + t.row * 36;
#pragma unroll
      for (int j = 0; j < CERT_ROWS; ++j) lp[l1 ? cert_step_row(1, j) : cert_step_row(0, j)] = bad ? nan : lam[j];
    }
    if (store && out.resid) {
      double* ro = out.resid + t.row * 12;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ro[(l1 ? 3 : 0) + a] = bad ? nan : res[a];
        ro[(l1 ? 9 : 6) + a] = bad ? nan : res[3 + a];
      }
    }
  }

  // ---- per instance: maxima, the number of active rows, whether a cap was reached
  if (!t.live) { mx[0] = 0.0; mx[1] = 0.0; mx[2] = 0.0; nact = 0; capped = 0; }
  group_max<3>(mx, lane, L);
  for (int m = 1; m < L; m <<= 1) nact += lane_read(nact, lane ^ m);
  capped = group_or(capped, lane, L);
  if (!t.in_batch || t.gl != 0) return;
  if (out.summary) {
    out.summary[t.inst * 4 + 0] = bad ? nan : mx[0];
    out.summary[t.inst * 4 + 2] = bad ? nan : mx[1];
    out.summary[t.inst * 4 + 3] = bad ? nan : mx[2];
  }
  if (out.n_active) out.n_active[t.inst] = bad ? -1 : nact;
  if (out.status) out.status[t.inst] = bad ? 2 : capped;
}

}  // namespace bmpc

#endif  // BMPC_CERTIFY_HIP
