// bmpc_evaluate_samples.hip -- S candidate plans per instance in one launch, ranked and blended on the device (gfx950 / CDNA4):
// the batched cost for samplers (MPPI, predictive sampling, plan refinement).  include/bmpc.h states what comes out.
//
// evaluate_samples_kernel.  The lane map of the evaluation family (bmpc_evaluate.hip): one lane per step, a group of
// L = eval_lanes(h) lanes of a wave.  A group owns ONE instance and a contiguous run ("chunk") of C of its samples, C =
// eval_samples_per_group(B, S), stated next to eval_lanes in bmpc_evaluate.hip; an instance has ceil(S / C) groups.
// Everything about step k that does not depend on the controls is done
// once per group: the loads other than controls, the generated references, the three sincos of the reference attitude, Rot,
// (Rot' I Rot)^-1, R_inv, the lever arms, contact and mu of the step, and the three sincos and body axes of x_fb for the line-foot
// rows.  Per sample the lane then loads twelve controls (those of sample s + 1 are requested before the arithmetic of sample s),
// forms the torque and force increments, runs the two group_prefix rounds of eval_recurrence, the step's cost and violation rows,
// ONE group_sum (the cost) and ONE group_max (four violation classes and the sample's bad flag), and lane 0 of the group stores.
// lane_read needs every lane of the wave active: the trip count is C for every group of the launch; groups past the batch and
// iterations past S clone the last sample with their stores suppressed, as lanes past the horizon clone the last step.
//
// A sample's values are a function of its instance's inputs and its own controls alone: the set-up holds no sample's data, the
// loop carries nothing from one sample to the next but the prefetched controls of the next, and the sums and maxima run in an
// order fixed by the lane's place in its group.  B, S, C and the sample's place play no part.
//
// Bad values: a bad INSTANCE (non-finite input or reference, singular reference pitch; found once per group) makes every sample
// NaN; a non-finite control entry or state makes THAT sample NaN (its flag rides the group_max as a fifth value).
//
// sample_reduce_kernel.  One workgroup per instance, behind the first kernel on the same stream: n_valid, best, the softmin
// weights, ess and the weighted mean plan from the scores.  No floating-point atomics; every sum runs in an order fixed by
// (S, h): per lane over s = lane, lane + NT, ... and then a tree over the lanes in LDS; u_mean per element in NT / (12 h) slices
// of the samples, four interleaved partial sums each, added in the order of the slices.
//
// The shared __forceinline__ functions of bmpc_evaluate.hip are called where they fit as they are (eval_load, eval_recurrence,
// eval_step_cost, group_sum / group_max / group_or); where one mixes set-up and per-sample work (eval_step_model,
// eval_step_violation, eval_bad) the split form is stated here: the same expressions in the same order.
//
// Compiles as plain C++ for tests/emu (BMPC_EMU) like the files it includes.
#ifndef BMPC_EVALUATE_SAMPLES_HIP
#define BMPC_EVALUATE_SAMPLES_HIP

#include "bmpc_evaluate.hip"

namespace bmpc {

constexpr int SAMPLES_MAX = 65536;             // S of bmpc_samples
constexpr int REDUCE_NT = 1024;                // lanes of a sample_reduce_kernel workgroup (>= 12 h at every horizon)

struct SamplesOut {          // device pointers; cost / violation nullable, score never (the reductions read it)
  double* cost;              // [B][S]
  double* violation;         // [B][S][4]
  double* score;             // [B][S]
};
struct SamplesPrice { double w[4]; };          // w_viol of bmpc_samples

struct ReduceOut {           // device pointers; weights never null (u_mean reads it), the others nullable
  int32_t* best;             // [B]
  int32_t* n_valid;          // [B]
  double* weights;           // [B][S]
  double* u_mean;            // [B][h][12]
  double* ess;               // [B]
};

// ---- eval_step_model, split: what of a step's model does not depend on the controls ...
__device__ __forceinline__ void samples_step_setup(const EvalParams& P, EvalStep& s) {
  const double* xr = s.xr;
  double sy, cy, sp, cp, sr, cr;               // REF:151-153: yaw = x[0], pitch = x[1], roll = x[2]
  sincos(xr[0], &sy, &cy);
  sincos(xr[1], &sp, &cp);
  sincos(xr[2], &sr, &cr);
  s.singular = !(fabs(cp) >= 0x1p-22);
  // Rot = Rx(roll) Ry(pitch) Rz(yaw)   (scipy 'zyx' extrinsic, REF:154-156)
  const double Rot[9] = {cp * cy, -cp * sy, sp,
                         cr * sy + sr * sp * cy, cr * cy - sr * sp * sy, -sr * cp,
                         sr * sy - cr * sp * cy, sr * cy + cr * sp * sy, cr * cp};
  double T[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      T[3 * a + b] = P.Iinv[3 * a] * Rot[b] + P.Iinv[3 * a + 1] * Rot[3 + b] + P.Iinv[3 * a + 2] * Rot[6 + b];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      s.Iw[3 * a + b] = Rot[a] * T[b] + Rot[3 + a] * T[3 + b] + Rot[6 + a] * T[6 + b];   // Rot' Iinv Rot = (Rot' I Rot)^-1
  const double tp = sp / cp;
  const double rv[9] = {cy / cp, sy / cp, 0, -sy, cy, 0, cy * tp, sy * tp, 1};           // REF:160-164 inverted
#pragma unroll
  for (int q = 0; q < 9; ++q) s.Rv[q] = rv[q];
#pragma unroll
  for (int g = 0; g < 2; ++g) {                // lever arms r_g = foot_ref_g - x_ref[3:6]  (REF:174-179)
    s.r[g][0] = s.fr[3 * g] - xr[3]; s.r[g][1] = s.fr[3 * g + 1] - xr[4]; s.r[g][2] = s.fr[3 * g + 2] - xr[5];
  }
}

// ... and what does: this step's increments of omega and v for the controls s.u -- B_k u_k and the gravity column of A_k
__device__ __forceinline__ void samples_step_inc(const EvalParams& P, const EvalStep& s, double (&inc)[6]) {
  const double dt = P.dt;
  const double* u = s.u;
  // net torque about the CoM: r_1 x f_1 + r_2 x f_2 + m_1 + m_2  (REF:174-179)
  double tau[3] = {u[6] + u[9], u[7] + u[10], u[8] + u[11]};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double* r = s.r[g];
    const double* f = &u[3 * g];
    tau[0] += r[1] * f[2] - r[2] * f[1];
    tau[1] += r[2] * f[0] - r[0] * f[2];
    tau[2] += r[0] * f[1] - r[1] * f[0];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    inc[a] = dt * (s.Iw[3 * a] * tau[0] + s.Iw[3 * a + 1] * tau[1] + s.Iw[3 * a + 2] * tau[2]);
    inc[3 + a] = P.kvm * (u[a] + u[3 + a]);                                              // REF:180
  }
  inc[5] -= P.g * dt;                                                                    // REF:169
}

// ---- eval_step_violation, split: the body axes of x_fb (REF:124-138, 193, 259-262) ...
__device__ __forceinline__ void samples_axes(const EvalStep& s, double (&ey)[3], double (&ez)[3]) {
  double s0, c0, s1, c1, s2, c2;
  sincos(s.xfb[0], &s0, &c0);
  sincos(s.xfb[1], &s1, &c1);
  sincos(s.xfb[2], &s2, &c2);
  body_axes(s0, c0, s1, c1, s2, c2, ey, ez);
}

// ... and the rows of Aqp z <= bqp of this step (REF:273-274) for the controls s.u: the largest positive part per class
__device__ __forceinline__ void samples_step_violation(const EvalParams& P, const EvalStep& s, const double (&con)[2],
                                                       const double (&ey)[3], const double (&ez)[3], double (&viol)[5]) {
  const double* u = s.u;
  const double* mu = s.mu;
  viol[0] = 0.0; viol[1] = 0.0; viol[2] = 0.0; viol[3] = 0.0;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double* f = &u[3 * g];
    const double* m = &u[6 + 3 * g];
    const double mf = mu[g] * f[2];
    viol[0] = fmax(viol[0], fmax(fmax(f[0] - mf, f[1] - mf), fmax(-f[0] - mf, -f[1] - mf)));          // REF:220-229
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                                                      // REF:235-251
      viol[1] = fmax(viol[1], fmax(f[a] - con[g] * P.f_max[a], con[g] * P.f_min[a] - f[a]));
      viol[2] = fmax(viol[2], fmax(m[a] - con[g] * P.tau_max[a], con[g] * P.tau_min[a] - m[a]));
    }
    const double fz = ez[0] * f[0] + ez[1] * f[1] + ez[2] * f[2], my = ey[0] * m[0] + ey[1] * m[1] + ey[2] * m[2];
    viol[3] = fmax(viol[3], fmax(my - P.lh * fz, -my - P.lt * fz));                                    // REF:259-262
  }
}

// ---- eval_bad, split: is everything of the INSTANCE that the lanes of this group saw finite, and no reference pitch singular ...
__device__ __forceinline__ int samples_bad_instance(const EvalLane& t, const EvalStep& s) {
  double mag = fabs(s.mu[0]) + fabs(s.mu[1]);
#pragma unroll
  for (int i = 0; i < 12; ++i) mag += fabs(s.xfb[i]) + fabs(s.xr[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) mag += fabs(s.fr[i]);
#pragma unroll
  for (int q = 0; q < 9; ++q) mag += fabs(s.Rv[q]);
  return group_or((t.live && (s.singular || !(mag <= 1.7976931348623157e308))) ? 1 : 0, t.lane, t.L);
}
// ... and of this lane's step of the SAMPLE: 1.0 if not (a value of the group_max)
__device__ __forceinline__ double samples_bad_step(const EvalLane& t, const EvalStep& s, const double (&x)[12]) {
  double mag = 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i) mag += fabs(s.u[i]) + fabs(x[i]);
  return (t.live && !(mag <= 1.7976931348623157e308)) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(EVAL_NT)
evaluate_samples_kernel(const EvalParams P, const int B, const int S, const int C,
                        const float* __restrict__ x_fb, const float* __restrict__ foot,
                        const uint8_t* __restrict__ contact, const int32_t* __restrict__ phase,
                        const float* __restrict__ x_cmd, const float* __restrict__ mu_in,
                        const float* __restrict__ x_ref, const float* __restrict__ foot_ref,
                        const float* __restrict__ controls, const SamplesPrice price, const SamplesOut out) {
  // ---- where the lane stands: its group = (instance, chunk of C samples), its place in the group = its step
  const int h = P.h;
  const long long chunks = ((long long)S + C - 1) / C;        // groups per instance
  EvalLane t;
  t.L = eval_lanes(h);
  t.lane = threadIdx.x & 63;
  t.gl = t.lane & (t.L - 1);
  const long long grp = ((long long)blockIdx.x * EVAL_NT + threadIdx.x) / t.L;
  t.in_batch = grp < (long long)B * chunks;
  const long long own = t.in_batch ? grp : (long long)B * chunks - 1;
  t.inst = (size_t)(own / chunks);
  const long long s0 = (own % chunks) * C;                    // first sample of the chunk (< S)
  t.live = t.gl < h;
  t.k = t.live ? t.gl : h - 1;
  t.row = t.inst * (size_t)h + (size_t)t.k;
  const size_t plan0 = t.inst * (size_t)S;                    // index of the instance's sample 0 among the B S plans
  const size_t plan_floats = (size_t)h * 12;

  // ---- once per group.  (eval_load addresses controls[row][12] with row = inst h + k: handed the array from plan
  // plan0 + s0 - inst on, it loads step k of the chunk's first sample)
  EvalStep s;
  eval_load(P, t, x_fb, foot, contact, phase, x_cmd, mu_in, x_ref, foot_ref, controls + (plan0 + (size_t)s0 - t.inst) * plan_floats, s);
  const double con[2] = {(double)contact[t.row * 2 + 0], (double)contact[t.row * 2 + 1]};
  samples_step_setup(P, s);
  double ey[3], ez[3];
  samples_axes(s, ey, ez);
  const int bad_inst = samples_bad_instance(t, s);
  const double nan = __builtin_nan("");

  // ---- per sample
#pragma unroll 1
  for (int j = 0; j < C; ++j) {
    const long long sj = s0 + j;                              // this iteration's sample; past S: a clone of sample S - 1, not stored
    const bool store = t.in_batch && t.gl == 0 && sj < (long long)S;
    const size_t plan = plan0 + (size_t)(sj < S ? sj : (long long)S - 1);
    float un[12];                                             // the next iteration's controls, on their way while this one computes
    {
      const long long sn = sj + 1 < (long long)S ? sj + 1 : (long long)S - 1;
      const float* p = controls + ((plan0 + (size_t)sn) * (size_t)h + (size_t)t.k) * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) un[i] = p[i];
    }
    double inc[6], x[12];                                     // x = state after step k
    samples_step_inc(P, s, inc);
    eval_recurrence(P, t, s, inc, x);
    double sum[1] = {0.0};
    eval_step_cost(P, s, x, sum[0]);
    double viol[5];                                           // four row classes, and the bad flag of the sample
    samples_step_violation(P, s, con, ey, ez, viol);
    viol[4] = samples_bad_step(t, s, x);
    if (!t.live) { sum[0] = 0.0; viol[0] = 0.0; viol[1] = 0.0; viol[2] = 0.0; viol[3] = 0.0; }
    group_sum<1>(sum, t.lane, t.L);
    group_max<5>(viol, t.lane, t.L);
    if (store) {
      const bool bad = bad_inst || viol[4] != 0.0;
      const double cost = bad ? nan : sum[0];
      if (out.cost) out.cost[plan] = cost;
      double score = cost;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double v = bad ? nan : viol[c];
        if (out.violation) out.violation[plan * 4 + c] = v;
        score += price.w[c] * v;
      }
      out.score[plan] = score;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) s.u[i] = (double)un[i];
  }
}

// ---- the reductions of one instance

// is the score that of a valid sample (finite)?
__device__ __forceinline__ bool sample_valid(const double score) { return fabs(score) <= 1.7976931348623157e308; }

// e_s of a sample: exp(-(score - m) / temperature) in fp64, exactly +0 where the sample is not valid (a select)
__device__ __forceinline__ double sample_e(const double score, const double m, const double temperature) {
  const double e = exp(-(score - m) / temperature);
  return sample_valid(score) ? e : 0.0;
}

// sum of v over the workgroup, to every lane: a tree over the lanes in LDS, the same order whatever the values
__device__ __forceinline__ double reduce_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int m = REDUCE_NT / 2; m > 0; m >>= 1) {
    if (tid < m) sh[tid] += sh[tid + m];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();                             // (sh may be written again)
  return r;
}

__global__ void __launch_bounds__(REDUCE_NT)
sample_reduce_kernel(const int h, const int S, const double temperature, const double* __restrict__ score,
                     const float* __restrict__ controls, const ReduceOut out) {
  __shared__ double sh[REDUCE_NT];
  __shared__ double sh_m[REDUCE_NT];
  __shared__ int sh_i[REDUCE_NT], sh_n[REDUCE_NT];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const double* sc = score + b * (size_t)S;
  double* w = out.weights + b * (size_t)S;

  // ---- n_valid; best: the smallest index among the valid samples of smallest score (exact, whatever the order)
  double m = 0.0;
  int best = -1, n = 0;
  for (int s = tid; s < S; s += REDUCE_NT) {
    const double v = sc[s];
    if (sample_valid(v)) {
      ++n;
      if (best < 0 || v < m) { m = v; best = s; }            // (s ascends: ties keep the lower index)
    }
  }
  sh_m[tid] = m; sh_i[tid] = best; sh_n[tid] = n;
  __syncthreads();
  for (int d = REDUCE_NT / 2; d > 0; d >>= 1) {
    if (tid < d) {
      const double om = sh_m[tid + d];
      const int oi = sh_i[tid + d];
      if (oi >= 0 && (sh_i[tid] < 0 || om < sh_m[tid] || (om == sh_m[tid] && oi < sh_i[tid]))) { sh_m[tid] = om; sh_i[tid] = oi; }
      sh_n[tid] += sh_n[tid + d];
    }
    __syncthreads();
  }
  m = sh_m[0]; best = sh_i[0]; n = sh_n[0];
  if (tid == 0) {
    if (out.best) out.best[b] = best;
    if (out.n_valid) out.n_valid[b] = n;
  }

  // ---- weights = e / sum e;  ess = 1 / sum weights^2.  No valid sample: sum e = 0, weights +0 (a select), ess NaN
  double part = 0.0;
  for (int s = tid; s < S; s += REDUCE_NT) part += sample_e(sc[s], m, temperature);
  const double total = reduce_sum(part, sh);
  part = 0.0;
  for (int s = tid; s < S; s += REDUCE_NT) {
    const double v = sc[s];
    const double ws = sample_valid(v) ? sample_e(v, m, temperature) / total : 0.0;
    w[s] = ws;
    part += ws * ws;
  }
  const double sq = reduce_sum(part, sh);      // (its barriers also put every lane's weights in front of the loads below)
  const double nan = __builtin_nan("");
  if (tid == 0 && out.ess) out.ess[b] = n > 0 ? 1.0 / sq : nan;

  // ---- u_mean = sum_s weights_s controls[b][s].  The lanes split into P = NT / (12 h) slices of 12 h lanes, a lane per element:
  // slice p takes the samples s = p, p + P, p + 2 P ... in four interleaved partial sums (so that loads are in flight), then
  // lane e of slice 0 adds the slices' sums in the order of p.  A sample without weight (invalid ones are: their controls may
  // be NaN) adds an exact zero (a select)
  if (!out.u_mean) return;
  const int E = h * 12;                        // (at most 480: every element has a lane)
  const int P = REDUCE_NT / E;
  const int p = tid / E, e = tid - p * E;
  const float* u = controls + b * (size_t)S * (size_t)E;
  if (p < P) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = p; s < S; s += 4 * P) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int sq = s + q * P;
        if (sq < S) {
          const double ws = w[sq];
          const double c = (double)u[(size_t)sq * (size_t)E + e];
          acc[q] += ws > 0.0 ? ws * c : 0.0;
        }
      }
    }
    sh[tid] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
  __syncthreads();
  if (p == 0) {
    double sum = sh[e];
    for (int q = 1; q < P; ++q) sum += sh[q * E + e];
    out.u_mean[b * (size_t)E + e] = n > 0 ? sum : nan;
  }
}

}  // namespace bmpc

#endif  // BMPC_EVALUATE_SAMPLES_HIP
