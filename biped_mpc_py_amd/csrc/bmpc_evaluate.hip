// bmpc_evaluate.hip -- evaluation of given control sequences (gfx950 / CDNA4): what the MPC's own model makes of a plan.
//
// Per instance, from the inputs of a solve (bmpc_inputs) and controls [h][12] (row k = [f1 f2 m1 m2], REF:302), all in fp64 on
// the fp32 inputs widened:
//   states     X(U) of the equality block REF:203-216: x_{k+1} = A_k x_k + B_k u_k, x_0 = [x_fb; 1], A_k / B_k of REF:148-185
//              linearised about x_ref[:, k], foot_ref[:, k] (supplied, or generated exactly as phase A of the solve does)
//   cost       sum_k (x_{k+1} - x_ref[:, k])' Q (x_{k+1} - x_ref[:, k]) + u_k' R u_k                     (REF:278-286 completed)
//   objective  1/2 z'Pz + q'z = cost - sum_k x_ref[:, k]' Q x_ref[:, k]   (row of ones included)         (REF:278-297)
//   violation  the largest positive part of Aqp z - bqp (REF:273-274) per row class: friction pyramid (REF:220-232), force
//              rows and moment rows of the box (REF:235-251), line foot (REF:254-271; body axes of eul2rotm(x_fb[0:3]), REF:193)
//
// Thread map: ONE lane per (instance, step).  An instance owns a group of L = 16 / 32 / 64 consecutive lanes of a wave (the power
// of two >= h), a wave holds 64 / L instances.  Everything about step k but the state recurrence is independent of the other
// steps -- the six sincos, Rot, I_w^-1, R_inv, the lever arms, B_k u_k, the control cost, every constraint row -- and A_k is the
// identity plus R_inv dt (euler <- omega), I dt (p <- v) and the gravity column, so the recurrence is two rounds of prefix sums
// over the group: first omega and v (increments B_k u_k and gravity), then euler and p (increments dt R_inv,k omega_k, dt v_k
// with the states BEFORE step k, taken from the lane below).  Prefix sums, the cost sums and the violation maxima go through
// lane_read (one wave-wide permute per value) in an order fixed by the lane's place in its GROUP: the result does not
// depend on the batch size or the instance's position.  No LDS, no barrier.  Lanes past the horizon (and past the batch) clone
// the last step (instance): same loads, same arithmetic, contributions masked, stores suppressed.
//
// An instance with a non-finite input, control or reference entry, or a reference pitch within fp32 rounding of +-90 degrees
// (|cos pitch| < 2^-22: the nearest fp32 to pi/2 is 4.4e-8 away from it, and R_inv, REF:160-164, is singular there), gets NaN in
// every output; the selects below keep its values out of every other group.
//
// Compiles as plain C++ for tests/emu (BMPC_EMU), where lane_read goes through a shared array between two wave barriers.
#ifndef BMPC_EVALUATE_HIP
#define BMPC_EVALUATE_HIP

#ifndef BMPC_EMU
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "bmpc.h"
#include "bmpc_model.hip"

namespace bmpc {

constexpr int EVAL_NT = 256;                   // lanes per workgroup (4 waves; no lane talks to another wave)
// lanes per instance at horizon h (one lane per step, rounded up to a power of two that divides the wave): THE rule for the
// kernels (eval_lane), the launch grid (bmpc_capi.hip) and the emulation's grid (tests/emu)
constexpr int eval_lanes(const int h) { return h <= 16 ? 16 : (h <= 32 ? 32 : 64); }
// samples per lane group of evaluate_samples_kernel (bmpc_evaluate_samples.hip), where a group owns one instance and a run of its
// samples: THE rule for the launch grid (bmpc_capi.hip), the kernel (handed in as `C`) and the emulation's grid.
// As many as SPG_MAX, so that the set-up is shared widely; halved while a group would own no sample in its upper half (small S),
// and, down to SPG_MIN, while the launch would have fewer than SPG_GROUPS groups: 8192 groups of 16 lanes are 2048 waves, two per
// SIMD on 256 CUs -- what the kernel's registers admit --, so a small B with a large S still fills the device.
constexpr int SPG_MAX = 32, SPG_MIN = 4;
constexpr long long SPG_GROUPS = 8192;
constexpr int eval_samples_per_group(const long long B, const long long S) {
  int C = SPG_MAX;
  while (C > 1 && (C / 2 >= S || (C > SPG_MIN && B * ((S + C - 1) / C) < SPG_GROUPS))) C /= 2;
  return C;
}

struct EvalParams {
  int h, half;
  double dt, kv, kvm, g, mu, lt, lh;           // kvm = dt / m;  lt, lh carry the REF:254-255 margins
  double x_cmd[12], Q[13], R[12], Iinv[9];
  double f_max[3], f_min[3], tau_max[3], tau_min[3];
};

struct EvalOut {             // all nullable, fp64, device pointers
  double* cost;              // [B]
  double* objective;         // [B]
  double* states;            // [B][h][13]
  double* violation;         // [B][4]: friction, force box, moment box, line foot
};

// The parameter block of the evaluation: the caller's bmpc_params as they are (fp64), Iinv = the inverse body inertia.
inline EvalParams eval_params(const bmpc_params& p, const double* Iinv) {
  EvalParams e;
  e.h = p.h; e.half = p.half;
  e.dt = p.dt; e.kv = p.kv; e.kvm = p.dt / p.m; e.g = p.g; e.mu = p.mu;
  e.lt = p.lt - 0.01;                          // REF:254
  e.lh = p.lh - 0.02;                          // REF:255
  for (int i = 0; i < 12; ++i) { e.x_cmd[i] = p.x_cmd[i]; e.R[i] = p.R[i]; }
  for (int i = 0; i < 13; ++i) e.Q[i] = p.Q[i];
  for (int i = 0; i < 9; ++i) e.Iinv[i] = Iinv[i];
  for (int i = 0; i < 3; ++i) {
    e.f_max[i] = p.f_max[i]; e.f_min[i] = p.f_min[i]; e.tau_max[i] = p.tau_max[i]; e.tau_min[i] = p.tau_min[i];
  }
  return e;
}

#ifndef BMPC_EMU
// value of lane `src` (0 .. 63) of the own wave: ds_bpermute_b32 per dword.  Call with all lanes of the wave active.
__device__ __forceinline__ double lane_read(double v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ int lane_read(int v, int src) { return __shfl(v, src, 64); }
#endif

// inclusive prefix sum over the lane's group of L lanes (gl = place in the group), N values at once: Hillis-Steele, shifts
// 1, 2, 4 ... L / 2.  A lane whose source would lie below its group adds an exact zero (a select: a neighbour group's NaN stays there).
template <int N>
__device__ __forceinline__ void group_prefix(double (&v)[N], const int lane, const int gl, const int L) {
  for (int sh = 1; sh < L; sh <<= 1) {
    const int src = (lane - sh) & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double o = lane_read(v[i], src);
      v[i] += gl >= sh ? o : 0.0;
    }
  }
}

// sum / maximum over the group, to every lane of it: butterfly over lane ^ 1, 2, 4 ... L / 2 (a + b is b + a: every lane of the
// group ends with the same bits)
template <int N>
__device__ __forceinline__ void group_sum(double (&v)[N], const int lane, const int L) {
  for (int m = 1; m < L; m <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += lane_read(v[i], lane ^ m);
  }
}
template <int N>
__device__ __forceinline__ void group_max(double (&v)[N], const int lane, const int L) {
  for (int m = 1; m < L; m <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = fmax(v[i], lane_read(v[i], lane ^ m));
  }
}
__device__ __forceinline__ int group_or(int v, const int lane, const int L) {
  for (int m = 1; m < L; m <<= 1) v |= lane_read(v, lane ^ m);
  return v;
}

// ---- the set-up of one (instance, step), shared by evaluate_kernel and evaluate_grad_kernel (bmpc_evaluate_grad.hip): the same
// expressions in the same order for both, so that what the two kernels have in common (states, cost, the NaN rule) is the same bits

struct EvalLane {            // where a lane stands: its group of L lanes = its instance, its place in the group = its step
  int L, lane, gl, k;
  bool in_batch, live;
  size_t inst, row;
};

__device__ __forceinline__ EvalLane eval_lane(const int h, const int B) {
  EvalLane t;
  t.L = eval_lanes(h);
  t.lane = threadIdx.x & 63;
  t.gl = t.lane & (t.L - 1);                   // place in the group = step
  const long long grp = ((long long)blockIdx.x * EVAL_NT + threadIdx.x) / t.L;
  t.in_batch = grp < (long long)B;
  t.inst = (size_t)(t.in_batch ? grp : (long long)B - 1);
  t.live = t.gl < h;
  t.k = t.live ? t.gl : h - 1;
  t.row = t.inst * (size_t)h + (size_t)t.k;
  return t;
}

struct EvalStep {            // what a lane holds of its (instance, step), fp64
  double xfb[12], u[12], xr[12], fr[6], mu[2];
  double Rv[9], Iw[9], r[2][3];                // R_inv (REF:160-164 inverted), (Rot' I Rot)^-1, lever arms foot_ref_g - x_ref[3:6]
  bool singular;                               // reference pitch within fp32 rounding of +-90 degrees
};

// inputs of this (instance, step), widened; x_ref[:, k] / foot_ref[:, k] supplied, or generated as phase A of the solve forms them
__device__ __forceinline__ void eval_load(const EvalParams& P, const EvalLane& t,
                                          const float* __restrict__ x_fb, const float* __restrict__ foot,
                                          const uint8_t* __restrict__ contact, const int32_t* __restrict__ phase,
                                          const float* __restrict__ x_cmd, const float* __restrict__ mu_in,
                                          const float* __restrict__ x_ref, const float* __restrict__ foot_ref,
                                          const float* __restrict__ controls, EvalStep& s) {
  const int h = P.h, k = t.k;
  const size_t inst = t.inst, row = t.row;
  const double dt = P.dt;
  double xc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    s.xfb[i] = (double)x_fb[inst * 12 + i];
    xc[i] = x_cmd ? (double)x_cmd[inst * 12 + i] : P.x_cmd[i];
    s.u[i] = (double)controls[row * 12 + i];
  }
  if (x_ref) {                                 // x_ref[:, k]: supplied, or REF:61-70 as phase A of the solve forms it
#pragma unroll
    for (int i = 0; i < 12; ++i) s.xr[i] = (double)x_ref[row * 12 + i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      if (k == 0) s.xr[i] = s.xfb[i];
      else if (i < 6) s.xr[i] = (xc[i + 6] != 0.0) ? s.xfb[i] + xc[i + 6] * ((double)k * dt) : xc[i];
      else s.xr[i] = xc[i];
    }
  }
  if (foot_ref) {                              // foot_ref[:, k]: supplied, or REF:72-109 likewise
#pragma unroll
    for (int i = 0; i < 6; ++i) s.fr[i] = (double)foot_ref[row * 6 + i];
  } else {
    const int c0 = contact[inst * (size_t)h * 2 + 0], c1 = contact[inst * (size_t)h * 2 + 1];
    const bool single = (c0 + c1) == 1;        // REF:102
    const int kk = phase[inst] % P.half;       // REF:101
#pragma unroll
    for (int i = 0; i < 6; ++i) s.fr[i] = (double)foot[inst * 6 + i];
    if (single && k >= P.half - kk) {
      const bool second = k >= 2 * P.half - kk;
      const double hor = second ? 0.5 * (double)h * dt : 0.5 * (double)h / 2.0 * dt;                    // REF:74, 78
      const double fx = s.xfb[3] + s.xfb[9] * hor + P.kv * (s.xfb[3] - xc[3]);
      const double fy = (second ? s.xfb[10] : s.xfb[4]) + s.xfb[10] * hor + P.kv * (s.xfb[4] - xc[4]);  // REF:87 quirk
      s.fr[0] = fx; s.fr[1] = fy; s.fr[2] = 0; s.fr[3] = fx; s.fr[4] = fy; s.fr[5] = 0;
    }
  }
  s.mu[0] = mu_in ? (double)mu_in[row * 2 + 0] : P.mu;
  s.mu[1] = mu_in ? (double)mu_in[row * 2 + 1] : P.mu;
}

// SRBM step data (REF:148-185) and this step's increments of omega and v: B_k u_k and the gravity column of A_k
__device__ __forceinline__ void eval_step_model(const EvalParams& P, EvalStep& s, double (&inc)[6]) {
  const double dt = P.dt;
  const double* xr = s.xr;
  const double* u = s.u;
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
  // net torque about the CoM: r_1 x f_1 + r_2 x f_2 + m_1 + m_2, r_g = foot_ref_g - x_ref[3:6]  (REF:174-179)
  double tau[3] = {u[6] + u[9], u[7] + u[10], u[8] + u[11]};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double r[3] = {s.fr[3 * g] - xr[3], s.fr[3 * g + 1] - xr[4], s.fr[3 * g + 2] - xr[5]};
    const double* f = &u[3 * g];
    tau[0] += r[1] * f[2] - r[2] * f[1];
    tau[1] += r[2] * f[0] - r[0] * f[2];
    tau[2] += r[0] * f[1] - r[1] * f[0];
    s.r[g][0] = r[0]; s.r[g][1] = r[1]; s.r[g][2] = r[2];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    inc[a] = dt * (s.Iw[3 * a] * tau[0] + s.Iw[3 * a + 1] * tau[1] + s.Iw[3 * a + 2] * tau[2]);
    inc[3 + a] = P.kvm * (u[a] + u[3 + a]);                                              // REF:180
  }
  inc[5] -= P.g * dt;                                                                    // REF:169
}

// the recurrence: omega, v after step k from the increments `inc`; then euler, p from the states before step k.  x = state after step k
__device__ __forceinline__ void eval_recurrence(const EvalParams& P, const EvalLane& t, const EvalStep& s, double (&inc)[6],
                                                double (&x)[12]) {
  const double dt = P.dt;
  group_prefix<6>(inc, t.lane, t.gl, t.L);
#pragma unroll
  for (int a = 0; a < 6; ++a) x[6 + a] = s.xfb[6 + a] + inc[a];
  {
    double before[6];                          // omega_k, v_k: the lane below's result, x_fb at step 0
    const int src = (t.lane - 1) & 63;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double o = lane_read(x[6 + a], src);
      before[a] = t.gl > 0 ? o : s.xfb[6 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      inc[a] = dt * (s.Rv[3 * a] * before[0] + s.Rv[3 * a + 1] * before[1] + s.Rv[3 * a + 2] * before[2]);   // REF:166
      inc[3 + a] = dt * before[3 + a];                                                                       // REF:167
    }
  }
  group_prefix<6>(inc, t.lane, t.gl, t.L);
#pragma unroll
  for (int a = 0; a < 6; ++a) x[a] = s.xfb[a] + inc[a];
}

// is everything the lanes of this group saw finite, and no reference pitch singular?  (a sum of magnitudes: NaN and Inf both fail
// the comparison).  Non-zero on every lane of a group that holds a bad live lane.
__device__ __forceinline__ int eval_bad(const EvalLane& t, const EvalStep& s, const double (&x)[12]) {
  double mag = fabs(s.mu[0]) + fabs(s.mu[1]);
#pragma unroll
  for (int i = 0; i < 12; ++i) mag += fabs(s.u[i]) + fabs(s.xr[i]) + fabs(x[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) mag += fabs(s.fr[i]);
#pragma unroll
  for (int q = 0; q < 9; ++q) mag += fabs(s.Rv[q]);
  return group_or((t.live && (s.singular || !(mag <= 1.7976931348623157e308))) ? 1 : 0, t.lane, t.L);
}

// cost of this step (REF:278-286 completed): sum_i Q_i (x_i - x_ref_i)^2 + R_i u_i^2, added to `acc`
__device__ __forceinline__ void eval_step_cost(const EvalParams& P, const EvalStep& s, const double (&x)[12], double& acc) {
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double e = x[i] - s.xr[i];
    acc += P.Q[i] * e * e + P.R[i] * s.u[i] * s.u[i];
  }
}

// rows of Aqp z <= bqp of this step (REF:273-274): the largest positive part per class -- friction, force box, moment box, line foot
__device__ __forceinline__ void eval_step_violation(const EvalParams& P, const EvalStep& s, const double (&con)[2], double (&viol)[4]) {
  const double* xfb = s.xfb;
  const double* u = s.u;
  const double* mu = s.mu;
  viol[0] = 0.0; viol[1] = 0.0; viol[2] = 0.0; viol[3] = 0.0;
  // body axes of the line-foot rows: columns y and z of R = eul2rotm(x_fb[0:3]) = Rz(e2) Ry(e1) Rx(e0)  (REF:124-138, 193, 259-262)
  double s0, c0, s1, c1, s2, c2, ey[3], ez[3];
  sincos(xfb[0], &s0, &c0);
  sincos(xfb[1], &s1, &c1);
  sincos(xfb[2], &s2, &c2);
  body_axes(s0, c0, s1, c1, s2, c2, ey, ez);
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

__global__ void __launch_bounds__(EVAL_NT)
evaluate_kernel(const EvalParams P, const int B,
                const float* __restrict__ x_fb, const float* __restrict__ foot,
                const uint8_t* __restrict__ contact, const int32_t* __restrict__ phase,
                const float* __restrict__ x_cmd, const float* __restrict__ mu_in,
                const float* __restrict__ x_ref, const float* __restrict__ foot_ref,
                const float* __restrict__ controls, const EvalOut out) {
  const EvalLane t = eval_lane(P.h, B);
  const int L = t.L, lane = t.lane, gl = t.gl;
  const bool in_batch = t.in_batch, live = t.live;
  const size_t inst = t.inst, row = t.row;

  EvalStep s;
  eval_load(P, t, x_fb, foot, contact, phase, x_cmd, mu_in, x_ref, foot_ref, controls, s);
  const double con[2] = {(double)contact[row * 2 + 0], (double)contact[row * 2 + 1]};
  double inc[6], x[12];                        // x = state after step k
  eval_step_model(P, s, inc);
  eval_recurrence(P, t, s, inc, x);
  const int bad = eval_bad(t, s, x);
  const double* xr = s.xr;

  // ---- cost of this step; the constant between cost and objective
  double sums[2] = {0.0, P.Q[12]};             // (the 13th state is 1 and so is its reference: no cost, Q[12] in the constant)
  eval_step_cost(P, s, x, sums[0]);
#pragma unroll
  for (int i = 0; i < 12; ++i) sums[1] += P.Q[i] * xr[i] * xr[i];
  if (!live) { sums[0] = 0.0; sums[1] = 0.0; }
  group_sum<2>(sums, lane, L);

  // ---- rows of Aqp z <= bqp of this step: the largest positive part per class
  double viol[4];
  eval_step_violation(P, s, con, viol);
  if (!live) { viol[0] = 0.0; viol[1] = 0.0; viol[2] = 0.0; viol[3] = 0.0; }
  group_max<4>(viol, lane, L);

  // ---- stores
  if (!in_batch) return;
  const double nan = __builtin_nan("");
  if (out.states && live) {
    double* so = out.states + row * 13;
#pragma unroll
    for (int i = 0; i < 12; ++i) so[i] = bad ? nan : x[i];
    so[12] = bad ? nan : 1.0;
  }
  if (gl == 0) {
    if (out.cost) out.cost[inst] = bad ? nan : sums[0];
    if (out.objective) out.objective[inst] = bad ? nan : sums[0] - sums[1];
    if (out.violation) {
#pragma unroll
      for (int c = 0; c < 4; ++c) out.violation[inst * 4 + c] = bad ? nan : viol[c];
    }
  }
}

}  // namespace bmpc

#endif  // BMPC_EVALUATE_HIP
