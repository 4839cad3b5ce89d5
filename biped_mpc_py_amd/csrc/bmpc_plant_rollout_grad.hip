// bmpc_plant_rollout_grad.hip -- the gradient of the plant roll-out (gfx950 / CDNA4): d cost / d (controls, x_fb, foot) of every
// plan of bmpc_plant_rollout.hip's roll-out, by the discrete adjoint of the chain the forward pass runs.  include/bmpc.h states
// what is differentiated and what is held fixed.
//
// plant_rollout_grad_kernel.  One thread per (instance b, plan s), flat index b S + s; 256 threads per workgroup; fp64 arithmetic
// on fp32 I/O.  The thread runs the forward pass first -- rollout_sample's periods, statement for statement: ground, push, plant_step,
// the state rounded to fp32 and stored, cost, landing -- and records the stored state of every period (in x_traj where the caller
// wants it, else in the handle's scratch) and the footholds every period started with (scratch, plan-minor).  Then the adjoint,
// period by period backwards, with lam the costate of the stored state and mu the costate of the footholds (6 values):
//   lam   += 2 Q (x_k - xr_k)
//   fold     a leg that lands after period k took foothold_target at x_k: mu of that leg goes into lam[3], lam[9] (x) and lam[4],
//            lam[10] (y) through the target's coefficients 1 + kv and h dt / 4, and is zeroed (with move_feet only)
//   step     plant_step_vjp: lam <- (dPhi/dx)' lam, and the costates of the applied control (12) and of the footholds (6, added to mu)
//   ground   plant_ground_vjp on the branch the forward call took; grad_u[k] = that + 2 R u, and exactly 2.0 * R_i * (double)u for
//            the six values of a leg the plant never sees (swing; with a ground, unloaded)
// What is left at k = 0 is grad_x0 = lam and grad_foot = mu.  The fp32 rounding of a stored state and of a scaled tangential force
// is the identity in the derivative; the linearisation point is the stored (rounded) values.  Held fixed: the reference rows, the
// commands, the body, mu, the push, the contact table.
//
// Re-materialisation, O(substeps) work per period: before a period's backward sweep its forward re-run writes every substep's
// start (e, w) to per-plan scratch (6 doubles per substep, plan-minor: a wave's accesses are consecutive); p and v at a substep
// are closed-form from the period's start.  Per substep the stage rates are re-formed forwards by plant_rate, as plant_step forms
// them, and the first three are kept in a per-lane LDS slab (18 doubles a lane, 36 KiB a workgroup) that only its own lane reads --
// no barrier, as in bmpc_certify.hip -- so that the rolled stage loops index no private array dynamically; then plant_rate_vjp
// transposes the stages in reverse order.  Euler is the one-stage case of the same code.
//
// A bad plan (bmpc_plant_rollout.hip's rules) has cost and every gradient entry NaN and first_bad at the period from which its
// state is NaN; no other plan is touched.
//
// Resources as built (gfx950, -O3): 428 registers of the unified file (256 VGPRs + 172 AGPRs), private segment 0, no vector
// spill, 36864 bytes of LDS, about 6400 instructions: one wave per SIMD, which is all the launch bound asks for -- the forward pass
// alone holds 253 registers in plant_rollout_samples_kernel, and the adjoint keeps the costates, the held costates and the body next
// to a stage's values.
//
// The functions compile as plain C++ for tests/emu (BMPC_EMU) like the ones they call; the slab is then an array of the caller's.
#ifndef BMPC_PLANT_ROLLOUT_GRAD_HIP
#define BMPC_PLANT_ROLLOUT_GRAD_HIP

#include "bmpc_plant_rollout.hip"

namespace bmpc {

constexpr int RGRAD_NT = 256;                  // threads per workgroup
constexpr int RGRAD_SLAB = 18;                 // doubles per lane: the rates (de, dw) of stages 0, 1, 2

// the outputs, device pointers, each null where not wanted: per plan (index b S + s)
struct RolloutGradOut {
  double *cost, *grad_u, *grad_x0, *grad_foot;   // [B][S], [B][S][h][12], [B][S][12], [B][S][6]
  float* x_traj;                                 // [B][S][h][12]
  int32_t* first_bad;                            // [B][S]
};

// the scratch of a launch of `plans` plans: x_rec [plans][h][12] (null where out.x_traj takes its place), foot_rec [h][6][plans],
// sub [substeps][6][plans]
struct RolloutGradScratch {
  float *x_rec, *foot_rec;
  double* sub;
  size_t plans;
};

// A lane's slab: element i at p[i * stride] (LDS: stride = the workgroup's threads, so that a wave's accesses of one element are
// consecutive; plain C++: 1).
struct LaneSlab { double* p; int stride; };

// c_j, b_j and c_{j-1} of plant_step's stage loop
__device__ __forceinline__ void plant_stage_coeffs(const PlantScheme& S, const int j, double& cj, double& bj, double& cprev) {
  cj = j == 0 ? 0.0 : (j == 3 ? S.hs : S.hh);
  bj = (j == 1 || j == 2) ? 2.0 : 1.0;
  cprev = j >= 2 ? S.hh : 0.0;
}

// p and v at the start of substep s, closed-form from the period's start p0, v0: v += hs a and p += hs v + half2 a, s times.
__device__ __forceinline__ void plant_substep_pv(const PlantScheme& S, const PlantHeld& H, const double (&p0)[3], const double (&v0)[3],
                                                 const int s, double (&p)[3], double (&v)[3]) {
  const double n = (double)s, ts = n * S.hs, qa = S.hs * S.hs * (0.5 * n * (n - 1.0)) + n * S.half2;
#pragma unroll
  for (int i = 0; i < 3; ++i) { v[i] = v0[i] + ts * H.a[i]; p[i] = p0[i] + ts * v0[i] + qa * H.a[i]; }
}

// One substep forwards from (e, w) at position p, velocity v, as plant_step takes it: the stage rates by plant_rate; those of
// stages 0 .. 2 go to the slab where one is given (L.p).  (e, w) become the substep's end.
__device__ __forceinline__ void plant_substep_rates(const PlantParams& P, const PlantScheme& S, const PlantHeld& H, double (&e)[3],
                                                    double (&om)[3], const double (&p)[3], const double (&v)[3], const LaneSlab& L) {
  double ke[3] = {0.0, 0.0, 0.0}, kw[3] = {0.0, 0.0, 0.0}, ae[3] = {0.0, 0.0, 0.0}, aw[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int j = 0; j < S.stages; ++j) {
    double cj, bj, cprev;
    plant_stage_coeffs(S, j, cj, bj, cprev);
    const double es[3] = {e[0] + cj * ke[0], e[1] + cj * ke[1], e[2] + cj * ke[2]};
    plant_rate(P, H, es, p, v, cprev, om, cj, kw, ke, kw);
#pragma unroll
    for (int i = 0; i < 3; ++i) { ae[i] += bj * ke[i]; aw[i] += bj * kw[i]; }
    if (L.p && j < 3) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { L.p[(j * 6 + i) * L.stride] = ke[i]; L.p[(j * 6 + 3 + i) * L.stride] = kw[i]; }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) { e[i] += S.wsum * ae[i]; om[i] += S.wsum * aw[i]; }
}

// The transpose of plant_rate at the stage state (es, w, ps): the costates (gde, gdw) of its rates to the costates ges, gw, gps
// of the stage state (written) and gFc, gT0 of the held force and torque (added to).  The sincos and the plane rotations are
// recomputed here, through the one rolled sincos body of plant_rate.
__device__ __forceinline__ void plant_rate_vjp(const PlantParams& P, const PlantHeld& H, const double (&es)[3], const double (&w)[3],
                                               const double (&ps)[3], const double (&gde)[3], const double (&gdw)[3], double (&ges)[3],
                                               double (&gw)[3], double (&gps)[3], double (&gFc)[3], double (&gT0)[3]) {
  double s0 = es[0], k0 = 0.0, s1 = es[1], k1 = 0.0, s2 = es[2], k2 = 0.0;
#pragma unroll 1
  for (int q = 0; q < 3; ++q) {
    double sn, cs;
    sincos(s0, &sn, &cs);
    s0 = s1; k0 = k1; s1 = s2; k1 = k2; s2 = sn; k2 = cs;
  }
  // forwards, as plant_rate
  const double wz0 = k2 * w[0] + s2 * w[1], wz1 = -s2 * w[0] + k2 * w[1];
  const double e0d = wz0 / k1;
  const double tau[3] = {H.T0[0] - (ps[1] * H.Fc[2] - ps[2] * H.Fc[1]), H.T0[1] - (ps[2] * H.Fc[0] - ps[0] * H.Fc[2]),
                         H.T0[2] - (ps[0] * H.Fc[1] - ps[1] * H.Fc[0])};
  const double wy0 = k1 * wz0 - s1 * w[2], wy2 = s1 * wz0 + k1 * w[2];
  const double wb[3] = {wy0, k0 * wz1 + s0 * wy2, -s0 * wz1 + k0 * wy2};
  const double tz0 = k2 * tau[0] + s2 * tau[1], tz1 = -s2 * tau[0] + k2 * tau[1];
  const double ty0 = k1 * tz0 - s1 * tau[2], ty2 = s1 * tz0 + k1 * tau[2];
  const double tb[3] = {ty0, k0 * tz1 + s0 * ty2, -s0 * tz1 + k0 * ty2};
  double Lb[3], ab[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Lb[i] = P.Ib[3 * i] * wb[0] + P.Ib[3 * i + 1] * wb[1] + P.Ib[3 * i + 2] * wb[2];
  const double y[3] = {tb[0] - (wb[1] * Lb[2] - wb[2] * Lb[1]), tb[1] - (wb[2] * Lb[0] - wb[0] * Lb[2]), tb[2] - (wb[0] * Lb[1] - wb[1] * Lb[0])};
#pragma unroll
  for (int i = 0; i < 3; ++i) ab[i] = P.Ibinv[3 * i] * y[0] + P.Ibinv[3 * i + 1] * y[1] + P.Ibinv[3 * i + 2] * y[2];
  const double ax1 = k0 * ab[1] - s0 * ab[2], ax2 = s0 * ab[1] + k0 * ab[2];
  const double ay0 = k1 * ab[0] + s1 * ax2;
  // backwards; gs_, gk_: the costates of the sines and cosines
  // dw = Rz (ay0, ax1, ay2)
  const double g_ay0 = k2 * gdw[0] + s2 * gdw[1], g_ax1 = -s2 * gdw[0] + k2 * gdw[1], g_ay2 = gdw[2];
  double gk2 = ay0 * gdw[0] + ax1 * gdw[1], gs2 = -ax1 * gdw[0] + ay0 * gdw[1];
  // (ay0, ay2) = Ry (ab0, ax2)
  const double g_ab0 = k1 * g_ay0 - s1 * g_ay2, g_ax2 = s1 * g_ay0 + k1 * g_ay2;
  double gk1 = ab[0] * g_ay0 + ax2 * g_ay2, gs1 = ax2 * g_ay0 - ab[0] * g_ay2;
  // (ax1, ax2) = Rx (ab1, ab2)
  const double g_ab[3] = {g_ab0, k0 * g_ax1 + s0 * g_ax2, -s0 * g_ax1 + k0 * g_ax2};
  double gk0 = ab[1] * g_ax1 + ab[2] * g_ax2, gs0 = -ab[2] * g_ax1 + ab[1] * g_ax2;
  // ab = I_b^-1 y;  y = tb - wb x Lb;  Lb = I_b wb
  double gy[3], g_wb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gy[i] = P.Ibinv[i] * g_ab[0] + P.Ibinv[3 + i] * g_ab[1] + P.Ibinv[6 + i] * g_ab[2];
  const double g_Lb[3] = {wb[1] * gy[2] - wb[2] * gy[1], wb[2] * gy[0] - wb[0] * gy[2], wb[0] * gy[1] - wb[1] * gy[0]};
  g_wb[0] = gy[1] * Lb[2] - gy[2] * Lb[1]; g_wb[1] = gy[2] * Lb[0] - gy[0] * Lb[2]; g_wb[2] = gy[0] * Lb[1] - gy[1] * Lb[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) g_wb[i] += P.Ib[i] * g_Lb[0] + P.Ib[3 + i] * g_Lb[1] + P.Ib[6 + i] * g_Lb[2];
  // tb = Rx' Ry' Rz' tau
  const double g_ty0 = gy[0], g_tz1 = k0 * gy[1] - s0 * gy[2], g_ty2 = s0 * gy[1] + k0 * gy[2];
  gk0 += tz1 * gy[1] + ty2 * gy[2]; gs0 += ty2 * gy[1] - tz1 * gy[2];
  const double g_tz0 = k1 * g_ty0 + s1 * g_ty2, g_tau2 = -s1 * g_ty0 + k1 * g_ty2;
  gk1 += tz0 * g_ty0 + tau[2] * g_ty2; gs1 += -tau[2] * g_ty0 + tz0 * g_ty2;
  const double g_tau[3] = {k2 * g_tz0 - s2 * g_tz1, s2 * g_tz0 + k2 * g_tz1, g_tau2};
  gk2 += tau[0] * g_tz0 + tau[1] * g_tz1; gs2 += tau[1] * g_tz0 - tau[0] * g_tz1;
  // wb = Rx' Ry' Rz' w
  const double g_wy0 = g_wb[0], g_wy2 = s0 * g_wb[1] + k0 * g_wb[2];
  double g_wz1 = k0 * g_wb[1] - s0 * g_wb[2];
  gk0 += wz1 * g_wb[1] + wy2 * g_wb[2]; gs0 += wy2 * g_wb[1] - wz1 * g_wb[2];
  double g_wz0 = k1 * g_wy0 + s1 * g_wy2, g_w2 = -s1 * g_wy0 + k1 * g_wy2;
  gk1 += wz0 * g_wy0 + w[2] * g_wy2; gs1 += -w[2] * g_wy0 + wz0 * g_wy2;
  // de = (e0d, wz1, w2 + s1 e0d), e0d = wz0 / k1
  const double g_e0d = gde[0] + s1 * gde[2];
  g_wz1 += gde[1]; g_w2 += gde[2]; gs1 += e0d * gde[2];
  g_wz0 += g_e0d / k1; gk1 -= e0d / k1 * g_e0d;
  // (wz0, wz1) = Rz' (w0, w1)
  gw[0] = k2 * g_wz0 - s2 * g_wz1; gw[1] = s2 * g_wz0 + k2 * g_wz1; gw[2] = g_w2;
  gk2 += w[0] * g_wz0 + w[1] * g_wz1; gs2 += w[1] * g_wz0 - w[0] * g_wz1;
  // tau = T0 - ps x Fc
  gps[0] = g_tau[1] * H.Fc[2] - g_tau[2] * H.Fc[1]; gps[1] = g_tau[2] * H.Fc[0] - g_tau[0] * H.Fc[2]; gps[2] = g_tau[0] * H.Fc[1] - g_tau[1] * H.Fc[0];
  gFc[0] += ps[1] * g_tau[2] - ps[2] * g_tau[1]; gFc[1] += ps[2] * g_tau[0] - ps[0] * g_tau[2]; gFc[2] += ps[0] * g_tau[1] - ps[1] * g_tau[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) gT0[i] += g_tau[i];
  ges[0] = gs0 * k0 - gk0 * s0; ges[1] = gs1 * k1 - gk1 * s1; ges[2] = gs2 * k2 - gk2 * s2;
}

// One control period backwards: lam, the costate of plant_step's next state, becomes the costate of its state x; gua (12) and gr
// (6) get the costates of the applied control and of the footholds.  sub: the plan's substep scratch, element q at
// sub[q * sub_stride]; L: the lane's slab.  First the period's forward re-run writes every substep's start (e, w) to sub; then,
// substep by substep backwards, the stage rates are re-formed (plant_substep_rates) and transposed in reverse stage order.  The
// costates of the held (Fc, T0, a) accumulate over the period and go through plant_held's transpose once.
__device__ __forceinline__ void plant_step_vjp(const PlantParams& P, const PlantScheme& S, const float (&x)[12], const float (&ua)[12],
                                               const float (&r)[6], const double c0, const double c1, const float (&w)[6],
                                               double* sub, const size_t sub_stride, const LaneSlab& L, double (&lam)[12],
                                               double (&gua)[12], double (&gr)[6]) {
  const PlantHeld H = plant_held(P, ua, r, c0, c1, w);
  double p0[3], v0[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { p0[i] = (double)x[3 + i]; v0[i] = (double)x[9 + i]; }
  {
    double e[3], om[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { e[i] = (double)x[i]; om[i] = (double)x[6 + i]; }
    const LaneSlab none = {nullptr, 0};
#pragma unroll 1
    for (int s = 0; s < S.substeps; ++s) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { sub[(size_t)(s * 6 + i) * sub_stride] = e[i]; sub[(size_t)(s * 6 + 3 + i) * sub_stride] = om[i]; }
      if (s + 1 < S.substeps) {
        double p[3], v[3];
        plant_substep_pv(S, H, p0, v0, s, p, v);
        plant_substep_rates(P, S, H, e, om, p, v, none);
      }
    }
  }
  double le[3], lp[3], lo[3], lv[3], gFc[3] = {0.0, 0.0, 0.0}, gT0[3] = {0.0, 0.0, 0.0}, ga[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) { le[i] = lam[i]; lp[i] = lam[3 + i]; lo[i] = lam[6 + i]; lv[i] = lam[9 + i]; }
#pragma unroll 1
  for (int s = S.substeps - 1; s >= 0; --s) {
    double e[3], om[3], p[3], v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { e[i] = sub[(size_t)(s * 6 + i) * sub_stride]; om[i] = sub[(size_t)(s * 6 + 3 + i) * sub_stride]; }
    plant_substep_pv(S, H, p0, v0, s, p, v);
    {
      double ee[3] = {e[0], e[1], e[2]}, oo[3] = {om[0], om[1], om[2]};
      plant_substep_rates(P, S, H, ee, oo, p, v, L);
    }
    // the closed-form updates of p and v: p' = p + hs v + half2 a, v' = v + hs a
    double ne[3], no[3], np_[3], nv[3], cke[3] = {0.0, 0.0, 0.0}, ckw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ne[i] = le[i]; no[i] = lo[i]; np_[i] = lp[i]; nv[i] = lv[i] + S.hs * lp[i];
      ga[i] += S.half2 * lp[i] + S.hs * lv[i];
    }
#pragma unroll 1
    for (int j = S.stages - 1; j >= 0; --j) {
      double cj, bj, cprev;
      plant_stage_coeffs(S, j, cj, bj, cprev);
      double es[3], ws[3], ps[3], gde[3], gdw[3], ges[3], gw[3], gps[3];
      const int jp = j > 0 ? j - 1 : 0;            // (stage 0 starts from the substep's state: c_0 = 0)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        es[i] = e[i] + cj * L.p[(jp * 6 + i) * L.stride];
        ws[i] = om[i] + cj * L.p[(jp * 6 + 3 + i) * L.stride];
        ps[i] = p[i] + cj * (v[i] + cprev * H.a[i]);
        gde[i] = S.wsum * bj * le[i] + cke[i];
        gdw[i] = S.wsum * bj * lo[i] + ckw[i];
      }
      plant_rate_vjp(P, H, es, ws, ps, gde, gdw, ges, gw, gps, gFc, gT0);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        ne[i] += ges[i]; no[i] += gw[i]; np_[i] += gps[i]; nv[i] += cj * gps[i];
        ga[i] += cj * cprev * gps[i];
        cke[i] = cj * ges[i]; ckw[i] = cj * gw[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { le[i] = ne[i]; lo[i] = no[i]; lp[i] = np_[i]; lv[i] = nv[i]; }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) { lam[i] = le[i]; lam[3 + i] = lp[i]; lam[6 + i] = lo[i]; lam[9 + i] = lv[i]; }
  // plant_held's transpose: a = (Fc + F) / m - g e_z;  Fc = sum_g c_g f_g;  T0 = sum_g c_g (r_g x f_g + m_g) + M
#pragma unroll
  for (int i = 0; i < 3; ++i) gFc[i] += ga[i] / P.m;
  const double c[2] = {c0, c1};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double f[3] = {(double)ua[3 * g], (double)ua[3 * g + 1], (double)ua[3 * g + 2]};
    const double a[3] = {(double)r[3 * g], (double)r[3 * g + 1], (double)r[3 * g + 2]};
    gua[3 * g] = c[g] * (gFc[0] + (gT0[1] * a[2] - gT0[2] * a[1]));
    gua[3 * g + 1] = c[g] * (gFc[1] + (gT0[2] * a[0] - gT0[0] * a[2]));
    gua[3 * g + 2] = c[g] * (gFc[2] + (gT0[0] * a[1] - gT0[1] * a[0]));
    gr[3 * g] = c[g] * (f[1] * gT0[2] - f[2] * gT0[1]);
    gr[3 * g + 1] = c[g] * (f[2] * gT0[0] - f[0] * gT0[2]);
    gr[3 * g + 2] = c[g] * (f[0] * gT0[1] - f[1] * gT0[0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) gua[6 + 3 * g + i] = c[g] * gT0[i];
  }
}

// The transpose of plant_ground on the branch its forward call took (flags): the costate gua of the applied control to the
// costate gu of the command.  seen[g]: whether leg g's six values reach the plant at all (a swing leg's and an unloaded stance
// leg's do not: their block is zero).  A loaded leg inside the cone passes its costate on; a slipping leg has the Jacobian of
// (fx, fy) mu fz / sqrt(fx^2 + fy^2) with respect to (fx, fy, fz); moments pass.
__device__ __forceinline__ void plant_ground_vjp(const float (&u)[12], const uint8_t flags, const bool c0, const bool c1, const double mu0,
                                                 const double mu1, const double (&gua)[12], double (&gu)[12], bool (&seen)[2]) {
  const bool c[2] = {c0, c1};
  const double mu[2] = {mu0, mu1};
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    seen[g] = c[g] && !((flags >> (2 + g)) & 1);
    double gx = gua[3 * g], gy = gua[3 * g + 1], gz = gua[3 * g + 2];
    if ((flags >> g) & 1) {
      const double fx = (double)u[3 * g], fy = (double)u[3 * g + 1], fz = (double)u[3 * g + 2];
      const double t2 = fx * fx + fy * fy, t = sqrt(t2), sc = mu[g] * fz / t, q = sc / t2, d = fy * gx - fx * gy;
      gz += mu[g] / t * (fx * gx + fy * gy);
      gx = q * fy * d; gy = -(q * fx * d);
    }
    gu[3 * g] = seen[g] ? gx : 0.0; gu[3 * g + 1] = seen[g] ? gy : 0.0; gu[3 * g + 2] = seen[g] ? gz : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) gu[6 + 3 * g + i] = seen[g] ? gua[6 + 3 * g + i] : 0.0;
  }
}

// Plan `plan` = b S + s of instance b: the forward pass, then the adjoint.
__device__ __forceinline__ void rollout_grad_plan(const PlantParams& P, const PlantScheme& Sc, const RolloutCost& C, const RolloutIn& in,
                                                  const RolloutGradOut& out, const RolloutGradScratch& W, const LaneSlab& L,
                                                  const size_t b, const size_t plan) {
  const int h = (int)P.h;
  float x[12], r[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = in.x_fb[b * 12 + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) r[i] = in.foot[b * 6 + i];
  PlantParams Pb;
  const bool body_ok = plant_body(P, in.m ? in.m + b : nullptr, in.I ? in.I + b * 9 : nullptr, in.g ? in.g + b : nullptr, Pb);
  const double mu0 = in.mu ? in.mu[b * 2] : in.mu_h, mu1 = in.mu ? in.mu[b * 2 + 1] : in.mu_h;
  float x0[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x0[i] = x[i];
  const uint8_t* con = in.contact + b * (size_t)h * 2;
  const float* up = in.controls + plan * (size_t)h * 12;
  float* xrec = (out.x_traj ? out.x_traj : W.x_rec) + plan * (size_t)h * 12;
  float* frec = W.foot_rec + plan;
  const double cx = in.x_cmd ? (double)in.x_cmd[b * 12 + 3] : P.cmd_x, cy = in.x_cmd ? (double)in.x_cmd[b * 12 + 4] : P.cmd_y;

  // ---- forwards: rollout_sample's periods
  double cost = 0.0;
  int32_t first_bad = -1;
#pragma unroll 1
  for (int k = 0; k < h; ++k) {
    float u[12], ua[12], w[6];
#pragma unroll
    for (int i = 0; i < 12; ++i) u[i] = up[(size_t)k * 12 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) frec[(size_t)(k * 6 + i) * W.plans] = r[i];
    const bool c0 = con[2 * k] != 0, c1 = con[2 * k + 1] != 0;
    if (in.ground) {
      uint8_t fl;
      float demand;
      plant_ground(u, c0, c1, mu0, mu1, 0.0, ua, fl, demand);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) ua[i] = u[i];
    }
    const bool push_on = in.push && k >= in.push_from && k - in.push_from < in.push_steps;
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = push_on ? in.push[b * 6 + i] : 0.f;
    double xn[12];
    bool ok = plant_step(Pb, Sc, x, ua, r, c0 ? 1.0 : 0.0, c1 ? 1.0 : 0.0, w, xn) && body_ok;
    double xr[12];
    rollout_reference(P.dt, C, in, b, h, k, x0, xr);
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && plant_finite(xr[i]);
    if (!ok && first_bad < 0) first_bad = k;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      x[i] = ok ? (float)xn[i] : __builtin_nanf("");
      xrec[(size_t)k * 12 + i] = x[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const double e = (double)x[i] - xr[i], ui = (double)u[i];
      cost += C.Q[i] * e * e + C.R[i] * ui * ui;
    }
    if (in.move_feet && k + 1 < h) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (con[2 * k + g] == 0 && con[2 * (k + 1) + g] != 0) {
          r[3 * g] = (float)foothold_target((double)x[3], (double)x[9], P.h, P.dt, P.kv, cx);
          r[3 * g + 1] = (float)(foothold_target((double)x[4], (double)x[10], P.h, P.dt, P.kv, cy) + 0.04 * (g == 0 ? 1.0 : -1.0));
          r[3 * g + 2] = 0.f;
        }
      }
    }
  }
  if (out.cost) out.cost[plan] = cost;
  if (out.first_bad) out.first_bad[plan] = first_bad;
  if (!out.grad_u && !out.grad_x0 && !out.grad_foot) return;
  if (first_bad >= 0) {
    const double nan = __builtin_nan("");
    if (out.grad_u) {
#pragma unroll 1
      for (int q = 0; q < h * 12; ++q) out.grad_u[plan * (size_t)h * 12 + q] = nan;
    }
    if (out.grad_x0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) out.grad_x0[plan * 12 + i] = nan;
    }
    if (out.grad_foot) {
#pragma unroll
      for (int i = 0; i < 6; ++i) out.grad_foot[plan * 6 + i] = nan;
    }
    return;
  }

  // ---- backwards
  const double tp = 1.0 + P.kv, tv = 0.5 * P.h / 2 * P.dt;     // foothold_target's coefficients of p and v
  double lam[12], mu[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) mu[i] = 0.0;
#pragma unroll 1
  for (int k = h - 1; k >= 0; --k) {
    float u[12], ua[12], w[6], xs[12];
    {
      double xr[12];
      rollout_reference(P.dt, C, in, b, h, k, x0, xr);
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] += 2.0 * C.Q[i] * ((double)xrec[(size_t)k * 12 + i] - xr[i]);
    }
    if (in.move_feet && k + 1 < h) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (con[2 * k + g] == 0 && con[2 * (k + 1) + g] != 0) {
          lam[3] += tp * mu[3 * g]; lam[9] += tv * mu[3 * g];
          lam[4] += tp * mu[3 * g + 1]; lam[10] += tv * mu[3 * g + 1];
          mu[3 * g] = 0.0; mu[3 * g + 1] = 0.0; mu[3 * g + 2] = 0.0;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      u[i] = up[(size_t)k * 12 + i];
      xs[i] = k > 0 ? xrec[(size_t)(k - 1) * 12 + i] : in.x_fb[b * 12 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) r[i] = frec[(size_t)(k * 6 + i) * W.plans];
    const bool c0 = con[2 * k] != 0, c1 = con[2 * k + 1] != 0;
    uint8_t fl = 0;
    if (in.ground) {
      float demand;
      plant_ground(u, c0, c1, mu0, mu1, 0.0, ua, fl, demand);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) ua[i] = u[i];
    }
    const bool push_on = in.push && k >= in.push_from && k - in.push_from < in.push_steps;
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = push_on ? in.push[b * 6 + i] : 0.f;
    double gua[12], gr[6], gu[12];
    plant_step_vjp(Pb, Sc, xs, ua, r, c0 ? 1.0 : 0.0, c1 ? 1.0 : 0.0, w, W.sub + plan, W.plans, L, lam, gua, gr);
#pragma unroll
    for (int i = 0; i < 6; ++i) mu[i] += gr[i];
    bool seen[2];
    plant_ground_vjp(u, fl, c0, c1, mu0, mu1, gua, gu, seen);
    if (out.grad_u) {
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const double own = 2.0 * C.R[i] * (double)u[i];
        out.grad_u[(plan * (size_t)h + (size_t)k) * 12 + i] = seen[(i / 3) & 1] ? gu[i] + own : own;
      }
    }
  }
  if (out.grad_x0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) out.grad_x0[plan * 12 + i] = lam[i];
  }
  if (out.grad_foot) {
#pragma unroll
    for (int i = 0; i < 6; ++i) out.grad_foot[plan * 6 + i] = mu[i];
  }
}

#ifndef BMPC_EMU
// One wave per SIMD is all that is asked for: the forward pass alone holds 253 registers in plant_rollout_samples_kernel.
__global__ void __launch_bounds__(RGRAD_NT, 1)
plant_rollout_grad_kernel(const PlantParams P, const PlantScheme Sc, const RolloutCost C, const RolloutIn in, const RolloutGradOut out,
                          const RolloutGradScratch W, const int B, const int S) {
  __shared__ double slab[RGRAD_SLAB * RGRAD_NT];
  const size_t plan = (size_t)blockIdx.x * RGRAD_NT + threadIdx.x;
  if (plan >= (size_t)B * (size_t)S) return;
  const LaneSlab L = {slab + threadIdx.x, RGRAD_NT};
  rollout_grad_plan(P, Sc, C, in, out, W, L, plan / (size_t)S, plan);
}
#endif

}  // namespace bmpc

#endif  // BMPC_PLANT_ROLLOUT_GRAD_HIP
