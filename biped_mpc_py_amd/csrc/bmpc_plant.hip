// bmpc_plant.hip -- the plant of the closed-loop simulation (gfx950 / CDNA4): the NONLINEAR single rigid body, integrated over one
// control period under held controls, and the feedback step that closes bmpc_simulate_device's loop on it.
//   plant_step               the per-instance body: values in, values out (also plain C++ for tests/emu, BMPC_EMU)
//   plant_step_kernel        one control period of B instances (bmpc_plant_step*)
//   simulate_feedback_kernel one closed-loop period: integrate x_fb under controls[:, 0], advance t, move landing feet, record
//   plant_body, plant_outcome, plant_step_body_kernel, simulate_body_feedback_kernel: the same with the rigid body (m, I_b, g) taken
//                            per instance, and each instance's fall outcome reduced over the periods (at the end of this file's parts)
//   plant_ground, plant_ground_reduce, plant_step_ground_kernel, simulate_ground_feedback_kernel: the same with a ground under the
//                            plant -- a friction cone and unilateral contact on what each stance leg transmits, per-leg friction
//                            per instance, and who slipped reduced over the periods (behind the body's parts)
// State x = [e(3), p(3), w(3), v(3)], e = [roll, pitch, yaw], w and v in the world frame (REF:13).  Held over the period: the
// controls u = [f1 f2 m1 m2], the feet r_0, r_1, the contact bits c_0, c_1 and an external wrench [F(3), M(3)] (world frame).
//   R = Rz(e2) Ry(e1) Rx(e0) (REF:124-138),  I_w = R I_b R'
//   e0' = (cos e2 wx + sin e2 wy) / cos e1,  e1' = -sin e2 wx + cos e2 wy,  e2' = wz + sin e1 e0'
//   p' = v
//   tau = sum_g c_g [(r_g - p) x f_g + m_g] + M,   w' = I_w^-1 (tau - w x I_w w)
//   v' = (sum_g c_g f_g + F) / m + (0, 0, -g)
// This is NOT the controller's model (REF:148-185): that one maps rates through Rot / R_inv of the reference attitude, has no
// gyroscopic term and does not gate a leg by its contact bit.  A leg with contact bit 0 transmits nothing here.
// Integration: n in [1, 64] substeps of dt / n, explicit Euler (every component from the old stage values: the form of
// A = I + Ac dt, REF:183-184) or classical RK4.  fp64 arithmetic on fp32 I/O.  A non-finite input, or |cos e1| < 2^-22 at any
// stage (the threshold of bmpc_evaluate.hip), makes the whole next state of that instance NaN; no other instance is touched.
// One thread per instance, no LDS, every array statically indexed; the angular rate equation is solved in the body frame
// with I_b^-1 from the parameter block.
// The lever arms enter as tau = T0 - p x Fc with T0, Fc formed once per period (plant_held): the same torque, 27 values fewer
// to keep in registers through the stages.
#ifndef BMPC_PLANT_HIP
#define BMPC_PLANT_HIP

#ifndef BMPC_EMU
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "bmpc_model.hip"

namespace bmpc {

constexpr int PLANT_EULER = 0, PLANT_RK4 = 1;
constexpr int PLANT_MAX_SUBSTEPS = 64;

struct PlantParams {
  double h, dt, kv, m, g;                      // h: the horizon as the foothold target uses it (REF:429)
  double cmd_x, cmd_y, Ib[9], Ibinv[9];        // cmd: the handle's x_cmd[3], x_cmd[4]
};

__device__ __forceinline__ bool plant_finite(const float v) { return fabsf(v) <= 3.402823466e+38f; }   // (false for NaN)

// What the held inputs contribute, formed once per period: the contact-gated force Fc = sum_g c_g f_g, the torque about the
// world origin T0 = sum_g c_g (r_g x f_g + m_g) + M (so that tau = T0 - p x Fc), and the acceleration a = (Fc + F) / m - g e_z.
struct PlantHeld { double Fc[3], T0[3], a[3]; };

__device__ __forceinline__ PlantHeld plant_held(const PlantParams& P, const float (&u)[12], const float (&r)[6], const double c0,
                                                const double c1, const float (&w)[6]) {
  const double c[2] = {c0, c1};
  PlantHeld H;
#pragma unroll
  for (int i = 0; i < 3; ++i) { H.Fc[i] = 0.0; H.T0[i] = (double)w[3 + i]; }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double f[3] = {(double)u[3 * g], (double)u[3 * g + 1], (double)u[3 * g + 2]};
    const double a[3] = {(double)r[3 * g], (double)r[3 * g + 1], (double)r[3 * g + 2]};
    H.T0[0] += c[g] * (a[1] * f[2] - a[2] * f[1] + (double)u[6 + 3 * g]);
    H.T0[1] += c[g] * (a[2] * f[0] - a[0] * f[2] + (double)u[7 + 3 * g]);
    H.T0[2] += c[g] * (a[0] * f[1] - a[1] * f[0] + (double)u[8 + 3 * g]);
#pragma unroll
    for (int i = 0; i < 3; ++i) H.Fc[i] += c[g] * f[i];
  }
  H.a[0] = (H.Fc[0] + (double)w[0]) / P.m; H.a[1] = (H.Fc[1] + (double)w[1]) / P.m; H.a[2] = (H.Fc[2] + (double)w[2]) / P.m - P.g;
  return H;
}

// The integration scheme of a period as the host resolves it (uniform values: kernel arguments, so that they sit in scalar
// registers; formed per thread they would each hold a vector register pair through the stage loop).
struct PlantScheme {
  int substeps, stages;                        // stages: 1 explicit Euler, 4 classical RK4
  double hs, hh, wsum, half2;                  // dt / substeps, hs / 2, the weight of the stage sum (hs or hs / 6), hs^2 / 2 (RK4) or 0
};
inline PlantScheme plant_scheme(const double dt, const int integrator, const int substeps) {
  PlantScheme S;
  const bool rk4 = integrator != PLANT_EULER;
  S.substeps = substeps; S.stages = rk4 ? 4 : 1;
  S.hs = dt / (double)substeps; S.hh = 0.5 * S.hs;
  S.wsum = rk4 ? S.hs / 6.0 : S.hs;
  S.half2 = rk4 ? 0.5 * S.hs * S.hs : 0.0;
  return S;
}

// The rates that depend on the state: de = e', dw = w' at attitude es, angular velocity w0 + cj kw and position
// p0 + cj (v0 + cprev a) -- both formed behind the sincos passes, where fewer values are alive (p' = v and v' = H.a need no
// evaluation); dw may be kw.  Returns false where |cos e1| < 2^-22.
__device__ __forceinline__ bool plant_rate(const PlantParams& P, const PlantHeld& H, const double (&es)[3], const double (&p0)[3],
                                           const double (&v0)[3], const double cprev, const double (&w0)[3], const double cj,
                                           const double (&kw)[3], double (&de)[3], double (&dw)[3]) {
  // The three fp64 sincos through ONE inlined body: a rolled loop over a ring of six registers (no indexed array).  Written out
  // three times the scheduler interleaves them, and their temporaries add up to more registers than the rest of the step.
  // The ring starts as (e0, -, e1, -, e2, -); a pass takes the angle at its head, turns the ring by two and puts (sin, cos) at
  // its tail, so that it ends as (sin e0, cos e0, sin e1, cos e1, sin e2, cos e2).
  double s0 = es[0], k0 = 0.0, s1 = es[1], k1 = 0.0, s2 = es[2], k2 = 0.0;
#pragma unroll 1
  for (int q = 0; q < 3; ++q) {
    double sn, cs;
    sincos(s0, &sn, &cs);
    s0 = s1; k0 = k1; s1 = s2; k1 = k2; s2 = sn; k2 = cs;
  }
  const double w[3] = {w0[0] + cj * kw[0], w0[1] + cj * kw[1], w0[2] + cj * kw[2]};
  const double ps[3] = {p0[0] + cj * (v0[0] + cprev * H.a[0]), p0[1] + cj * (v0[1] + cprev * H.a[1]), p0[2] + cj * (v0[2] + cprev * H.a[2])};
  const double wz0 = k2 * w[0] + s2 * w[1], wz1 = -s2 * w[0] + k2 * w[1];        // Rz' w: also the numerators of the Euler rates
  const double e0d = wz0 / k1;
  de[0] = e0d;
  de[1] = wz1;
  de[2] = w[2] + s1 * e0d;
  const double tau[3] = {H.T0[0] - (ps[1] * H.Fc[2] - ps[2] * H.Fc[1]), H.T0[1] - (ps[2] * H.Fc[0] - ps[0] * H.Fc[2]),
                         H.T0[2] - (ps[0] * H.Fc[1] - ps[1] * H.Fc[0])};
  // w' = I_w^-1 (tau - w x I_w w) = R I_b^-1 (R' tau - wb x I_b wb), wb = R' w: a cross product turns with its factors.  R' and R
  // are applied as the three plane rotations they are made of (R' = Rx' Ry' Rz'): the nine entries of R are never formed.
  const double wy0 = k1 * wz0 - s1 * w[2], wy2 = s1 * wz0 + k1 * w[2];           // Ry' (Rz' w)
  const double wb[3] = {wy0, k0 * wz1 + s0 * wy2, -s0 * wz1 + k0 * wy2};         // Rx' ...
  const double tz0 = k2 * tau[0] + s2 * tau[1], tz1 = -s2 * tau[0] + k2 * tau[1];
  const double ty0 = k1 * tz0 - s1 * tau[2], ty2 = s1 * tz0 + k1 * tau[2];
  const double tb[3] = {ty0, k0 * tz1 + s0 * ty2, -s0 * tz1 + k0 * ty2};
  double Lb[3], ab[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Lb[i] = P.Ib[3 * i] * wb[0] + P.Ib[3 * i + 1] * wb[1] + P.Ib[3 * i + 2] * wb[2];
  const double y[3] = {tb[0] - (wb[1] * Lb[2] - wb[2] * Lb[1]), tb[1] - (wb[2] * Lb[0] - wb[0] * Lb[2]), tb[2] - (wb[0] * Lb[1] - wb[1] * Lb[0])};
#pragma unroll
  for (int i = 0; i < 3; ++i) ab[i] = P.Ibinv[3 * i] * y[0] + P.Ibinv[3 * i + 1] * y[1] + P.Ibinv[3 * i + 2] * y[2];
  const double ax1 = k0 * ab[1] - s0 * ab[2], ax2 = s0 * ab[1] + k0 * ab[2];     // Rx ab
  const double ay0 = k1 * ab[0] + s1 * ax2, ay2 = -s1 * ab[0] + k1 * ax2;        // Ry ...
  dw[0] = k2 * ay0 - s2 * ax1; dw[1] = s2 * ay0 + k2 * ax1; dw[2] = ay2;         // Rz ...
  return fabs(k1) >= 0x1p-22;
}

// One control period: xn = the state after S.substeps steps of S.hs from x.  c0, c1: the contact bits as 0.0 / 1.0.  The inputs
// come as the fp32 values of the ABI and are widened where they are used: widened up front, 36 of them hold 72 registers at once.
// Returns false, with xn all NaN, for a bad instance.
// Both integrators are one loop over stages with ONE call of plant_rate: stage j starts from the step's state + c_j hs (rate of
// stage j - 1), its rate enters the step with weight b_j; Euler is the one-stage scheme c = {0}, b = {1}, RK4
// c = {0, 1/2, 1/2, 1}, b = {1, 2, 2, 1} / 6.  The acceleration a is constant over the period, so v's stage rates are a and p's
// are v + c_{j-1} hs a: their weighted sums are written out (v += hs a;  p += hs v, + hs^2 / 2 a under RK4) instead of being
// carried -- the same scheme, 24 values fewer in registers.
__device__ __forceinline__ bool plant_step(const PlantParams& P, const PlantScheme& S, const float (&x)[12],
                                           const float (&u)[12], const float (&r)[6], const double c0, const double c1,
                                           const float (&w)[6], double (&xn)[12]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && plant_finite(x[i]) && plant_finite(u[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && plant_finite(r[i]) && plant_finite(w[i]);
  const PlantHeld H = plant_held(P, u, r, c0, c1, w);
  double e[3], p[3], om[3], v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { e[i] = (double)x[i]; p[i] = (double)x[3 + i]; om[i] = (double)x[6 + i]; v[i] = (double)x[9 + i]; }
  for (int s = 0; s < S.substeps; ++s) {
    double ke[3] = {0.0, 0.0, 0.0}, kw[3] = {0.0, 0.0, 0.0}, ae[3] = {0.0, 0.0, 0.0}, aw[3] = {0.0, 0.0, 0.0};
    double cprev = 0.0;
#pragma unroll 1
    for (int j = 0; j < S.stages; ++j) {
      const double cj = j == 0 ? 0.0 : (j == 3 ? S.hs : S.hh), bj = (j == 1 || j == 2) ? 2.0 : 1.0;
      const double es[3] = {e[0] + cj * ke[0], e[1] + cj * ke[1], e[2] + cj * ke[2]};
      ok = plant_rate(P, H, es, p, v, cprev, om, cj, kw, ke, kw) && ok;
#pragma unroll
      for (int i = 0; i < 3; ++i) { ae[i] += bj * ke[i]; aw[i] += bj * kw[i]; }
      cprev = cj;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      e[i] += S.wsum * ae[i]; om[i] += S.wsum * aw[i];
      p[i] += S.hs * v[i] + S.half2 * H.a[i];
      v[i] += S.hs * H.a[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) { xn[i] = e[i]; xn[3 + i] = p[i]; xn[6 + i] = om[i]; xn[9 + i] = v[i]; }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 12; ++i) xn[i] = __builtin_nan("");
  }
  return ok;
}

// The landing rule of the closed loop: leg g (side +1 for leg 0, -1 for leg 1) lands when its row-0 contact bit is 0 at schedule
// step k0 (this period) and 1 at k1 (the next); its foothold then becomes the swing controller's own target (REF:428-435) at
// the state x, on the ground.  Returns whether the leg lands; r is rewritten only then.
__device__ __forceinline__ bool plant_land(const PlantParams& P, const int k0, const int k1, const int offset, const int period,
                                           const int duty, const double side, const double (&x)[12], const double cmd_x,
                                           const double cmd_y, double (&r)[3]) {
  const bool lands = !in_stance(k0, offset, period, duty) && in_stance(k1, offset, period, duty);
  if (lands) {
    r[0] = foothold_target(x[3], x[9], P.h, P.dt, P.kv, cmd_x);
    r[1] = foothold_target(x[4], x[10], P.h, P.dt, P.kv, cmd_y) + 0.04 * side;
    r[2] = 0.0;
  }
  return lands;
}

// ---- The body per instance: the PLANT's m, I_b, g of one instance in place of the handle's (one controller model, many bodies).

__device__ __forceinline__ bool plant_finite(const double v) { return fabs(v) <= 1.7976931348623157e+308; }   // (false for NaN)

// Pb = P with this instance's m, I9 (row-major I_b) and g, each a pointer to the instance's value or null: the handle's.
// I_b^-1 is formed here in fp64, adjugate over determinant; without I9 it stays the handle's, bit for bit.  kv, dt, h and the
// commands are the controller's and stay.  Returns false for a bad body: a supplied value that is not finite, m <= 0, a
// determinant that is zero or not finite, an entry of the inverse that is not finite.
__device__ __forceinline__ bool plant_body(const PlantParams& P, const double* m, const double* I9, const double* g, PlantParams& Pb) {
  Pb = P;
  bool ok = true;
  if (m) { Pb.m = *m; ok = ok && plant_finite(Pb.m) && Pb.m > 0.0; }
  if (g) { Pb.g = *g; ok = ok && plant_finite(Pb.g); }
  if (I9) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { Pb.Ib[i] = I9[i]; ok = ok && plant_finite(Pb.Ib[i]); }
    const double(&a)[9] = Pb.Ib;
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02, id = 1.0 / det;
    ok = ok && plant_finite(det) && det != 0.0;
    Pb.Ibinv[0] = c00 * id; Pb.Ibinv[1] = (a[2] * a[7] - a[1] * a[8]) * id; Pb.Ibinv[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    Pb.Ibinv[3] = c01 * id; Pb.Ibinv[4] = (a[0] * a[8] - a[2] * a[6]) * id; Pb.Ibinv[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    Pb.Ibinv[6] = c02 * id; Pb.Ibinv[7] = (a[1] * a[6] - a[0] * a[7]) * id; Pb.Ibinv[8] = (a[0] * a[4] - a[1] * a[3]) * id;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && plant_finite(Pb.Ibinv[i]);
  }
  return ok;
}

// plant_step of the instance's own body; a bad body makes the next state all NaN like a bad state.
__device__ __forceinline__ bool plant_step_body(const PlantParams& P, const double* m, const double* I9, const double* g,
                                                const PlantScheme& S, const float (&x)[12], const float (&u)[12], const float (&r)[6],
                                                const double c0, const double c1, const float (&w)[6], double (&xn)[12]) {
  PlantParams Pb;
  bool ok = plant_body(P, m, I9, g, Pb);
  ok = plant_step(Pb, S, x, u, r, c0, c1, w, xn) && ok;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 12; ++i) xn[i] = __builtin_nan("");
  }
  return ok;
}

// The fall outcome of one instance, reduced over the periods: x is the state after period s as stored (fp32).  Fallen at s iff
// !(|x0| <= tilt_max && |x1| <= tilt_max && x5 >= z_min), the fp32 values widened against the fp64 thresholds, so that a NaN
// state counts as fallen.  first_fall: the first such s (-1 so far: none); max_tilt, min_z: the extrema of max(|x0|, |x1|) and
// of x5 over the periods that are not NaN (fmaxf / fminf from a NaN start).
__device__ __forceinline__ void plant_outcome(const double tilt_max, const double z_min, const float (&x)[12], const int s,
                                              int32_t& first_fall, float& max_tilt, float& min_z) {
  const bool up = fabs((double)x[0]) <= tilt_max && fabs((double)x[1]) <= tilt_max && (double)x[5] >= z_min;
  if (!up && first_fall < 0) first_fall = s;
  max_tilt = fmaxf(max_tilt, fmaxf(fabsf(x[0]), fabsf(x[1])));
  min_z = fminf(min_z, x[5]);
}

// ---- The ground under the plant: what of the commanded controls a flat floor at z = 0 with Coulomb friction transmits.

constexpr int GROUND_SLIP = 1, GROUND_UNLOADED = 4;      // flag bits of leg 0; leg 1: shifted left by one

// One instance, once per control period, before the integration (the controls are held and the ground is flat, so the rule does
// not depend on the state).  Leg g with contact bit c_g, commanded f = (fx, fy, fz), m and true friction mu_g transmits
//   c_g == 0:                 nothing (its six values are +0), as plant_held gates it
//   c_g == 1, not fz > 0:     nothing either -- the ground cannot pull, and passes no moment without load; flag UNLOADED << g
//   c_g == 1, fz > 0:         fz and m with their bits; fx, fy with their bits while t = sqrt(fx^2 + fy^2) <= lim = mu_g fz, else
//                             scaled by lim / t in fp64 and rounded to fp32 once each; flag SLIP << g
// ua: the applied controls in the layout of u.  mu_g may be +inf (no friction limit; it is multiplied for loaded legs only).
// demand: the largest t / fz over the loaded legs with fz >= fz_floor, as fp32, NaN if there is none.  Returns false, with ua
// and demand all NaN and no flag, for a bad instance: a mu that is NaN or negative, or a control that is not finite (either leg,
// whatever its contact bit).  No contraction here: every operation is the correctly rounded one of its line.
// Not modelled: a slipping foot does not slide (its foothold stays), moments have no limit (centre of pressure, torsion), static
// and kinetic friction are one number.
__device__ __forceinline__ bool plant_ground(const float (&u)[12], const bool c0, const bool c1, const double mu0, const double mu1,
                                             const double fz_floor, float (&ua)[12], uint8_t& flags, float& demand) {
#pragma clang fp contract(off)
  const bool c[2] = {c0, c1};
  const double mu[2] = {mu0, mu1};
  bool ok = mu0 >= 0.0 && mu1 >= 0.0;            // (false for NaN)
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && plant_finite(u[i]);
  int fl = 0;
  double dem = __builtin_nan("");
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const float fx = u[3 * g], fy = u[3 * g + 1], fz = u[3 * g + 2];
    const bool loaded = c[g] && fz > 0.f;
    if (c[g] && !loaded) fl |= GROUND_UNLOADED << g;
    float ax = loaded ? fx : 0.f, ay = loaded ? fy : 0.f;
    if (loaded) {
      const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
      const double t = sqrt(dx * dx + dy * dy), lim = mu[g] * dz;
      if (t > lim) {
        const double sc = lim / t;
        ax = (float)(dx * sc); ay = (float)(dy * sc);
        fl |= GROUND_SLIP << g;
      }
      if (dz >= fz_floor) dem = fmax(dem, t / dz);
    }
    ua[3 * g] = ax; ua[3 * g + 1] = ay; ua[3 * g + 2] = loaded ? fz : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) ua[6 + 3 * g + i] = loaded ? u[6 + 3 * g + i] : 0.f;
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 12; ++i) ua[i] = __builtin_nanf("");
    fl = 0; dem = __builtin_nan("");
  }
  flags = (uint8_t)fl;
  demand = (float)dem;
  return ok;
}

// A ground step: plant_step_body under what the ground transmits of u, with the same contact bits -- exactly
// plant_step_body(ua).  A bad ground makes ua, and with it the next state, all NaN.
__device__ __forceinline__ bool plant_step_ground(const PlantParams& P, const double* m, const double* I9, const double* g,
                                                  const double mu0, const double mu1, const double fz_floor, const PlantScheme& S,
                                                  const float (&x)[12], const float (&u)[12], const float (&r)[6], const bool c0,
                                                  const bool c1, const float (&w)[6], double (&xn)[12], float (&ua)[12],
                                                  uint8_t& flags, float& demand) {
  const bool ok = plant_ground(u, c0, c1, mu0, mu1, fz_floor, ua, flags, demand);
  return plant_step_body(P, m, I9, g, S, x, ua, r, c0 ? 1.0 : 0.0, c1 ? 1.0 : 0.0, w, xn) && ok;
}

// What the closed loop keeps of the ground per instance, reduced over the periods: the flags and the demand of period s into
// first_slip (the first s with a slip bit; -1 so far: none), the periods each leg slipped / was unloaded, and the largest demand
// (fmaxf from a NaN start: periods without a demand are skipped).
__device__ __forceinline__ void plant_ground_reduce(const uint8_t flags, const float demand, const int s, int32_t& first_slip,
                                                    int32_t (&slip)[2], int32_t (&unloaded)[2], float& mu_demand) {
  if ((flags & (GROUND_SLIP | GROUND_SLIP << 1)) && first_slip < 0) first_slip = s;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    slip[g] += (flags >> g) & 1;
    unloaded[g] += (flags >> (2 + g)) & 1;
  }
  mu_demand = fmaxf(mu_demand, demand);
}

}  // namespace bmpc

#ifndef BMPC_EMU
#include "bmpc_lowlevel.hip"                   // GaitParams, py_floordiv: the schedule step of a time, as gait_kernel finds it

namespace bmpc {

// the gait rule as the landing needs it: bmpc_gait, and whether landing legs get a new foothold
struct PlantGait { int period, offset[2], duty[2], move_feet; };

// Both kernels ask for four waves per SIMD (the second launch bound): 128 registers, which the step fits without spilling; left
// to itself the scheduler spreads the same code over a few more.
// x_next[B][12] from x_fb[B][12], u0[B][12], foot[B][6], contact0[B][2] and wrench[B][6] (or null: none)
__global__ void __launch_bounds__(256, 4)
plant_step_kernel(const PlantParams P, const PlantScheme S, const int B, const float* __restrict__ x_fb, const float* __restrict__ u0,
                  const float* __restrict__ foot, const uint8_t* __restrict__ contact0, const float* __restrict__ wrench,
                  float* __restrict__ x_next) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float x[12], u[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[(size_t)b * 12 + i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = wrench ? wrench[(size_t)b * 6 + i] : 0.f; }
  const double c0 = contact0[(size_t)b * 2] ? 1.0 : 0.0, c1 = contact0[(size_t)b * 2 + 1] ? 1.0 : 0.0;
  plant_step(P, S, x, u, r, c0, c1, w, xn);
#pragma unroll
  for (int i = 0; i < 12; ++i) x_next[(size_t)b * 12 + i] = (float)xn[i];
}

// One closed-loop period of bmpc_simulate_device, in place of rollout_feedback_kernel: the plant integrates x_fb under
// controls[b, 0, :], foot[b], row 0 of this period's contact table and the push (null: not active in this period); t += dt;
// with G.move_feet the legs that land at the new time get the foothold target at the NEW state; the applied control, the new
// state, the footholds after the update and the iteration count are recorded, status_any |= status (| BMPC_NUMERICAL for a
// bad plant step).  One thread per instance.
__global__ void __launch_bounds__(256, 4)
simulate_feedback_kernel(const PlantParams P, const PlantScheme S, const PlantGait G, const int B,
                         const float* __restrict__ controls, const uint8_t* __restrict__ contact, const int32_t* __restrict__ iters,
                         const int32_t* __restrict__ status, const float* __restrict__ push, const float* __restrict__ x_cmd,
                         float* __restrict__ x_fb, float* foot, double* __restrict__ t, float* __restrict__ u0_out,
                         float* __restrict__ x_out, float* __restrict__ foot_out, int32_t* __restrict__ iters_out,
                         int32_t* __restrict__ status_any) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int h = (int)P.h;
  const float* u0 = controls + (size_t)b * h * 12;
  float x[12], u[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = push ? push[(size_t)b * 6 + i] : 0.f; }
  // What does not depend on the step comes first (the applied control, the iteration count, the solver's status): behind the
  // step, its loads are hoisted above the stages and sit in registers there.
  if (u0_out) {
#pragma unroll
    for (int i = 0; i < 12; ++i) u0_out[(size_t)b * 12 + i] = u[i];
  }
  if (iters_out) iters_out[b] = iters[b];
  if (status_any) status_any[b] |= status[b];
  const uint8_t* row0 = contact + (size_t)b * h * 2;
  const bool ok = plant_step(P, S, x, u, r, row0[0] ? 1.0 : 0.0, row0[1] ? 1.0 : 0.0, w, xn);
  if (!ok && status_any) status_any[b] |= 2;      // BMPC_NUMERICAL
  float xf[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    xf[i] = (float)xn[i];
    x_fb[(size_t)b * 12 + i] = xf[i];
    if (x_out) x_out[(size_t)b * 12 + i] = xf[i];
  }
  const double t0 = t[b], t1 = t0 + P.dt;
  t[b] = t1;
  // the schedule steps of t0 and t1, as gait_kernel finds them (REF:56-57)
  double ka = fmod(py_floordiv(t0, P.dt), P.h), kb = fmod(py_floordiv(t1, P.dt), P.h);
  if (ka < 0) ka += P.h;
  if (kb < 0) kb += P.h;
  const int k0 = (int)ka, k1 = (int)kb;
  float rf[6];                                   // (`foot` is not __restrict__: read again here, not carried through the stages)
#pragma unroll
  for (int i = 0; i < 6; ++i) rf[i] = foot[(size_t)b * 6 + i];
  if (G.move_feet) {
    // the target is taken at the fp32 state the next solve will see
    double xs[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) xs[i] = xf[i];
    const double cx = x_cmd ? (double)x_cmd[(size_t)b * 12 + 3] : P.cmd_x, cy = x_cmd ? (double)x_cmd[(size_t)b * 12 + 4] : P.cmd_y;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double rg[3];
      if (plant_land(P, k0, k1, G.offset[g], G.period, G.duty[g], g == 0 ? 1.0 : -1.0, xs, cx, cy, rg)) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          rf[3 * g + i] = (float)rg[i];
          foot[(size_t)b * 6 + 3 * g + i] = rf[3 * g + i];
        }
      }
    }
  }
  if (foot_out) {
#pragma unroll
    for (int i = 0; i < 6; ++i) foot_out[(size_t)b * 6 + i] = rf[i];
  }
}


// the per-instance body as the kernels get it: m [B], I [B][9] row-major, g [B], each null for the handle's value
struct PlantBody { const double *m, *I, *g; };
// the fall outcome of bmpc_simulate_body_device: thresholds, first_fall [B], max_tilt [B], min_z [B] (each null: not wanted)
struct PlantOutcome { double tilt_max, z_min; int32_t* first_fall; float *max_tilt, *min_z; };

// One instance of plant_step_body_kernel: plant_step_kernel's with the body from Bd.
__device__ __forceinline__ void plant_step_body_instance(const PlantParams& P, const PlantBody& Bd, const PlantScheme& S, const int b,
                                                    const float* __restrict__ x_fb, const float* __restrict__ u0,
                                                    const float* __restrict__ foot, const uint8_t* __restrict__ contact0,
                                                    const float* __restrict__ wrench, float* __restrict__ x_next) {
  float x[12], u[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[(size_t)b * 12 + i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = wrench ? wrench[(size_t)b * 6 + i] : 0.f; }
  const double c0 = contact0[(size_t)b * 2] ? 1.0 : 0.0, c1 = contact0[(size_t)b * 2 + 1] ? 1.0 : 0.0;
  plant_step_body(P, Bd.m ? Bd.m + b : nullptr, Bd.I ? Bd.I + (size_t)b * 9 : nullptr, Bd.g ? Bd.g + b : nullptr, S, x, u, r, c0, c1, w, xn);
#pragma unroll
  for (int i = 0; i < 12; ++i) x_next[(size_t)b * 12 + i] = (float)xn[i];
}

// One instance of simulate_body_feedback_kernel: simulate_feedback_kernel's period, statement for statement, with the body from Bd
// and the outcome O of period s reduced where it is asked for.  (Written out a second time on purpose: the two kernels above are
// held to their instruction sequence, and routed through a shared function they compile to another one, with spills.)
__device__ __forceinline__ void feedback_body_instance(const PlantParams& P, const PlantBody& Bd, const PlantOutcome& O, const int s,
                                                  const PlantScheme& S, const PlantGait& G, const int b,
                                                  const float* __restrict__ controls, const uint8_t* __restrict__ contact,
                                                  const int32_t* __restrict__ iters, const int32_t* __restrict__ status,
                                                  const float* __restrict__ push, const float* __restrict__ x_cmd,
                                                  float* __restrict__ x_fb, float* foot, double* __restrict__ t,
                                                  float* __restrict__ u0_out, float* __restrict__ x_out, float* __restrict__ foot_out,
                                                  int32_t* __restrict__ iters_out, int32_t* __restrict__ status_any) {
  const int h = (int)P.h;
  const float* u0 = controls + (size_t)b * h * 12;
  float x[12], u[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = push ? push[(size_t)b * 6 + i] : 0.f; }
  // What does not depend on the step comes first (the applied control, the iteration count, the solver's status): behind the
  // step, its loads are hoisted above the stages and sit in registers there.
  if (u0_out) {
#pragma unroll
    for (int i = 0; i < 12; ++i) u0_out[(size_t)b * 12 + i] = u[i];
  }
  if (iters_out) iters_out[b] = iters[b];
  if (status_any) status_any[b] |= status[b];
  const uint8_t* row0 = contact + (size_t)b * h * 2;
  const bool ok = plant_step_body(P, Bd.m ? Bd.m + b : nullptr, Bd.I ? Bd.I + (size_t)b * 9 : nullptr, Bd.g ? Bd.g + b : nullptr, S, x,
                                  u, r, row0[0] ? 1.0 : 0.0, row0[1] ? 1.0 : 0.0, w, xn);
  if (!ok && status_any) status_any[b] |= 2;      // BMPC_NUMERICAL
  float xf[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    xf[i] = (float)xn[i];
    x_fb[(size_t)b * 12 + i] = xf[i];
    if (x_out) x_out[(size_t)b * 12 + i] = xf[i];
  }
  if (O.first_fall || O.max_tilt || O.min_z) {
    // (the entry initialised the three arrays on the stream: -1, NaN, NaN)
    int32_t first = O.first_fall ? O.first_fall[b] : 0;
    float mt = O.max_tilt ? O.max_tilt[b] : 0.f, mz = O.min_z ? O.min_z[b] : 0.f;
    plant_outcome(O.tilt_max, O.z_min, xf, s, first, mt, mz);
    if (O.first_fall) O.first_fall[b] = first;
    if (O.max_tilt) O.max_tilt[b] = mt;
    if (O.min_z) O.min_z[b] = mz;
  }
  const double t0 = t[b], t1 = t0 + P.dt;
  t[b] = t1;
  // the schedule steps of t0 and t1, as gait_kernel finds them (REF:56-57)
  double ka = fmod(py_floordiv(t0, P.dt), P.h), kb = fmod(py_floordiv(t1, P.dt), P.h);
  if (ka < 0) ka += P.h;
  if (kb < 0) kb += P.h;
  const int k0 = (int)ka, k1 = (int)kb;
  float rf[6];                                   // (`foot` is not __restrict__: read again here, not carried through the stages)
#pragma unroll
  for (int i = 0; i < 6; ++i) rf[i] = foot[(size_t)b * 6 + i];
  if (G.move_feet) {
    // the target is taken at the fp32 state the next solve will see
    double xs[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) xs[i] = xf[i];
    const double cx = x_cmd ? (double)x_cmd[(size_t)b * 12 + 3] : P.cmd_x, cy = x_cmd ? (double)x_cmd[(size_t)b * 12 + 4] : P.cmd_y;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double rg[3];
      if (plant_land(P, k0, k1, G.offset[g], G.period, G.duty[g], g == 0 ? 1.0 : -1.0, xs, cx, cy, rg)) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          rf[3 * g + i] = (float)rg[i];
          foot[(size_t)b * 6 + 3 * g + i] = rf[3 * g + i];
        }
      }
    }
  }
  if (foot_out) {
#pragma unroll
    for (int i = 0; i < 6; ++i) foot_out[(size_t)b * 6 + i] = rf[i];
  }
}

// The two kernels above with the body per instance (Bd: m, I_b, g of each instance where given, plant_body) and, in the closed
// loop, the outcome of period s reduced into O.  Eighteen more values per thread (I_b, I_b^-1) live in vector registers here
// where the handle's sit in scalar ones: three waves per SIMD (168 registers) instead of four.
__global__ void __launch_bounds__(256, 3)
plant_step_body_kernel(const PlantParams P, const PlantBody Bd, const PlantScheme S, const int B, const float* __restrict__ x_fb,
                       const float* __restrict__ u0, const float* __restrict__ foot, const uint8_t* __restrict__ contact0,
                       const float* __restrict__ wrench, float* __restrict__ x_next) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  plant_step_body_instance(P, Bd, S, b, x_fb, u0, foot, contact0, wrench, x_next);
}

__global__ void __launch_bounds__(256, 3)
simulate_body_feedback_kernel(const PlantParams P, const PlantBody Bd, const PlantOutcome O, const int s, const PlantScheme S,
                              const PlantGait G, const int B, const float* __restrict__ controls,
                              const uint8_t* __restrict__ contact, const int32_t* __restrict__ iters,
                              const int32_t* __restrict__ status, const float* __restrict__ push, const float* __restrict__ x_cmd,
                              float* __restrict__ x_fb, float* foot, double* __restrict__ t, float* __restrict__ u0_out,
                              float* __restrict__ x_out, float* __restrict__ foot_out, int32_t* __restrict__ iters_out,
                              int32_t* __restrict__ status_any) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  feedback_body_instance(P, Bd, O, s, S, G, b, controls, contact, iters, status, push, x_cmd, x_fb, foot, t, u0_out, x_out, foot_out,
                          iters_out, status_any);
}

// The ground as the kernels get it: mu [B][2] per leg (null: mu_h, the handle's, for both legs), and what is recorded of THIS
// period: u_applied [B][12] and flags [B] (each null: not wanted).
struct PlantGround {
  const double* mu;
  double mu_h;
  float* u_applied;
  uint8_t* flags;
};
// What the closed loop reduces of the ground over the periods: the floor of the demand, first_slip [B], slip_periods [B][2],
// unloaded_periods [B][2], mu_demand [B] (each null: not wanted).
struct PlantGroundSum {
  double fz_floor;
  int32_t *first_slip, *slip_periods, *unloaded_periods;
  float* mu_demand;
};

// One instance of plant_step_ground_kernel: plant_step_body_instance's with the ground Gr in front of the step.
__device__ __forceinline__ void plant_step_ground_instance(const PlantParams& P, const PlantBody& Bd, const PlantGround& Gr,
                                                           const PlantScheme& S, const int b, const float* __restrict__ x_fb,
                                                           const float* __restrict__ u0, const float* __restrict__ foot,
                                                           const uint8_t* __restrict__ contact0, const float* __restrict__ wrench,
                                                           float* __restrict__ x_next) {
  float x[12], u[12], ua[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[(size_t)b * 12 + i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = wrench ? wrench[(size_t)b * 6 + i] : 0.f; }
  const bool c0 = contact0[(size_t)b * 2] != 0, c1 = contact0[(size_t)b * 2 + 1] != 0;
  const double mu0 = Gr.mu ? Gr.mu[(size_t)b * 2] : Gr.mu_h, mu1 = Gr.mu ? Gr.mu[(size_t)b * 2 + 1] : Gr.mu_h;
  uint8_t fl;
  float demand;                                  // (not wanted here: the floor does not matter)
  plant_ground(u, c0, c1, mu0, mu1, 0.0, ua, fl, demand);
  // (what does not depend on the step comes first, as in the feedback kernels)
  if (Gr.u_applied) {
#pragma unroll
    for (int i = 0; i < 12; ++i) Gr.u_applied[(size_t)b * 12 + i] = ua[i];
  }
  if (Gr.flags) Gr.flags[b] = fl;
  plant_step_body(P, Bd.m ? Bd.m + b : nullptr, Bd.I ? Bd.I + (size_t)b * 9 : nullptr, Bd.g ? Bd.g + b : nullptr, S, x, ua, r,
                  c0 ? 1.0 : 0.0, c1 ? 1.0 : 0.0, w, xn);
#pragma unroll
  for (int i = 0; i < 12; ++i) x_next[(size_t)b * 12 + i] = (float)xn[i];
}

// One instance of simulate_ground_feedback_kernel: feedback_body_instance's period, statement for statement, with the ground Gr
// in front of the step -- the plant integrates what the ground transmits of the commanded control, u0_out keeps recording the
// command.  (Written out a third time for the reason given there: the kernels above are held to their instruction sequences.
// What is reduced of the ground over the periods is ground_reduce_kernel's: this kernel holds every scalar register it can get
// where the body is formed, and four more pointers made it spill them.)
__device__ __forceinline__ void feedback_ground_instance(const PlantParams& P, const PlantBody& Bd, const PlantOutcome& O,
                                                         const PlantGround& Gr, const int s, const PlantScheme& S, const PlantGait& G,
                                                         const int b, const float* __restrict__ controls,
                                                         const uint8_t* __restrict__ contact, const int32_t* __restrict__ iters,
                                                         const int32_t* __restrict__ status, const float* __restrict__ push,
                                                         const float* __restrict__ x_cmd, float* __restrict__ x_fb, float* foot,
                                                         double* __restrict__ t, float* __restrict__ u0_out, float* __restrict__ x_out,
                                                         float* __restrict__ foot_out, int32_t* __restrict__ iters_out,
                                                         int32_t* __restrict__ status_any) {
  const int h = (int)P.h;
  const float* u0 = controls + (size_t)b * h * 12;
  float x[12], u[12], ua[12], r[6], w[6];
  double xn[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { x[i] = x_fb[(size_t)b * 12 + i]; u[i] = u0[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { r[i] = foot[(size_t)b * 6 + i]; w[i] = push ? push[(size_t)b * 6 + i] : 0.f; }
  // What does not depend on the step comes first (the commanded and the applied control, the ground's flags, the
  // iteration count, the solver's status): behind the step, its loads are hoisted above the stages and sit in registers there.
  if (u0_out) {
#pragma unroll
    for (int i = 0; i < 12; ++i) u0_out[(size_t)b * 12 + i] = u[i];
  }
  if (iters_out) iters_out[b] = iters[b];
  if (status_any) status_any[b] |= status[b];
  const uint8_t* row0 = contact + (size_t)b * h * 2;
  const bool c0 = row0[0] != 0, c1 = row0[1] != 0;
  const double mu0 = Gr.mu ? Gr.mu[(size_t)b * 2] : Gr.mu_h, mu1 = Gr.mu ? Gr.mu[(size_t)b * 2 + 1] : Gr.mu_h;
  uint8_t fl;
  float demand;                                  // (not wanted here: the floor does not matter)
  plant_ground(u, c0, c1, mu0, mu1, 0.0, ua, fl, demand);
  if (Gr.u_applied) {
#pragma unroll
    for (int i = 0; i < 12; ++i) Gr.u_applied[(size_t)b * 12 + i] = ua[i];
  }
  if (Gr.flags) Gr.flags[b] = fl;
  const bool ok = plant_step_body(P, Bd.m ? Bd.m + b : nullptr, Bd.I ? Bd.I + (size_t)b * 9 : nullptr, Bd.g ? Bd.g + b : nullptr, S, x,
                                  ua, r, c0 ? 1.0 : 0.0, c1 ? 1.0 : 0.0, w, xn);
  if (!ok && status_any) status_any[b] |= 2;      // BMPC_NUMERICAL
  float xf[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    xf[i] = (float)xn[i];
    x_fb[(size_t)b * 12 + i] = xf[i];
    if (x_out) x_out[(size_t)b * 12 + i] = xf[i];
  }
  if (O.first_fall || O.max_tilt || O.min_z) {
    // (the entry initialised the three arrays on the stream: -1, NaN, NaN)
    int32_t first = O.first_fall ? O.first_fall[b] : 0;
    float mt = O.max_tilt ? O.max_tilt[b] : 0.f, mz = O.min_z ? O.min_z[b] : 0.f;
    plant_outcome(O.tilt_max, O.z_min, xf, s, first, mt, mz);
    if (O.first_fall) O.first_fall[b] = first;
    if (O.max_tilt) O.max_tilt[b] = mt;
    if (O.min_z) O.min_z[b] = mz;
  }
  const double t0 = t[b], t1 = t0 + P.dt;
  t[b] = t1;
  // the schedule steps of t0 and t1, as gait_kernel finds them (REF:56-57)
  double ka = fmod(py_floordiv(t0, P.dt), P.h), kb = fmod(py_floordiv(t1, P.dt), P.h);
  if (ka < 0) ka += P.h;
  if (kb < 0) kb += P.h;
  const int k0 = (int)ka, k1 = (int)kb;
  float rf[6];                                   // (`foot` is not __restrict__: read again here, not carried through the stages)
#pragma unroll
  for (int i = 0; i < 6; ++i) rf[i] = foot[(size_t)b * 6 + i];
  if (G.move_feet) {
    // the target is taken at the fp32 state the next solve will see
    double xs[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) xs[i] = xf[i];
    const double cx = x_cmd ? (double)x_cmd[(size_t)b * 12 + 3] : P.cmd_x, cy = x_cmd ? (double)x_cmd[(size_t)b * 12 + 4] : P.cmd_y;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double rg[3];
      if (plant_land(P, k0, k1, G.offset[g], G.period, G.duty[g], g == 0 ? 1.0 : -1.0, xs, cx, cy, rg)) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          rf[3 * g + i] = (float)rg[i];
          foot[(size_t)b * 6 + 3 * g + i] = rf[3 * g + i];
        }
      }
    }
  }
  if (foot_out) {
#pragma unroll
    for (int i = 0; i < 6; ++i) foot_out[(size_t)b * 6 + i] = rf[i];
  }
}

// The two body kernels with the ground under the plant (Gr; plant_ground): the body stays optional (null members of Bd: the
// handle's) and the fall outcome is still reduced.  Three waves per SIMD like the body kernels: the ground is done before the
// stages begin and leaves twelve fp32 values where the command was.
// ground_reduce_kernel: what the closed loop keeps of the ground over the periods (R; plant_ground_reduce), from the same inputs
// as the feedback kernel of period s -- controls[b, 0, :], row 0 of the contact table, mu -- through the same plant_ground, so
// that its flags are the recorded ones bit for bit.  It reads nothing the feedback kernel writes.
__global__ void __launch_bounds__(256, 3)
plant_step_ground_kernel(const PlantParams P, const PlantBody Bd, const PlantGround Gr, const PlantScheme S, const int B,
                         const float* __restrict__ x_fb, const float* __restrict__ u0, const float* __restrict__ foot,
                         const uint8_t* __restrict__ contact0, const float* __restrict__ wrench, float* __restrict__ x_next) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  plant_step_ground_instance(P, Bd, Gr, S, b, x_fb, u0, foot, contact0, wrench, x_next);
}

__global__ void __launch_bounds__(256, 3)
simulate_ground_feedback_kernel(const PlantParams P, const PlantBody Bd, const PlantOutcome O, const PlantGround Gr, const int s,
                                const PlantScheme S, const PlantGait G, const int B, const float* __restrict__ controls,
                                const uint8_t* __restrict__ contact, const int32_t* __restrict__ iters,
                                const int32_t* __restrict__ status, const float* __restrict__ push, const float* __restrict__ x_cmd,
                                float* __restrict__ x_fb, float* foot, double* __restrict__ t, float* __restrict__ u0_out,
                                float* __restrict__ x_out, float* __restrict__ foot_out, int32_t* __restrict__ iters_out,
                                int32_t* __restrict__ status_any) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  feedback_ground_instance(P, Bd, O, Gr, s, S, G, b, controls, contact, iters, status, push, x_cmd, x_fb, foot, t, u0_out, x_out,
                           foot_out, iters_out, status_any);
}

__global__ void __launch_bounds__(256)
ground_reduce_kernel(const double* __restrict__ mu, const double mu_h, const PlantGroundSum R, const int s, const int B, const int h,
                     const float* __restrict__ controls, const uint8_t* __restrict__ contact) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* u0 = controls + (size_t)b * h * 12;
  const uint8_t* row0 = contact + (size_t)b * h * 2;
  float u[12], ua[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) u[i] = u0[i];
  uint8_t fl;
  float demand;
  plant_ground(u, row0[0] != 0, row0[1] != 0, mu ? mu[(size_t)b * 2] : mu_h, mu ? mu[(size_t)b * 2 + 1] : mu_h, R.fz_floor, ua, fl, demand);
  // (the entry initialised the four arrays on the stream: -1, 0, 0, NaN)
  int32_t first = R.first_slip ? R.first_slip[b] : 0;
  int32_t sl[2] = {0, 0}, un[2] = {0, 0};
  if (R.slip_periods) { sl[0] = R.slip_periods[(size_t)b * 2]; sl[1] = R.slip_periods[(size_t)b * 2 + 1]; }
  if (R.unloaded_periods) { un[0] = R.unloaded_periods[(size_t)b * 2]; un[1] = R.unloaded_periods[(size_t)b * 2 + 1]; }
  float dm = R.mu_demand ? R.mu_demand[b] : 0.f;
  plant_ground_reduce(fl, demand, s, first, sl, un, dm);
  if (R.first_slip) R.first_slip[b] = first;
  if (R.slip_periods) { R.slip_periods[(size_t)b * 2] = sl[0]; R.slip_periods[(size_t)b * 2 + 1] = sl[1]; }
  if (R.unloaded_periods) { R.unloaded_periods[(size_t)b * 2] = un[0]; R.unloaded_periods[(size_t)b * 2 + 1] = un[1]; }
  if (R.mu_demand) R.mu_demand[b] = dm;
}

}  // namespace bmpc
#endif
#endif
