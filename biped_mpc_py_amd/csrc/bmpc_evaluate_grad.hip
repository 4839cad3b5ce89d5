// bmpc_evaluate_grad.hip -- gradient of the evaluated cost (gfx950 / CDNA4): which way a control sequence gets better.
//
// Per instance, from the inputs of an evaluation (bmpc_evaluate.hip: bmpc_inputs and controls [h][12]), fp64 on the fp32 inputs
// widened:
//   cost     sum_k e_k' Q e_k + u_k' R u_k, e_k = x_{k+1} - x_ref[:, k]: the same value and bits as evaluate_kernel's
//   grad_u   [h][12]: d cost / d controls, row k = 2 R u_k + B_k' lambda_k
//   grad_x0  [12]: d cost / d x_fb THROUGH THE INITIAL CONDITION ONLY, A_0' lambda_0: references, lever arms and linearisation are
//            held fixed, whether they were supplied or generated (generated references depend on x_fb; that is not differentiated)
//
// The cost is an exact quadratic in the controls, so the gradient is one adjoint sweep.  Forward: the state recurrence of
// evaluate_kernel, through the very functions it uses (same thread map: one lane per (instance, step), groups of L = 16 / 32 / 64
// lanes, lane_read permutes only, no LDS, no barrier).  Backward: lambda_k = d cost / d x_{k+1} = 2 Q e_k + A_{k+1}' lambda_{k+1},
// nothing above k = h - 1.  A is the identity plus dt R_inv (euler <- omega) and dt I (p <- v), so the adjoint is two rounds of
// SUFFIX sums over the group, the mirror image of the forward pass: first the euler / p costates (increments 2 Q e), then the
// omega / v costates (increments 2 Q e plus dt R_inv,k+1' lambda_eul,k+1 and dt lambda_p,k+1, which lane k + 1 computes and lane k
// reads).  With w = dt I_w,k' lambda_omega (B_k' of REF:174-180): the force of leg g gets kvm lambda_v + w x r_g, its moment w.
//
// A source lane above the horizon or in the next group contributes an exact zero by a select, never by a multiply: a neighbour's
// NaN stays in its own group, as in group_prefix.  Bad instances (bmpc_evaluate.hip) get NaN in every output.
//
// Compiles as plain C++ for tests/emu (BMPC_EMU) like bmpc_evaluate.hip.
#ifndef BMPC_EVALUATE_GRAD_HIP
#define BMPC_EVALUATE_GRAD_HIP

#include "bmpc_evaluate.hip"

namespace bmpc {

struct GradOut {             // all nullable, fp64, device pointers
  double* cost;              // [B]
  double* grad_u;            // [B][h][12]
  double* grad_x0;           // [B][12]
};

// inclusive suffix sum over the lane's group of L lanes (gl = place in the group), N values at once: group_prefix mirrored, shifts
// 1, 2, 4 ... L / 2.  A lane whose source would lie above its group adds an exact zero (a select: a neighbour group's NaN stays there).
template <int N>
__device__ __forceinline__ void group_suffix(double (&v)[N], const int lane, const int gl, const int L) {
  for (int sh = 1; sh < L; sh <<= 1) {
    const int src = (lane + sh) & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double o = lane_read(v[i], src);
      v[i] += gl + sh < L ? o : 0.0;
    }
  }
}

__global__ void __launch_bounds__(EVAL_NT)
evaluate_grad_kernel(const EvalParams P, const int B,
                     const float* __restrict__ x_fb, const float* __restrict__ foot,
                     const uint8_t* __restrict__ contact, const int32_t* __restrict__ phase,
                     const float* __restrict__ x_cmd, const float* __restrict__ mu_in,
                     const float* __restrict__ x_ref, const float* __restrict__ foot_ref,
                     const float* __restrict__ controls, const GradOut out) {
  const EvalLane t = eval_lane(P.h, B);
  const int L = t.L, lane = t.lane, gl = t.gl;
  const double dt = P.dt;

  // ---- forward: exactly evaluate_kernel's
  EvalStep s;
  eval_load(P, t, x_fb, foot, contact, phase, x_cmd, mu_in, x_ref, foot_ref, controls, s);
  double inc[6], x[12];                        // x = state after step k
  eval_step_model(P, s, inc);
  eval_recurrence(P, t, s, inc, x);
  const int bad = eval_bad(t, s, x);
  double cost[1] = {0.0};
  eval_step_cost(P, s, x, cost[0]);
  if (!t.live) cost[0] = 0.0;
  group_sum<1>(cost, lane, L);

  // (From here to the stores: bmpc_certify.hip holds this backward pass a second time, statement for statement, as eval_adjoint --
  //  sharing one function moved this kernel's `cost` by an ulp.  An edit here goes there too; tests/test_gpu_certify.py compares the bits.)
  // ---- backward, round 1: lambda_eul, lambda_p = suffix sums of 2 Q e  (lanes past the horizon hold clones: zero by a select)
  double lam[12];                              // lambda_k in the order of the state: euler, p, omega, v
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double ge = 2.0 * P.Q[i] * (x[i] - s.xr[i]);
    lam[i] = t.live ? ge : 0.0;
  }
  double lo[6] = {lam[0], lam[1], lam[2], lam[3], lam[4], lam[5]};
  group_suffix<6>(lo, lane, gl, L);
  // what A_k' sends from (lambda_eul, lambda_p) of THIS lane to (omega, v) of the lane below: dt R_inv,k' lambda_eul, dt lambda_p
  double down[6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    down[a] = dt * (s.Rv[a] * lo[0] + s.Rv[3 + a] * lo[1] + s.Rv[6 + a] * lo[2]);
    down[3 + a] = dt * lo[3 + a];
  }
  // ---- round 2: lambda_omega, lambda_v = suffix sums of 2 Q e + the lane above's `down`
  double hi[6];
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
  double gu[12];
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

  // ---- stores
  if (!t.in_batch) return;
  const double nan = __builtin_nan("");
  if (out.grad_u && t.live) {
    double* go = out.grad_u + t.row * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) go[i] = bad ? nan : gu[i];
  }
  if (gl == 0) {
    if (out.cost) out.cost[t.inst] = bad ? nan : cost[0];
    if (out.grad_x0) {                         // A_0' lambda_0: lane 0's own `down` joins its omega / v costates
      double* go = out.grad_x0 + t.inst * 12;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        go[a] = bad ? nan : lo[a];
        go[6 + a] = bad ? nan : hi[a] + down[a];
      }
    }
  }
}

}  // namespace bmpc

#endif  // BMPC_EVALUATE_GRAD_HIP
