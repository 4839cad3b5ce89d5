#!/usr/bin/env python3
"""Duration of one `plant_rollout_grad_device` launch next to one `plant_rollout_samples_device` launch on the same inputs, each
taken with one HIP event pair around the call on torch's current stream: python tools/rollout_grad_timing.py [B S h substeps]
(default 256 64 10 4, RK4).  Walking instances of `synth_batch`, plans = stance-gated noise around a weight-bearing nominal.  The
median of `--reps` launches after `--warmup` is printed as one JSON line; the figures are reported, not asserted (docs/history_r26.md)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dims", nargs="*", type=int, default=[256, 64, 10, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, S, h, substeps = a.dims
    import torch
    import __graft_entry__ as ge
    ge.build()
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd.synth import synth_batch
    mpc = bm.MPC()
    mpc.h = h
    s = bm.BatchSolver(mpc=mpc, biped=bm.Biped(), max_batch=B)
    g = synth_batch(B, h, 3, gait="walking", vx_cmd=True)
    rng = np.random.default_rng(1)
    con = g["contact"].astype(np.float64)
    nominal = np.zeros((B, h, 12))
    for leg in range(2):
        nominal[:, :, 3 * leg + 2] = con[:, :, leg] * 12.0 * 9.81 / np.maximum(con.sum(2), 1.0)
    noise = rng.normal(0, 1.0, (B, S, h, 12)) * con[:, None, :, [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]]      # [f1 f2 m1 m2] by leg
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v.astype(dt))).cuda()
    x, f, c, u = dev(g["x_fb"], np.float32), dev(g["foot"], np.float32), dev(g["contact"], np.uint8), dev(nominal[:, None] + noise, np.float32)
    kw = dict(integrator="rk4", substeps=substeps)

    def median_ms(call):
        out = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                out.append(e0.elapsed_time(e1))
        return float(np.median(out))

    want_g = ["cost", "grad_u", "grad_x0", "grad_foot"]
    fwd = median_ms(lambda: s.plant_rollout_samples_device(x, f, c, u, want=["cost"], **kw))
    grad = median_ms(lambda: s.plant_rollout_grad_device(x, f, c, u, want=want_g, **kw))
    bad = int((s.plant_rollout_grad_device(x, f, c, u, want=["first_bad"], **kw)["first_bad"] >= 0).sum())
    print(json.dumps(dict(B=B, S=S, h=h, integrator="rk4", substeps=substeps, rollout_samples_ms=round(fwd, 4), rollout_grad_ms=round(grad, 4),
                          ratio=round(grad / fwd, 2), bad_plans=bad, reps=a.reps)))
    s.close()


if __name__ == "__main__":
    main()
