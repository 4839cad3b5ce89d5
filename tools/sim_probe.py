#!/usr/bin/env python3
"""What the closed loop on the plant costs next to the roll-out, and how many instances survive a push.  B = 4096, h = 10, K = 20,
walking, warm start shift 1, on the same box in the same process: per-period milliseconds of `simulate_device` (RK4, 4 substeps)
and of `rollout_device`, interleaved over `reps` repetitions (median), then the share of instances whose height stays above 0.3 m
after a 40 N lateral push of 3 periods.  Measured, not gated.  Usage: python tools/sim_probe.py [batch] [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from biped_mpc_py_amd import BatchSolver  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    K = 20
    s = BatchSolver(max_batch=B)
    rng = np.random.default_rng(5)
    x0 = np.zeros((B, 12), np.float32)
    x0[:, 5] = 0.55 + rng.uniform(-0.02, 0.02, B)
    x0[:, 0:3] = rng.uniform(-0.03, 0.03, (B, 3))
    x0[:, 9:12] = rng.uniform(-0.05, 0.05, (B, 3))
    foot0 = np.tile(np.array([-0.0195, 0.089, 0, -0.0195, -0.089, 0], np.float32), (B, 1))
    t0 = rng.integers(0, 10, B) * 0.04 + 0.01
    s.set_warm_start(True, shift=1)

    def run(which, **kw):
        x, f, t = (torch.from_numpy(a.copy()).cuda() for a in (x0, foot0, t0))
        s.reset_warm_start()
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        r = getattr(s, which)(x, f, t, K, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t_a) * 1e3 / K, r

    ms = {"rollout_device": [], "simulate_device": []}
    for which in ms:                                   # warm-up: allocations, code objects
        run(which)
    for _ in range(reps):
        for which in ms:
            ms[which].append(run(which)[0])
    for which, v in ms.items():
        print(f"{which}: {np.median(v):.3f} ms per period (median of {reps}; min {min(v):.3f}, max {max(v):.3f}), B = {B}, K = {K}")
    push = torch.zeros((B, 6), dtype=torch.float32, device="cuda")
    push[:, 1] = 40.0
    for name, kw in (("no push", {}), ("40 N lateral, periods 5-7", dict(push=push, push_from=5, push_steps=3))):
        _, r = run("simulate_device", **kw)
        z = r["x"][:, :, 5]
        alive = (torch.nan_to_num(z, nan=0.0) > 0.3).all(0)
        print(f"{name}: {100.0 * alive.float().mean().item():.2f} % of {B} instances keep p_z > 0.3 m over {K} periods; "
              f"status_any != 0 on {int((r['status_any'] != 0).sum())}")


if __name__ == "__main__":
    main()
