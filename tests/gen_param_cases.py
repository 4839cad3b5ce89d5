"""Generates tests/golden/param_cases_stage.npz: the oracle's optima (`orc.solve_mpc`, fp64, on the fp32-rounded inputs) of the
stage-family parameter test -- every case of param_cases.SOLVE_CASES and the defaults at h = 7, 10, 26 on the B = 8 instances of
`param_cases.stage_batch`.  Numeric arrays only.  The h = 26 solves take 1.5 s each; 430 solves do not fit a test, so they are
made once here and tests/test_param_cases_cpu.py solves a sample again to hold the file to the oracle.

    python -m tests.gen_param_cases [--jobs N]

Every solve must converge (the active-set polish succeeded, every KKT residual <= 1e-7 absolute, at forces of order 100 N; the largest
seen is 1.1e-8, at Q_x100 and h = 26, whose Hessian is 100 x the default's): an instance that does not gets another seed in
param_cases.STAGE_SEEDS, it is never dropped.  Keys: h<h>/<case> (8,h,12) controls, h<h>/x_fb (8,12) the inputs the answers belong
to, h<h>/kkt (cases,8) the largest KKT residual of each solve."""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import param_cases as pc            # noqa: E402
from tests import util                         # noqa: E402

KKT_TOL = 1e-7


def _solve(job):
    h, name, i = job
    _, controls, info = pc.oracle_solve(pc.stage_batch(h), i, h, name, return_info=True)
    return controls, bool(info["polished"]), float(max(info["kkt"].values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    names = ["default"] + pc.SOLVE_CASES
    jobs = [(h, n, i) for h in pc.STAGE_HORIZONS for n in names for i in range(pc.STAGE_B)]
    with Pool(args.jobs) as pool:
        res = pool.map(_solve, jobs, chunksize=1)
    out = {}
    for h in pc.STAGE_HORIZONS:
        out[f"h{h}/x_fb"] = pc.stage_batch(h)["x_fb"]
        kkt = []
        for n in names:
            r = [res[k] for k, j in enumerate(jobs) if j[0] == h and j[1] == n]
            bad = [i for i, (_, polished, k) in enumerate(r) if not polished or k > KKT_TOL]
            assert not bad, f"h = {h}, case {n}: the oracle did not converge on instances {bad}: take another seed"
            out[f"h{h}/{n}"] = np.stack([c for c, _, _ in r])
            kkt.append([k for _, _, k in r])
        out[f"h{h}/kkt"] = np.array(kkt)
        print(f"h = {h}: {len(names)} cases x {pc.STAGE_B} instances, largest KKT residual {np.max(kkt):.2e}")
    path = os.path.join(util.GOLDEN, "param_cases_stage.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
