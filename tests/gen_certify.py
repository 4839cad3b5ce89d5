"""Generates tests/golden/certify.npz and tests/golden/certify_<set>_<kind>.npz (certify_cases.fixture_file): the yardstick of the certificate tests (tests/certify_cases.py) for every case set, from the
oracle and SciPy's NNLS.  Numeric arrays only.

    python -m tests.gen_certify                          # the oracle's optima and their perturbations
    python -m tests.gen_certify --solver-controls FILE   # also the `solver_*` entries: the yardstick of the SOLVER's own controls,
                                                         # which FILE (an .npz written by test_gpu_certify.py --dump, see there)
                                                         # brings from a machine with a GPU
    python -m tests.gen_certify --measure                # additionally runs the kernel's source on the CPU (tests/emu) and prints
                                                         # the largest deviations: the figures behind certify_cases.MEASURED_*

Without --solver-controls the controls of the `solver_*` entries of the existing files are read back and their yardstick is formed
again.  A regeneration reproduces the unique quantities (resid, summary, lam on unique rows) to rounding (1e-14 relative: BLAS
thread counts change summation orders); lam on rows whose multiplier is not unique, and lam_qp there, may come out as another valid
split, which no test compares.
Per case set (a golden set with one kind of controls: optimum, perturbed, a solver family's) it picks ONE act_tol.  Optimum and
solver's controls: the first of certify_cases.ACT_TOL_CANDIDATES for which no slack of any instance lies within a factor 2 of its
threshold; asserted to exist.  Perturbed controls: the same if one exists, else the candidate with the largest margin, asserted to be
at least certify_cases.PERT_MIN_MARGIN (why the factor 2 cannot hold there: certify_cases).  Every instance of every set is kept."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import certify_cases as cc          # noqa: E402
from tests import eval_cases as ec             # noqa: E402

ARRAYS = ("lam", "resid", "summary", "n_active", "active", "indep")


def pick_act_tol(mats, U, where, perturbed):
    """(act_tol, its margin over all instances)."""
    seen = []
    for tol in cc.ACT_TOL_CANDIDATES:
        m = min(cc.margin(mats[i], U[i], tol) for i in range(len(mats)))
        seen.append((m, tol))
        if m >= 2.0:
            print(f"  {where}: act_tol {tol:g} margin {m:.3g}")
            return tol, m
    m, tol = max(seen)
    print(f"  {where}: NO candidate keeps the factor 2; margins " + " ".join(f"{t:g}: {v:.6g}" for v, t in seen) + f"; taking {tol:g}")
    assert perturbed, f"{where}: no candidate act_tol keeps every slack a factor 2 away from its threshold"
    assert m >= cc.PERT_MIN_MARGIN, (where, m)
    return tol, m


def stack(ys):
    return {k: np.stack([np.asarray(y[k]) for y in ys]) for k in ARRAYS + ("slack",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver-controls")
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--sets", nargs="*", help="only these golden sets ('small': all that share the main file); files of other sets stay")
    args = ap.parse_args()
    files = {}                                 # path -> arrays to write
    kept = {}                                  # "<set>/solver_<family>/controls" of the existing files: inputs, written nowhere as such
    if not args.solver_controls:
        for name in cc.BIG_SETS:
            for fam in ("solver_dense", "solver_stage"):
                path = cc.fixture_file(name, fam)
                if os.path.exists(path):
                    old = np.load(path)
                    kept.update({k: old[k] for k in old.files if k.endswith("/controls")})
    solver = np.load(args.solver_controls) if args.solver_controls else None
    worst, worst_qp = 0.0, 0.0
    for g in cc.optimum_groups():
        name, n = g["name"], g["controls"].shape[0]
        if args.sets and (name if name in cc.BIG_SETS else "small") not in args.sets:
            continue
        print(name, "h", g["h"], "n", n, flush=True)
        mats = [cc.condensed(g, i) for i in range(n)]
        sets = {"opt": g["controls"], "pert": cc.perturbed(g, cc.pert_seed(name))}
        if solver is not None:
            sets.update({k.split("/")[1]: solver[k].astype(np.float64) for k in solver.files if k.startswith(name + "/solver_")})
        else:
            sets.update({k.split("/")[1]: kept[k].astype(np.float64) for k in kept if k.startswith(name + "/solver_")})
        for kind, U in sets.items():
            out = files.setdefault(cc.fixture_file(name, kind), {})
            tol, mg = pick_act_tol(mats, U, f"{name}/{kind}", kind == "pert")
            out[f"{name}/{kind}/act_tol"] = np.float64(tol)
            out[f"{name}/{kind}/margin"] = np.float64(mg)
            ref = stack([cc.yardstick(mats[i], U[i], tol) for i in range(n)])
            for k in ARRAYS + (("slack",) if kind.startswith("solver_") else ()):
                out[f"{name}/{kind}/{k}"] = ref[k]
            out[f"{name}/{kind}/controls"] = np.asarray(U, np.float32)
            if kind == "opt":
                out[f"{name}/opt/lam_qp"] = np.stack([cc.qp_duals(m) for m in mats])
            rel = ref["summary"][:, 0] / ref["summary"][:, 3]
            print(f"  {kind}: stationarity / grad_scale max {rel.max():.3e}  n_active {ref['n_active'].min()}..{ref['n_active'].max()}"
                  f"  unique rows {int(ref['indep'].sum())} of {int(ref['active'].sum())} active", flush=True)
            if args.measure:
                import __graft_entry__ as ge
                ge.build()
                from tests.emu import emu_eval
                gg = dict(g, controls=U)
                got = emu_eval.certify(ec.cparams_of(gg), **ec.kernel_args(gg), act_tol=tol)
                dev = {k: float(v.max()) for k, v in cc.deviations(got, {k: v for k, v in ref.items() if k != "slack" or kind.startswith("solver_")}).items()}
                if not kind.startswith("solver_"):   # MEASURED_REL is taken over the sets that exist without a GPU
                    worst = max(worst, max(dev.values()))
                print("  emulation deviations", " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
                if kind == "opt":
                    q = float(cc.qp_deviation(got["lam"], dict(ref, lam_qp=out[f"{name}/opt/lam_qp"])).max())
                    worst_qp = max(worst_qp, q)
                    print(f"  emulation lam against solve_qp: {q:.3e}")
    for path, arrays in files.items():
        if not arrays:
            continue
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20, path
    if args.measure:
        print(f"MEASURED_REL = {worst:.3e}   MEASURED_QP_REL = {worst_qp:.3e}")


if __name__ == "__main__":
    main()
