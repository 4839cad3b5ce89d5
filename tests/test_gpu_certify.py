"""KKT certificate on the MI355X (`bmpc_certify`, `bmpc_certify_device`, `BatchSolver.solve(certify=True)`) against the yardstick of
tests/certify_cases.py read from tests/golden/certify.npz (the oracle's matrices and SciPy's NNLS; neither is needed here), against
the merged evaluation and gradient, on the solver's own answers, behind a solve on one stream, and timed next to the gradient.

`python -m tests.test_gpu_certify --dump FILE` solves every instance of cfg2 / cfg4 with both kernel families and writes
their controls to FILE, for `python -m tests.gen_certify --solver-controls FILE` to put their yardstick into the fixture."""
import functools

import numpy as np
import pytest

from tests import certify_cases as cc
from tests import eval_cases as ec
from tests import util
from tests import gpu_common
from tests.gpu_common import (  # noqa: F401 (_built: the autouse fixture)
    built as _built, dev_args as _dev_args, solver as _solver, synth_group as _synth_group)

pytestmark = pytest.mark.gpu

KEYS = cc.KEYS
_identical = functools.partial(gpu_common.identical, keys=KEYS)
FAMILIES = {"solver_dense": 1, "solver_stage": 2}            # bmpc_params.path
SOLVER_SETS = ("cfg2_standing_h10", "cfg4_walking_h10")


@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture()


def _both(solver, a, act_tol):
    """The host entry and the device entry on the same arguments: NumPy dicts."""
    import torch
    host = solver.certify(**a, act_tol=act_tol)
    dev = solver.certify_device(**_dev_args(a), act_tol=act_tol)
    torch.cuda.synchronize()
    return host, {k: dev[k].cpu().numpy() for k in KEYS}


def test_optima_and_worse_plans_match_the_yardstick_through_both_entries(fx):
    """Cases 1 and 3: the oracle's optima and their perturbations through `certify` against the fixture within
    certify_cases.REL_BOUND (the bound fixed from the emulation); `certify_device` bit-identical to it; lam against solve_qp's on
    the unique rows; the perturbed plan certifies worse on every instance."""
    worst = {}
    for g in cc.optimum_groups():
        solver = _solver(g)
        res = {}
        for kind in ("opt", "pert"):
            ref = cc.expected(fx, g["name"], kind)
            gg = dict(g, controls=ref["controls"].astype(np.float64))
            host, dev = _both(solver, ec.kernel_args(gg), ref["act_tol"])
            d = cc.check(host, ref, f"{g['name']}/{kind}")
            worst.update({k: max(v, worst.get(k, 0.0)) for k, v in d.items()})
            _identical(host, dev, g["name"])
            res[kind] = host
        solver.close()
        q = cc.qp_deviation(res["opt"]["lam"], cc.expected(fx, g["name"], "opt"))
        print("certify lam against solve_qp", g["name"], "%.3e" % q.max(), "bound %.3e" % cc.QP_REL_BOUND)
        worst["lam_qp"] = max(float(q.max()), worst.get("lam_qp", 0.0))
        assert q.max() <= cc.QP_REL_BOUND, (g["name"], q.max())
        cc.assert_worse(g, cc.expected(fx, g["name"], "pert")["controls"], res["opt"], res["pert"])
    print("certify worst deviations over all sets:", " ".join(f"{k}={v:.3e}" for k, v in worst.items()))


def test_no_active_rows_gives_the_gradient_back():
    """Case 2: act_tol = -1: lam all zero, resid bit-identical to `evaluate_grad`'s grad_u, primal_ineq to the maximum of
    `evaluate`'s four violations."""
    for g in cc.optimum_groups():
        solver = _solver(g)
        a = ec.kernel_args(g)
        host, dev = _both(solver, a, -1.0)
        gu = solver.evaluate_grad(**a)["grad_u"]
        viol = solver.evaluate(**a)["violation"]
        solver.close()
        _identical(host, dev, g["name"])
        assert not host["lam"].any() and not host["n_active"].any() and not host["status"].any(), g["name"]
        assert np.array_equal(host["resid"], gu), g["name"]
        assert np.array_equal(host["summary"][:, 1], viol.max(1)), g["name"]
        assert np.array_equal(host["summary"][:, 0], np.abs(gu).reshape(gu.shape[0], -1).max(1)), g["name"]


@pytest.mark.parametrize("h", [10, 20, 40])
def test_result_does_not_depend_on_the_batch(h):
    """Case 4: alone and inside a shuffled batch of 200, identical bits in every output."""
    g, perm = cc.batch_group(h)
    solver = _solver(g, max_batch=200)
    full = solver.certify(**ec.kernel_args(g, perm))
    assert (full["status"] == 0).all() and (full["n_active"] > 0).all()
    for pos in cc.BATCH_POSITIONS:
        one = solver.certify(**ec.kernel_args(g, perm[pos:pos + 1]))
        for k in KEYS:
            assert np.array_equal(one[k][0], full[k][pos]), (pos, k)
    solver.close()


def test_bad_instances_get_nan_and_touch_nobody():
    """Case 5: the spoiled instances give NaN / -1 / 2, the clean ones the clean batch's bits, through both entries."""
    clean, bad, idx = ec.bad_batch()
    solver = _solver(clean)
    a, _ = _both(solver, ec.kernel_args(clean), 1e-4)
    b, bd = _both(solver, ec.kernel_args_unchecked(bad), 1e-4)
    solver.close()
    _identical(b, bd)
    ok = [i for i in range(8) if i not in idx]
    for k in ("lam", "resid", "summary"):
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    assert (b["n_active"][idx] == -1).all() and (b["status"][idx] == 2).all()
    assert np.array_equal(a["n_active"][ok], b["n_active"][ok]) and (b["status"][ok] == 0).all() and (a["status"] == 0).all()


def _solve_set(name, family, **kw):
    g = next(x for x in cc.optimum_groups() if x["name"] == name)
    solver = _solver(g, FAMILIES[family])
    assert solver._lib.bmpc_solver_path(solver._h) == FAMILIES[family]
    inp = {k: v for k, v in ec.kernel_args(g).items() if k != "controls"}
    _, controls, info = solver.solve(**inp, **kw)
    assert (info["status"] == 0).all()
    return g, solver, inp, controls, info


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("name", SOLVER_SETS)
def test_solve_with_certify_and_the_solvers_own_answers(fx, name, family):
    """Case 7: `solve(..., certify=True)` puts into info["kkt"] what `certify` gives on the returned controls, bit for bit; the
    certificate of the solver's controls recorded in the fixture matches the fixture's yardstick for those controls."""
    ref = cc.expected(fx, name, family)
    g, solver, inp, controls, info = _solve_set(name, family, certify=True, act_tol=ref["act_tol"])
    again = solver.certify(**inp, controls=controls, act_tol=ref["act_tol"])
    for k, v in info["kkt"].items():
        assert np.array_equal(v, again[k]), (name, family, k)
    assert set(info["kkt"]) == {"stationarity", "primal_ineq", "complementarity", "grad_scale", "n_active", "status", "lam"}
    got = solver.certify(**inp, controls=ref["controls"].astype(np.float64), act_tol=ref["act_tol"])
    solver.close()
    print("solver controls of this run equal the fixture's:", bool(np.array_equal(controls.astype(np.float32), ref["controls"])),
          "rel err %.2e" % util.rel_err(controls, ref["controls"].astype(np.float64)).max())
    cc.check(got, ref, f"{name}/{family}")
    rel = got["summary"][:, 0] / got["summary"][:, 3]
    print("solver stationarity / grad_scale", name, family, "act_tol %g:" % ref["act_tol"], " ".join("%.2e" % v for v in np.sort(rel)))


@pytest.mark.parametrize("h,gait", [(10, "standing"), (10, "walking"), (20, "walking")])
@pytest.mark.parametrize("path", [1, 2])
def test_distribution_on_the_solvers_own_answers(h, path, gait):
    """Recorded in docs/history_r11.md, not asserted beyond sanity: stationarity / grad_scale of the solver's answers over a
    4096-instance batch under the default act_tol."""
    B = 4096
    g = _synth_group(B, h, gait, 700 + h)
    solver = _solver(g, path, B)
    inp = {k: v for k, v in ec.kernel_args(g).items() if k != "controls"}
    _, controls, info = solver.solve(**inp, certify=True)
    solver.close()
    k = info["kkt"]
    rel = k["stationarity"] / k["grad_scale"]
    qs = np.quantile(rel, [0.0, 0.5, 0.9, 0.99, 1.0])
    print("solver certificate h=%d path=%d %s B=%d: stationarity / grad_scale min %.2e median %.2e p90 %.2e p99 %.2e max %.2e; "
          "primal_ineq max %.2e complementarity max %.2e n_active %d..%d status counts %s"
          % (h, path, gait, B, *qs, k["primal_ineq"].max(), k["complementarity"].max(), k["n_active"].min(), k["n_active"].max(),
             np.bincount(k["status"], minlength=3)))
    assert np.isfinite(rel).all() and (k["status"] <= 1).all() and (k["lam"] >= 0).all()


def test_queued_behind_a_solve_on_the_same_stream():
    """`solve_device` then `certify_device` with that call's `controls` tensor on one stream, nothing synchronised in between,
    gives the bits of the host entry on the solve's controls."""
    import torch
    g = _synth_group(1024, 10, "walking", 3)
    solver = _solver(g, 0, 1024)
    a = ec.kernel_args(g)
    d_in = {k: v for k, v in _dev_args(a).items() if k != "controls"}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        u_dev, _ = solver.solve_device(**d_in)
        ce = solver.certify_device(**d_in, controls=u_dev)
    st.synchronize()
    host = solver.certify(**dict(a, controls=u_dev.cpu().numpy()))
    _identical(host, {k: ce[k].cpu().numpy() for k in KEYS})
    assert np.isfinite(host["resid"]).all() and host["lam"].max() > 0
    solver.close()


def test_time_of_one_launch_next_to_the_gradient():
    """Recorded in docs/history_r11.md, not asserted: HIP events around single `certify_device` and `evaluate_grad_device` launches
    at B = 4096, h = 10 on a solver's own controls, interleaved in one process after warm-up, 5 brackets of 21 pairs each; the
    median of the brackets' medians (the method of the gradient's figure in docs/history_r10.md)."""
    import torch
    B, h = 4096, 10
    g = _synth_group(B, h, "standing", 1)
    solver = _solver(g, 0, B)
    d = _dev_args(ec.kernel_args(g))
    d_in = {k: v for k, v in d.items() if k != "controls"}
    u, _ = solver.solve_device(**d_in)
    co = solver.certify_device(**d_in, controls=u)
    go = solver.evaluate_grad_device(**d_in, controls=u)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    f_cert = lambda: solver.certify_device(**d_in, controls=u, **co)
    f_grad = lambda: solver.evaluate_grad_device(**d_in, controls=u, cost=go["cost"], grad_u=go["grad_u"], grad_x0=go["grad_x0"])
    for _ in range(5):
        f_cert(); f_grad()
    torch.cuda.synchronize()
    meds = []
    for _ in range(5):
        tc, tg = [], []
        for _ in range(21):
            tc.append(timed(f_cert))
            tg.append(timed(f_grad))
        meds.append((float(np.median(tc)), float(np.median(tg))))
    mc, mg = float(np.median([m[0] for m in meds])), float(np.median([m[1] for m in meds]))
    print("certify_device B=%d h=%d: %.1f us, evaluate_grad_device %.1f us, ratio %.2f; brackets (certify, grad) us: %s; n_active mean %.1f"
          % (B, h, mc, mg, mc / mg, " ".join("(%.1f, %.1f)" % m for m in meds), float(co["n_active"].double().mean())))
    assert mc > 0 and mg > 0
    solver.close()


def _dump(path):
    import __graft_entry__ as ge
    ge.build()
    out = {}
    for name in SOLVER_SETS:
        for family in sorted(FAMILIES):
            _, solver, _, controls, _ = _solve_set(name, family)
            solver.close()
            out[f"{name}/{family}"] = controls.astype(np.float32)
    np.savez(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    _dump(ap.parse_args().dump)
