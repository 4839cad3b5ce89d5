"""Gradient of the evaluated cost on the MI355X (`bmpc_evaluate_grad`, `bmpc_evaluate_grad_device`, `BatchSolver.cost_torch`) against the
oracle's matrices (tests/eval_grad_cases.py `yardstick`), against the merged evaluation, behind a solve, through autograd, on the
solver's own optima at scale, and timed next to the evaluation."""
import functools

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import eval_grad_cases as gc
from tests import util
from tests import gpu_common
from tests.gpu_common import (  # noqa: F401 (_built: the autouse fixture)
    built as _built, dev_args as _dev_args, solver as _solver, synth_group as _synth_group)

pytestmark = pytest.mark.gpu

KEYS = gc.KEYS
_identical = functools.partial(gpu_common.identical, keys=KEYS)


def _both(solver, a):
    """The host entry and the device entry on the same arguments, and the merged evaluation's device cost: NumPy dicts."""
    import torch
    host = solver.evaluate_grad(**a)
    d = _dev_args(a)
    dev = solver.evaluate_grad_device(**d)
    ev = solver.evaluate_device(**d)
    torch.cuda.synchronize()
    return host, {k: dev[k].cpu().numpy() for k in KEYS}, ev["cost"].cpu().numpy()


def test_case_sets_against_the_yardstick_through_both_entries():
    """Tests 8 / 9, CPU case 1: every case set through `evaluate_grad` against the yardstick; `evaluate_grad_device` bit-identical to
    it; `cost` bit-identical to `evaluate_device`'s."""
    for g in gc.all_groups():
        solver = _solver(g)
        host, dev, ev_cost = _both(solver, ec.kernel_args(g))
        solver.close()
        gc.check(host, gc.yardstick_group(g), g["name"])
        _identical(host, dev, g["name"])
        assert np.array_equal(host["cost"], ev_cost), g["name"]


@pytest.mark.parametrize("h", [10, 20, 40])
def test_result_does_not_depend_on_the_batch(h):
    """Test 8, CPU case 2: alone and inside a shuffled batch of 200, identical bits in every output."""
    g, perm = gc.batch_group(h)
    solver = _solver(g, max_batch=200)
    full = solver.evaluate_grad(**ec.kernel_args(g, perm))
    for pos in gc.BATCH_POSITIONS:
        one = solver.evaluate_grad(**ec.kernel_args(g, perm[pos:pos + 1]))
        for k in KEYS:
            assert np.array_equal(one[k][0], full[k][pos]), (pos, k)
    solver.close()
    gc.check({k: v[:8] for k, v in full.items()}, gc.yardstick_group(g, perm[:8]), f"batch200_h{h}")


def test_bad_instances_get_nan_and_touch_nobody():
    """Test 8, CPU case 3, through both entries."""
    clean, bad, idx = ec.bad_batch()
    solver = _solver(clean)
    a, a_dev, a_cost = _both(solver, ec.kernel_args(clean))
    b, b_dev, b_cost = _both(solver, ec.kernel_args_unchecked(bad))
    solver.close()
    _identical(a, a_dev)
    _identical(b, b_dev)
    assert np.array_equal(b["cost"], b_cost, equal_nan=True)
    ok = [i for i in range(8) if i not in idx]
    for k in KEYS:
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k


def test_gradient_is_the_difference_of_the_merged_evaluation():
    """Test 8, CPU case 4: (cost(U + D) - cost(U - D)) / 2 of `evaluate` equals grad_u . D of `evaluate_grad`; second difference >= 0."""
    groups = ec.ref_tracking_groups() + [g for g in ec.horizon_groups() if g["h"] in (1, 13, 40)] + ec.generated_groups()[-1:]
    for n, g in enumerate(groups):
        U, D = gc.grid_pair(g, 4000 + n)
        solver = _solver(g)
        a = ec.kernel_args(g)
        cost_of = lambda c: solver.evaluate(**dict(a, controls=c))["cost"]
        gc.check_identity(cost_of, solver.evaluate_grad(**dict(a, controls=U))["grad_u"], g, U, D, g["name"])
        solver.close()


def test_queued_behind_a_solve_on_the_same_stream():
    """Test 10: `solve_device` then `evaluate_grad_device` with that call's `controls` tensor on one stream, nothing synchronised in
    between, gives the bits of the host entry on the solve's controls."""
    import torch
    g = _synth_group(1024, 10, "walking", 3)
    solver = _solver(g, 0, 1024)
    a = ec.kernel_args(g)
    d_in = {k: v for k, v in _dev_args(a).items() if k != "controls"}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        u_dev, _ = solver.solve_device(**d_in)
        gr = solver.evaluate_grad_device(**d_in, controls=u_dev)
    st.synchronize()
    host = solver.evaluate_grad(**dict(a, controls=u_dev.cpu().numpy()))
    _identical(host, {k: gr[k].cpu().numpy() for k in KEYS})
    assert np.isfinite(host["grad_u"]).all() and np.abs(host["grad_u"]).max() > 0
    solver.close()


def test_cost_torch_backward():
    """Test 11: `cost_torch(...).sum().backward()` leaves the float32 casts of grad_u / grad_x0 in controls.grad / x_fb.grad; a
    weighted sum scales them per instance; no input tensor is modified; a second forward / backward gives the same bits."""
    import torch
    g = ec.ref_tracking_groups()[1]
    B = g["x_fb"].shape[0]
    solver = _solver(g)
    d = _dev_args(ec.kernel_args(g))
    before = {k: None if v is None else v.clone() for k, v in d.items()}
    ref = solver.evaluate_grad_device(**d)
    rest = {k: v for k, v in d.items() if k not in ("x_fb", "controls")}

    def run(weights=None):
        u = d["controls"].clone().requires_grad_(True)
        x = d["x_fb"].clone().requires_grad_(True)
        cost = solver.cost_torch(x, rest["foot"], rest["contact"], rest["phase"], u, x_cmd=rest["x_cmd"], mu=rest["mu"], x_ref=rest["x_ref"],
                                 foot_ref=rest["foot_ref"])
        assert cost.dtype == torch.float64 and tuple(cost.shape) == (B,) and cost.requires_grad
        (cost.sum() if weights is None else (cost * weights).sum()).backward()
        assert u.grad.dtype == torch.float32 and x.grad.dtype == torch.float32
        assert torch.equal(u.detach(), d["controls"]) and torch.equal(x.detach(), d["x_fb"])
        return cost.detach(), u.grad, x.grad

    c1, gu1, gx1 = run()
    assert torch.equal(c1, ref["cost"])
    assert torch.equal(gu1, ref["grad_u"].to(torch.float32)) and torch.equal(gx1, ref["grad_x0"].to(torch.float32))
    c2, gu2, gx2 = run()
    assert torch.equal(c1, c2) and torch.equal(gu1, gu2) and torch.equal(gx1, gx2)
    w = torch.linspace(-2.0, 3.0, B, dtype=torch.float64, device="cuda")
    _, guw, gxw = run(w)
    assert torch.equal(guw, (w[:, None, None] * ref["grad_u"]).to(torch.float32))
    assert torch.equal(gxw, (w[:, None] * ref["grad_x0"]).to(torch.float32))
    u = d["controls"].clone().requires_grad_(True)           # only one of the two asks for a gradient
    solver.cost_torch(d["x_fb"], rest["foot"], rest["contact"], rest["phase"], u, x_ref=rest["x_ref"], foot_ref=rest["foot_ref"],
                      x_cmd=rest["x_cmd"]).sum().backward()
    assert torch.equal(u.grad, gu1) and d["x_fb"].grad is None
    for k, v in d.items():
        assert v is None or torch.equal(v, before[k]), k
    solver.close()


@pytest.mark.parametrize("h", [10, 16, 20])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("gait", ["standing", "walking"])
def test_the_solvers_own_optima_satisfy_the_variational_inequality(h, path, gait):
    """Test 12: -(grad_u . U) / max(1, cost) >= -OPT_TOL_SOLVER[h] for EVERY instance of a 4096-instance batch solved by either kernel
    family at the default bounds (u = 0 feasible: V = 0 in g . (V - U) >= 0)."""
    B = 4096
    g = _synth_group(B, h, gait, 700 + h)
    solver = _solver(g, path, B)
    assert solver._lib.bmpc_solver_path(solver._h) == path
    a = ec.kernel_args(g)
    inp = {k: v for k, v in a.items() if k != "controls"}
    _, controls, info = solver.solve(**inp)
    assert (info["status"] == 0).all(), np.bincount(info["status"])
    r = solver.evaluate_grad(**inp, controls=controls)
    solver.close()
    q = gc.optimality(r["grad_u"], controls, r["cost"])
    print("solver optimality h=%d path=%d %s: min %.3e median %.3e max %.3e, cost %.3g .. %.3g, tol %.1e"
          % (h, path, gait, q.min(), np.median(q), q.max(), r["cost"].min(), r["cost"].max(), gc.OPT_TOL_SOLVER[h]))
    assert np.isfinite(q).all()
    assert (q >= -gc.OPT_TOL_SOLVER[h]).all(), (int((q < -gc.OPT_TOL_SOLVER[h]).sum()), q.min())


def test_time_of_one_launch_next_to_the_evaluation():
    """Test 13 (recorded in docs/history_r10.md, not asserted): HIP events around single `evaluate_grad_device` and `evaluate_device`
    launches at B = 4096, h = 10, interleaved in one process, 5 brackets of 21 pairs each; the median of the brackets' medians."""
    import torch
    B, h = 4096, 10
    g = _synth_group(B, h, "standing", 1)
    solver = _solver(g, 0, B)
    d = _dev_args(ec.kernel_args(g))
    d_in = {k: v for k, v in d.items() if k != "controls"}
    u, _ = solver.solve_device(**d_in)
    go = solver.evaluate_grad_device(**d_in, controls=u)
    eo = solver.evaluate_device(**d_in, controls=u)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    f_grad = lambda: solver.evaluate_grad_device(**d_in, controls=u, cost=go["cost"], grad_u=go["grad_u"], grad_x0=go["grad_x0"])
    f_eval = lambda: solver.evaluate_device(**d_in, controls=u, cost=eo["cost"], objective=eo["objective"], violation=eo["violation"])
    for _ in range(5):
        f_grad(); f_eval()
    torch.cuda.synchronize()
    meds = []
    for _ in range(5):
        tg, te = [], []
        for _ in range(21):
            tg.append(timed(f_grad))
            te.append(timed(f_eval))
        meds.append((float(np.median(tg)), float(np.median(te))))
    mg, me = float(np.median([m[0] for m in meds])), float(np.median([m[1] for m in meds]))
    print("evaluate_grad_device B=%d h=%d: %.1f us, evaluate_device %.1f us, ratio %.2f; brackets (grad, eval) us: %s"
          % (B, h, mg, me, mg / me, " ".join("(%.1f, %.1f)" % m for m in meds)))
    assert mg > 0 and me > 0
    solver.close()
