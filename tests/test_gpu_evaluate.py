"""Evaluation of given controls on the MI355X (`bmpc_evaluate`, `bmpc_evaluate_device`; include/bmpc.h ABI 13) against the oracle's
matrices (tests/eval_cases.py `yardstick`), at scale, behind a solve, and timed against the solve."""
import functools

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import refs_cases as rc
from tests import util
from tests import gpu_common
from tests.gpu_common import (  # noqa: F401 (_built: the autouse fixture)
    built as _built, dev_args as _dev_args, solver as _solver)

pytestmark = pytest.mark.gpu

KEYS = ("cost", "objective", "violation", "states")
_identical = functools.partial(gpu_common.identical, keys=KEYS)


def _both(solver, a):
    """The host entry and the device entry on the same arguments: (host result, device result as NumPy)."""
    import torch
    host = solver.evaluate(**a, want_states=True)
    dev = solver.evaluate_device(**_dev_args(a), want_states=True)
    torch.cuda.synchronize()
    return host, {k: dev[k].cpu().numpy() for k in KEYS}


def test_case_sets_against_the_yardstick_through_both_entries():
    """Cases 1-3 of tests/test_evaluate_cpu.py through `bmpc_evaluate` (host) and `bmpc_evaluate_device`: against the yardstick, and
    the two entries bit-identical to each other."""
    viol = []
    for g in ec.ref_tracking_groups() + ec.ref_tracking_groups(breaking=True) + ec.generated_groups() + ec.horizon_groups():
        solver = _solver(g)
        host, dev = _both(solver, ec.kernel_args(g))
        solver.close()
        ref = ec.yardstick_group(g)
        ec.check(host, ref, g["name"])
        _identical(host, dev, g["name"])
        if g["name"].endswith("_broken"):
            viol.append(ref["violation"])
    v = np.concatenate(viol)
    assert (v.max(0) > 1.0).all() and (v == 0.0).any()


def test_non_finite_instances_get_nan_and_touch_nobody():
    """Case 5 through both entries: NaN in all outputs of the three spoiled instances, the other five bit-identical to the clean batch."""
    clean, bad, idx = ec.bad_batch()
    solver = _solver(clean)
    a, a_dev = _both(solver, ec.kernel_args(clean))
    b, b_dev = _both(solver, ec.kernel_args_unchecked(bad))
    solver.close()
    _identical(a, a_dev)
    _identical(b, b_dev)
    ok = [i for i in range(8) if i not in idx]
    for k in KEYS:
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    ec.check(a, ec.yardstick_group(clean), "bad_batch_clean")


@pytest.mark.parametrize("h,path", [(10, 1), (20, 1), (13, 2), (32, 2)])
def test_at_scale(h, path):
    """4096 reference-tracking instances with seeded controls of the size of a solve's: 256 sampled instances against the yardstick;
    an instance of the 4096 bit-identical to itself in a batch of 1; dense- and stage-handle results bit-identical at h = 10."""
    B = 4096
    s = rc.make_batch(B, h, 500 + h, "abcde")
    rng = np.random.default_rng(h)
    g = ec._group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], ec.seeded_controls(s["contact"], rng),
                  x_ref=s["x_ref"], foot_ref=s["foot_ref"])
    solver = _solver(g, path, B)
    assert solver._lib.bmpc_solver_path(solver._h) == path
    full, dev = _both(solver, ec.kernel_args(g))
    _identical(full, dev)
    idx = np.sort(rng.choice(B, 256, replace=False))
    ec.check({k: full[k][idx] for k in KEYS}, ec.yardstick_group(g, idx), f"scale_h{h}")
    for i in (0, 1, 2047, 4095):
        one = solver.evaluate(**ec.kernel_args(g, slice(i, i + 1)), want_states=True)
        for k in KEYS:
            assert np.array_equal(one[k][0], full[k][i]), (i, k)
    solver.close()
    if h == 10:
        other = _solver(g, 2, B)
        assert other._lib.bmpc_solver_path(other._h) == 2
        _identical(full, other.evaluate(**ec.kernel_args(g), want_states=True), "dense vs stage handle")
        other.close()


def _solve_groups():
    s2 = util.synth_batch(4096, 10, 1, gait="standing")
    s4 = util.synth_batch(4096, 10, 3, gait="mixed", vx_cmd=True)
    sr = rc.make_batch(1024, 10, 41, "abcde")
    z = np.zeros((1, 10, 12))
    mk = lambda s, **kw: ec._group(10, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"],
                                   np.repeat(z, s["x_fb"].shape[0], 0), **kw)
    return [("cfg2", 0, mk(s2)), ("cfg4", 0, mk(s4)), ("refs_stage", 2, mk(sr, x_ref=sr["x_ref"], foot_ref=sr["foot_ref"]))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_solve_then_evaluate(which):
    """`solve(..., evaluate=True)`'s info equals a separate `evaluate` of the returned controls bit for bit; `solve_device` followed by
    `evaluate_device` on the same stream, nothing synchronised in between, gives those bits again; `evaluate`'s states within REL_TOL
    of the solve's; every violation at most 2e-3 (the feasibility tolerance test_baseline_config_shapes_at_scale holds the solver
    to); and cost(0.9 u*) > cost(u*) for every instance (u = 0 is feasible at the default bounds and the QP is convex)."""
    import torch
    name, path, g = _solve_groups()[which]
    B = g["x_fb"].shape[0]
    solver = _solver(g, path, B)
    a = ec.kernel_args(g)
    inp = {k: v for k, v in a.items() if k != "controls"}
    states, controls, info = solver.solve(**inp, evaluate=True)
    assert (info["status"] == 0).all(), np.bincount(info["status"])
    ev = solver.evaluate(**inp, controls=controls, want_states=True)
    for k in ("cost", "objective", "violation"):
        assert np.array_equal(info[k], ev[k]), k
    # device: solve -> evaluate on one stream, no synchronisation in between
    d = _dev_args(a)
    d_in = {k: v for k, v in d.items() if k != "controls"}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        u_dev, _ = solver.solve_device(**d_in)
        ev_dev = solver.evaluate_device(**d_in, controls=u_dev, want_states=True)
    st.synchronize()
    assert np.array_equal(u_dev.cpu().numpy().astype(np.float64), controls)
    _identical(ev, {k: ev_dev[k].cpu().numpy() for k in KEYS}, name)
    print(name, "states vs solve %.3e" % util.rel_err(ev["states"], states).max(), "violation max", ev["violation"].max(0),
          "cost min %.4g max %.4g" % (ev["cost"].min(), ev["cost"].max()))
    assert util.rel_err(ev["states"], states).max() <= util.REL_TOL
    assert ev["violation"].max() <= 2e-3, ev["violation"].max(0)
    c09 = solver.evaluate(**inp, controls=0.9 * controls)["cost"]
    print(name, "smallest cost(0.9 u*) / cost(u*): %.6f" % (c09 / ev["cost"]).min())
    assert (c09 > ev["cost"]).all(), int((c09 <= ev["cost"]).sum())
    idx = np.arange(0, B, B // 16)
    ec.check({k: ev[k][idx] for k in KEYS}, ec.yardstick_group(dict(g, controls=controls), idx), name)
    solver.close()


def test_the_solve_is_untouched():
    """With evaluate=False `info` has exactly today's keys; a solve, an evaluation, and the same solve again (cold, and once more with
    warm start enabled around it) return identical bits and iteration counts; last_kernel_ms() after solve -> evaluate is the solve's."""
    s = util.synth_batch(1024, 10, 1, gait="standing")
    g = ec._group(10, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], np.zeros((1024, 10, 12)))
    solver = _solver(g, 0, 1024)
    inp = {k: v for k, v in ec.kernel_args(g).items() if k != "controls"}

    def run():
        st, u, info = solver.solve(**inp)
        return st, u, info, solver.last_kernel_ms()

    st0, u0, info0, ms0 = run()
    assert sorted(info0) == ["iters", "nfactor", "residuals", "status"]
    ev = solver.evaluate(**inp, controls=u0, want_states=True)
    assert solver.last_kernel_ms() == ms0 and ms0 > 0          # the event pair still holds the solve
    st1, u1, info1, _ = run()
    for x, y in ((st0, st1), (u0, u1), (info0["iters"], info1["iters"]), (info0["nfactor"], info1["nfactor"])):
        assert np.array_equal(x, y)
    solver.set_warm_start(True, shift=0, theta=0.5)
    _, uw0, iw0, _ = run()                                     # first warm-enabled solve starts cold
    solver.evaluate(**inp, controls=uw0)
    _, uw1, iw1, _ = run()                                     # starts from the stored state: the evaluation has not touched it
    solver.set_warm_start(False)
    assert np.array_equal(uw0, u0) and np.array_equal(iw0["iters"], info0["iters"])
    ref = _solver(g, 0, 1024)                                  # the same two warm solves with no evaluation in between
    ref.set_warm_start(True, shift=0, theta=0.5)
    ref.solve(**inp)
    _, ur1, ir1 = ref.solve(**inp)
    assert np.array_equal(uw1, ur1) and np.array_equal(iw1["iters"], ir1["iters"])
    assert not np.array_equal(iw1["iters"], info0["iters"])    # (the warm start was really in effect)
    ref.close()
    solver.close()
    assert np.isfinite(ev["cost"]).all()


def test_evaluation_is_faster_than_the_solve():
    """HIP events around 20 `evaluate_device` launches at B = 4096, h = 10, all four outputs, against last_kernel_ms() of the solve of
    the same batch in the same process: the evaluation's median must be below the solve's (about 1/1000 of the flops)."""
    import torch
    B, h = 4096, 10
    s = util.synth_batch(B, h, 1, gait="standing")
    g = ec._group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], np.zeros((B, h, 12)))
    solver = _solver(g, 0, B)
    d = _dev_args(ec.kernel_args(g))
    d_in = {k: v for k, v in d.items() if k != "controls"}
    u, _ = solver.solve_device(**d_in)
    solve_ms = solver.last_kernel_ms()
    out = solver.evaluate_device(**d_in, controls=u, want_states=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        solver.evaluate_device(**d_in, controls=u, cost=out["cost"], objective=out["objective"], violation=out["violation"],
                               states=out["states"])
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times))
    # compulsory traffic per instance: x_fb, foot, phase, x_cmd, contact, controls in; cost, objective, violation, states out
    bytes_inst = 12 * 4 + 6 * 4 + 4 + 12 * 4 + h * 2 + h * 12 * 4 + 8 + 8 + 32 + h * 13 * 8
    print("evaluate_device B=%d h=%d: median %.1f us (min %.1f), solve %.1f us, ratio %.4f, %.1f GB/s over %d B/instance"
          % (B, h, med * 1e3, min(times) * 1e3, solve_ms * 1e3, med / solve_ms, B * bytes_inst / (med * 1e-3) / 1e9, bytes_inst))
    assert med < solve_ms
    solver.close()
