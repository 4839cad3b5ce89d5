"""The receding-horizon warm start (`bmpc_set_warm_start`), for every kernel variant.

ADMM reaches the same optimum from any start, so a wrong index in the load -- another lane or step, a clamp at another place, a
stride that fits one horizon only, a vote that quietly falls back to a cold start -- costs iterations and changes no output.  These
tests pin what the kernels load: the optimum whatever was loaded (against the oracle), the stored state as a fixed point of the
iteration (the test a wrong store / load pair and a silent cold start fail), the rules for a cold start bit for bit, the argument
checks, and closed loops on variants other than the workload's h = 10.  One case per kernel variant: the dense kernels h = 8, 12,
16, 20 (`Dims<H>` lane maps; 12: no secant step; 20: spills) and the stage kernels with two to five steps per lane on one wave
(h = 4, 13, 18, 22) and on two (26, 33, 40), with and without phantom steps.  The index map itself is checked exactly on the CPU
(tests/test_emu.py), where the buffer is the test's own array."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

PATH_DENSE, PATH_STAGE = 1, 2
B = 48
VARIANTS = [(PATH_DENSE, 8), (PATH_DENSE, 12), (PATH_DENSE, 16), (PATH_DENSE, 20),
            (PATH_STAGE, 4), (PATH_STAGE, 13), (PATH_STAGE, 18), (PATH_STAGE, 22), (PATH_STAGE, 26), (PATH_STAGE, 33), (PATH_STAGE, 40)]
_IDS = ["%s-h%d" % ("dense" if p == PATH_DENSE else "stage", h) for p, h in VARIANTS]
KEYS = ("controls", "states", "iters", "nfactor", "residuals")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _solver(path, h, half, max_batch=B):
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = h
    sol = bm.BatchSolver(mpc=mpc, half=half, max_batch=max_batch, solver_options=dict(path=path))
    assert sol._lib.bmpc_solver_path(sol._h) == path
    return sol


def _solve(sol, p, n=None):
    """Problem p (its first n instances) through `BatchSolver.solve`: one dict of the results and the per-instance counters."""
    cut = slice(None) if n is None else slice(0, n)
    st, u, info = sol.solve(p["x_fb"][cut], p["foot"][cut], p["contact"][cut], p["phase"][cut], x_cmd=p["x_cmd"][cut])
    return dict(states=st, controls=u, **info)


def _identical(a, b, where, idx=None):
    for k in KEYS:
        x, y = (a[k], b[k]) if idx is None else (a[k][idx], b[k][idx])
        assert np.array_equal(x, y), (where, k)


def _r32(v):
    return np.asarray(v).astype(np.float32).astype(float)


_ctx = {}


def _case(path, h):
    """Per (family, h), solved once and shared (nothing below modifies it): problem P1 (48 walking instances, commanded v_x), its
    cold solve on a fresh handle, P2 -- P1 one control period later: state feedback x_fb <- states[:, 0, :12], t <- t + dt,
    phase and contact from the solver's own scheduler -- and P2's cold solve on a fresh handle.  `oracle(i)`: the fp64 oracle's
    (states, controls) of instance i of P2 on the fp32-rounded inputs the device sees, computed on first use."""
    key = (path, h)
    if key in _ctx:
        return _ctx[key]
    import biped_mpc_py_amd as bm
    from oracle import bmpc_oracle as orc
    s = util.synth_batch(B, h, 900 + h, gait="walking", vx_cmd=True)
    half = s["half"]
    p1 = {k: s[k] for k in ("x_fb", "foot", "contact", "phase", "x_cmd")}
    sol = _solver(path, h, half)
    cold1 = _solve(sol, p1)
    assert (cold1["status"] == 0).all()
    dt = bm.MPC().dt
    t2 = (s["phase"] + 0.5) * dt + dt
    phase2, contact2 = sol.contact_sequence(t2)
    assert np.array_equal(phase2, (s["phase"] + 1) % h)
    sol.close()
    p2 = dict(p1, x_fb=cold1["states"][:, 0, :12].copy(), phase=phase2, contact=contact2)
    sol = _solver(path, h, half)
    cold2 = _solve(sol, p2)
    assert (cold2["status"] == 0).all()
    sol.close()
    memo = {}

    def oracle(i):
        if i not in memo:
            m = orc.MPC()
            m.h = h
            m.x_cmd = _r32(p2["x_cmd"][i])
            memo[i] = orc.solve_mpc(_r32(p2["x_fb"][i]), float(t2[i]), _r32(p2["foot"][i]), m, orc.Biped(), contact2[i], half=half)
        return memo[i]

    _ctx[key] = dict(half=half, p1=p1, p2=p2, cold1=cold1, cold2=cold2, oracle=oracle)
    return _ctx[key]


def _warm_pair(path, h, c, shift, theta):
    """A fresh handle with the warm start on: P1 (stores, starts cold), then P2 warm.  Returns both results."""
    sol = _solver(path, h, c["half"])
    sol.set_warm_start(True, shift=shift, theta=theta)
    a = _solve(sol, c["p1"])
    b = _solve(sol, c["p2"])
    sol.close()
    return a, b


@pytest.mark.parametrize("path,h", VARIANTS, ids=_IDS)
def test_same_optimum_whatever_was_loaded(path, h):
    """P2 warm, from what P1 left, for every shift in {0, 1, 3, h - 1} ({0, 1, 2, 3} at h = 4) and theta in {0, 0.5, 1}: every
    instance converges, all 48 agree with a cold solve of P2 from a fresh handle and four of them -- the one with the most
    iterations among them -- with the oracle, controls and states, to the north_star tolerance.  A shift that does not match the
    schedule (it moved by one step) is a bad guess, not an error."""
    c = _case(path, h)
    cold2 = c["cold2"]
    for shift in ((0, 1, 2, 3) if h == 4 else (0, 1, 3, h - 1)):
        for theta in (0.0, 0.5, 1.0):
            _, w = _warm_pair(path, h, c, shift, theta)
            where = "h=%d path %d shift %d theta %.1f" % (h, path, shift, theta)
            eu, ex = util.rel_err(w["controls"], cold2["controls"]), util.rel_err(w["states"], cold2["states"])
            hardest = int(np.argmax(w["iters"]))
            idx = ([hardest] + [i for i in (0, 17, 31, 44) if i != hardest])[:4]
            ou = np.stack([c["oracle"](i)[1] for i in idx])
            ox = np.stack([c["oracle"](i)[0] for i in idx])
            fu, fx = util.rel_err(w["controls"][idx], ou), util.rel_err(w["states"][idx], ox)
            print("%s: iters warm %.1f (max %d) cold %.1f; vs cold %.1e / %.1e, vs oracle %s %.1e / %.1e" % (
                where, w["iters"].mean(), w["iters"].max(), cold2["iters"].mean(), eu.max(), ex.max(), idx, fu.max(), fx.max()))
            assert (w["status"] == 0).all(), (where, w["status"])
            assert eu.max() <= util.REL_TOL and ex.max() <= util.REL_TOL, where
            assert fu.max() <= util.REL_TOL and fx.max() <= util.REL_TOL, where


@pytest.mark.parametrize("path,h", VARIANTS, ids=_IDS)
def test_stored_state_is_a_fixed_point(path, h):
    """After a converged solve of P, a warm solve of the same P with shift 0 and theta 1 starts at a state that already met the
    stopping criteria: it leaves at its first stopping test (iters == check_every) with the one factorisation it started with,
    at the same controls.  What fails this: a store / load pair that disagrees on the lane or step of any variable, a phantom
    slot that is read but never written, a silent cold start (the iterations would be the cold solve's)."""
    c = _case(path, h)
    sol = _solver(path, h, c["half"])
    every = int(sol.cparams.check_every)
    sol.set_warm_start(True, shift=0, theta=1.0)
    a = _solve(sol, c["p1"])
    b = _solve(sol, c["p1"])
    sol.close()
    it, cnt = np.unique(b["iters"], return_counts=True)
    nf, ncnt = np.unique(b["nfactor"], return_counts=True)
    print("fixed point h=%d path %d: iters %s x %s, nfactor %s x %s (first solve: iters mean %.1f)" % (
        h, path, it.tolist(), cnt.tolist(), nf.tolist(), ncnt.tolist(), a["iters"].mean()))
    _identical(a, c["cold1"], "the storing solve starts cold")
    assert (b["status"] == 0).all()
    assert (b["iters"] == every).all(), (it.tolist(), cnt.tolist())
    assert (b["nfactor"] == 1).all(), (nf.tolist(), ncnt.tolist())
    assert util.rel_err(b["controls"], a["controls"]).max() <= util.REL_TOL


@pytest.mark.parametrize("path,h", [(PATH_DENSE, 16), (PATH_STAGE, 26)], ids=["dense-h16", "stage-h26"])
def test_cold_rules_bit_for_bit(path, h):
    """include/bmpc.h: "the first call after enabling, after bmpc_reset_warm_start, or with another B starts cold", and a stored
    state that is not finite is ignored as a whole -- for that instance only.  Each reproduces a cold solve from a fresh handle
    exactly: controls, states, iterations, factorisations, residuals.  (Stage h = 26: the vote on the stored state crosses waves.)"""
    c = _case(path, h)
    p1, p2, cold1, cold2 = c["p1"], c["p2"], c["cold1"], c["cold2"]
    sol = _solver(path, h, c["half"])
    sol.set_warm_start(True, shift=1, theta=0.5)
    _identical(_solve(sol, p1), cold1, "(a) first solve after enabling")
    w = _solve(sol, p2)
    assert not np.array_equal(w["iters"], cold2["iters"])           # (the handle does start warm: the rules below have something to drop)
    sol.reset_warm_start()
    _identical(_solve(sol, p1), cold1, "(b) after reset_warm_start")
    fresh = _solver(path, h, c["half"])
    cold47 = _solve(fresh, p1, B - 1)
    fresh.close()
    _identical(_solve(sol, p1, B - 1), cold47, "(c) another B: 47 after 48")
    _identical(_solve(sol, p2), cold2, "(c) another B: 48 after 47")
    sol.close()
    # (d) instance i failed in the previous solve (NaN in its x_fb: status 2, a state that is not finite): it alone starts cold
    i = 5
    others = np.arange(B) != i
    bad = dict(p1, x_fb=p1["x_fb"].copy())
    bad["x_fb"][i, 3] = np.nan
    sol = _solver(path, h, c["half"])
    sol.set_warm_start(True, shift=1, theta=0.5)
    a1 = _solve(sol, bad)
    assert a1["status"][i] == 2 and (a1["status"][others] == 0).all()
    _identical(a1, cold1, "(d) the neighbours of a failing instance", others)
    a2 = _solve(sol, p2)
    sol.close()
    _, b2 = _warm_pair(path, h, c, 1, 0.5)
    assert (a2["status"] == 0).all()
    _identical(a2, cold2, "(d) the instance whose stored state is not finite", [i])
    _identical(a2, b2, "(d) the other instances start warm all the same", others)
    assert not np.array_equal(b2["iters"][others], cold2["iters"][others])


@pytest.mark.parametrize("first,then", [(PATH_DENSE, PATH_STAGE), (PATH_STAGE, PATH_DENSE)], ids=["dense-to-stage", "stage-to-dense"])
def test_change_of_kernel_family_drops_the_state(first, then):
    """(e) `bmpc_set_params` that moves the handle to the other kernel family (h = 10 has both) drops the stored state -- the two
    families keep different ones: the next solve is a fresh handle's cold solve, bit for bit."""
    import biped_mpc_py_amd as bm
    h = 10
    c = _case(then, h)
    sol = _solver(first, h, c["half"])
    sol.set_warm_start(True, shift=1, theta=0.5)
    assert (_solve(sol, c["p1"])["status"] == 0).all()
    sol.set_params(bm.pack_params(bm.MPC(), bm.Biped(), half=c["half"], solver_options=dict(path=then)))
    assert sol._lib.bmpc_solver_path(sol._h) == then
    _identical(_solve(sol, c["p2"]), c["cold2"], "(e) after a change of family")
    w = _solve(sol, c["p2"])                                       # and the warm start is still on, in the new family's layout
    sol.close()
    assert (w["status"] == 0).all() and not np.array_equal(w["iters"], c["cold2"]["iters"])


def test_argument_checks_leave_the_setting_alone():
    """`bmpc_set_warm_start` refuses a shift outside [0, h) and a theta outside [0, 1] (NaN included) with BMPC_ERR_INVALID, and a
    refused call changes nothing: the next solve is the warm solve of a handle that never saw the bad calls, bit for bit."""
    import biped_mpc_py_amd as bm
    path, h = PATH_DENSE, 16
    c = _case(path, h)
    sol = _solver(path, h, c["half"])
    sol.set_warm_start(True, shift=1, theta=0.5)
    _solve(sol, c["p1"])
    for enable in (True, False):
        for shift, theta in ((-1, 0.5), (h, 0.5), (1, -0.01), (1, 1.01), (1, float("nan")), (1, float("inf")), (h + 7, 2.0)):
            with pytest.raises(bm.BmpcError) as e:
                sol.set_warm_start(enable, shift=shift, theta=theta)
            assert e.value.code == -1, (shift, theta, e.value)      # BMPC_ERR_INVALID
    got = _solve(sol, c["p2"])
    sol.set_warm_start(True, shift=h - 1, theta=0.0)                # the ends of both ranges are inside
    sol.set_warm_start(True, shift=0, theta=1.0)
    sol.close()
    _, want = _warm_pair(path, h, c, 1, 0.5)
    _identical(got, want, "warm solve after refused calls")
    assert not np.array_equal(want["iters"], c["cold2"]["iters"])


@pytest.mark.parametrize("path,h", [(PATH_DENSE, 16), (PATH_STAGE, 13), (PATH_STAGE, 26)], ids=["dense-h16", "stage-h13", "stage-h26"])
def test_closed_loop_on_other_variants(path, h):
    """`bmpc_rollout_device`, 6 periods of 6 walking instances, with the warm start (shift 1, theta 0.5) and without, against the
    oracle's own closed loop: applied control and state per period to the north_star tolerance.  The warm / cold iteration
    ratios of periods 2 .. K are printed and recorded in DESIGN.md section 8b, not asserted: 6 instances are no sample for a threshold."""
    Bc, K = 6, 6
    x0, foot, t0 = util.closed_loop_start(Bc)
    ref_u, ref_x = util.oracle_closed_loop(x0, foot, t0, K, h)
    out = {}
    for warm in (None, (1, 0.5)):
        out[warm], eu, ex = util.device_closed_loop(x0, foot, t0, K, ref_u, ref_x, h, warm=warm, path=path)
        print("h=%d path %d %s: u0 err max %.2e  x err max %.2e  mean iters %.1f (periods 2..K: %.1f)" % (
            h, path, "warm" if warm else "cold", eu, ex, out[warm].mean(), out[warm][1:].mean()))
        assert eu <= util.REL_TOL and ex <= util.REL_TOL
    assert np.array_equal(out[None][0], out[(1, 0.5)][0])           # the first period starts cold either way
    print("h=%d path %d: warm / cold iterations, periods 2..K: %.3f" % (h, path, out[(1, 0.5)][1:].mean() / out[None][1:].mean()))
