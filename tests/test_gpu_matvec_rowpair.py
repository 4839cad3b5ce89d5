"""The dense h = 10 kernel on the GPU where its iteration now reads V in the row-pair layout (bmpc_kernels.hip, phases P3 / P4)
and keeps a scheduled penalty move over the reduction: a single instance and an odd batch of 37, on a turning batch with a
mixed gait and a friction coefficient per step and foot.

What is new against the sweep's own test (test_gpu_sweep_rowpair.py): beta is published in quarters and read by the quad, the
clone quad of every wave stays a copy of the quad below it between factorisations, the kept move sits in LDS the sweep owns,
and a warm-started solve rebuilds the carried products before the first mat-vec.  One seeded batch, one oracle solve of it and
one device solve of it are shared by the checks, cold and warm-started alike: parity against the oracle at the suite's tolerance
(util.REL_TOL), six repeated solves equal to the bit, and instance 0 solved alone equal to the bit to its row of the batch.
With max_iter = 1 -- one factorisation, one pass through P3 / P4 -- the controls are finite and equal across repeats."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

PATH_DENSE = 1
H = 10
B = 37
KEYS = ("iters", "status", "nfactor")
_CACHE = {}


def _solver(half, warm=False, **options):
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = H
    sol = bm.BatchSolver(mpc=mpc, half=half, max_batch=B, solver_options=dict(path=PATH_DENSE, **options))
    assert sol._lib.bmpc_solver_path(sol._h) == PATH_DENSE
    if warm:
        sol.set_warm_start(True, shift=0, theta=0.5)
    return sol


def _solve(sol, s, n):
    st, u, info = sol.solve(s["x_fb"][:n], s["foot"][:n], s["contact"][:n], s["phase"][:n], x_cmd=s["x_cmd"][:n], mu=s["mu"][:n])
    return np.array(st), np.array(u), {k: np.array(info[k]) for k in KEYS}      # (copies: a later solve may reuse what these view)


def _second(s, n, warm):
    """The solve the checks look at, on a fresh handle: the cold solve, or the warm-started second solve of the same problem
    (the first one stores its final state, the second starts from it with the penalties pulled half way back)."""
    sol = _solver(s["half"], warm)
    out = _solve(sol, s, n)
    if warm:
        out = _solve(sol, s, n)
    sol.close()
    return out


def _case():
    """(batch, oracle controls of the batch), made once."""
    if not _CACHE:
        from oracle import bmpc_oracle as orc
        s = util.synth_batch(B, H, 2510, gait="mixed", vx_cmd=True, turn=True, per_step_mu=True)
        r32 = lambda v: np.asarray(v).astype(np.float32).astype(float)
        ref = np.zeros((B, H, 12))
        for i in range(B):
            m = orc.MPC()
            m.h = H
            m.x_cmd = r32(s["x_cmd"][i])
            _, ref[i] = orc.solve_mpc(r32(s["x_fb"][i]), (s["phase"][i] + 0.5) * m.dt, r32(s["foot"][i]), m, orc.Biped(),
                                      s["contact"][i], half=s["half"], mu_steps=r32(s["mu"][i]))
        ref.setflags(write=False)
        _CACHE["case"] = (s, ref)
    return _CACHE["case"]


def _full(warm):
    """The solve of the whole batch, cold or warm-started, made once."""
    if ("full", warm) not in _CACHE:
        _CACHE[("full", warm)] = _second(_case()[0], B, warm)
    return _CACHE[("full", warm)]


WARM = pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])


@WARM
@pytest.mark.parametrize("n", [1, B])
def test_parity_against_the_oracle(n, warm):
    s, ref = _case()
    states, u, info = _full(warm) if n == B else _second(s, n, warm)
    e = util.rel_err(u, ref[:n])
    print("B=%d %s: err max %.2e  iters mean %.1f max %d  nfactor mean %.1f" % (
        n, "warm" if warm else "cold", e.max(), info["iters"].mean(), info["iters"].max(), info["nfactor"].mean()))
    assert (info["status"] == 0).all(), info["status"]
    assert e.max() <= util.REL_TOL


@WARM
@pytest.mark.parametrize("n", [1, B])
def test_six_repeated_solves_are_bit_equal(n, warm):
    s, _ = _case()
    st0, u0, i0 = _full(warm) if n == B else _second(s, n, warm)
    for rep in range(5):
        st, u, info = _second(s, n, warm)
        assert np.array_equal(u, u0) and np.array_equal(st, st0), (n, warm, rep)
        for k in KEYS:
            assert np.array_equal(info[k], i0[k]), (n, warm, rep, k)


@WARM
def test_an_instance_alone_equals_its_row_of_the_batch(warm):
    s, _ = _case()
    stB, uB, iB = _full(warm)
    st1, u1, i1 = _second(s, 1, warm)
    assert np.array_equal(u1[0], uB[0]) and np.array_equal(st1[0], stB[0])
    for k in KEYS:
        assert i1[k][0] == iB[k][0], (k, i1[k][0], iB[k][0])


@pytest.mark.parametrize("n", [1, B])
def test_one_iteration_returns_finite_controls_equal_across_repeats(n):
    s, _ = _case()
    sol = _solver(s["half"], max_iter=1)
    st0, u0, i0 = _solve(sol, s, n)
    print("B=%d max_iter=1: iters %s status %s |u| max %.3g" % (n, np.unique(i0["iters"]), np.unique(i0["status"]), np.abs(u0).max()))
    assert (i0["iters"] == 1).all() and (i0["nfactor"] == 1).all()
    assert np.isfinite(u0).all() and np.isfinite(st0).all()
    assert np.abs(u0).max() > 0
    for rep in range(5):
        st, u, info = _solve(sol, s, n)
        assert np.array_equal(u, u0) and np.array_equal(st, st0), (n, rep)
    sol.close()
