"""The dense family's sweep on the GPU at the shapes where its row-pair form (bmpc_kernels.hip, factor()) can go wrong: a
single instance and an odd batch of 37 at h = 10 (the form: quads of two rows, the clone quad of every wave, two waves at the
barrier) and at h = 16 (three waves, rows dense over the lanes: the row-half form, which must not have moved).

Per horizon one seeded batch, one oracle solve of it and one device solve of it are shared by the checks: parity against the
oracle at the suite's tolerance (util.REL_TOL, north_star), six repeated solves equal to the bit (a race between the lanes
that publish pivot columns and the lanes that read them shows as results that change from run to run), and instance 0 solved
alone equal to the bit to its row of the batch (nothing of a solve may depend on the neighbours in the launch)."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

PATH_DENSE = 1
B = 37
HORIZONS = (10, 16)
KEYS = ("iters", "status", "nfactor")


def _solver(h, half, max_batch):
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = h
    sol = bm.BatchSolver(mpc=mpc, half=half, max_batch=max_batch, solver_options=dict(path=PATH_DENSE))
    assert sol._lib.bmpc_solver_path(sol._h) == PATH_DENSE
    return sol


def _solve(sol, s, n):
    return sol.solve(s["x_fb"][:n], s["foot"][:n], s["contact"][:n], s["phase"][:n], x_cmd=s["x_cmd"][:n],
                     mu=None if s["mu"] is None else s["mu"][:n])


_CACHE = {}


def _case(h):
    """(batch, oracle controls of the batch, device solve of the batch, the solver) of horizon h, made once."""
    if h not in _CACHE:
        from oracle import bmpc_oracle as orc
        s = util.synth_batch(B, h, 2400 + h, gait="mixed", vx_cmd=True)
        ref = np.zeros((B, h, 12))
        for i in range(B):
            m, b = orc.MPC(), orc.Biped()
            m.h = h
            m.x_cmd = s["x_cmd"][i]
            _, ref[i] = orc.solve_mpc(s["x_fb"][i].astype(np.float32).astype(float), (s["phase"][i] + 0.5) * m.dt,
                                      s["foot"][i].astype(np.float32).astype(float), m, b, s["contact"][i], half=s["half"])
        ref.setflags(write=False)
        sol = _solver(h, s["half"], B)
        st, u, info = _solve(sol, s, B)            # (copies: a later solve of the handle may reuse what these view)
        _CACHE[h] = (s, ref, (np.array(st), np.array(u), {k: np.array(info[k]) for k in KEYS}), sol)
    return _CACHE[h]


@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("n", [1, B])
def test_parity_against_the_oracle(h, n):
    s, ref, full, sol = _case(h)
    states, u, info = full if n == B else _solve(sol, s, n)
    e = util.rel_err(u, ref[:n])
    print("h=%d B=%d: err max %.2e  iters mean %.1f max %d  nfactor mean %.1f" % (
        h, n, e.max(), info["iters"].mean(), info["iters"].max(), info["nfactor"].mean()))
    assert (info["status"] == 0).all(), info["status"]
    assert e.max() <= util.REL_TOL


@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("n", [1, B])
def test_six_repeated_solves_are_bit_equal(h, n):
    s, _, _, sol = _case(h)
    st0, u0, i0 = _solve(sol, s, n)
    st0, u0, i0 = np.array(st0), np.array(u0), {k: np.array(i0[k]) for k in KEYS}
    for rep in range(5):
        st, u, info = _solve(sol, s, n)
        assert np.array_equal(u, u0) and np.array_equal(st, st0), (h, n, rep)
        for k in KEYS:
            assert np.array_equal(info[k], i0[k]), (h, n, rep, k)


@pytest.mark.parametrize("h", HORIZONS)
def test_an_instance_alone_equals_its_row_of_the_batch(h):
    s, _, full, sol = _case(h)
    stB, uB, iB = full
    st1, u1, i1 = _solve(sol, s, 1)
    assert np.array_equal(u1[0], uB[0]) and np.array_equal(st1[0], stB[0])
    for k in KEYS:
        assert i1[k][0] == iB[k][0], (k, i1[k][0], iB[k][0])
