"""GPU: the plant entries (`plant_step`, `plant_step_device`) against the NumPy restatement of the plant (tests/plant_model.py), and
`simulate_device` as the composition of verified parts: every recorded period is checked from the recorded state before it -- a cold
solve reproduces the applied control bit for bit, the model's step reproduces the next state within 2 fp32 ulps (both sides compute
in fp64: only the final rounding can differ, one ulp, the second is margin), the landing rule reproduces the footholds -- so no error
accumulates and no closed-loop tolerance is needed."""
import numpy as np
import pytest

from tests import plant_model as pm
from tests import util

pytestmark = pytest.mark.gpu
K = 12


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _solver(h, path, max_batch=512):
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = h
    return bm.BatchSolver(mpc=mpc, biped=bm.Biped(), solver_options=dict(path=path), max_batch=max_batch)


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


@pytest.mark.parametrize("B", [67, 257])
def test_plant_step_matches_model_and_host_equals_device(B):
    import torch
    s = _solver(10, 0)
    x, u, foot, c, w = pm.batch(B)
    for integrator in ("euler", "rk4"):
        for wr in (w, None):
            host = s.plant_step(x, u, foot, c, wr, integrator=integrator, substeps=4)
            dev = s.plant_step_device(_cuda(x, np.float32), _cuda(u, np.float32), _cuda(foot, np.float32), _cuda(c, np.uint8),
                                      None if wr is None else _cuda(wr, np.float32), integrator=integrator, substeps=4)
            torch.cuda.synchronize()
            assert np.array_equal(host.astype(np.float32), dev.cpu().numpy())
            ref = pm.step_batch(x, u, foot, c, wr, integrator=integrator, substeps=4)
            d = pm.ulp_diff(dev.cpu().numpy(), ref)
            print(integrator, "wrench" if wr is not None else "none", "max ulps", d.max())
            assert d.max() <= 2.0


def _start(B, seed=5):
    x0, foot, t0 = util.closed_loop_start(B, seed)
    rng = np.random.default_rng(seed + 1)
    x0[:, 6:9] = rng.uniform(-0.1, 0.1, (B, 3))
    t0 = rng.integers(0, 10, B) * 0.04 + 0.01          # mixed phases, away from the period boundaries
    return x0, foot, t0


def _simulate(s, x0, foot0, t0, **kw):
    import torch
    x, f, t = _cuda(x0, np.float32), _cuda(foot0, np.float32), _cuda(t0, np.float64)
    r = s.simulate_device(x, f, t, K, **kw)
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}
    out.update(x_end=x.cpu().numpy(), foot_end=f.cpu().numpy(), t_end=t.cpu().numpy())
    return out


def _times(t0, dt):
    ts = [np.asarray(t0, np.float64).copy()]
    for _ in range(K):
        ts.append(ts[-1] + dt)                         # the device's own `t += dt`, repeated
    return ts


def _check_periods(s, x0, foot0, t0, r, push=None, window=(0, 0), expect_wrench=True, plant_kw=None, x_cmd=None, gait=None,
                   integrator="rk4", substeps=4):
    """(a) - (d) of the module docstring for every period; returns the number of landings seen per leg.  `plant_kw`: the model's
    I_b, m, g where the handle's are not the defaults; `x_cmd` (B,12): the per-instance commands the simulation ran with; `gait`
    (period, offset, duty), `integrator`, `substeps`: what it ran with where that was not the default."""
    import torch
    h, dt = s.h, float(s.cparams.dt)
    half = int(s.cparams.half)
    gait_kw = {} if gait is None else dict(period=gait[0], offset=gait[1], duty=gait[2])
    gait = (2 * half, (0, half), (half, half)) if gait is None else gait
    plant_kw = {k: v for k, v in (plant_kw or {}).items() if k != "dt"}
    cmd_dev = None if x_cmd is None else _cuda(x_cmd, np.float32)
    ts = _times(t0, dt)
    landed = np.zeros(2, int)
    B = x0.shape[0]
    for k in range(K):
        xs = x0 if k == 0 else r["x"][k - 1]
        fs = foot0 if k == 0 else r["foot"][k - 1]
        phase, contact = s.contact_sequence_device(_cuda(ts[k], np.float64), **gait_kw)
        s.reset_warm_start()
        u, _ = s.solve_device(_cuda(xs, np.float32), _cuda(fs, np.float32), contact, phase, x_cmd=cmd_dev)
        assert torch.equal(u[:, 0, :].cpu(), torch.from_numpy(r["u0"][k])), ("u0", k)                          # (a)
        c0 = contact[:, 0, :].cpu().numpy()
        active = push is not None and window[0] <= k < window[0] + window[1]
        ref = pm.step_batch(xs, r["u0"][k], fs, c0, push if (active and expect_wrench) else None, integrator=integrator,
                            substeps=substeps, dt=dt, **plant_kw)
        d = pm.ulp_diff(r["x"][k], ref)
        if active and not expect_wrench:
            pushed = np.abs(push).max(1) > 0
            assert d[pushed].max() > 2.0 and d[~pushed].max() <= 2.0, ("push must show", k)
        else:
            assert d.max() <= 2.0, ("x", k, d.max())                                                               # (b)
        k0 = s.contact_sequence_device(_cuda(ts[k], np.float64))[0].cpu().numpy()
        k1 = s.contact_sequence_device(_cuda(ts[k + 1], np.float64))[0].cpu().numpy()
        for b in range(B):
            cmd = (float(s.cparams.x_cmd[3]), float(s.cparams.x_cmd[4])) if x_cmd is None else x_cmd[b, 3:5].astype(np.float64)
            fr, lands = pm.landing(r["x"][k][b].astype(np.float64), fs[b], int(k0[b]), int(k1[b]), gait[0], gait[1], gait[2], h=h, dt=dt,
                                   kv=float(s.cparams.kv), cmd=cmd)
            assert pm.ulp_diff(r["foot"][k][b], fr, atol=0.0).max() <= 1.0, ("foot", k, b)                         # (c)
            for g in range(2):
                if not lands[g]:
                    assert np.array_equal(r["foot"][k][b, 3 * g:3 * g + 3], fs[b, 3 * g:3 * g + 3])
                landed[g] += lands[g]
    assert np.array_equal(r["t_end"], ts[K])                                                                      # (d)
    assert np.array_equal(r["x_end"], r["x"][K - 1]) and np.array_equal(r["foot_end"], r["foot"][K - 1])
    return landed


@pytest.mark.parametrize("h,path", [(10, 1), (7, 2)])
def test_simulate_is_the_composition_of_verified_parts(h, path):
    B = 67
    s = _solver(h, path)
    assert s._lib.bmpc_solver_path(s._h) == path
    x0, foot0, t0 = _start(B)
    r = _simulate(s, x0, foot0, t0)
    landed = _check_periods(s, x0, foot0, t0, r)
    assert (landed >= B // 2).all(), landed             # both legs land
    assert (r["status_any"] == 0).all() and np.isfinite(r["x"]).all()


@pytest.mark.parametrize("run", ["combined_h7_stage", "euler_h10_dense"])
def test_simulate_at_a_parameter_case_with_per_instance_commands(run):
    """The closed loop away from the defaults (tests/param_cases.py CLOSED_LOOP_RUNS), checked period by period like the default one:
    the combined case (m, a non-diagonal I_b, g, dt) on the h = 7 stage family under a custom gait, and explicit Euler with three
    substeps at I_nondiagonal on the h = 10 dense family -- both with per-instance commands whose x, y entries are not zero, the branch
    of the landing rule that reads them.  B = 33, 12 periods; every instance lands each leg at least once."""
    import biped_mpc_py_amd as bm
    from tests import param_cases as pc
    assert K == pc.CLOSED_LOOP_K
    c = pc.CLOSED_LOOP_RUNS[run]
    mpc, biped = pc.objects(bm, c["case"], h=c["h"])
    s = bm.BatchSolver(mpc=mpc, biped=biped, solver_options=dict(path=c["path"]), max_batch=64)
    assert s._lib.bmpc_solver_path(s._h) == c["path"]
    x0, foot0, t0, x_cmd = pc.closed_loop_start(run)
    period, offset, duty = c["gait"]
    r = _simulate(s, x0, foot0, t0, x_cmd=_cuda(x_cmd, np.float32), period=period, offset=offset, duty=duty,
                  integrator=c["integrator"], substeps=c["substeps"])
    landed = _check_periods(s, x0, foot0, t0, r, plant_kw=pc.plant_kw(c["case"]), x_cmd=x_cmd, gait=c["gait"],
                            integrator=c["integrator"], substeps=c["substeps"])
    print(run, "landings per leg", landed, "iterations mean %.1f max %d" % (r["iters"].mean(), r["iters"].max()))
    assert (landed >= x0.shape[0]).all(), landed            # (every instance lands each leg: test_the_closed_loop_runs_let_both_legs_land)
    assert (r["status_any"] == 0).all() and np.isfinite(r["x"]).all()
    # the commands were read: the footholds of the same run without them differ
    plain = _simulate(s, x0, foot0, t0, period=period, offset=offset, duty=duty, integrator=c["integrator"], substeps=c["substeps"])
    assert not np.array_equal(plain["foot_end"], r["foot_end"])


def test_move_feet_off_leaves_the_footholds():
    s = _solver(10, 0)
    x0, foot0, t0 = _start(33)
    r = _simulate(s, x0, foot0, t0, move_feet=False)
    assert np.array_equal(r["foot_end"], foot0)
    assert all(np.array_equal(r["foot"][k], foot0) for k in range(K))


def test_push_acts_in_its_window_only():
    B = 34
    s = _solver(10, 0)
    x0, foot0, t0 = _start(B)
    push = np.zeros((B, 6), np.float32)
    push[::2, 1] = 40.0
    push[::2, 3] = 2.0
    plain = _simulate(s, x0, foot0, t0)
    r = _simulate(s, x0, foot0, t0, push=_cuda(push, np.float32), push_from=2, push_steps=3)
    for k in (0, 1):
        for key in ("x", "u0", "foot", "iters"):
            assert np.array_equal(plain[key][k], r[key][k]), (key, k)
    assert not np.array_equal(plain["x"][2][::2], r["x"][2][::2]) and np.array_equal(plain["x"][2][1::2], r["x"][2][1::2])
    _check_periods(s, x0, foot0, t0, r, push=push, window=(2, 3), expect_wrench=True)
    _check_periods(s, x0, foot0, t0, r, push=push, window=(2, 3), expect_wrench=False)


def test_rollout_is_unchanged_by_a_simulation_on_the_same_handle():
    import torch
    B = 67
    s = _solver(10, 0)
    x0, foot0, t0 = _start(B)

    def rollout():
        s.reset_warm_start()
        x, f, t = _cuda(x0, np.float32), _cuda(foot0, np.float32), _cuda(t0, np.float64)
        r = s.rollout_device(x, f, t, 6)
        torch.cuda.synchronize()
        return [v.cpu().numpy() for v in (r["u0"], r["x"], r["iters"], r["status_any"], x, t)]

    before = rollout()
    s.reset_warm_start()
    _simulate(s, x0, foot0, t0)
    after = rollout()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_a_bad_instance_shows_and_touches_no_neighbour():
    B = 9
    s = _solver(10, 0)
    x0, foot0, t0 = _start(B)
    push = np.zeros((B, 6), np.float32)
    push[3, 0] = np.inf
    plain = _simulate(s, x0, foot0, t0)
    r = _simulate(s, x0, foot0, t0, push=_cuda(push, np.float32), push_from=1, push_steps=1)
    assert r["status_any"][3] != 0 and np.isnan(r["x"][1:, 3]).all() and np.isfinite(r["x"][0, 3]).all()
    keep = np.arange(B) != 3
    for key in ("x", "u0", "foot"):
        assert np.array_equal(plain[key][:, keep], r[key][:, keep]), key
    assert np.array_equal(plain["status_any"][keep], r["status_any"][keep])
