"""GPU: the ground under the plant (`plant_step`, `plant_step_device`, `simulate_device` with `ground=`) against the NumPy
restatement of the rule (tests/ground_cases.py) and of the plant (tests/plant_model.py, tests/body_cases.py).

Bounds.  What the ground does not scale is a copy or +0: equal to the bit; a scaled entry within 1 fp32 ulp (ground_cases.
assert_applied).  A ground step is exactly the body step at u_applied: compared bit for bit against the existing entries, and within
the plant's 2-ulp bound against the model at u_applied (both sides compute in fp64, only the final rounding can differ).  The closed
loop is checked as the composition of verified parts, like tests/test_gpu_simulate.py: per recorded period from the recorded state
before it, so no error accumulates and no closed-loop tolerance is needed.  Whether a leg slips is a comparison in fp64 whose two
sides the shared controls keep 1e-6 apart; in the closed loop the friction of run B is half the largest demand of run A, so the
deciding period sits a factor 2 from its cone."""
import ctypes as C

import numpy as np
import pytest

from tests import body_cases as bc
from tests import ground_cases as gc
from tests import plant_model as pm
from tests import test_gpu_simulate as sim

pytestmark = pytest.mark.gpu
K = sim.K
PUSH_FROM, PUSH_STEPS = 2, 3


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _dev(a):
    return sim._cuda(a, np.float64)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("B", [67, 257])
def test_plant_step_with_ground(B):
    """A partial wave and a block boundary, both integrators, with and without bodies and wrench."""
    import torch
    s = sim._solver(10, 0)
    x, _, foot, _, w = pm.batch(B)
    u, c = gc.controls(B)
    mu = gc.grounds(B)
    ref_ua, ref_flags, _, scaled = gc.transmit(u, c, mu)
    perm = np.random.default_rng(3).permutation(B)
    dx, du, df, dc = (sim._cuda(a, t) for a, t in ((x, np.float32), (u, np.float32), (foot, np.float32), (c, np.uint8)))
    for integrator in ("euler", "rk4"):
        for wr in (w, None):
            for body in (None, bc.bodies(B)):
                tag = (integrator, "wrench" if wr is not None else "none", "bodies" if body else "handle's body")
                kw = dict(integrator=integrator, substeps=4)
                dw = None if wr is None else sim._cuda(wr, np.float32)
                dbody = None if body is None else {k: _dev(v) for k, v in body.items()}
                xh, uah, flh = s.plant_step(x, u, foot, c, wr, body=body, ground=dict(mu=mu), want_applied=True, **kw)
                xd, uad, fld = s.plant_step_device(dx, du, df, dc, dw, body=dbody, ground=dict(mu=_dev(mu)), want_applied=True, **kw)
                torch.cuda.synchronize()
                xd, uad, fld = _np(xd), _np(uad), _np(fld)
                # host equals device to the bit
                assert np.array_equal(xh.astype(np.float32), xd) and np.array_equal(uah.view(np.uint32), uad.view(np.uint32)), tag
                assert np.array_equal(flh, fld) and uad.dtype == np.float32 and fld.dtype == np.uint8, tag
                # u_applied and flags against the rule
                worst = gc.assert_applied(uad, fld, ref_ua, ref_flags, scaled, tag)
                # the next state against the model at u_applied
                ref = bc.step_batch(x, uad, foot, c, wr, body=body, **kw)
                d = pm.ulp_diff(xd, ref)
                print(*tag, "scaled entries max ulps", worst, "x max ulps", d.max())
                assert np.isfinite(ref).all() and d.max() <= 2.0, (tag, d.max())
                # exactly the existing entry at u_applied
                plain = s.plant_step_device(dx, sim._cuda(uad, np.float32), df, dc, dw, body=dbody, **kw)
                assert np.array_equal(_np(plain), xd), tag
                # without want_applied: the state alone
                assert np.array_equal(_np(s.plant_step_device(dx, du, df, dc, dw, body=dbody, ground=dict(mu=_dev(mu)), **kw)), xd), tag
                # a permuted batch gives the permuted result
                pbody = None if body is None else {k: np.ascontiguousarray(v[perm]) for k, v in body.items()}
                xp, uap, flp = s.plant_step(x[perm], u[perm], foot[perm], c[perm], None if wr is None else wr[perm], body=pbody,
                                            ground=dict(mu=np.ascontiguousarray(mu[perm])), want_applied=True, **kw)
                assert np.array_equal(xp, xh[perm]) and np.array_equal(uap.view(np.uint32), uah[perm].view(np.uint32)), tag
                assert np.array_equal(flp, flh[perm]), tag
            # {}: the handle's mu for both legs
            own = s.plant_step(x, u, foot, c, wr, ground={}, want_applied=True, **kw)
            full = s.plant_step(x, u, foot, c, wr, ground=dict(mu=np.full((B, 2), float(s.cparams.mu))), want_applied=True, **kw)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(own, full)), tag
            m_ua, m_fl, _, m_sc = gc.transmit(u, c, np.full((B, 2), float(s.cparams.mu)))
            gc.assert_applied(own[1], own[2], m_ua, m_fl, m_sc, tag)
            # no ground: the C entry runs the existing entries, and refuses to record
            plant = s._plant(integrator, 4)
            args = [dx.data_ptr(), du.data_ptr(), df.data_ptr(), dc.data_ptr(), None if dw is None else dw.data_ptr()]
            out = torch.empty((B, 12), dtype=torch.float32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            assert s._lib.bmpc_plant_step_ground_device(s._h, B, C.byref(plant), None, None, *args, out.data_ptr(), None, None, st) == 0
            assert torch.equal(out, s.plant_step_device(dx, du, df, dc, dw, **kw)), tag
            assert s._lib.bmpc_plant_step_ground_device(s._h, B, C.byref(plant), None, None, *args, out.data_ptr(), out.data_ptr(), None,
                                                        st) == -1


def _push(B):
    """A lateral push (40 N, 2 N m about x) on every other instance, periods 2 to 4."""
    push = np.zeros((B, 6), np.float32)
    push[::2, 1] = 40.0
    push[::2, 3] = 2.0
    return push


def _run(s, x0, foot0, t0, mu=None, **kw):
    """`simulate_device` with the push and, where mu (B,2) is given, that ground."""
    push = sim._cuda(_push(x0.shape[0]), np.float32)
    if mu is not None:
        kw["ground"] = dict(mu=_dev(mu))
    return sim._simulate(s, x0, foot0, t0, push=push, push_from=PUSH_FROM, push_steps=PUSH_STEPS, **kw)


def _gait_kw(gait):
    return {} if gait is None else dict(period=gait[0], offset=gait[1], duty=gait[2])


def _contact_rows(s, t0, gait=None):
    """Row 0 of every period's contact table (K,B,2) and the schedule steps (K+1,B), from the device's own schedule."""
    ts = sim._times(t0, float(s.cparams.dt))
    rows, steps = [], []
    for k in range(K + 1):
        phase, contact = s.contact_sequence_device(sim._cuda(ts[k], np.float64), **_gait_kw(gait))
        rows.append(_np(contact[:, 0, :]))
        steps.append(_np(phase))
    return np.stack(rows[:K]), np.stack(steps), ts


def _model(u0, rows, mu, fz_floor=0.0):
    """The rule applied to recorded commands u0 (K,B,12) under the contact rows: (u_applied, flags, demand, scaled) per period."""
    out = [gc.transmit(u0[k], rows[k], mu, fz_floor) for k in range(len(u0))]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def _assert_ground_outputs(r, rows, mu, where, fz_floor=0.0):
    """Everything the ground records against the rule applied to the run's own commands."""
    ua, flags, demand, scaled = _model(r["u0"], rows, mu, fz_floor)
    for k in range(K):
        gc.assert_applied(r["u_applied"][k], r["contact_flags"][k], ua[k], flags[k], scaled[k], (where, k))
    first, slip, unloaded, mu_demand = gc.reduce(flags, demand)
    assert r["first_slip"].dtype == np.int32 and r["slip_periods"].dtype == np.int32 and r["mu_demand"].dtype == np.float32
    assert np.array_equal(r["first_slip"], first) and np.array_equal(r["slip_periods"], slip), where
    assert np.array_equal(r["unloaded_periods"], unloaded) and np.array_equal(r["mu_demand"], mu_demand, equal_nan=True), where
    return flags, demand


def _check_periods(s, x0, foot0, t0, r, steps, gait=None):
    """Per period, from the recorded state before it: a cold solve reproduces the recorded COMMAND bit for bit, the model at the
    recorded u_applied reproduces the next state within 2 ulps, the landing rule reproduces the footholds."""
    import torch
    h, dt, half = s.h, float(s.cparams.dt), int(s.cparams.half)
    gait_kw = _gait_kw(gait)
    gait = (2 * half, (0, half), (half, half)) if gait is None else gait
    push = _push(x0.shape[0])
    ts = sim._times(t0, dt)
    worst = 0.0
    for k in range(K):
        xs = x0 if k == 0 else r["x"][k - 1]
        fs = foot0 if k == 0 else r["foot"][k - 1]
        phase, contact = s.contact_sequence_device(sim._cuda(ts[k], np.float64), **gait_kw)
        s.reset_warm_start()
        u, _ = s.solve_device(sim._cuda(xs, np.float32), sim._cuda(fs, np.float32), contact, phase)
        assert torch.equal(u[:, 0, :].cpu(), torch.from_numpy(r["u0"][k])), ("u0", k)
        active = PUSH_FROM <= k < PUSH_FROM + PUSH_STEPS
        ref = pm.step_batch(xs, r["u_applied"][k], fs, _np(contact[:, 0, :]), push if active else None, dt=dt)
        d = pm.ulp_diff(r["x"][k], ref)
        worst = max(worst, d.max())
        assert d.max() <= 2.0, ("x", k, d.max())
        for b in range(x0.shape[0]):
            fr, lands = pm.landing(r["x"][k][b].astype(np.float64), fs[b], int(steps[k][b]), int(steps[k + 1][b]), *gait, h=h, dt=dt,
                                   kv=float(s.cparams.kv), cmd=(float(s.cparams.x_cmd[3]), float(s.cparams.x_cmd[4])))
            assert pm.ulp_diff(r["foot"][k][b], fr, atol=0.0).max() <= 1.0, ("foot", k, b)
            for g in range(2):
                if not lands[g]:
                    assert np.array_equal(r["foot"][k][b, 3 * g:3 * g + 3], fs[b, 3 * g:3 * g + 3])
    assert np.array_equal(r["t_end"], ts[K]) and np.array_equal(r["x_end"], r["x"][K - 1]) and np.array_equal(r["foot_end"], r["foot"][K - 1])
    return worst


TRAJ = ("u0", "x", "foot", "iters")
GROUND = ("u_applied", "contact_flags", "first_slip", "slip_periods", "unloaded_periods", "mu_demand")


# Start, push and gait of the closed-loop test.  Where the controller wants no vertical force from a stance leg (a body above its
# commanded height) the force bound is active and ADMM leaves fz at -1e-6 .. -1e-12: the ground rightly calls that leg unloaded.  How
# many instances never meet that in 12 periods depends on the start and the gait; at seed 6 it is 42 of 67 at h = 10 under the
# default gait, and 48 of 67 at h = 7 under a gait of period 4 (16 under its default of period 6) -- docs/history_r18.md.
SEED = 6
GAITS = {10: None, 7: (4, (0, 2), (2, 2))}


@pytest.mark.parametrize("h,path", [(10, 1), (7, 2)])
def test_simulate_on_a_ground(h, path):
    B = 67
    s = sim._solver(h, path)
    assert s._lib.bmpc_solver_path(s._h) == path
    x0, foot0, t0 = sim._start(B, SEED)
    gait = GAITS[h]
    rows, steps, _ = _contact_rows(s, t0, gait)
    _run_g = lambda *a, **kw: _run(*a, **kw, **_gait_kw(gait))
    inf = np.full((B, 2), np.inf)

    # run A: no friction limit.  Its records are the rule applied to its own commands.
    A = _run_g(s, x0, foot0, t0, mu=inf)
    flags_a, demand_a = _assert_ground_outputs(A, rows, inf, "A")
    assert (A["first_slip"] == -1).all() and not A["slip_periods"].any() and (A["status_any"] & 2 == 0).all()
    # ... and where the ground never stepped in, the run is the plain one bit for bit
    plain = _run_g(s, x0, foot0, t0)
    assert "u_applied" not in plain
    clean = (flags_a == 0).all(0)
    print("h %d: instances the ground never touched %d of %d; unloaded periods per leg %s; demand %.3f .. %.3f" % (
        h, clean.sum(), B, A["unloaded_periods"].sum(0), np.nanmin(A["mu_demand"]), np.nanmax(A["mu_demand"])))
    assert clean.sum() >= (B + 1) // 2
    for key in TRAJ:
        assert np.array_equal(plain[key][:, clean], A[key][:, clean]), key
    for key in ("status_any", "x_end", "foot_end", "t_end"):
        assert np.array_equal(plain[key][clean], A[key][clean]), key
    worst = _check_periods(s, x0, foot0, t0, A, steps, gait)

    # run B: half the friction each instance asked for.  It slips first where the rule says so on run A's commands, and is run A
    # until then.
    finite = np.isfinite(A["mu_demand"])
    assert finite.sum() > B // 2
    mu_b = np.where(finite, 0.5 * A["mu_demand"].astype(np.float64), np.inf)[:, None].repeat(2, 1)
    Bn = _run_g(s, x0, foot0, t0, mu=mu_b)
    slips = (_model(A["u0"], rows, mu_b)[1] & 3) != 0
    first = np.where(slips.any(0), slips.argmax(0), -1)
    assert np.array_equal(Bn["first_slip"], first) and (first[finite] >= 0).all()
    for b in range(B):
        upto = K if first[b] < 0 else first[b]
        for key in TRAJ + ("u_applied", "contact_flags"):
            assert np.array_equal(Bn[key][:upto, b], A[key][:upto, b], equal_nan=key == "u_applied"), (key, b)
        if first[b] >= 0:
            assert np.array_equal(Bn["u0"][upto, b], A["u0"][upto, b]), b       # (the slipping period starts from the same state)
    _assert_ground_outputs(Bn, rows, mu_b, "B")
    assert np.isfinite(Bn["x"]).all()
    worst = max(worst, _check_periods(s, x0, foot0, t0, Bn, steps, gait))
    print("h %d: first slip at periods %s; x against the model at u_applied: max ulps %.4f" % (h, np.bincount(first[first >= 0], minlength=K), worst))

    # run C: twice the friction each instance asked for is as good as no limit
    mu_c = np.where(finite, 2.0 * A["mu_demand"].astype(np.float64), np.inf)[:, None].repeat(2, 1)
    Cn = _run_g(s, x0, foot0, t0, mu=mu_c)
    for key in TRAJ + GROUND + ("status_any", "x_end", "foot_end", "t_end"):
        assert np.array_equal(Cn[key], A[key], equal_nan=True), key

    # one bad ground: BMPC_NUMERICAL for that instance, the other 66 as in the clean run
    bad = inf.copy()
    bad[5, 1] = np.nan
    D = _run_g(s, x0, foot0, t0, mu=bad)
    assert D["status_any"][5] & 2 and np.isnan(D["x"][:, 5]).all() and np.isnan(D["u_applied"][:, 5]).all()
    assert not D["contact_flags"][:, 5].any() and D["first_slip"][5] == -1 and np.isnan(D["mu_demand"][5])
    keep = np.arange(B) != 5
    for key in TRAJ + ("u_applied", "contact_flags"):
        assert np.array_equal(D[key][:, keep], A[key][:, keep], equal_nan=True), key
    for key in GROUND[2:] + ("status_any",):
        assert np.array_equal(D[key][keep], A[key][keep], equal_nan=True), key


def test_ground_with_bodies_and_fall_keeps_both():
    """The body stays optional and the fall outcome is still reduced: with a ground that never steps in (mu = +inf, instances without
    an unloaded leg) the run with bodies and `fall=` is the existing one bit for bit, outcome included; fz_floor reaches the demand."""
    B = 67
    s = sim._solver(10, 1)
    x0, foot0, t0 = sim._start(B)
    body = bc.bodies(B)
    body["m"] = 10.0 + (body["m"] - 8.0) * (5.0 / 12.0)
    dbody = {k: _dev(v) for k, v in body.items()}
    # thresholds at the medians of the run itself: both classes are non-empty by construction
    first_run = _run(s, x0, foot0, t0, body=dbody)
    fall = (float(np.median(np.abs(first_run["x"][:, :, 0:2]).max((0, 2)))), float(np.median(first_run["x"][:, :, 5].min(0))))
    base = _run(s, x0, foot0, t0, body=dbody, fall=fall)
    r = _run(s, x0, foot0, t0, mu=np.full((B, 2), np.inf), body=dbody, fall=fall, fz_floor=30.0)
    clean = (r["contact_flags"] == 0).all(0)
    print("instances the ground never touched", clean.sum(), "of", B, "fallen", (base["first_fall"] >= 0).sum())
    assert clean.any() and (base["first_fall"] >= 0).any() and (base["first_fall"] < 0).any()
    for key in TRAJ:
        assert np.array_equal(base[key][:, clean], r[key][:, clean]), key
    for key in ("first_fall", "max_tilt", "min_z", "status_any"):
        assert np.array_equal(base[key][clean], r[key][clean], equal_nan=True), key
    first, mt, mz = bc.outcome(r["x"], *fall)
    assert np.array_equal(r["first_fall"], first) and np.array_equal(r["max_tilt"], mt, equal_nan=True)
    assert np.array_equal(r["min_z"], mz, equal_nan=True)
    rows, _, _ = _contact_rows(s, t0)
    inf = np.full((B, 2), np.inf)
    _assert_ground_outputs(r, rows, inf, "floor", fz_floor=30.0)
    # (the floor matters on these commands: without it other legs decide the demand)
    assert not np.array_equal(gc.reduce(*_model(r["u0"], rows, inf)[1:3])[3], r["mu_demand"], equal_nan=True)


def test_malformed_device_grounds_are_value_errors():
    import torch
    B = 8
    s = sim._solver(10, 0)
    x, _, foot, _, _ = pm.batch(B)
    u, c = gc.controls(B)
    dx, du, df, dc = (sim._cuda(a, t) for a, t in ((x, np.float32), (u, np.float32), (foot, np.float32), (c, np.uint8)))
    x0, foot0, t0 = sim._start(B)
    good = _dev(gc.grounds(B))
    wide = torch.ones((B, 4), dtype=torch.float64, device="cuda")
    for mu in (good.float(), good[:-1], good.reshape(2, B), wide[:, :2], good.cpu(), gc.grounds(B), 0.5):
        with pytest.raises(ValueError):
            s.plant_step_device(dx, du, df, dc, ground=dict(mu=mu))
        with pytest.raises(ValueError):
            s.simulate_device(sim._cuda(x0, np.float32), sim._cuda(foot0, np.float32), sim._cuda(t0, np.float64), 2, ground=dict(mu=mu))
    r = s.simulate_device(sim._cuda(x0, np.float32), sim._cuda(foot0, np.float32), sim._cuda(t0, np.float64), 0, ground={})
    torch.cuda.synchronize()                            # no period: as the entry would initialise them
    assert (r["first_slip"] == -1).all() and not r["slip_periods"].any() and torch.isnan(r["mu_demand"]).all()
    assert r["u_applied"].shape == (0, B, 12) and r["contact_flags"].shape == (0, B)


def test_rollout_is_unchanged_by_a_simulation_on_a_ground_on_the_same_handle():
    import torch
    B = 67
    s = sim._solver(10, 0)
    x0, foot0, t0 = sim._start(B)

    def rollout():
        s.reset_warm_start()
        x, f, t = sim._cuda(x0, np.float32), sim._cuda(foot0, np.float32), sim._cuda(t0, np.float64)
        r = s.rollout_device(x, f, t, 6)
        torch.cuda.synchronize()
        return [v.cpu().numpy() for v in (r["u0"], r["x"], r["iters"], r["status_any"], x, t)]

    before = rollout()
    s.reset_warm_start()
    _run(s, x0, foot0, t0, mu=gc.grounds(B))
    after = rollout()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
