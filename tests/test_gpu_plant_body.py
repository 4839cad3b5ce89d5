"""GPU: the plant with a body per instance (`plant_step`, `plant_step_device`, `simulate_device` with `body=`) against the NumPy
restatement at each instance's body (tests/body_cases.py over tests/plant_model.py), and the fall outcome (`fall=`) against its
restatement on the recorded trajectory.  The closed loop is checked like tests/test_gpu_simulate.py checks it, as the composition of
verified parts: per recorded period a cold solve reproduces the applied control bit for bit (the controller saw nothing of the body),
the model at the instance's body reproduces the next state within 2 fp32 ulps, the landing rule reproduces the footholds -- so no
error accumulates and no closed-loop tolerance is needed.  The 2-ulp bound is the plant's own (both sides compute in fp64, only the
final rounding can differ; cond(I) <= 48 keeps the inverse's error nine orders below an fp32 ulp: tests/test_plant_body_cpu.py)."""
import numpy as np
import pytest

from tests import body_cases as bc
from tests import plant_model as pm
from tests import test_gpu_simulate as sim

pytestmark = pytest.mark.gpu
K = sim.K


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _dev(body):
    return {k: sim._cuda(v, np.float64) for k, v in body.items()}


def _take(body, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in body.items()}


@pytest.mark.parametrize("B", [67, 257])
def test_plant_step_with_bodies(B):
    """A partial wave and a block boundary: host entry == device entry bit for bit, both within 2 ulps of the model at the body; a
    permuted batch gives the permuted result; an empty body is the existing entry, a body equal to the handle's own values is within
    one ulp of it (both sit within half an ulp of the same fp64 result, up to fp64 rounding)."""
    import torch
    s = sim._solver(10, 0)
    x, u, foot, c, w = pm.batch(B)
    full = bc.bodies(B)
    perm = np.random.default_rng(3).permutation(B)
    own = dict(m=np.full(B, s.cparams.m), I=np.tile(np.asarray(s.cparams.I, np.float64), (B, 1)), g=np.full(B, s.cparams.g))
    for integrator in ("euler", "rk4"):
        for wr in (w, None):
            tag = (integrator, "wrench" if wr is not None else "none")
            kw = dict(integrator=integrator, substeps=4)
            dx, du, df, dc = (sim._cuda(a, t) for a, t in ((x, np.float32), (u, np.float32), (foot, np.float32), (c, np.uint8)))
            dw = None if wr is None else sim._cuda(wr, np.float32)
            base = s.plant_step(x, u, foot, c, wr, **kw)
            for members in ((bc.MEMBERS,) if B > 67 else (("m",), ("I",), ("g",), bc.MEMBERS)):      # (the full body last)
                body = bc.subset(full, members)
                host = s.plant_step(x, u, foot, c, wr, body=body, **kw)
                dev = s.plant_step_device(dx, du, df, dc, dw, body=_dev(body), **kw)
                torch.cuda.synchronize()
                assert np.array_equal(host.astype(np.float32), dev.cpu().numpy()), (tag, members)
                ref = bc.step_batch(x, u, foot, c, wr, body=body, **kw)
                d = pm.ulp_diff(dev.cpu().numpy(), ref)
                print(*tag, "+".join(members), "max ulps", d.max())
                assert d.max() <= 2.0, (tag, members, d.max())
            # the permuted batch
            got = s.plant_step(x[perm], u[perm], foot[perm], c[perm], None if wr is None else wr[perm], body=_take(full, perm), **kw)
            assert np.array_equal(got, host[perm]), tag
            # the flat (B,9) inertia is the same body
            flat = dict(full, I=full["I"].reshape(B, 9))
            assert np.array_equal(s.plant_step(x, u, foot, c, wr, body=flat, **kw), host), tag
            # no member: the existing kernel; the handle's own values: another kernel, the same fp64 result
            assert np.array_equal(s.plant_step(x, u, foot, c, wr, body={}, **kw), base), tag
            assert torch.equal(s.plant_step_device(dx, du, df, dc, dw, body={}, **kw), s.plant_step_device(dx, du, df, dc, dw, **kw)), tag
            same = s.plant_step(x, u, foot, c, wr, body=own, **kw)
            print(*tag, "body = the handle's: identical share %.4f" % (same == base).mean())
            assert pm.ulp_diff(same.astype(np.float32), base).max() <= 1.0, tag


def _loop_bodies(B):
    """bodies(B) with m narrowed to [10, 15], so that the controller (which believes in 12 kg) keeps the loop on its feet."""
    body = bc.bodies(B)
    body["m"] = 10.0 + (body["m"] - 8.0) * (5.0 / 12.0)
    return body


def _check_periods(s, x0, foot0, t0, r, body):
    """(a) - (d) of tests/test_gpu_simulate.py for every period, the model taken at each instance's body; returns the landings per leg."""
    import torch
    h, dt, half = s.h, float(s.cparams.dt), int(s.cparams.half)
    gait = (2 * half, (0, half), (half, half))
    ts = sim._times(t0, dt)
    landed = np.zeros(2, int)
    worst = 0.0
    for k in range(K):
        xs = x0 if k == 0 else r["x"][k - 1]
        fs = foot0 if k == 0 else r["foot"][k - 1]
        phase, contact = s.contact_sequence_device(sim._cuda(ts[k], np.float64))
        s.reset_warm_start()
        u, _ = s.solve_device(sim._cuda(xs, np.float32), sim._cuda(fs, np.float32), contact, phase)
        assert torch.equal(u[:, 0, :].cpu(), torch.from_numpy(r["u0"][k])), ("u0", k)                              # (a)
        ref = bc.step_batch(xs, r["u0"][k], fs, contact[:, 0, :].cpu().numpy(), None, body=body, dt=dt)
        d = pm.ulp_diff(r["x"][k], ref)
        worst = max(worst, d.max())
        assert d.max() <= 2.0, ("x", k, d.max())                                                                   # (b)
        k0 = phase.cpu().numpy()
        k1 = s.contact_sequence_device(sim._cuda(ts[k + 1], np.float64))[0].cpu().numpy()
        for b in range(x0.shape[0]):
            fr, lands = pm.landing(r["x"][k][b].astype(np.float64), fs[b], int(k0[b]), int(k1[b]), *gait, h=h, dt=dt,
                                   kv=float(s.cparams.kv), cmd=(float(s.cparams.x_cmd[3]), float(s.cparams.x_cmd[4])))
            assert pm.ulp_diff(r["foot"][k][b], fr, atol=0.0).max() <= 1.0, ("foot", k, b)                         # (c)
            for g in range(2):
                if not lands[g]:
                    assert np.array_equal(r["foot"][k][b, 3 * g:3 * g + 3], fs[b, 3 * g:3 * g + 3])
                landed[g] += lands[g]
    assert np.array_equal(r["t_end"], ts[K])                                                                      # (d)
    assert np.array_equal(r["x_end"], r["x"][K - 1]) and np.array_equal(r["foot_end"], r["foot"][K - 1])
    print("closed loop: max ulps over the periods", worst)
    return landed


@pytest.mark.parametrize("h,path", [(10, 1), (7, 2)])
def test_simulate_with_bodies_is_the_composition_of_verified_parts(h, path):
    B = 67
    s = sim._solver(h, path)
    assert s._lib.bmpc_solver_path(s._h) == path
    x0, foot0, t0 = sim._start(B)
    body = _loop_bodies(B)
    r = sim._simulate(s, x0, foot0, t0, body=_dev(body))
    assert (r["status_any"] & 2 == 0).all() and np.isfinite(r["x"]).all()
    # the loop stays on its feet: the step of a body that tumbles through pitch = +-90 degrees is ill-conditioned (rates over cos e1),
    # for the kernel and the model alike, and says nothing about either (measured: 0.400 rad at h = 10, 0.224 at h = 7)
    assert np.abs(r["x"][:, :, 1]).max() < 1.0
    landed = _check_periods(s, x0, foot0, t0, r, body)
    assert (landed >= B // 2).all(), landed
    plain = sim._simulate(s, x0, foot0, t0)
    assert np.array_equal(plain["u0"][0], r["u0"][0])                  # the first solve saw the same state
    for k in range(K):
        assert not np.array_equal(plain["x"][k], r["x"][k]), k         # ... and the bodies show from period 0 on


def _assert_outcome(r, tilt_max, z_min):
    first, mt, mz = bc.outcome(r["x"], tilt_max, z_min)
    assert r["first_fall"].dtype == np.int32 and r["max_tilt"].dtype == np.float32 and r["min_z"].dtype == np.float32
    assert np.array_equal(r["first_fall"], first)
    assert np.array_equal(r["max_tilt"], mt, equal_nan=True) and np.array_equal(r["min_z"], mz, equal_nan=True)


def test_fall_outcome_is_the_restatement_on_the_recorded_trajectory():
    B = 67
    s = sim._solver(10, 1)
    x0, foot0, t0 = sim._start(B)
    body = _loop_bodies(B)
    plain = sim._simulate(s, x0, foot0, t0, body=_dev(body))
    assert "first_fall" not in plain
    # thresholds at the medians of the run itself: both classes are non-empty by construction
    z_min = float(np.median(plain["x"][:, :, 5].min(0)))
    tilt_max = float(np.median(np.abs(plain["x"][:, :, 0:2]).max((0, 2))))
    fallen = bc.outcome(plain["x"], tilt_max, z_min)[0] >= 0
    print("thresholds", tilt_max, z_min, "fallen", fallen.sum(), "of", B)
    assert fallen.sum() >= B / 4 and (~fallen).sum() >= B / 4
    r = sim._simulate(s, x0, foot0, t0, body=_dev(body), fall=(tilt_max, z_min))
    for key in ("u0", "x", "foot", "iters", "status_any", "x_end", "foot_end", "t_end"):
        assert np.array_equal(plain[key], r[key]), key
    _assert_outcome(r, tilt_max, z_min)
    assert np.array_equal(r["first_fall"] >= 0, fallen) and np.isfinite(r["max_tilt"]).all() and np.isfinite(r["min_z"]).all()
    # the outcome alone, on the handle's own body: simulate_body_feedback_kernel with null body pointers next to
    # simulate_feedback_kernel, whose period it writes out a second time.  The first period starts from the same state: the same
    # control and iteration count, the state within one ulp (both within half an ulp of the same fp64 result) and the footholds,
    # taken at that state, with it; a bookkeeping step that drifted apart would show at once.  Later periods compare only while
    # the states are identical, which is printed.
    own = sim._simulate(s, x0, foot0, t0, fall=(tilt_max, z_min))
    _assert_outcome(own, tilt_max, z_min)
    assert np.isfinite(own["max_tilt"]).all() and np.isfinite(own["min_z"]).all()
    base = sim._simulate(s, x0, foot0, t0)
    same = [k for k in range(K) if all(np.array_equal(base[key][k], own[key][k]) for key in ("u0", "x", "foot", "iters"))]
    print("null body against the existing kernel: identical periods", len(same), "of", K)
    assert np.array_equal(base["u0"][0], own["u0"][0]) and np.array_equal(base["iters"][0], own["iters"][0])
    assert pm.ulp_diff(own["x"][0], base["x"][0].astype(np.float64)).max() <= 1.0
    assert np.abs(own["foot"][0].astype(np.float64) - base["foot"][0]).max() <= 2.0 * np.spacing(np.float32(1.0))
    assert np.array_equal(base["t_end"], own["t_end"]) and np.array_equal(base["status_any"], own["status_any"])
    # one bad body: fallen at once, no extremum, BMPC_NUMERICAL, and no neighbour touched
    bad = {k: v.copy() for k, v in body.items()}
    bad["m"][5] = np.nan
    rb = sim._simulate(s, x0, foot0, t0, body=_dev(bad), fall=(tilt_max, z_min))
    assert rb["first_fall"][5] == 0 and np.isnan(rb["max_tilt"][5]) and np.isnan(rb["min_z"][5])
    assert rb["status_any"][5] & 2 and np.isnan(rb["x"][:, 5]).all()
    keep = np.arange(B) != 5
    for key in ("x", "u0", "foot"):
        assert np.array_equal(rb[key][:, keep], r[key][:, keep]), key
    for key in ("status_any", "first_fall", "max_tilt", "min_z"):
        assert np.array_equal(rb[key][keep], r[key][keep]), key        # (finite: the clean run is)


def test_malformed_device_bodies_are_value_errors():
    """`plant_step_device` and `simulate_device` check a body before any library call: dtype, shape, contiguity, device, keys."""
    import torch
    B = 8
    s = sim._solver(10, 0)
    x, u, foot, c, _ = pm.batch(B)
    dx, du, df, dc = (sim._cuda(a, t) for a, t in ((x, np.float32), (u, np.float32), (foot, np.float32), (c, np.uint8)))
    x0, foot0, t0 = sim._start(B)
    good = _dev(bc.bodies(B))
    wide = torch.ones((B, 2), dtype=torch.float64, device="cuda")
    bad = [dict(m=good["m"].float()), dict(m=good["m"][:-1]), dict(g=good["g"].reshape(B, 1)), dict(I=good["I"].reshape(B, 9)[:, :8]),
           dict(I=good["I"].transpose(1, 2)), dict(m=wide[:, 0]), dict(m=good["m"].cpu()), dict(g=bc.bodies(B)["g"]),
           dict(mass=good["m"]), [good["m"]]]
    for body in bad:
        with pytest.raises(ValueError):
            s.plant_step_device(dx, du, df, dc, body=body)
        with pytest.raises(ValueError):
            s.simulate_device(sim._cuda(x0, np.float32), sim._cuda(foot0, np.float32), sim._cuda(t0, np.float64), 2, body=body)
    s.plant_step_device(dx, du, df, dc, body=dict(I=good["I"].reshape(B, 9)))         # (the flat form is well-formed)
    torch.cuda.synchronize()


def test_rollout_is_unchanged_by_a_simulation_with_bodies_on_the_same_handle():
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
    sim._simulate(s, x0, foot0, t0, body=_dev(_loop_bodies(B)), fall=(0.3, 0.4))
    after = rollout()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_time_per_period_with_and_without_bodies():
    """Printed, not asserted (docs/history_r17.md): B = 4096, h = 10, 20 periods, with events, the two variants interleaved on one
    handle.  The feedback step is one thread per instance next to a solve of about 0.8 ms per period."""
    import torch
    B, steps = 4096, 20
    s = sim._solver(10, 1, max_batch=B)
    x0, foot0, t0 = sim._start(B)
    body = _dev(_loop_bodies(B))
    variants = {"plain": {}, "bodies": dict(body=body), "bodies+fall": dict(body=body, fall=(0.3, 0.4))}
    ms = {k: [] for k in variants}
    for rep in range(4):
        for name, kw in variants.items():
            x, f, t = sim._cuda(x0, np.float32), sim._cuda(foot0, np.float32), sim._cuda(t0, np.float64)
            s.reset_warm_start()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.simulate_device(x, f, t, steps, **kw)
            e1.record()
            torch.cuda.synchronize()
            if rep:                                    # (the first round warms up)
                ms[name].append(e0.elapsed_time(e1) / steps)
    for name, v in ms.items():
        print("simulate_device B %d h 10: %-12s %.4f ms per period (median of %d, min %.4f, max %.4f)"
              % (B, name, float(np.median(v)), len(v), min(v), max(v)))
