"""GPU: S candidate plans per instance rolled out on the plant (`plant_rollout_samples`, `plant_rollout_samples_device`) against the
NumPy restatement (tests/rollout_cases.py) and against the chain of `plant_step_device` calls it replaces.

Bounds.  Per period against the model, from the RECORDED state before it: 2 fp32 ulps, the plant tests' bound (both sides compute in
fp64: only the final rounding can differ, the second ulp is margin).  Against the chain: 1 fp32 ulp -- both are one fp32 rounding of
fp64 values that agree far below an fp32 ulp; bit equality is expected and the count of differing entries is printed.  Flags, the
ground's reductions, the outcome: rules on stored values, exact.  foot_end: to the bit where no leg landed, within 1 fp32 ulp on a
landed coordinate (the target's fp64 expression may be associated or contracted differently); which happened is printed.  cost
against a long-double recomputation from x_traj, the controls and the reference: (24 h + 4) 2^-52 relative (non-negative terms, fixed
order); score: sample_cases.SCORE_REL; the reductions: sample_cases.reduce_bound(S) on the kernel's own scores."""
import ctypes as C

import numpy as np
import pytest

from tests import plant_model as pm
from tests import rollout_cases as rc
from tests import sample_cases as sc

pytestmark = pytest.mark.gpu
_SOLVERS = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()
    yield
    for s in _SOLVERS.values():
        s.close()
    _SOLVERS.clear()


def _solver(h):
    if h not in _SOLVERS:
        import biped_mpc_py_amd as bm
        mpc = bm.MPC()
        mpc.h = h
        _SOLVERS[h] = bm.BatchSolver(mpc=mpc, biped=bm.Biped(), max_batch=512)
    return _SOLVERS[h]


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _device_kw(kw):
    """The keyword arguments of the host method as the device method takes them."""
    out = dict(kw)
    for k in ("x_cmd", "x_ref", "push"):
        if out.get(k) is not None:
            out[k] = _cuda(out[k], np.float32)
    if out.get("body") is not None:
        out["body"] = {m: _cuda(v, np.float64) for m, v in out["body"].items()}
    if out.get("ground") is not None:
        out["ground"] = {m: _cuda(v, np.float64) for m, v in out["ground"].items()}
    return out


def _device(s, args, kw):
    import torch
    x, f, c, u = args
    r = s.plant_rollout_samples_device(_cuda(x, np.float32), _cuda(f, np.float32), _cuda(c, np.uint8), _cuda(u, np.float32), **_device_kw(kw))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(a, b, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


def _args(c, U, idx=slice(None)):
    return c["x_fb"][idx], c["foot"][idx], c["contact"][idx], U[idx]


PRICES = dict(w_fall=rc.W_FALL, w_slip=rc.W_SLIP, w_unloaded=rc.W_UNLOADED, fall=(0.25, 0.3))


@pytest.mark.parametrize("h,shape,integrator,substeps,name", [
    (10, (5, 13), "rk4", 4, "full"), (10, (5, 67), "euler", 1, "plain"), (10, (1, 1), "euler", 4, "full"), (3, (5, 67), "rk4", 4, "full"),
    (3, (5, 13), "rk4", 1, "plain"), (1, (5, 67), "rk4", 4, "plain"), (1, (1, 1), "euler", 1, "full")])
def test_every_period_matches_the_model(h, shape, integrator, substeps, name):
    """1, 3: x_traj per period, flags and reductions, outcome, foot_end, cost and score (rollout_cases.check)."""
    s = _solver(h)
    p = rc.params_of(s.cparams)
    c = rc.case(h)
    B, S = shape
    idx = slice(0, B) if B > 1 else slice(4, 5)
    U = rc.plans(c, S)
    kw = dict(rc.take(rc.variant(c, name), idx), integrator=integrator, substeps=substeps, **PRICES)
    if name == "full":
        kw["fz_floor"] = 20.0
    got = _device(s, _args(c, U, idx), kw)
    assert set(got) == set(rc.PER_SAMPLE + rc.REDUCED + (rc.GROUND_ONLY if name == "full" else ()))
    rc.check(p, got, _args(c, U, idx), kw, (h, shape, integrator, substeps, name))
    assert np.isfinite(got["cost"]).all()


@pytest.mark.parametrize("h,name", [(10, "full"), (3, "plain")])
def test_rollout_is_the_chain_of_plant_steps(h, name):
    """2: period k of every plan against `plant_step_device` from the recorded state before it on B S replicated instances."""
    s = _solver(h)
    p = rc.params_of(s.cparams)
    c = rc.case(h)
    S = 67
    U = rc.plans(c, S)
    kw = rc.variant(c, name)
    got = _device(s, _args(c, U), dict(kw, want=["x_traj"]))
    xt = got["x_traj"]
    feet = rc.footholds(p, c["foot"], c["contact"], xt, kw.get("x_cmd"))
    rep = lambda a: np.repeat(np.asarray(a), S, axis=0)
    body = None if "body" not in kw else {m: _cuda(rep(v), np.float64) for m, v in kw["body"].items()}
    ground = None if "ground" not in kw else {m: _cuda(rep(v), np.float64) for m, v in kw["ground"].items()}
    differing = total = 0
    worst = 0.0
    for k in range(h):
        xs = rep(c["x_fb"]) if k == 0 else xt[:, :, k - 1].reshape(-1, 12)
        active = "push" in kw and rc.PUSH_FROM <= k < rc.PUSH_FROM + rc.PUSH_STEPS
        step = s.plant_step_device(_cuda(xs, np.float32), _cuda(U[:, :, k].reshape(-1, 12), np.float32), _cuda(feet[:, :, k].reshape(-1, 6), np.float32),
                                   _cuda(rep(c["contact"][:, k]), np.uint8), _cuda(rep(c["push"]), np.float32) if active else None,
                                   body=body, ground=ground).cpu().numpy()
        mine = xt[:, :, k].reshape(-1, 12)
        differing += int((step.view(np.uint32) != mine.view(np.uint32)).sum())
        total += mine.size
        worst = max(worst, float(pm.ulp_diff(mine, step.astype(np.float64), atol=0.0).max()))
    print("rollout against the chain", (h, name), f"{differing} of {total} entries differ, max ulps {worst}")
    assert worst <= 1.0


def test_supplied_generated_reference_gives_the_generated_bits():
    """3: x_ref = the generated reference (`reference_trajectories_batch`) against x_ref=None.  The supplied rows are fp32, so the
    case is one whose generated rows are fp32 values: per-instance commands with every rate command zero (rows k > 0 are then the
    commands themselves, row 0 is x_fb)."""
    import biped_mpc_py_amd as bm
    h = 10
    s = _solver(h)
    c = rc.case(h)
    x_cmd = c["x_cmd"].copy()
    x_cmd[:, 6:] = 0.0
    mpc = bm.MPC()
    mpc.h = h
    xr, _ = bm.reference_trajectories_batch(c["x_fb"], None, c["foot"], c["contact"], mpc=mpc, biped=bm.Biped(), x_cmd=x_cmd,
                                            phase=np.zeros(rc.N, np.int32))
    xr, _ = bm.references_to_kernel_layout(xr, None, h)
    assert np.array_equal(xr, xr.astype(np.float32)) and np.array_equal(xr, rc.references(rc.params_of(s.cparams), c["x_fb"], x_cmd))
    U = rc.plans(c, 13)
    gen = _device(s, _args(c, U), dict(x_cmd=x_cmd, **PRICES))
    sup = _device(s, _args(c, U), dict(x_cmd=x_cmd, x_ref=xr, **PRICES))
    _same(gen, sup)
    off = _device(s, _args(c, U), dict(x_cmd=x_cmd, x_ref=xr + np.float32(0.01), **PRICES))
    assert (off["cost"] != gen["cost"]).all() and np.array_equal(off["x_traj"], gen["x_traj"])


def test_a_plan_does_not_depend_on_its_place():
    """4: sample (b, s) of the (5, 13) launch has the bits of the same plan alone and inside (5, 67); a permuted batch gives the
    permuted result."""
    h = 10
    s = _solver(h)
    c = rc.case(h)
    kw = dict(rc.variant(c, "full"), **PRICES)
    U13, U67 = rc.plans(c, 13), rc.plans(c, 67)
    assert np.array_equal(U13, U67[:, :13])
    mid, big = _device(s, _args(c, U13), kw), _device(s, _args(c, U67), kw)
    per_sample = rc.PER_SAMPLE + rc.GROUND_ONLY
    for k in per_sample:
        assert np.array_equal(mid[k], big[k][:, :13], equal_nan=True), k
    for b, j in ((0, 0), (2, 3), (4, 12), (1, 7), (3, 4)):
        one = s.plant_rollout_samples(*_args(c, U13[:, j:j + 1], [b]), **rc.take(kw, [b]))
        for k in per_sample:
            assert np.array_equal(one[k][0, 0], mid[k][b, j], equal_nan=True), (b, j, k)
    perm = np.random.default_rng(3).permutation(rc.N)
    shuffled = _device(s, _args(c, U13, perm), rc.take(kw, perm))
    for k in shuffled:
        assert np.array_equal(shuffled[k], mid[k][perm], equal_nan=True), k


def test_bad_data_stays_with_its_sample_or_instance():
    """5: one NaN control entry at period 2 of one sample; one bad instance (mu = NaN; separately m = 0)."""
    h = 10
    s = _solver(h)
    c = rc.case(h)
    U = rc.plans(c, 13)
    kw = dict(rc.variant(c, "full"), w_fall=rc.W_FALL, w_slip=rc.W_SLIP, w_unloaded=rc.W_UNLOADED)
    clean = _device(s, _args(c, U), kw)
    assert np.isfinite(clean["cost"]).all() and (clean["first_fall"] == -1).all() and (clean["n_valid"] == 13).all()
    per_sample = rc.PER_SAMPLE + rc.GROUND_ONLY
    bad = U.copy()
    bad[1, 5, 2, 7] = np.nan
    got = _device(s, _args(c, bad), kw)
    assert got["first_fall"][1, 5] == 2 and np.isnan(got["cost"][1, 5]) and np.isnan(got["score"][1, 5])
    assert np.isnan(got["x_traj"][1, 5, 2:]).all() and np.array_equal(got["x_traj"][1, 5, :2], clean["x_traj"][1, 5, :2])
    assert np.isnan(got["x_end"][1, 5]).all() and got["weights"][1, 5] == 0 and got["n_valid"].tolist() == [13, 12, 13, 13, 13]
    keep = np.ones((rc.N, 13), bool)
    keep[1, 5] = False
    for k in per_sample:
        assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), k
    others = [0, 2, 3, 4]
    _same({k: got[k][others] for k in rc.REDUCED}, {k: clean[k][others] for k in rc.REDUCED})
    for what in ("mu", "m"):
        kb = dict(kw, body=dict(kw["body"]), ground=dict(kw["ground"]))
        if what == "mu":
            kb["ground"]["mu"] = kw["ground"]["mu"].copy()
            kb["ground"]["mu"][3, 0] = np.nan
        else:
            kb["body"]["m"] = kw["body"]["m"].copy()
            kb["body"]["m"][3] = 0.0
        got = _device(s, _args(c, U), kb)
        assert np.isnan(got["cost"][3]).all() and np.isnan(got["score"][3]).all() and np.isnan(got["x_traj"][3]).all(), what
        assert (got["first_fall"][3] == 0).all() and got["n_valid"][3] == 0 and got["best"][3] == -1, what
        assert not got["weights"][3].any() and np.isnan(got["u_mean"][3]).all() and np.isnan(got["ess"][3]), what
        for k in got:
            assert np.array_equal(got[k][[0, 1, 2, 4]], clean[k][[0, 1, 2, 4]], equal_nan=True), (what, k)


def test_falls_and_slips_both_occur_and_still_match_their_rules():
    """6: thresholds from a first run with everything switched off, so that both outcomes of both splits are well populated."""
    h, S = 3, 67
    s = _solver(h)
    p = rc.params_of(s.cparams)
    c = rc.case(h)
    U = rc.spread_plans(c, S)
    base = dict(x_cmd=c["x_cmd"], push=c["push"], push_from=rc.PUSH_FROM, push_steps=rc.PUSH_STEPS)
    first = _device(s, _args(c, U), dict(base, ground=dict(mu=np.full((rc.N, 2), np.inf))))
    assert (first["first_fall"] == -1).all() and (first["first_slip"] == -1).all()
    tilt_max = float(np.median(first["max_tilt"]))
    mu = 0.5 * float(np.median(first["mu_demand"][np.isfinite(first["mu_demand"])]))
    kw = dict(base, ground=dict(mu=np.full((rc.N, 2), mu)), fall=(tilt_max, -np.inf), **{k: PRICES[k] for k in ("w_fall", "w_slip", "w_unloaded")})
    got = _device(s, _args(c, U), kw)
    fell, slipped = (got["first_fall"] >= 0).mean(), (got["first_slip"] >= 0).mean()
    print("tilt_max", tilt_max, "mu", mu, "fell", fell, "slipped", slipped)
    assert 0.2 <= fell <= 0.8 and 0.2 <= slipped <= 0.8
    rc.check(p, got, _args(c, U), kw, "falls and slips")
    assert (got["score"][got["first_fall"] >= 0] >= rc.W_FALL).all()


@pytest.mark.parametrize("h,S", [(10, 13), (3, 67)])
def test_reductions_match_numpy_on_the_kernels_scores(h, S):
    """7: best, n_valid, weights, u_mean, ess at sample_cases.temperatures, without and with invalid samples."""
    s = _solver(h)
    c = rc.case(h)
    U = rc.plans(c, S)
    kw = dict(rc.variant(c, "full"), **PRICES)
    score = _device(s, _args(c, U), dict(kw, want=["score"]))["score"]
    spoiled = U.copy()
    spoiled[0, ::3, h - 1, 2] = np.inf                 # a third of instance 0's samples
    spoiled[2, :, 0, 9] = np.nan                       # every sample of instance 2
    spoiled[4, S - 1, 0, 0] = np.nan
    for T in sc.temperatures(score):
        for V, tag in ((U, "clean"), (spoiled, "spoiled")):
            got = _device(s, _args(c, V), dict(kw, temperature=T))
            ref = sc.check_reduced(got, V.astype(np.float64), T, (h, S, tag))
            assert np.array_equal(got["score"], score, equal_nan=True) == (tag == "clean")
            if tag == "spoiled":
                assert ref["n_valid"].tolist() == [S - len(range(0, S, 3)), S, 0, S, S - 1] and got["best"][2] == -1
            # without the scores and the weights, from the handle's scratch: the same bits
            few = _device(s, _args(c, V), dict(kw, temperature=T, want=["best", "u_mean", "ess"]))
            assert set(few) == {"best", "u_mean", "ess"}
            _same(few, {k: got[k] for k in few})


def test_the_handle_is_left_alone_and_host_equals_device():
    """8: a closed-loop roll-out before and after; B = 0; the host entry against the device entry."""
    import torch
    h = 10
    s = _solver(h)
    c = rc.case(h)
    U = rc.plans(c, 13)
    kw = dict(rc.variant(c, "full"), **PRICES)

    def closed_loop():
        x, f, t = _cuda(c["x_fb"], np.float32), _cuda(c["foot"], np.float32), _cuda(np.zeros(rc.N), np.float64)
        r = s.rollout_device(x, f, t, 4)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items() if v is not None}, s.last_kernel_ms()

    before, ms = closed_loop()
    host = s.plant_rollout_samples(*_args(c, U), **kw)
    assert s.last_kernel_ms() == ms                     # still the last solve's
    dev = _device(s, _args(c, U), kw)
    _same(host, dev)
    after, _ = closed_loop()
    _same(before, after)
    # B = 0 succeeds, on both entries
    empty = s.plant_rollout_samples(c["x_fb"][:0], c["foot"][:0], c["contact"][:0], U[:0], **rc.take(kw, slice(0, 0)))
    assert empty["cost"].shape == (0, 13) and empty["u_mean"].shape == (0, h, 12)
    empty = _device(s, _args(c, U, slice(0, 0)), rc.take(kw, slice(0, 0)))
    assert empty["x_traj"].shape == (0, 13, h, 12)
    one = torch.zeros(16, device="cuda")
    from biped_mpc_py_amd import _lib
    price = _lib.CRolloutPrice(13, 0, 0.0, 0.0, 0.0, np.inf, np.inf, -np.inf, 0.0)
    out = _lib.CRolloutOut(cost=one.data_ptr())
    a = [one.data_ptr()] * 3 + [None] * 3 + [one.data_ptr(), None, None, None, C.byref(price), C.byref(out)]
    assert s._lib.bmpc_plant_rollout_samples_device(s._h, 0, *a, None) == 0
    assert s._lib.bmpc_plant_rollout_samples_device(s._h, 513, *a, None) == -1 and b"max_batch" in s._lib.bmpc_last_error()
    assert s._lib.bmpc_plant_rollout_samples_device(s._h, 0, *a[:-1], C.byref(_lib.CRolloutOut()), None) == -1
