"""GPU: every kernel held to its reference AWAY from the default parameters (tests/param_cases.py has the cases; the sensitivity of
every (case, entry) pair used here is a CPU test, tests/test_param_cases_cpu.py).
  2. the stage-structured solve family (one wave with phantom slots, one wave, two waves) against the oracle's optima;
  3. evaluate / evaluate_grad / certify through the host and the device entry against the yardsticks at the case;
  4. the plant step against plant_model at the case (the closed loop at a case: tests/test_gpu_simulate.py);
  5. the low-level kernels against the oracle at the case: full gain matrices, hip offset by side, negative times;
  6. `set_params` on a live handle against fresh handles, bit for bit."""
import functools

import numpy as np
import pytest

from tests import certify_cases as cc
from tests import eval_cases as ec
from tests import eval_grad_cases as gc
from tests import gpu_common
from tests import param_cases as pc
from tests import plant_model as pm
from tests import util
from tests.gpu_common import built as _built, dev_args as _dev_args  # noqa: F401 (_built: the autouse fixture)

pytestmark = pytest.mark.gpu

PATH_DENSE, PATH_STAGE = 1, 2


def _solver(name, h, path=0, max_batch=512, half=None):
    import biped_mpc_py_amd as bm
    mpc, biped = pc.objects(bm, name, h=h)
    return bm.BatchSolver(mpc=mpc, biped=biped, half=half, solver_options=dict(path=path) if path else None, max_batch=max_batch)


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


# ---- 2. the stage family against the oracle -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stage_fixture():
    return util.load("param_cases_stage")


@functools.lru_cache(maxsize=None)
def _default_iters(h):
    """Mean iteration count of the stage family on the same inputs at the default parameters."""
    s = pc.stage_batch(h)
    sol = _solver("default", h, PATH_STAGE, half=s["half"])
    _, _, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], want_states=False)
    sol.close()
    return float(info["iters"].mean())


@pytest.mark.parametrize("h", pc.STAGE_HORIZONS)
@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_stage_family_vs_oracle_at_the_case(name, h):
    """h = 7: one wave with phantom step slots; h = 10: the inputs both families take, whose answers must also agree with each other;
    h = 26: the smallest two-wave variant.  Every status 0 and util.rel_err <= util.REL_TOL against `orc.solve_mpc` at the same case on
    the fp32-rounded inputs (tests/golden/param_cases_stage.npz, from tests/gen_param_cases.py).  The iteration count against the
    default parameters is printed, not asserted: convergence speed is not correctness (docs/history_r16.md has the ratios)."""
    s = pc.stage_batch(h)
    f = _stage_fixture()
    assert np.array_equal(f[f"h{h}/x_fb"], s["x_fb"])
    ref = f[f"h{h}/{name}"]
    sol = _solver(name, h, PATH_STAGE, half=s["half"])
    assert sol._lib.bmpc_solver_path(sol._h) == PATH_STAGE
    _, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], want_states=False)
    sol.close()
    rel = util.rel_err(u, ref)
    print("stage %-14s h=%-2d err max %.2e iters mean %.1f max %d ratio to default %.2f" % (
        name, h, rel.max(), info["iters"].mean(), info["iters"].max(), info["iters"].mean() / _default_iters(h)))
    assert (info["status"] == 0).all(), info["status"]
    assert rel.max() <= util.REL_TOL, rel
    if h == 10:
        dense = _solver(name, h, PATH_DENSE, half=s["half"])
        assert dense._lib.bmpc_solver_path(dense._h) == PATH_DENSE
        _, ud, infod = dense.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], want_states=False)
        dense.close()
        both = util.rel_err(u, ud)
        print("stage %-14s h=10 against the dense family %.2e (dense against the oracle %.2e)" % (name, both.max(), util.rel_err(ud, ref).max()))
        assert (infod["status"] == 0).all() and both.max() <= util.REL_TOL, both


# ---- 3. evaluate, evaluate_grad, certify ------------------------------------------------------------------------------------------------

def _both_entries(solver, kind, keys, a, **kw):
    """Host entry and device entry of `kind` on the same arguments: (host result, device result as NumPy)."""
    import torch
    host = getattr(solver, kind)(**a, **kw)
    dev = getattr(solver, kind + "_device")(**_dev_args(a), **kw)
    torch.cuda.synchronize()
    return host, {k: dev[k].cpu().numpy() for k in keys}


@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_evaluation_family_at_the_case(name):
    """h = 10 on both kernel families' handles, h = 13 on the stage family's, h = 26 on the two-wave variant's: 16 instances (at h = 26
    eight of them are compared, param_cases.EVAL_CHECKED) whose controls break every row class and make the case show, through
    `bmpc_evaluate*`, `bmpc_evaluate_grad*` and `bmpc_certify*`, host and device entry (bit-identical to each other), against the
    yardsticks at the case."""
    import biped_mpc_py_amd as bm
    viol = []
    for h, path in pc.EVAL_GROUPS:
        g = pc.eval_group(h, name)
        solver = bm.BatchSolver(cparams=ec.cparams_of(g, path), max_batch=pc.EVAL_B)
        assert solver._lib.bmpc_solver_path(solver._h) == path
        a = ec.kernel_args(g)
        where = f"{g['name']}/path{path}"
        ev_keys = ("cost", "objective", "violation", "states")
        host, dev = _both_entries(solver, "evaluate", ev_keys, a, want_states=True)
        gpu_common.identical(host, dev, where, keys=ev_keys)
        idx = pc.eval_indices(h)
        at = lambda r: {k: v[idx] for k, v in r.items()}
        ref = ec.yardstick_group(g, idx)
        ec.check(at(host), ref, where, reg_bound=pc.PARAM_REG_BOUND)
        viol.append(ref["violation"])
        host, dev = _both_entries(solver, "evaluate_grad", gc.KEYS, a)
        gpu_common.identical(host, dev, where, keys=gc.KEYS)
        gc.check(at(host), gc.yardstick_group(g, idx), where, reg_bound=pc.PARAM_GRAD_REG_BOUND)
        ref, tol = pc.certify_yardstick(g, idx)
        host, dev = _both_entries(solver, "certify", cc.KEYS, a, act_tol=tol)
        gpu_common.identical(host, dev, where, keys=cc.KEYS)
        cc.check(at(host), ref, where, bound=pc.PARAM_CERT_REL_BOUND)
        solver.close()
    v = np.concatenate(viol)
    assert (v.max(0) > 1.0).all() and (v == 0.0).any(), v.max(0)


# ---- 4. the plant -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [67, 257])
@pytest.mark.parametrize("name", pc.PLANT_CASES)
def test_plant_step_matches_the_model_at_the_case(name, B):
    """Euler and RK4, 1 and 4 substeps, with and without a wrench, against plant_model.step_batch at the case's I_b, m, g, dt within
    the derived 2 fp32 ulps + 1e-12; the host entry equals the device entry bit for bit.  B = 257: a partial last workgroup."""
    import torch
    s = _solver(name, 10)
    kw = pc.plant_kw(name)
    x, u, foot, c, w = pm.batch(B)
    worst = 0.0
    for integrator in ("euler", "rk4"):
        for n in (1, 4):
            for wr in (w, None):
                host = s.plant_step(x, u, foot, c, wr, integrator=integrator, substeps=n)
                dev = s.plant_step_device(_cuda(x, np.float32), _cuda(u, np.float32), _cuda(foot, np.float32), _cuda(c, np.uint8),
                                          None if wr is None else _cuda(wr, np.float32), integrator=integrator, substeps=n)
                torch.cuda.synchronize()
                assert np.array_equal(host.astype(np.float32), dev.cpu().numpy()), (integrator, n)
                ref = pm.step_batch(x, u, foot, c, wr, integrator=integrator, substeps=n, **kw)
                d = pm.ulp_diff(dev.cpu().numpy(), ref)
                worst = max(worst, d.max())
                assert np.isfinite(ref).all() and d.max() <= 2.0, (integrator, n, wr is not None, d.max())
    print("plant", name, "B", B, "max ulps", worst)
    s.close()


# ---- 5. the low-level kernels -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["default"] + list(pc.LOWLEVEL_CASES))
def test_low_level_kernels_at_the_case(name):
    """`foot_position_world` and `low_level_control` at B = 300 (a partial last workgroup, above 256) against
    orc.getFootPositionWorld / orc.lowLevelControl at the same case on the fp32-rounded inputs: attitudes up to +-0.6 rad (R' is far
    from R), t in [-1, 3] with exact multiples of the swing period and negative values (the reference's np.remainder, REF:436, puts a
    negative time into [0, Ts): the kernel's branch for it), all four contact patterns.  Tolerances of the existing test."""
    d = pc.lowlevel_batch(name)
    s = _solver(name, 10)
    pf = s.foot_position_world(d["x_fb"], d["q"])
    tau = s.low_level_control(d["x_fb"], d["t"], pf, d["q"], d["qd"], d["contact0"], d["u0"])
    s.close()
    e_fk = np.abs(pf - pc.lowlevel_fk_ref(name, d)).max()
    ref = pc.lowlevel_tau_ref(name, d, pf)
    e_tau = np.abs(tau - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))
    neg = d["t"] < 0
    print("low level %-16s FK %.2e tau %.2e (t < 0: %.2e, multiples of Ts: %.2e) max|tau| %.1f" % (
        name, e_fk, e_tau.max(), e_tau[neg].max(), e_tau[:24].max(), np.abs(ref).max()))
    assert e_fk <= pc.FK_TOL
    assert e_tau.max() <= pc.TAU_TOL, int(e_tau.argmax())


# ---- 6. set_params on a live handle -----------------------------------------------------------------------------------------------------

def _everything(s, h, inputs):
    """solve (cold), evaluate, plant_step and low_level_control of one handle on fixed inputs: a dict of arrays."""
    sb, g, pb, lb = inputs
    out = {}
    s.reset_warm_start()
    st, u, info = s.solve(sb["x_fb"], sb["foot"], sb["contact"], sb["phase"], x_cmd=sb["x_cmd"])
    out.update(states=st, controls=u, iters=info["iters"], status=info["status"])
    ev = s.evaluate(**ec.kernel_args(g), want_states=True)
    out.update({"ev_" + k: v for k, v in ev.items()})
    x, uu, foot, c, w = pb
    out["plant"] = s.plant_step(x, uu, foot, c, w)
    pf = s.foot_position_world(lb["x_fb"], lb["q"])
    out["pf"], out["tau"] = pf, s.low_level_control(lb["x_fb"], lb["t"], pf, lb["q"], lb["qd"], lb["contact0"], lb["u0"])
    return out


@pytest.mark.parametrize("h,path", [(10, PATH_DENSE), (7, PATH_STAGE)])
def test_set_params_on_a_live_handle_equals_a_fresh_handle(h, path):
    """A handle created at the default parameters is moved by `set_params` to I_nondiagonal, to the combined case and back; after
    each move `solve` (warm start off), `evaluate`, `plant_step` and `low_level_control` give the bits of a fresh handle created at
    that block, and the blocks really differ in every one of them."""
    import biped_mpc_py_amd as bm
    B = 16
    sb = util.synth_batch(B, h, 640 + h, gait="mixed", vx_cmd=True)
    g = pc.eval_group(h, "default")
    lb = pc.lowlevel_batch("default", B=B)
    inputs = (sb, g, pm.batch(B), lb)
    block = lambda name: bm.pack_params(*pc.objects(bm, name, h=h), half=sb["half"], solver_options=dict(path=path))
    live = bm.BatchSolver(cparams=block("default"), max_batch=B)
    seen = {}
    for name in ("default", "I_nondiagonal", "combined", "default"):
        if name != "default" or seen:
            live.set_params(block(name))
        assert live._lib.bmpc_solver_path(live._h) == path
        got = _everything(live, h, inputs)
        fresh = bm.BatchSolver(cparams=block(name), max_batch=B)
        want = _everything(fresh, h, inputs)
        fresh.close()
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)
        assert (got["status"] == 0).all()
        if name in seen:
            for k in want:
                assert np.array_equal(got[k], seen[name][k], equal_nan=True), ("back at", name, k)
        seen[name] = got
    live.close()
    for k in ("controls", "ev_cost", "ev_states", "plant"):
        assert not np.array_equal(seen["default"][k], seen["I_nondiagonal"][k]), k
        assert not np.array_equal(seen["I_nondiagonal"][k], seen["combined"][k]), k
    assert not np.array_equal(seen["default"]["tau"], seen["combined"]["tau"])        # (dt: the swing period and the foothold target)
