"""S candidate plans per instance on the MI355X (`bmpc_evaluate_samples`, `bmpc_evaluate_samples_device`; include/bmpc.h) against the
oracle's matrices and NumPy (tests/sample_cases.py), against `BatchSolver.evaluate` on replicated inputs, behind a solve, and timed
against the replicated evaluation."""
import functools

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import sample_cases as sc
from tests import util
from tests import gpu_common
from tests.gpu_common import (  # noqa: F401 (_built: the autouse fixture)
    built as _built, dev_args as _dev_args, solver as _solver)

pytestmark = pytest.mark.gpu

KEYS = ("cost", "violation", "score", "best", "n_valid", "weights", "u_mean", "ess")
_identical = functools.partial(gpu_common.identical, keys=KEYS)
C_SMALL = 4                              # samples per group of the small launches (asserted against the emulation's copy of the rule)


def _dev_samples(a):
    """sample_args as CUDA tensors."""
    import torch
    d = _dev_args({k: v for k, v in a.items() if k != "controls"})
    d["controls"] = torch.from_numpy(np.ascontiguousarray(a["controls"].astype(np.float32))).cuda()
    return d


def _both(solver, a, where="", **kw):
    """The host entry and the device entry on the same arguments, bit-identical to each other: the host result."""
    import torch
    host = solver.evaluate_samples(**a, **kw)
    dev = solver.evaluate_samples_device(**_dev_samples(a), **kw)
    torch.cuda.synchronize()
    _identical(host, {k: dev[k].cpu().numpy() for k in KEYS}, where)
    return host


@functools.lru_cache(maxsize=None)
def _case(h, supplied):
    g = sc.horizon_group(h, supplied)
    return g, sc.sample_controls(g, 2 * C_SMALL + 5)


def test_the_rule_of_the_small_launches():
    from tests.emu import emu_samples
    spg = emu_samples.samples_per_group
    assert spg(5, 13) == C_SMALL and spg(1, 1) == 1 and spg(64, 1024) == 8 and spg(256, 1024) == 32


@pytest.mark.parametrize("h", sc.HORIZONS)
def test_per_sample_values_through_both_entries(h):
    """CPU test 1 through both entries: against the yardstick on replicated inputs and against `BatchSolver.evaluate` on the same
    replicated inputs, bounds util.REL_TOL and eval_cases.REG_BOUND; bit-equality with `evaluate` printed."""
    Cs = C_SMALL
    for supplied, B, S in ((True, 5, 2 * Cs + 5), (True, 1, Cs - 1), (False, 3, Cs + 1), (False, 1, 1)):
        g, U = _case(h, supplied)
        gb, Ub = sc.take(g, range(B)), U[:B, :S]
        where = f"{g['name']} B={B} S={S}"
        solver = _solver(gb, 0, 16)
        res = _both(solver, sc.sample_args(gb, Ub), where, w_viol=sc.W_VIOL)
        solver.close()
        rep = sc.replicated(gb, Ub)
        ref = ec.yardstick_group(rep)
        sc.check_per_sample(res, ref, where)
        big = _solver(rep, 0, max(16, B * S))
        one = big.evaluate(**ec.kernel_args(rep))
        big.close()
        sc.check_per_sample(res, dict(ref, cost=one["cost"], violation=one["violation"]), where + " vs evaluate")
        got = sc.as_instances(res)
        print("bit-identical to evaluate:", where, "cost", np.array_equal(got["cost"], one["cost"]),
              "violation", np.array_equal(got["violation"], one["violation"]))


def test_per_step_mu():
    g = sc.mu_group(3)
    U = sc.sample_controls(g, C_SMALL + 1)
    solver = _solver(g, 0, 16)
    res = _both(solver, sc.sample_args(g, U), "mu", w_viol=sc.W_VIOL)
    solver.close()
    sc.check_per_sample(res, ec.yardstick_group(sc.replicated(g, U)), "per-step mu h=20 B=3")


@pytest.mark.parametrize("h", [10, 33])
def test_a_sample_does_not_depend_on_its_launch(h):
    """Sample (b, s) of the (5, 2 C + 5) launch is bit-identical to the same plan alone (B = 1, S = 1: C = 1) and to the same plan
    -- at h = 10 -- in a launch of 64 instances x 1024 samples, where the rule picks C = 8 (the five instances and thirteen plans, tiled)."""
    g, U = _case(h, True)
    B, S = U.shape[:2]
    solver = _solver(g, 0, 64)
    full = _both(solver, sc.sample_args(g, U), w_viol=sc.W_VIOL)
    for b, s in ((0, 0), (2, 3), (4, S - 1), (1, 7), (3, 4)):
        one = solver.evaluate_samples(**sc.sample_args(g, U[:, s:s + 1], [b]), w_viol=sc.W_VIOL)
        for k in ("cost", "violation", "score"):
            assert np.array_equal(one[k][0, 0], full[k][b, s]), (b, s, k)
    if h != 10:                                      # (the large launch once: 65536 plans)
        solver.close()
        return
    ib, js = np.arange(64) % B, np.arange(1024) % S
    big = solver.evaluate_samples(**sc.sample_args(g, U[:, js], ib), w_viol=sc.W_VIOL, temperature=100.0)
    solver.close()
    for k in ("cost", "violation", "score"):
        assert np.array_equal(big[k], full[k][ib][:, js]), k
    # the reduced values of an instance depend neither on B nor on its place: the twelve copies of each instance agree bit for bit
    for k in ("best", "n_valid", "weights", "u_mean", "ess"):
        for b in range(B, 64):
            assert np.array_equal(big[k][b], big[k][b % B]), (k, b)
    sc.check_reduced({k: v[:B] for k, v in big.items()}, U[:, js], 100.0, f"tiled h={h}")


@pytest.mark.parametrize("h", [1, 10, 33])
def test_reductions_against_numpy_at_three_temperatures(h):
    g, U = _case(h, True)
    S = U.shape[1]
    solver = _solver(g, 0, 16)
    a = sc.sample_args(g, U)
    base = _both(solver, a, w_viol=sc.W_VIOL)
    ref = sc.score_reference(base["cost"], base["violation"], sc.W_VIOL)
    assert (np.abs(base["score"] - ref) / ref).max() <= sc.SCORE_REL
    t_inf, t_med, t_cold = sc.temperatures(base["score"])
    for T in (t_inf, t_med, t_cold):
        res = base if T == t_inf else _both(solver, a, w_viol=sc.W_VIOL, temperature=T)
        assert np.array_equal(res["score"], base["score"])
        ref = sc.check_reduced(res, U, T, f"h={h}")
        if T == t_inf:
            assert np.array_equal(res["weights"], np.broadcast_to(1.0 / res["n_valid"][:, None], res["weights"].shape))
            assert (res["n_valid"] == S).all()
        elif T == t_med:
            assert (ref["ess"] >= 1.5).all() and (ref["ess"] <= S - 0.5).all(), ref["ess"]
        else:
            assert (res["weights"][np.arange(len(res["best"])), res["best"]] == 1.0).all()
    solver.close()


def test_bad_samples_and_instances():
    """CPU test 5 through both entries: a NaN control spoils its sample only; an instance without a valid sample; the three spoiled
    instances of eval_cases.bad_batch fail as a whole."""
    h = 10
    g, U = _case(h, True)
    S = C_SMALL + 1
    U = U[:, :S]
    solver = _solver(g, 0, 16)
    T = 5000.0
    clean = _both(solver, sc.sample_args(g, U), w_viol=sc.W_VIOL, temperature=T)
    b, s = 2, int(clean["best"][2])
    bad = U.copy()
    bad[b, s, h // 2, 7] = np.nan
    res = _both(solver, sc.sample_args(g, bad), w_viol=sc.W_VIOL, temperature=T)
    keep = np.ones((U.shape[0], S), bool); keep[b, s] = False
    for k in ("cost", "violation", "score"):
        assert np.isnan(res[k][b, s]).all(), k
        assert np.array_equal(res[k][keep], clean[k][keep]) and np.isfinite(clean[k]).all(), k
    assert res["weights"][b, s] == 0.0 and not np.signbit(res["weights"][b, s])
    assert res["best"][b] != s and res["best"][b] >= 0 and res["n_valid"][b] == S - 1
    assert np.isfinite(res["u_mean"]).all() and np.isfinite(res["ess"]).all()
    sc.check_reduced(res, bad, T, "nan control")
    others = [i for i in range(U.shape[0]) if i != b]
    for k in ("best", "n_valid", "weights", "u_mean", "ess"):
        assert np.array_equal(res[k][others], clean[k][others]), k
    # every sample of one instance bad
    bad = U.copy()
    bad[3, :, 0, 2] = np.inf
    res = _both(solver, sc.sample_args(g, bad), w_viol=sc.W_VIOL, temperature=T)
    solver.close()
    assert res["best"][3] == -1 and res["n_valid"][3] == 0 and np.isnan(res["u_mean"][3]).all() and np.isnan(res["ess"][3])
    assert (res["weights"][3] == 0).all() and not np.signbit(res["weights"][3]).any()
    for k in KEYS:
        assert np.array_equal(res[k][[0, 1, 2, 4]], clean[k][[0, 1, 2, 4]]), k
    # bad_batch
    cl, sp, idx = ec.bad_batch()
    Uc = sc.sample_controls(cl, S)
    Ub = Uc.copy()
    Ub[1] = sc.sample_controls(sp, S)[1]
    solver = _solver(cl, 0, 16)
    a = _both(solver, sc.sample_args(cl, Uc), w_viol=sc.W_VIOL, temperature=50.0)
    r = _both(solver, sc.sample_args(sp, Ub, unchecked=True), w_viol=sc.W_VIOL, temperature=50.0)
    solver.close()
    ok = [i for i in range(8) if i not in idx]
    for k in ("cost", "violation", "score", "u_mean", "ess"):
        assert np.isnan(r[k][idx]).all(), k
    assert (r["best"][idx] == -1).all() and (r["n_valid"][idx] == 0).all() and (r["weights"][idx] == 0).all()
    for k in KEYS:
        assert np.array_equal(a[k][ok], r[k][ok]) and np.isfinite(a[k]).all(), k


def test_repeatable_and_optional_outputs():
    """Two identical calls give identical bits in every output; a call that asks only for best and u_mean (scores and weights in the
    handle's scratch) gives the bits of the call that asks for everything."""
    import torch
    g, U = _case(10, True)
    ib, js = np.arange(48) % 5, np.arange(301) % U.shape[1]
    a = sc.sample_args(g, U[:, js], ib)
    d = _dev_samples(a)
    solver = _solver(g, 0, 64)
    kw = dict(w_viol=sc.W_VIOL, temperature=300.0)
    r1 = solver.evaluate_samples_device(**d, **kw)
    r2 = solver.evaluate_samples_device(**d, **kw)
    only = solver.evaluate_samples_device(**d, **kw, want=("best", "u_mean"))
    torch.cuda.synchronize()
    _identical({k: v.cpu().numpy() for k, v in r1.items()}, {k: v.cpu().numpy() for k, v in r2.items()})
    assert all(only[k] is None for k in KEYS if k not in ("best", "u_mean"))
    for k in ("best", "u_mean"):
        assert np.array_equal(only[k].cpu().numpy(), r1[k].cpu().numpy(), equal_nan=True), k
    host = solver.evaluate_samples(**a, **kw)
    _identical(host, {k: v.cpu().numpy() for k, v in r1.items()})
    solver.close()


def test_behind_a_solve_on_one_stream():
    """solve_device -> samples built from its controls -> evaluate_samples_device on one stream, nothing synchronised in between:
    sample 0 is u*, the others 0.9 u* and 1.1 u*; with w_viol = 1e6 per class u* wins in every instance of a standing batch of 256
    at h = 10.  A second identical solve returns the bits and iteration counts of the first: the handle's solve state is untouched."""
    import torch
    B, h = 256, 10
    g = gpu_common.synth_group(B, h, "standing", 1)
    solver = _solver(g, 0, B)
    d_in = {k: v for k, v in _dev_args(ec.kernel_args(g)).items() if k != "controls"}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        it1 = torch.empty(B, dtype=torch.int32, device="cuda")
        u1, _ = solver.solve_device(**d_in, iters=it1)
        ms1 = None
        plans = torch.stack([u1, 0.9 * u1, 1.1 * u1], 1).contiguous()
        res = solver.evaluate_samples_device(**d_in, controls=plans, w_viol=(1e6,) * 4, temperature=1.0, want=("best", "score", "n_valid"))
        it2 = torch.empty(B, dtype=torch.int32, device="cuda")
        u2, _ = solver.solve_device(**d_in, iters=it2)
    st.synchronize()
    ms1 = solver.last_kernel_ms()
    score = res["score"].cpu().numpy()
    print("score(0.9 u*) / score(u*) min %.6f, score(1.1 u*) / score(u*) min %.6f" % ((score[:, 1] / score[:, 0]).min(),
                                                                                      (score[:, 2] / score[:, 0]).min()))
    assert (res["n_valid"].cpu().numpy() == 3).all()
    assert (res["best"].cpu().numpy() == 0).all(), np.bincount(res["best"].cpu().numpy() + 1)
    assert torch.equal(u1, u2) and torch.equal(it1, it2) and ms1 > 0
    solver.close()


def test_faster_than_the_replicated_evaluation():
    """B = 256 instances x S = 1024 samples at h = 10, cost and violation only, against `evaluate_device` on the same 262144 plans
    with every input replicated (a handle of max_batch 262144): HIP events, both sides warmed up, 20 launches of each alternating
    in one process; the new entry's median must be below the replicated evaluation's.  Measured on the MI355X (docs/history_r20.md):
    see the figures this test prints."""
    import torch
    import biped_mpc_py_amd as bm
    B, S, h = 256, 1024, 10
    g = gpu_common.synth_group(B, h, "walking", 3)
    d_in = {k: v for k, v in _dev_args(ec.kernel_args(g)).items() if k != "controls"}
    gen = torch.Generator(device="cuda").manual_seed(5)
    con = d_in["contact"].to(torch.float32).repeat_interleave(3, dim=2).repeat(1, 1, 2)             # (B,h,12): leg of each entry
    nominal = torch.zeros((B, h, 12), device="cuda"); nominal[:, :, 2] = 59.0; nominal[:, :, 5] = 59.0
    plans = ((nominal[:, None] + 6.0 * torch.randn((B, S, h, 12), device="cuda", generator=gen)) * con[:, None]).contiguous()
    rep = {k: None if v is None else v.repeat_interleave(S, dim=0).contiguous() for k, v in d_in.items()}
    flat = plans.view(B * S, h, 12)
    new = _solver(g, 0, B)
    old = bm.BatchSolver(cparams=ec.cparams_of(g), max_batch=B * S)
    o_new = new.evaluate_samples_device(**d_in, controls=plans, want=("cost", "violation"))
    o_old = old.evaluate_device(**rep, controls=flat)
    o_all = new.evaluate_samples_device(**d_in, controls=plans, w_viol=sc.W_VIOL, temperature=1000.0)
    o_ps = {k: o_all[k] for k in ("cost", "violation", "score")}
    torch.cuda.synchronize()
    same = torch.equal(o_new["cost"].view(-1), o_old["cost"]) and torch.equal(o_new["violation"].view(-1, 4), o_old["violation"])
    rel = ((o_new["cost"].view(-1) - o_old["cost"]).abs() / o_old["cost"].abs().clamp(min=1.0)).max().item()
    assert rel <= ec.REG_BOUND["cost"], rel

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    run_new = lambda: new.evaluate_samples_device(**d_in, controls=plans, cost=o_new["cost"], violation=o_new["violation"], want=())
    run_old = lambda: old.evaluate_device(**rep, controls=flat, cost=o_old["cost"], objective=o_old["objective"], violation=o_old["violation"])
    run_all = lambda: new.evaluate_samples_device(**d_in, controls=plans, w_viol=sc.W_VIOL, temperature=1000.0, **o_all)
    run_ps = lambda: new.evaluate_samples_device(**d_in, controls=plans, w_viol=sc.W_VIOL, temperature=1000.0, want=(), **o_ps)
    for fn in (run_new, run_old, run_all, run_ps) * 3:
        fn()
    torch.cuda.synchronize()
    t_new, t_old, t_all, t_ps = [], [], [], []
    for _ in range(20):
        t_new.append(timed(run_new)); t_old.append(timed(run_old))
    for _ in range(10):
        t_all.append(timed(run_all)); t_ps.append(timed(run_ps))
    m_new, m_old, m_all, m_ps = (float(np.median(t)) for t in (t_new, t_old, t_all, t_ps))
    # compulsory traffic: the inputs of an instance once, per plan its controls in and cost and violation out
    nbytes = B * (12 * 4 + 6 * 4 + 4 + 12 * 4 + h * 2) + B * S * (h * 12 * 4 + 8 + 32)
    print("evaluate_samples_device B=%d S=%d h=%d: median %.1f us (min %.1f); replicated evaluate_device %.1f us (min %.1f); ratio %.3f; "
          "%.0f GB/s over %.1f MB compulsory; reductions %.1f us (all outputs %.1f us - per-sample with score %.1f us); bit-identical to evaluate: %s"
          % (B, S, h, m_new * 1e3, min(t_new) * 1e3, m_old * 1e3, min(t_old) * 1e3, m_new / m_old, nbytes / (m_new * 1e-3) / 1e9,
             nbytes / 1e6, (m_all - m_ps) * 1e3, m_all * 1e3, m_ps * 1e3, same))
    assert m_new < m_old
    new.close(); old.close()
