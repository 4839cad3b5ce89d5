"""S candidate plans per instance (`bmpc_evaluate_samples*`, include/bmpc.h) without a GPU: the two kernels' sources run on the CPU
over the library's grids (tests/emu/bmpc_emu_samples.cpp) against the oracle's matrices (tests/eval_cases.py `yardstick`) and NumPy
(tests/sample_cases.py), and the C ABI's argument checks through the library itself."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import sample_cases as sc


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")
B_MAX = 5


def _build():
    import __graft_entry__ as ge
    ge.build()


def _spg(B, S):
    _build()
    from tests.emu import emu_samples
    return emu_samples.samples_per_group(B, S)


def _small_c():
    """C of the small launches of this file: the rule's value at (B_MAX, 2 C + 5), which it keeps for S = C - 1 and C + 1."""
    Cs = _spg(B_MAX, 13)
    assert Cs == 4 and _spg(B_MAX, 2 * Cs + 5) == Cs and _spg(1, Cs - 1) == Cs and _spg(3, Cs + 1) == Cs
    return Cs


def _emu(g, controls, idx=None, unchecked=False, **kw):
    _build()
    from tests.emu import emu_samples
    return emu_samples.evaluate_samples(ec.cparams_of(g), **sc.sample_args(g, controls, idx, unchecked), **kw)


@functools.lru_cache(maxsize=None)
def _case(h, supplied):
    """(group, sample set (5, 2 C + 5, h, 12)) at horizon h: computed once, sliced by the tests."""
    g = sc.horizon_group(h, supplied)
    return g, sc.sample_controls(g, 2 * _small_c() + 5)


@functools.lru_cache(maxsize=None)
def _yardstick(h, supplied, B, S):
    g, U = _case(h, supplied)
    return ec.yardstick_group(sc.replicated(sc.take(g, range(B)), U[:B, :S]))


@functools.lru_cache(maxsize=None)
def _full(h, supplied, temperature=float("inf"), priced=True):
    """The whole (5, 2 C + 5) launch at horizon h with every output."""
    g, U = _case(h, supplied)
    return _emu(g, U, w_viol=sc.W_VIOL if priced else (0, 0, 0, 0), temperature=temperature)


# ---- 1. per-sample values ----------------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("h", sc.HORIZONS)
def test_per_sample_values_against_the_yardstick_and_the_evaluation(h):
    """cost and violation of every plan as B S instances against the oracle's matrices on replicated inputs, and against the
    evaluation kernel's emulation on the same replicated inputs (bit-equality printed, not asserted).  Per horizon: B = 5 with
    S = 2 C + 5 and B = 1 with S = C - 1 on supplied references, B = 3 with S = C + 1 and B = 1 with S = 1 on generated ones."""
    from tests.emu import emu_eval
    Cs = _small_c()
    for supplied, B, S in ((True, 5, 2 * Cs + 5), (True, 1, Cs - 1), (False, 3, Cs + 1), (False, 1, 1)):
        g, U = _case(h, supplied)
        gb, Ub = sc.take(g, range(B)), U[:B, :S]
        res = _full(h, supplied) if (B, S) == U.shape[:2] else _emu(gb, Ub, w_viol=sc.W_VIOL)
        ref = _yardstick(h, supplied, 5 if supplied else 3, 2 * Cs + 5 if supplied else Cs + 1)
        pick = (np.arange(B)[:, None] * (2 * Cs + 5 if supplied else Cs + 1) + np.arange(S)[None, :]).reshape(-1)
        ref = {k: v[pick] for k, v in ref.items()}
        where = f"{g['name']} B={B} S={S}"
        sc.check_per_sample(res, ref, where)
        rep = sc.replicated(gb, Ub)
        one = emu_eval.evaluate(ec.cparams_of(rep), **ec.kernel_args(rep), want_states=False)
        got = sc.as_instances(res)
        sc.check_per_sample(res, dict(ref, cost=one["cost"], violation=one["violation"]), where + " vs evaluate")
        print("bit-identical to evaluate:", where, "cost", np.array_equal(got["cost"], one["cost"]),
              "violation", np.array_equal(got["violation"], one["violation"]))


@needs_emu
def test_per_step_mu():
    g = sc.mu_group(3)
    U = sc.sample_controls(g, _small_c() + 1)
    res = _emu(g, U, w_viol=sc.W_VIOL)
    sc.check_per_sample(res, ec.yardstick_group(sc.replicated(g, U)), "per-step mu h=20 B=3")


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("h", [10, 33])
def test_a_sample_does_not_depend_on_its_launch(h):
    """Sample (b, s) of the (5, 2 C + 5) launch is bit-identical to the same plan alone (B = 1, S = 1: the rule picks C = 1) and in a
    launch of two samples (C = 2)."""
    g, U = _case(h, True)
    full = _full(h, True)
    S = U.shape[1]
    assert _spg(1, 1) == 1 and _spg(1, 2) == 2 and _spg(B_MAX, S) == _small_c()
    for b, s in ((0, 0), (2, 3), (4, S - 1), (1, 7), (3, 4)):
        one = _emu(g, U[:, s:s + 1], [b], w_viol=sc.W_VIOL)
        two = _emu(g, U[:, [s, (s + 5) % S]], [b], w_viol=sc.W_VIOL)
        for k in ("cost", "violation", "score"):
            assert np.array_equal(one[k][0, 0], full[k][b, s]), (b, s, k)
            assert np.array_equal(two[k][0, 0], full[k][b, s]) and np.array_equal(two[k][0, 1], full[k][b, (s + 5) % S]), (b, s, k)


# ---- 3. score ----------------------------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("h", [3, 20])
def test_score_is_cost_plus_priced_violations(h):
    res = _full(h, True)
    ref = sc.score_reference(res["cost"], res["violation"], sc.W_VIOL)
    err = np.abs(res["score"] - ref) / ref
    print("score rel err", h, err.max())
    assert (ref > 0).all() and err.max() <= sc.SCORE_REL
    assert (res["violation"][:, 3::4].max(-1) > 1.0).all()              # the broken samples do break rows: the prices matter
    free = _full(h, True, priced=False)
    assert np.array_equal(free["score"], free["cost"]) and np.array_equal(free["cost"], res["cost"])


# ---- 4. reductions -----------------------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("h", [1, 10, 33])
def test_reductions_against_numpy_at_three_temperatures(h):
    g, U = _case(h, True)
    base = _full(h, True)
    S = U.shape[1]
    t_inf, t_med, t_cold = sc.temperatures(base["score"])
    for T in (t_inf, t_med, t_cold):
        res = base if T == t_inf else _emu(g, U, w_viol=sc.W_VIOL, temperature=T)
        assert np.array_equal(res["score"], base["score"])
        ref = sc.check_reduced(res, U, T, f"h={h}")
        if T == t_inf:
            assert np.array_equal(res["weights"], np.broadcast_to(1.0 / res["n_valid"][:, None], res["weights"].shape))
            assert (res["n_valid"] == S).all()
        elif T == t_med:
            print("reference ess at the median temperature", ref["ess"])
            assert (ref["ess"] >= 1.5).all() and (ref["ess"] <= S - 0.5).all(), ref["ess"]
        else:
            assert (res["weights"][np.arange(len(res["best"])), res["best"]] == 1.0).all()


# ---- 5. bad samples and instances --------------------------------------------------------------------------------------------------

@needs_emu
def test_a_nan_control_spoils_its_sample_only():
    h = 10
    g, U = _case(h, True)
    S = _small_c() + 1
    U = U[:, :S]
    _, T, _ = sc.temperatures(_full(h, True)["score"])
    clean = _emu(g, U, w_viol=sc.W_VIOL, temperature=T)
    b, s = 2, int(clean["best"][2])                                      # the sample that would have won
    bad = U.copy()
    bad[b, s, h // 2, 7] = np.nan
    res = _emu(g, bad, w_viol=sc.W_VIOL, temperature=T)
    for k in ("cost", "violation", "score"):
        assert np.isnan(res[k][b, s]).all(), k
        keep = np.ones((U.shape[0], S), bool); keep[b, s] = False
        assert np.array_equal(res[k][keep], clean[k][keep]) and np.isfinite(clean[k]).all(), k
    assert res["weights"][b, s] == 0.0 and not np.signbit(res["weights"][b, s])
    assert res["best"][b] != s and res["best"][b] >= 0 and res["n_valid"][b] == S - 1
    assert np.isfinite(res["u_mean"]).all() and np.isfinite(res["ess"]).all()
    sc.check_reduced(res, bad, T, "nan control")                         # (the reference runs over the valid samples)
    others = [i for i in range(U.shape[0]) if i != b]
    for k in ("best", "n_valid", "weights", "u_mean", "ess"):
        assert np.array_equal(res[k][others], clean[k][others]), k


@needs_emu
def test_an_instance_without_a_valid_sample():
    h = 10
    g, U = _case(h, True)
    U = U[:, :_small_c() + 1]
    clean = _emu(g, U, w_viol=sc.W_VIOL, temperature=50.0)
    bad = U.copy()
    bad[3, :, 0, 2] = np.inf
    res = _emu(g, bad, w_viol=sc.W_VIOL, temperature=50.0)
    assert res["best"][3] == -1 and res["n_valid"][3] == 0
    assert np.isnan(res["u_mean"][3]).all() and np.isnan(res["ess"][3])
    assert (res["weights"][3] == 0).all() and not np.signbit(res["weights"][3]).any()
    for k in ("cost", "violation", "score"):
        assert np.isnan(res[k][3]).all(), k
    others = [0, 1, 2, 4]
    for k in sc_keys():
        assert np.array_equal(res[k][others], clean[k][others]), k


def sc_keys():
    from tests.emu import emu_samples
    return emu_samples.KEYS


@needs_emu
def test_spoiled_instances_fail_as_a_whole():
    """eval_cases.bad_batch: a NaN in the nominal controls (every sample inherits it), an Inf in x_ref, a reference pitch of 90
    degrees -- every sample of the three NaN, no valid sample; the other five bit-identical to the clean batch."""
    clean, bad, idx = ec.bad_batch()
    S = _small_c() + 1
    U = sc.sample_controls(clean, S)
    Ub = U.copy()
    Ub[1] = sc.sample_controls(bad, S)[1]
    assert np.isnan(Ub[1]).reshape(S, -1).any(1).all()                            # every sample of instance 1 holds a NaN
    a = _emu(clean, U, w_viol=sc.W_VIOL, temperature=50.0)
    b = _emu(bad, Ub, unchecked=True, w_viol=sc.W_VIOL, temperature=50.0)
    ok = [i for i in range(8) if i not in idx]
    for k in ("cost", "violation", "score", "u_mean", "ess"):
        assert np.isnan(b[k][idx]).all(), k
    assert (b["best"][idx] == -1).all() and (b["n_valid"][idx] == 0).all() and (b["weights"][idx] == 0).all()
    for k in sc_keys():
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    sc.check_reduced(b, Ub, 50.0, "bad_batch")


# ---- 6. ties -----------------------------------------------------------------------------------------------------------------------

@needs_emu
def test_the_lower_index_wins_a_tie():
    h = 10
    g, U = _case(h, True)
    base = _full(h, True)
    S = U.shape[1]
    tied = U.copy()
    twin = np.empty(U.shape[0], int)
    for b in range(U.shape[0]):
        sb = int(base["best"][b])
        twin[b] = (sb + 3) % S if b % 2 else (sb - 3) % S                # a twin above or below the winner
        tied[b, twin[b]] = U[b, sb]
    res = _emu(g, tied, w_viol=sc.W_VIOL, want=("score", "best", "n_valid"))
    assert np.array_equal(res["best"], np.minimum(base["best"], twin)), (res["best"], base["best"], twin)
    assert (twin < base["best"]).any() and (twin > base["best"]).any()
    rows = np.arange(U.shape[0])
    assert np.array_equal(res["score"][rows, twin], res["score"][rows, base["best"]])
    assert res["cost"] is None and res["weights"] is None


@needs_emu
def test_optional_outputs_leave_the_others_as_they_are():
    """best and u_mean alone (scores and weights in scratch) give the bits of the call that asks for everything."""
    g, U = _case(10, True)
    full = _emu(g, U, w_viol=sc.W_VIOL, temperature=40.0)
    only = _emu(g, U, w_viol=sc.W_VIOL, temperature=40.0, want=("best", "u_mean"))
    assert np.array_equal(only["best"], full["best"]) and np.array_equal(only["u_mean"], full["u_mean"])
    assert all(only[k] is None for k in ("cost", "violation", "score", "n_valid", "weights", "ess"))


# ---- 7. argument validation through the library ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    _build()
    from biped_mpc_py_amd import _lib
    return _lib.load()


def test_argument_checks_without_a_device(lib):
    """Every rejected case of include/bmpc.h is BMPC_ERR_INVALID before a device is touched: the sampling descriptor first (NULL,
    S, w_viol, temperature -- checked even without a handle), then a NULL handle, `in`, `controls`, `out`; with a device also all
    outputs NULL, foot == NULL without foot_ref and B out of range.  B = 0 succeeds."""
    from biped_mpc_py_amd import _lib
    assert "bmpc_evaluate_samples" in _lib.EXPORTS and "bmpc_evaluate_samples_device" in _lib.EXPORTS
    h, S = 10, 3
    ptr = lambda a: a.ctypes.data
    x = np.zeros((1, 12), np.float32); ft = np.zeros((1, 6), np.float32); con = np.ones((1, h, 2), np.uint8); ph = np.zeros(1, np.int32)
    u = np.zeros((1, S, h, 12), np.float32)
    cost = np.zeros((1, S))
    inp = _lib.CInputs(ptr(x), ptr(ft), ptr(con), ptr(ph), None, None, None, None)
    so = _lib.CSamplesOut(ptr(cost), None, None, None, None, None, None, None)

    def smp(S=S, w=(0, 0, 0, 0), T=1.0):
        return _lib.CSamples(S, 0, (C.c_double * 4)(*w), T)

    entries = ((lib.bmpc_evaluate_samples, []), (lib.bmpc_evaluate_samples_device, [None]))
    inf, nan = float("inf"), float("nan")
    for handle in (None, "device"):
        hd = C.c_void_p()
        if handle is not None:
            cp = _lib.CParams()
            lib.bmpc_default_params(C.byref(cp), h)
            if lib.bmpc_create(C.byref(hd), C.byref(cp), 0, 16) != 0:
                return                                 # no device here: what runs without a handle has run
        try:
            for fn, extra in entries:
                call = lambda s, i=inp, c=ptr(u), o=so, B=1: fn(hd, B, None if i is None else C.byref(i), c,
                                                               None if s is None else C.byref(s), None if o is None else C.byref(o), *extra)
                for bad, word in ((None, b"bmpc_samples"), (smp(S=0), b"S ="), (smp(S=65537), b"S ="), (smp(S=-1), b"S ="),
                                  (smp(w=(0, nan, 0, 0)), b"w_viol[1]"), (smp(w=(-1e-300, 0, 0, 0)), b"w_viol[0]"),
                                  (smp(w=(0, 0, 0, inf)), b"w_viol[3]"), (smp(T=nan), b"temperature"), (smp(T=0.0), b"temperature"),
                                  (smp(T=-1.0), b"temperature")):
                    assert call(bad) == -1 and word in lib.bmpc_last_error(), (word, lib.bmpc_last_error())
                if handle is None:
                    assert call(smp()) == -1 and b"handle" in lib.bmpc_last_error()
                    assert call(smp(T=inf)) == -1 and b"handle" in lib.bmpc_last_error()      # (+inf is a temperature)
                    continue
                assert call(smp(), i=None) == -1 and b"bmpc_inputs" in lib.bmpc_last_error()
                assert call(smp(), c=None) == -1 and b"controls" in lib.bmpc_last_error()
                assert call(smp(), o=None) == -1 and b"bmpc_samples_out" in lib.bmpc_last_error()
                assert call(smp(), o=_lib.CSamplesOut()) == -1 and b"at least one" in lib.bmpc_last_error()
                assert call(smp(), B=17) == -1 and call(smp(), B=-1) == -1
                nofoot = _lib.CInputs(ptr(x), None, ptr(con), ptr(ph), None, None, None, None)
                assert call(smp(), i=nofoot) == -1 and b"foot" in lib.bmpc_last_error()
                assert call(smp(), B=0) == 0
        finally:
            if hd:
                lib.bmpc_destroy(hd)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_python_surface_checks_before_any_solver_exists():
    import inspect
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import api
    h = 10
    mpc = bm.MPC()
    before = dict(api._SOLVERS)
    con = np.ones((1, h, 2), int)
    good = np.zeros((1, 3, h, 12))
    for bad in (np.zeros((1, h, 12)), np.zeros((1, 3, h, 11)), np.zeros((1, 0, h, 12)), np.zeros((1, 3, h, 12), int)):
        with pytest.raises(ValueError, match="controls"):
            bm.evaluate_samples_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con, bad, mpc=mpc)
    for kw, word in ((dict(w_viol=(1, 2, 3)), "w_viol"), (dict(w_viol=(0, -1, 0, 0)), "w_viol"), (dict(temperature=0.0), "temperature"),
                     (dict(temperature=float("nan")), "temperature")):
        with pytest.raises(ValueError, match=word):
            bm.evaluate_samples_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con, good, mpc=mpc, **kw)
    assert api._SOLVERS == before                      # no handle was created on the way
    assert list(inspect.signature(bm.BatchSolver.evaluate_samples).parameters)[1:] == [
        "x_fb", "foot", "contact", "phase", "controls", "x_cmd", "mu", "x_ref", "foot_ref", "w_viol", "temperature"]
    sig = inspect.signature(bm.BatchSolver.evaluate_samples)
    assert sig.parameters["w_viol"].default == (0, 0, 0, 0) and sig.parameters["temperature"].default == float("inf")
    assert hasattr(bm.BatchSolver, "evaluate_samples_device")
