"""Evaluation of given controls (include/bmpc.h ABI 13) without a GPU: the kernel's source run on the CPU (tests/emu/bmpc_emu.cpp)
against the oracle's matrices (tests/eval_cases.py `yardstick`), the C ABI's struct and argument checks, and the Python surface."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import util


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")


def _emu(g, idx=None, args=None, **kw):
    import __graft_entry__ as ge
    ge.build()
    from tests.emu import emu_eval
    return emu_eval.evaluate(ec.cparams_of(g), **(args if args is not None else ec.kernel_args(g, idx)), **kw)


# ---- the kernel's source on the CPU against the yardstick --------------------------------------------------------------------------

@needs_emu
def test_fixture_controls_with_supplied_references():
    """Case 1: every instance of ref_tracking.npz with the fixture's own controls.  Also `states` against the fixture's (the
    reference's own solve_mpc output) and `objective` against z'Pz/2 + q'z from the fixture's captured q, P = 2 diag(Q.., R..)."""
    from oracle import bmpc_oracle as orc
    for g in ec.ref_tracking_groups():
        got = _emu(g)
        ec.check(got, ec.yardstick_group(g), g["name"])
        h = g["h"]
        assert util.rel_err(got["states"], g["fix_states"]).max() <= util.REL_TOL
        mpc = orc.MPC()
        pd = 2 * np.concatenate([np.tile(mpc.Q, h), np.tile(mpc.R, h)])
        z = np.concatenate([got["states"].reshape(-1, 13 * h), ec.r32(g["controls"]).reshape(-1, 12 * h)], 1)
        obj = 0.5 * np.sum(pd * z * z, 1) + np.sum(g["fix_q"] * z, 1)
        assert (np.abs(got["objective"] - obj) / np.maximum(1.0, np.abs(obj))).max() <= ec.REG_BOUND["objective"]
        assert (got["cost"] >= 0).all()


@needs_emu
def test_controls_that_break_every_row_class():
    """Case 2: U' = 1.3 U + d.  The test cannot pass on zeros: over the case set the yardstick's violation exceeds 1 in each class
    for some instance and is exactly 0 in some class for some instance."""
    refs = []
    for g in ec.ref_tracking_groups(breaking=True):
        ref = ec.yardstick_group(g)
        ec.check(_emu(g), ref, g["name"])
        refs.append(ref["violation"])
    v = np.concatenate(refs)
    assert (v.max(0) > 1.0).all(), v.max(0)
    assert (v == 0.0).any()


@needs_emu
def test_generated_references_and_every_lane_group():
    """Case 3: generated references (x_ref, foot_ref NULL) on the golden fixtures -- tilted bodies, commanded rates, bounds off their
    defaults, per-step friction at h = 20 -- and h = 1, 3, 13, 33, 40 (lane groups of 16 / 32 / 64, idle lanes past the horizon)."""
    from tests.emu import emu_eval
    for g in ec.generated_groups() + ec.horizon_groups():
        ec.check(_emu(g), ec.yardstick_group(g), g["name"])
    assert [emu_eval.lanes(h) for h in (1, 3, 13, 16, 17, 33, 40)] == [16, 16, 16, 16, 32, 64, 64]


@needs_emu
@pytest.mark.parametrize("h", [10, 20, 40])
def test_result_does_not_depend_on_the_batch(h):
    """Case 4: an instance evaluated alone and inside a batch of 200 in shuffled order gives identical bits."""
    from tests import refs_cases as rc
    s = rc.make_batch(200, h, 31 + h, "abcde")
    rng = np.random.default_rng(h)
    g = ec._group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], ec.seeded_controls(s["contact"], rng),
                  x_ref=s["x_ref"], foot_ref=s["foot_ref"])
    perm = rng.permutation(200)
    full = _emu(g, perm)
    for pos in (0, 3, 77, 199):                                  # (first of a wave, inside a wave, last group of the last workgroup)
        one = _emu(g, perm[pos:pos + 1])
        for k in ("cost", "objective", "violation", "states"):
            assert np.array_equal(one[k][0], full[k][pos]), (pos, k)
    ec.check({k: v[:8] for k, v in full.items()}, ec.yardstick_group(g, perm[:8]), f"batch200_h{h}")


@needs_emu
def test_non_finite_instances_get_nan_and_touch_nobody():
    """Case 5: NaN in a control entry, Inf in x_ref, a reference pitch of 90 degrees: NaN in all outputs of those three, the other
    five bit-identical to the clean batch."""
    clean, bad, idx = ec.bad_batch()
    a = _emu(clean)
    b = _emu(bad, args=ec.kernel_args_unchecked(bad))
    ok = [i for i in range(8) if i not in idx]
    for k in ("cost", "objective", "violation", "states"):
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    only = _emu(clean, want_states=False)                        # optional outputs: NULL states leaves the others as they are
    assert only["states"] is None and np.array_equal(only["cost"], a["cost"]) and np.array_equal(only["violation"], a["violation"])


def test_scaling_an_optimum_down_costs_more():
    """The ranking property of GPU test 3 pinned on the CPU with the yardstick: u = 0 satisfies every row at the default bounds and
    the QP is convex, so cost(0.9 u*) > cost(u*) for the reference's own optima (ref_tracking.npz, rounded to fp32)."""
    for g in ec.ref_tracking_groups():
        c1 = ec.yardstick_group(g)["cost"]
        c09 = ec.yardstick_group(dict(g, controls=0.9 * ec.r32(g["controls"])))["cost"]
        c0 = ec.yardstick_group(dict(g, controls=0.0 * g["controls"]))["cost"]
        print("cost ratios h", g["h"], (c09 / c1).min(), (c0 / c1).min())
        assert (c09 > c1).all() and (c0 > c1).all()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    return _lib.load()


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
def test_bmpc_eval_out_layout_matches_ctypes(tmp_path):
    from biped_mpc_py_amd import _lib
    fields = [f[0] for f in _lib.CEvalOut._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpc.h"\nint main(void) {\n  printf("%zu", sizeof(bmpc_eval_out));\n'
                   + "".join(f'  printf(" %zu", offsetof(bmpc_eval_out, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(util.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.CEvalOut)] + [getattr(_lib.CEvalOut, n).offset for n in fields]
    assert fields == ["cost", "objective", "states", "violation"]


def test_abi_version_and_argument_checks_without_a_device(lib):
    """bmpc_abi_version() == 13; a NULL handle, descriptor, controls or out is BMPC_ERR_INVALID before anything touches a device;
    with a device also all four outputs NULL, foot == NULL without foot_ref and B out of range."""
    from biped_mpc_py_amd import _lib
    assert lib.bmpc_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert "bmpc_evaluate" in _lib.EXPORTS and "bmpc_evaluate_device" in _lib.EXPORTS
    inp, eo = _lib.CInputs(), _lib.CEvalOut()
    u = np.zeros((1, 10, 12), np.float32)
    assert lib.bmpc_evaluate(None, 1, C.byref(inp), u.ctypes.data, C.byref(eo)) == -1
    assert lib.bmpc_evaluate_device(None, 1, C.byref(inp), u.ctypes.data, C.byref(eo), None) == -1
    assert b"handle" in lib.bmpc_last_error()
    h = C.c_void_p()
    cp = _lib.CParams()
    lib.bmpc_default_params(C.byref(cp), 10)
    if lib.bmpc_create(C.byref(h), C.byref(cp), 0, 16) != 0:
        return                                     # no device here: the null-handle check above is what runs without one
    try:
        x = np.zeros((1, 12), np.float32); ft = np.zeros((1, 6), np.float32); con = np.ones((1, 10, 2), np.uint8); ph = np.zeros(1, np.int32)
        cost = np.zeros(1); ptr = lambda a: a.ctypes.data
        inp = _lib.CInputs(ptr(x), ptr(ft), ptr(con), ptr(ph), None, None, None, None)
        eo = _lib.CEvalOut(ptr(cost), None, None, None)
        for fn, extra in ((lib.bmpc_evaluate, []), (lib.bmpc_evaluate_device, [None])):
            assert fn(h, 1, None, ptr(u), C.byref(eo), *extra) == -1
            assert fn(h, 1, C.byref(inp), None, C.byref(eo), *extra) == -1
            assert fn(h, 1, C.byref(inp), ptr(u), None, *extra) == -1
            assert fn(h, 1, C.byref(inp), ptr(u), C.byref(_lib.CEvalOut()), *extra) == -1
            assert b"at least one" in lib.bmpc_last_error()
            assert fn(h, 17, C.byref(inp), ptr(u), C.byref(eo), *extra) == -1
            assert fn(h, -1, C.byref(inp), ptr(u), C.byref(eo), *extra) == -1
            nofoot = _lib.CInputs(ptr(x), None, ptr(con), ptr(ph), None, None, None, None)
            assert fn(h, 1, C.byref(nofoot), ptr(u), C.byref(eo), *extra) == -1
            assert b"foot" in lib.bmpc_last_error()
            assert fn(h, 0, C.byref(inp), ptr(u), C.byref(eo), *extra) == 0
    finally:
        lib.bmpc_destroy(h)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_wrong_controls_shape_raises_before_any_solver_exists():
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import api
    h = 10
    mpc = bm.MPC()
    before = dict(api._SOLVERS)
    con = np.ones((h, 2), int)
    for bad in (np.zeros((h, 13)), np.zeros((h - 1, 12)), np.zeros((2, h, 12))):
        with pytest.raises(ValueError, match="controls"):
            bm.evaluate_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, bad)
    for bad in (np.zeros((1, h, 11)), np.zeros((1, h + 1, 12)), np.zeros((h, 12)), np.zeros((1, h, 12), int)):
        with pytest.raises(ValueError, match="controls"):
            bm.evaluate_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], bad, mpc=mpc)
    assert api._SOLVERS == before                  # no handle was created on the way


def test_evaluate_mpc_takes_the_reference_orientation():
    """`evaluate_mpc*` take x_ref (13,h) / foot_ref (6,h) as `solve_mpc*` do: the same conversion and the same checks, before the call."""
    import biped_mpc_py_amd as bm
    h = 10
    mpc = bm.MPC()
    x13 = np.vstack([np.zeros((12, h)), np.ones((1, h))])
    u = np.zeros((h, 12))
    con = np.ones((h, 2), int)
    with pytest.raises(ValueError, match="shape"):
        bm.evaluate_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, u, x_ref=x13.T)           # the kernel layout is refused
    bad = x13.copy(); bad[12] = 2.0
    with pytest.raises(ValueError, match="ones"):
        bm.evaluate_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, u, x_ref=bad)
    with pytest.raises(ValueError, match="shape"):
        bm.evaluate_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], u[None], mpc=mpc, foot_ref=np.zeros((1, h, 6)))
    import inspect
    sig = inspect.signature(bm.BatchSolver.solve)
    assert sig.parameters["evaluate"].default is False
    assert list(inspect.signature(bm.BatchSolver.evaluate).parameters)[1:] == [
        "x_fb", "foot", "contact", "phase", "controls", "x_cmd", "mu", "x_ref", "foot_ref", "want_states"]
