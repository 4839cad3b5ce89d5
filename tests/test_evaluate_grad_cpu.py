"""Gradient of the evaluated cost (include/bmpc.h `bmpc_evaluate_grad*`) without a GPU: the kernel's source run on the CPU
(tests/emu/bmpc_emu.cpp) against the oracle's matrices (tests/eval_grad_cases.py `yardstick`) and against the merged
evaluation, the C ABI's struct and argument checks, and the Python surface."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import eval_cases as ec
from tests import eval_grad_cases as gc
from tests import util


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")


def _grad(g, idx=None, args=None, **kw):
    import __graft_entry__ as ge
    ge.build()
    from tests.emu import emu_eval
    return emu_eval.evaluate_grad(ec.cparams_of(g), **(args if args is not None else ec.kernel_args(g, idx)), **kw)


def _eval(g, idx=None, args=None):
    import __graft_entry__ as ge
    ge.build()
    from tests.emu import emu_eval
    return emu_eval.evaluate(ec.cparams_of(g), **(args if args is not None else ec.kernel_args(g, idx)), want_states=False)


# ---- the kernel's source on the CPU ------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("which", ["ref_tracking", "ref_tracking_broken", "generated", "horizons"])
def test_gradient_against_the_yardstick(which):
    """Case 1: grad_u, grad_x0 and cost against the yardstick on the case sets of eval_cases; cost bit-identical to the merged
    evaluation's."""
    groups = dict(ref_tracking=ec.ref_tracking_groups, ref_tracking_broken=lambda: ec.ref_tracking_groups(breaking=True),
                  generated=ec.generated_groups, horizons=ec.horizon_groups)[which]()
    assert groups
    for g in groups:
        got = _grad(g)
        gc.check(got, gc.yardstick_group(g), g["name"])
        assert np.array_equal(got["cost"], _eval(g)["cost"]), g["name"]


@needs_emu
@pytest.mark.parametrize("h", [10, 20, 40])
def test_result_does_not_depend_on_the_batch(h):
    """Case 2: an instance alone and inside a batch of 200 in shuffled order gives identical bits in every output."""
    g, perm = gc.batch_group(h)
    full = _grad(g, perm)
    for pos in gc.BATCH_POSITIONS:
        one = _grad(g, perm[pos:pos + 1])
        for k in gc.KEYS:
            assert np.array_equal(one[k][0], full[k][pos]), (pos, k)
    gc.check({k: v[:8] for k, v in full.items()}, gc.yardstick_group(g, perm[:8]), f"batch200_h{h}")


@needs_emu
def test_bad_instances_get_nan_and_touch_nobody():
    """Case 3: the three spoiled instances of eval_cases.bad_batch are NaN in all outputs, the other five bit-identical to the clean
    batch; each nullable output can be left out without changing the others."""
    clean, bad, idx = ec.bad_batch()
    a = _grad(clean)
    b = _grad(bad, args=ec.kernel_args_unchecked(bad))
    ok = [i for i in range(8) if i not in idx]
    for k in gc.KEYS:
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    for left_out in gc.KEYS:
        want = tuple(k for k in gc.KEYS if k != left_out)
        part = _grad(bad, args=ec.kernel_args_unchecked(bad), want=want)
        assert part[left_out] is None
        for k in want:
            assert np.array_equal(part[k], b[k], equal_nan=True), (left_out, k)
    only = _grad(clean, want=("grad_x0",))
    assert only["cost"] is None and only["grad_u"] is None and np.array_equal(only["grad_x0"], a["grad_x0"])


@needs_emu
def test_gradient_is_the_difference_of_the_merged_evaluation():
    """Case 4, two independent code paths: with U and D on a 2^-10 grid (U +- D exact in fp32), (cost(U + D) - cost(U - D)) / 2 from
    the evaluation kernel equals grad_u . D from the gradient kernel, and the second difference is non-negative."""
    groups = ec.ref_tracking_groups() + [g for g in ec.horizon_groups() if g["h"] in (1, 13, 40)] + ec.generated_groups()[-1:]
    for n, g in enumerate(groups):
        U, D = gc.grid_pair(g, 4000 + n)
        cost_of = lambda c: _eval(dict(g, controls=c))["cost"]
        gc.check_identity(cost_of, _grad(dict(g, controls=U))["grad_u"], g, U, D, g["name"])


@needs_emu
def test_the_references_own_optima_satisfy_the_variational_inequality():
    """Case 5: on the fixture controls of ref_tracking.npz (the reference's own optima), -(grad_u . U*) / max(1, cost) >= -OPT_TOL[h]
    (V = 0 in g . (V - U*) >= 0).  The yardstick's own figure is printed next to the kernel's."""
    for g in ec.ref_tracking_groups():
        got = _grad(g)
        ref = gc.yardstick_group(g)
        q, qy = gc.optimality(got["grad_u"], g["controls"], got["cost"]), gc.optimality(ref["grad_u"], g["controls"], ref["cost"])
        print("optimality h", g["h"], "kernel min %.3e" % q.min(), "yardstick min %.3e" % qy.min(), "tol %.1e" % gc.OPT_TOL[g["h"]])
        assert (q >= -gc.OPT_TOL[g["h"]]).all(), (g["h"], q.min())


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    return _lib.load()


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
def test_bmpc_grad_out_layout_matches_ctypes(tmp_path):
    from biped_mpc_py_amd import _lib
    fields = [f[0] for f in _lib.CGradOut._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpc.h"\nint main(void) {\n  printf("%zu", sizeof(bmpc_grad_out));\n'
                   + "".join(f'  printf(" %zu", offsetof(bmpc_grad_out, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(util.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.CGradOut)] + [getattr(_lib.CGradOut, n).offset for n in fields]
    assert fields == ["cost", "grad_u", "grad_x0"]


def test_argument_checks_without_a_device(lib):
    """The ABI version stays 13 and the entries are found by their symbols; a NULL handle, descriptor, controls or out is
    BMPC_ERR_INVALID before anything touches a device and bmpc_last_error names the argument; with a device also all three outputs
    NULL, foot == NULL without foot_ref and B out of range, and B = 0 succeeds."""
    from biped_mpc_py_amd import _lib
    assert lib.bmpc_abi_version() == 13
    assert "bmpc_evaluate_grad" in _lib.EXPORTS and "bmpc_evaluate_grad_device" in _lib.EXPORTS
    inp, go = _lib.CInputs(), _lib.CGradOut()
    u = np.zeros((1, 10, 12), np.float32)
    ptr = lambda a: a.ctypes.data
    fake = C.c_void_p(8)                               # a non-NULL handle that must never be dereferenced: the NULL checks come first
    for fn, extra in ((lib.bmpc_evaluate_grad, []), (lib.bmpc_evaluate_grad_device, [None])):
        assert fn(None, 1, C.byref(inp), ptr(u), C.byref(go), *extra) == -1
        assert b"handle" in lib.bmpc_last_error()
        assert fn(fake, 1, None, ptr(u), C.byref(go), *extra) == -1
        assert b"bmpc_inputs" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), None, C.byref(go), *extra) == -1
        assert b"controls" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), ptr(u), None, *extra) == -1
        assert b"bmpc_grad_out" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), ptr(u), C.byref(_lib.CGradOut()), *extra) == -1
        assert b"at least one" in lib.bmpc_last_error()
    h = C.c_void_p()
    cp = _lib.CParams()
    lib.bmpc_default_params(C.byref(cp), 10)
    if lib.bmpc_create(C.byref(h), C.byref(cp), 0, 16) != 0:
        return                                         # no device here: the checks above are what runs without one
    try:
        x = np.zeros((1, 12), np.float32); ft = np.zeros((1, 6), np.float32); con = np.ones((1, 10, 2), np.uint8); ph = np.zeros(1, np.int32)
        cost = np.zeros(1)
        inp = _lib.CInputs(ptr(x), ptr(ft), ptr(con), ptr(ph), None, None, None, None)
        go = _lib.CGradOut(ptr(cost), None, None)
        for fn, extra in ((lib.bmpc_evaluate_grad, []), (lib.bmpc_evaluate_grad_device, [None])):
            assert fn(h, 17, C.byref(inp), ptr(u), C.byref(go), *extra) == -1
            assert fn(h, -1, C.byref(inp), ptr(u), C.byref(go), *extra) == -1
            nofoot = _lib.CInputs(ptr(x), None, ptr(con), ptr(ph), None, None, None, None)
            assert fn(h, 1, C.byref(nofoot), ptr(u), C.byref(go), *extra) == -1
            assert b"foot" in lib.bmpc_last_error()
            assert fn(h, 0, C.byref(inp), ptr(u), C.byref(go), *extra) == 0
    finally:
        lib.bmpc_destroy(h)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_wrong_controls_raise_before_any_solver_exists():
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import api
    h = 10
    mpc = bm.MPC()
    before = dict(api._SOLVERS)
    con = np.ones((h, 2), int)
    for bad in (np.zeros((h, 13)), np.zeros((h - 1, 12)), np.zeros((2, h, 12))):
        with pytest.raises(ValueError, match="controls"):
            bm.evaluate_grad_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, bad)
    for bad in (np.zeros((1, h, 11)), np.zeros((1, h + 1, 12)), np.zeros((h, 12)), np.zeros((1, h, 12), int)):
        with pytest.raises(ValueError, match="controls"):
            bm.evaluate_grad_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], bad, mpc=mpc)
    assert api._SOLVERS == before                      # no handle was created on the way


def test_evaluate_grad_mpc_takes_the_reference_orientation():
    """`evaluate_grad_mpc*` take x_ref (13,h) / foot_ref (6,h) as `evaluate_mpc*` do and refuse the kernel layout; the new methods
    exist with the documented signatures and the old ones keep theirs."""
    import inspect
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import api
    h = 10
    mpc = bm.MPC()
    before = dict(api._SOLVERS)
    x13 = np.vstack([np.zeros((12, h)), np.ones((1, h))])
    u = np.zeros((h, 12))
    con = np.ones((h, 2), int)
    with pytest.raises(ValueError, match="shape"):
        bm.evaluate_grad_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, u, x_ref=x13.T)
    bad = x13.copy(); bad[12] = 2.0
    with pytest.raises(ValueError, match="ones"):
        bm.evaluate_grad_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, u, x_ref=bad)
    with pytest.raises(ValueError, match="shape"):
        bm.evaluate_grad_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], u[None], mpc=mpc, foot_ref=np.zeros((1, h, 6)))
    assert api._SOLVERS == before
    args = ["x_fb", "foot", "contact", "phase", "controls", "x_cmd", "mu", "x_ref", "foot_ref"]
    assert list(inspect.signature(bm.BatchSolver.evaluate_grad).parameters)[1:] == args
    assert list(inspect.signature(bm.BatchSolver.cost_torch).parameters)[1:] == args
    assert list(inspect.signature(bm.BatchSolver.evaluate_grad_device).parameters)[1:] == args + ["cost", "grad_u", "grad_x0", "stream"]
    assert "fixed" in bm.BatchSolver.cost_torch.__doc__
