"""KKT certificate of given controls (include/bmpc.h `bmpc_certify*`) without a GPU: the kernel's source run on the CPU
(tests/emu/bmpc_emu.cpp) against the yardstick of tests/certify_cases.py (the oracle's matrices and SciPy's NNLS, read from
tests/golden/certify.npz), against the merged evaluation and gradient, the C ABI's struct and argument checks, and the Python
surface."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import certify_cases as cc
from tests import eval_cases as ec
from tests import util


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")


def _cert(g, idx=None, args=None, **kw):
    import __graft_entry__ as ge
    ge.build()
    from tests.emu import emu_eval
    return emu_eval.certify(ec.cparams_of(g), **(args if args is not None else ec.kernel_args(g, idx)), **kw)


def _grad(g):
    from tests.emu import emu_eval
    return emu_eval.evaluate_grad(ec.cparams_of(g), **ec.kernel_args(g))


def _eval(g):
    from tests.emu import emu_eval
    return emu_eval.evaluate(ec.cparams_of(g), **ec.kernel_args(g), want_states=False)


@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture()


# ---- the kernel's source on the CPU ------------------------------------------------------------------------------------------------

@needs_emu
def test_oracle_optima_match_the_yardstick(fx):
    """Case 1: on the oracle's optima rounded to fp32, everything matches the yardstick within certify_cases.REL_BOUND, n_active is
    equal, lam is >= 0 and exactly 0 on inactive rows, and duals_to_reference_order(lam) matches solve_qp's multipliers on the rows
    whose multiplier is unique within certify_cases.QP_REL_BOUND."""
    groups = cc.optimum_groups()
    assert len(groups) == 20
    for g in groups:
        ref = cc.expected(fx, g["name"], "opt")
        assert np.array_equal(ref["controls"], g["controls"].astype(np.float32)), g["name"]
        got = _cert(g, act_tol=ref["act_tol"])
        cc.check(got, ref, g["name"] + "/opt")
        q = cc.qp_deviation(got["lam"], ref)
        print("certify lam against solve_qp", g["name"], "%.3e" % q.max(), "bound %.3e" % cc.QP_REL_BOUND)
        assert q.max() <= cc.QP_REL_BOUND, (g["name"], q.max())


@needs_emu
def test_no_active_rows_gives_the_gradient_back():
    """Case 2: act_tol = -1 activates nothing: lam is all zero, n_active 0, resid is bit-identical to evaluate_grad's grad_u and
    primal_ineq to the maximum of evaluate's four violations."""
    for g in cc.optimum_groups():
        got = _cert(g, act_tol=-1.0)
        assert not got["lam"].any() and not got["n_active"].any() and not got["status"].any(), g["name"]
        gu = _grad(g)["grad_u"]
        assert np.array_equal(got["resid"], gu), g["name"]
        assert np.array_equal(got["summary"][:, 1], _eval(g)["violation"].max(1)), g["name"]
        assert np.array_equal(got["summary"][:, 0], np.abs(gu).reshape(gu.shape[0], -1).max(1)), g["name"]
        assert np.array_equal(got["summary"][:, 3], got["summary"][:, 0]) and not got["summary"][:, 2].any(), g["name"]


@needs_emu
def test_a_worse_plan_certifies_worse(fx):
    """Case 3: the optimum with 1 % relative noise, clipped back into the box, matches the yardstick too, and its stationarity /
    grad_scale is larger than the optimum's on every instance (certify_cases.assert_worse: an instance whose box is the single
    point 0 has no other plan; there the two certificates must be the same bits)."""
    for g in cc.optimum_groups():
        opt, pert = cc.expected(fx, g["name"], "opt"), cc.expected(fx, g["name"], "pert")
        U = cc.perturbed(g, cc.pert_seed(g["name"]))
        assert np.array_equal(pert["controls"], U.astype(np.float32)), g["name"]
        a = _cert(g, act_tol=opt["act_tol"])
        b = _cert(dict(g, controls=U), act_tol=pert["act_tol"])
        cc.check(b, pert, g["name"] + "/pert")
        ra, rb = a["summary"][:, 0] / a["summary"][:, 3], b["summary"][:, 0] / b["summary"][:, 3]
        print("certify worse plan", g["name"], "optimum max %.3e" % ra.max(), "perturbed min %.3e" % rb.min())
        cc.assert_worse(g, U, a, b)


@needs_emu
@pytest.mark.parametrize("h", [10, 20, 40])
def test_result_does_not_depend_on_the_batch(h):
    """Case 4: an instance alone and inside a batch of 200 in shuffled order gives identical bits in every output."""
    g, perm = cc.batch_group(h)
    full = _cert(g, perm)
    assert (full["status"] == 0).all() and (full["n_active"] > 0).all()
    for pos in cc.BATCH_POSITIONS:
        one = _cert(g, perm[pos:pos + 1])
        for k in cc.KEYS:
            assert np.array_equal(one[k][0], full[k][pos]), (pos, k)


@needs_emu
def test_bad_instances_get_nan_and_touch_nobody():
    """Case 5: the three spoiled instances of eval_cases.bad_batch are NaN / -1 / 2, the other five bit-identical to the clean
    batch; each nullable output can be left out without changing the others."""
    clean, bad, idx = ec.bad_batch()
    a = _cert(clean)
    b = _cert(bad, args=ec.kernel_args_unchecked(bad))
    ok = [i for i in range(8) if i not in idx]
    for k in ("lam", "resid", "summary"):
        assert np.isnan(b[k][idx]).all(), k
        assert np.array_equal(a[k][ok], b[k][ok]) and np.isfinite(a[k]).all(), k
    assert (b["n_active"][idx] == -1).all() and (b["status"][idx] == 2).all()
    assert np.array_equal(a["n_active"][ok], b["n_active"][ok]) and (b["status"][ok] == 0).all() and (a["status"] == 0).all()
    for left_out in cc.KEYS:
        want = tuple(k for k in cc.KEYS if k != left_out)
        part = _cert(bad, args=ec.kernel_args_unchecked(bad), want=want)
        assert part[left_out] is None
        for k in want:
            assert np.array_equal(part[k], b[k], equal_nan=True), (left_out, k)
    only = _cert(clean, want=("status",))
    assert all(only[k] is None for k in cc.KEYS if k != "status") and np.array_equal(only["status"], a["status"])


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    return _lib.load()


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
def test_bmpc_cert_out_layout_matches_ctypes(tmp_path):
    from biped_mpc_py_amd import _lib
    fields = [f[0] for f in _lib.CCertOut._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpc.h"\nint main(void) {\n  printf("%zu", sizeof(bmpc_cert_out));\n'
                   + "".join(f'  printf(" %zu", offsetof(bmpc_cert_out, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(util.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.CCertOut)] + [getattr(_lib.CCertOut, n).offset for n in fields]
    assert fields == ["lam", "resid", "summary", "n_active", "status"]


def test_argument_checks_without_a_device(lib):
    """The ABI version stays 13 and the entries are found by their symbols; a NULL handle, descriptor, controls or out, all five
    outputs NULL and a NaN act_tol are BMPC_ERR_INVALID before anything touches a device and bmpc_last_error names the argument;
    with a device also foot == NULL without foot_ref and B out of range, and B = 0 succeeds."""
    from biped_mpc_py_amd import _lib
    assert lib.bmpc_abi_version() == 13
    assert "bmpc_certify" in _lib.EXPORTS and "bmpc_certify_device" in _lib.EXPORTS
    inp, co = _lib.CInputs(), _lib.CCertOut()
    u = np.zeros((1, 10, 12), np.float32)
    ptr = lambda a: a.ctypes.data
    fake = C.c_void_p(8)                               # a non-NULL handle that must never be dereferenced: the NULL checks come first
    for fn, extra in ((lib.bmpc_certify, []), (lib.bmpc_certify_device, [None])):
        assert fn(None, 1, C.byref(inp), ptr(u), 1e-4, C.byref(co), *extra) == -1
        assert b"handle" in lib.bmpc_last_error()
        assert fn(fake, 1, None, ptr(u), 1e-4, C.byref(co), *extra) == -1
        assert b"bmpc_inputs" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), None, 1e-4, C.byref(co), *extra) == -1
        assert b"controls" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), ptr(u), 1e-4, None, *extra) == -1
        assert b"bmpc_cert_out" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), ptr(u), 1e-4, C.byref(_lib.CCertOut()), *extra) == -1
        assert b"at least one" in lib.bmpc_last_error()
        assert fn(fake, 1, C.byref(inp), ptr(u), float("nan"), C.byref(co), *extra) == -1
        assert b"act_tol" in lib.bmpc_last_error()
    h = C.c_void_p()
    cp = _lib.CParams()
    lib.bmpc_default_params(C.byref(cp), 10)
    if lib.bmpc_create(C.byref(h), C.byref(cp), 0, 16) != 0:
        return                                         # no device here: the checks above are what runs without one
    try:
        x = np.zeros((1, 12), np.float32); ft = np.zeros((1, 6), np.float32); con = np.ones((1, 10, 2), np.uint8); ph = np.zeros(1, np.int32)
        status = np.zeros(1, np.int32)
        inp = _lib.CInputs(ptr(x), ptr(ft), ptr(con), ptr(ph), None, None, None, None)
        co = _lib.CCertOut(None, None, None, None, ptr(status))
        for fn, extra in ((lib.bmpc_certify, []), (lib.bmpc_certify_device, [None])):
            assert fn(h, 17, C.byref(inp), ptr(u), 1e-4, C.byref(co), *extra) == -1
            assert fn(h, -1, C.byref(inp), ptr(u), 1e-4, C.byref(co), *extra) == -1
            nofoot = _lib.CInputs(ptr(x), None, ptr(con), ptr(ph), None, None, None, None)
            assert fn(h, 1, C.byref(nofoot), ptr(u), 1e-4, C.byref(co), *extra) == -1
            assert b"foot" in lib.bmpc_last_error()
            assert fn(h, 0, C.byref(inp), ptr(u), 1e-4, C.byref(co), *extra) == 0
    finally:
        lib.bmpc_destroy(h)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_wrong_arguments_raise_before_any_solver_exists():
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import api
    h = 10
    mpc = bm.MPC()
    before = dict(api._SOLVERS)
    con = np.ones((h, 2), int)
    for bad in (np.zeros((h, 13)), np.zeros((h - 1, 12)), np.zeros((2, h, 12))):
        with pytest.raises(ValueError, match="controls"):
            bm.certify_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, bad)
    for bad in (np.zeros((1, h, 11)), np.zeros((1, h + 1, 12)), np.zeros((h, 12)), np.zeros((1, h, 12), int)):
        with pytest.raises(ValueError, match="controls"):
            bm.certify_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], bad, mpc=mpc)
    with pytest.raises(ValueError, match="act_tol"):
        bm.certify_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), con[None], np.zeros((1, h, 12)), mpc=mpc, act_tol=float("nan"))
    x13 = np.vstack([np.zeros((12, h)), np.ones((1, h))])
    with pytest.raises(ValueError, match="shape"):
        bm.certify_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), con, np.zeros((h, 12)), x_ref=x13.T)
    assert api._SOLVERS == before                      # no handle was created on the way


def test_python_surface():
    """The new methods exist with the documented signatures and the default act_tol of 1e-4, `solve` keeps its earlier parameters
    in place, and duals_to_reference_order puts row r of step k where REF:273 has it."""
    import inspect
    import biped_mpc_py_amd as bm
    args = ["x_fb", "foot", "contact", "phase", "controls", "x_cmd", "mu", "x_ref", "foot_ref"]
    sig = inspect.signature(bm.BatchSolver.certify)
    assert list(sig.parameters)[1:] == args + ["act_tol"] and sig.parameters["act_tol"].default == 1e-4
    sig = inspect.signature(bm.BatchSolver.certify_device)
    assert list(sig.parameters)[1:] == args + ["lam", "resid", "summary", "n_active", "status", "act_tol", "stream"]
    assert sig.parameters["act_tol"].default == 1e-4
    sig = inspect.signature(bm.BatchSolver.solve)
    assert list(sig.parameters)[1:] == ["x_fb", "foot", "contact", "phase", "x_cmd", "mu", "want_states", "out", "x_ref", "foot_ref",
                                        "evaluate", "certify", "act_tol"]
    assert sig.parameters["certify"].default is False
    assert inspect.signature(bm.certify_mpc).parameters["act_tol"].default == 1e-4
    assert inspect.signature(bm.certify_mpc_batch).parameters["act_tol"].default == 1e-4
    h = 3
    lam = np.zeros((2, h, 36))
    for k in range(h):
        lam[:, k, :] = 1000 * k + np.arange(36)
    flat = bm.duals_to_reference_order(lam)
    assert flat.shape == (2, 36 * h)
    for k in range(h):
        assert np.array_equal(flat[0, 8 * k:8 * k + 8], 1000 * k + np.arange(8))
        assert np.array_equal(flat[0, 8 * h + 24 * k:8 * h + 24 * k + 24], 1000 * k + np.arange(8, 32))
        assert np.array_equal(flat[0, 32 * h + 4 * k:32 * h + 4 * k + 4], 1000 * k + np.arange(32, 36))
    assert np.array_equal(flat[:, cc.ref_index(h)], lam)
    with pytest.raises(ValueError, match="lam"):
        bm.duals_to_reference_order(np.zeros((h, 35)))
