"""Reference tracking without a GPU: the fixture (the reference's own solve_mpc with its generators replaced, tests/gen_ref_tracking.py)
pinned to the oracle, the kernels' source run on the CPU with supplied references (tests/emu/bmpc_emu.cpp), the C ABI's
`bmpc_inputs` descriptor and argument checks, and the Python layout conversion and checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import refs_cases as rc
from tests import util

FIX = "ref_tracking"
HORIZONS = (10, 16, 20)


def _fix(h):
    d = util.load(FIX)
    p = f"h{h}_"
    return {k[len(p):]: d[k] for k in d.files if k.startswith(p)}


def _row(d, i):
    return {k: d[k][i] for k in ("x_fb", "foot", "contact", "phase", "t", "x_cmd", "x_ref", "foot_ref")} | {"half": int(d["half"])}


def _dense(rcv, n, shape):
    M = np.zeros(shape)
    M[rcv[0], rcv[1]] = n
    return M


@pytest.mark.parametrize("h", HORIZONS)
def test_fixture_is_the_oracle_with_its_generators_replaced(h):
    """The captured QP of every fixture instance is what orc.build_sparse_qp builds with the oracle's generators monkeypatched to
    return the supplied arrays (q, h, b for all; P, G, A for the instances whose triplets are stored), and the fixture covers
    every kind, the line-foot trap (e) and the exact generator output (f) among them."""
    from oracle import bmpc_oracle as orc
    d = _fix(h)
    n = d["x_fb"].shape[0]
    assert set(d["kind"]) == set(rc.KINDS) and d["certified"].all()
    for i in range(n):
        c = _row(d, i)
        mpc = orc.MPC()
        mpc.h, mpc.x_cmd = h, np.asarray(c["x_cmd"], float)
        with rc.supplied(orc, c["x_ref"], c["foot_ref"]):
            sp = orc.build_sparse_qp(np.asarray(c["x_fb"], float), float(c["t"]), np.asarray(c["foot"], float), mpc, orc.Biped(),
                                     np.asarray(c["contact"]), half=c["half"])
        for key, got in (("q", sp["q"]), ("hvec", sp["h"]), ("b", sp["b"])):
            ref = d[key][i]
            assert np.abs(np.reshape(got, -1) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (h, i, key)
        for name in ("P", "G", "A"):
            if f"{name}{i}_rc" in d:
                M = _dense(d[f"{name}{i}_rc"], d[f"{name}{i}_v"], sp[name].shape)
                assert np.abs(sp[name] - M).max() <= 1e-12 * max(1.0, np.abs(M).max()), (h, i, name)
    # kind e: the supplied x_ref is level while x_fb is tilted -- the case where the body axes must come from x_fb
    e = np.flatnonzero(d["kind"] == "e")
    assert np.abs(d["x_fb"][e][:, 0:3]).min() > 0.15 and np.abs(d["x_ref"][e][:, 0:3]).max() == 0.0
    # kind f: the supplied arrays equal the generators' output and are exact in fp32
    for i in np.flatnonzero(d["kind"] == "f"):
        c = _row(d, i)
        mpc = orc.MPC()
        mpc.h, mpc.x_cmd = h, np.asarray(c["x_cmd"], float)
        assert np.array_equal(orc.get_reference_trajectory(np.asarray(c["x_fb"], float), mpc), c["x_ref"])
        assert np.array_equal(orc.get_reference_foot_trajectory(np.asarray(c["x_fb"], float), c["t"], c["foot"], mpc, c["contact"],
                                                                half=c["half"]), c["foot_ref"])
        assert np.array_equal(c["x_ref"].astype(np.float32).astype(float), c["x_ref"])


# ---- the kernels' source on the CPU ------------------------------------------------------------------------------------------------

def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


# (path, h, instances of the fixture at that h): dense at h = 10 / 16 / 20, stage (2,1) at h = 10; (3,1) at h = 13 and (3,2) at
# h = 26 (the two-wave workgroup) run instances generated here against the oracle
_EMU_FIX = [(1, 10, "abcdef"), (1, 16, "ef"), (1, 20, "ae"), (2, 10, "abcdef")]


@pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")
@pytest.mark.parametrize("path,h,kinds", _EMU_FIX)
def test_kernel_source_tracks_supplied_references_on_cpu(path, h, kinds):
    import __graft_entry__ as ge
    ge.build()
    import biped_mpc_py_amd as bm
    from tests.emu import emu
    d = _fix(h)
    idx = [int(np.flatnonzero(d["kind"] == k)[0]) for k in kinds]
    mpc = bm.MPC()
    mpc.h = h
    cp = bm.pack_params(mpc, bm.Biped(), half=int(d["half"]), solver_options=dict(path=path))
    xr, fr = bm.references_to_kernel_layout(d["x_ref"][idx], d["foot_ref"][idx], h)
    o = emu.solve(cp, d["x_fb"][idx], d["foot"][idx], d["contact"][idx], d["phase"][idx], x_cmd=d["x_cmd"][idx],
                       x_ref=xr, foot_ref=fr)
    assert (o["status"] == 0).all(), o["status"]
    assert util.rel_err(o["controls"].astype(float), d["controls"][idx]).max() <= util.REL_TOL
    assert util.rel_err(o["states"].astype(float), d["states"][idx]).max() <= util.REL_TOL
    assert np.array_equal(o["x_ref"], xr) and np.array_equal(o["foot_ref"], fr)    # the debug views: the supplied arrays, widened
    # kind f: supplying the generators' own output changes nothing, bit for bit
    f = [k for k, i in enumerate(idx) if d["kind"][i] == "f"]
    if f:
        g = emu.solve(cp, d["x_fb"][idx][f], d["foot"][idx][f], d["contact"][idx][f], d["phase"][idx][f], x_cmd=d["x_cmd"][idx][f])
        for key in ("controls", "states", "iters", "nfactor", "status"):
            assert np.array_equal(o[key][f], g[key]), key


@pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")
@pytest.mark.parametrize("h,kinds", [(13, "ae"), (26, "ce")])
def test_stage_kernel_source_tracks_supplied_references_on_cpu(h, kinds):
    """The stage variants (3,1) at h = 13 (phantom steps past the horizon) and (3,2) at h = 26 (two waves) with supplied references,
    against the oracle with its generators replaced."""
    import __graft_entry__ as ge
    ge.build()
    import biped_mpc_py_amd as bm
    from tests.emu import emu
    rng = np.random.default_rng(7 + h)
    cases = [rc.make_case(k, h, rng) for k in kinds]
    mpc = bm.MPC()
    mpc.h = h
    cp = bm.pack_params(mpc, bm.Biped(), half=cases[0]["half"], solver_options=dict(path=2))
    st = lambda k: np.stack([c[k] for c in cases])
    xr, fr = bm.references_to_kernel_layout(st("x_ref"), st("foot_ref"), h)
    o = emu.solve(cp, st("x_fb"), st("foot"), st("contact"), st("phase"), x_cmd=st("x_cmd"), x_ref=xr, foot_ref=fr)
    ref = np.stack([rc.oracle_solve(c, h)[0] for c in cases])
    assert (o["status"] == 0).all(), o["status"]
    assert util.rel_err(o["controls"].astype(float), ref).max() <= util.REL_TOL


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    return _lib.load()


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
def test_bmpc_inputs_layout_matches_ctypes(tmp_path):
    from biped_mpc_py_amd import _lib
    fields = [f[0] for f in _lib.CInputs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpc.h"\nint main(void) {\n  printf("%zu", sizeof(bmpc_inputs));\n'
                   + "".join(f'  printf(" %zu", offsetof(bmpc_inputs, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(util.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.CInputs)] + [getattr(_lib.CInputs, n).offset for n in fields]
    assert fields == ["x_fb", "foot", "contact", "phase", "x_cmd", "mu", "x_ref", "foot_ref"]


def test_new_entries_reject_bad_arguments_without_a_device(lib):
    """A null handle, a null descriptor, and foot == NULL without foot_ref are BMPC_ERR_INVALID -- checked before anything touches a
    device (this machine may have none)."""
    from biped_mpc_py_amd import _lib
    inp = _lib.CInputs()
    for fn, extra in ((lib.bmpc_solve_inputs_f64, [None] * 6), (lib.bmpc_solve_inputs_device, [None] * 7),
                      (lib.bmpc_debug_assemble_inputs, [None] * 4)):
        assert fn(None, 1, C.byref(inp), *extra) == -1
        assert fn(None, 1, None, *extra) == -1
    # a handle needs a device; the argument check of the descriptor itself is reached through the null-handle-free path below
    h = C.c_void_p()
    cp = _lib.CParams()
    lib.bmpc_default_params(C.byref(cp), 10)
    if lib.bmpc_create(C.byref(h), C.byref(cp), 0, 16) != 0:
        return                                     # no device here: the null checks above are what runs without one
    try:
        x = np.zeros((1, 12), np.float32); con = np.ones((1, 10, 2), np.uint8); ph = np.zeros(1, np.int32)
        u = np.zeros((1, 10, 12)); ptr = lambda a: a.ctypes.data
        assert lib.bmpc_solve_inputs_f64(h, 1, None, ptr(u), None, None, None, None, None) == -1
        inp = _lib.CInputs(ptr(x), None, ptr(con), ptr(ph), None, None, None, None)
        assert lib.bmpc_solve_inputs_f64(h, 1, C.byref(inp), ptr(u), None, None, None, None, None) == -1
        assert b"foot" in lib.bmpc_last_error()
    finally:
        lib.bmpc_destroy(h)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_orientation_conversion_is_exact():
    import biped_mpc_py_amd as bm
    rng = np.random.default_rng(3)
    h = 10
    x13 = np.vstack([rng.standard_normal((12, h)), np.ones((1, h))])
    f6 = rng.standard_normal((6, h))
    xr, fr = bm.references_to_kernel_layout(x13, f6, h)
    assert xr.shape == (h, 12) and fr.shape == (h, 6)
    assert np.array_equal(xr, x13[:12].T) and np.array_equal(fr, f6.T)
    xb, fb = bm.references_to_kernel_layout(np.stack([x13, x13]), np.stack([f6, f6]), h)
    assert np.array_equal(xb[1], x13[:12].T) and np.array_equal(fb[0], f6.T)
    x12, _ = bm.references_to_kernel_layout(x13[:12], None, h)       # (12, h): no row of ones, the same rows
    assert np.array_equal(x12, xr)


def test_python_checks_raise_before_the_call():
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd.api import _kernel_refs
    h = 10
    x13 = np.vstack([np.zeros((12, h)), np.ones((1, h))])
    f6 = np.zeros((6, h))
    with pytest.raises(ValueError, match="shape"):
        bm.references_to_kernel_layout(x13[:, :h - 1], None, h)
    with pytest.raises(ValueError, match="shape"):
        bm.references_to_kernel_layout(None, np.zeros((5, h)), h)
    bad = x13.copy(); bad[12, 3] = 0.0
    with pytest.raises(ValueError, match="ones"):
        bm.references_to_kernel_layout(bad, None, h)
    bad = x13.copy(); bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        bm.references_to_kernel_layout(bad, None, h)
    bad = f6.copy(); bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        bm.references_to_kernel_layout(None, bad, h)
    with pytest.raises(ValueError, match="shape"):
        _kernel_refs(np.zeros((2, h, 13)), None, 2, h)
    with pytest.raises(ValueError, match="non-finite"):
        _kernel_refs(None, np.full((1, h, 6), np.nan), 1, h)
    # the drop-ins check before any solver (or device) is touched
    mpc = bm.MPC()
    bad = x13.copy(); bad[12] = 2.0
    with pytest.raises(ValueError, match="ones"):
        bm.solve_mpc(np.zeros(12), 0.0, np.zeros(6), mpc, bm.Biped(), np.ones((h, 2), int), x_ref=bad)
    with pytest.raises(ValueError, match="shape"):
        bm.solve_mpc_batch(np.zeros((1, 12)), [0.0], np.zeros((1, 6)), np.ones((1, h, 2), int), mpc=mpc,
                           foot_ref=np.zeros((1, 6, h + 1)))
