"""The mat-vec of the iteration on the row-pair layout, and a scheduled move's penalties kept over the reduction, against the
code they replace, on the CPU emulation (no GPU needed).

After a row-pair sweep V stays in the row-pair layout and phase P4 (gamma = V beta, bmpc_kernels.hip) runs on it
(-DBMPC_ROWPAIR_MATVEC): values are not moved back, beta is published in the quarters of a pivot column, and the four chains of
the sum run over the same columns in the same order.  A scheduled penalty move is formed once instead of before and behind the
reduction (-DBMPC_RECLASSIFY_ONCE).  Neither changes any arithmetic, so the emulation built with each on and off -- all four
combinations -- must agree to the bit in everything a solve returns: on a standing batch, on a turning one with a mixed gait,
and, both forms on against both off, through the regularised repeat of a sweep that met a lost pivot (the pivot floor raised
at compile time, -DBMPC_PIV_MIN, so that every factorisation takes the repeat)."""
import os
import subprocess

import numpy as np
import pytest

from tests import util
from tests.emu import emu

B = 3
H = 10
KEYS = ("controls", "states", "residuals", "iters", "status", "nfactor")
# (mat-vec, kept move): the parent's code is "00"
FORMS = ("00", "10", "01", "11")
REPEAT_FORMS = ("00", "11")       # through the regularised repeat: the parent's code against both forms at once
needs_clang = pytest.mark.skipif(not os.path.exists(emu.CLANG), reason="host clang not available")


@pytest.fixture(scope="module")
def emulations(tmp_path_factory):
    """name -> the emulation library built with the defines of that name: the four forms, plain and with the repeat forced."""
    from biped_mpc_py_amd.synth import kernel_source_paths
    out = tmp_path_factory.mktemp("emu_matvec")
    assert kernel_source_paths()
    procs = {}
    for form in FORMS:
        for tag, extra in (("", []), ("_repeat", ["-DBMPC_PIV_MIN=1.0e-2f"])):
            if tag and form not in REPEAT_FORMS:
                continue
            name = form + tag
            so = str(out / ("libbmpc_emu_%s.so" % name))
            defs = ["-DBMPC_ROWPAIR_HN=30", "-DBMPC_ROWPAIR_MATVEC=" + form[0], "-DBMPC_RECLASSIFY_ONCE=" + form[1]] + extra
            procs[name] = (so, subprocess.Popen(
                [emu.CLANG, "-std=c++20", "-O1", "-w", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE", "-ffp-contract=off",
                 "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", os.path.join(emu.HERE, "bmpc_emu.cpp"), "-o", so] + defs))
    libs = {}
    for name, (so, pr) in procs.items():
        assert pr.wait() == 0, name
        libs[name] = so
    return libs


def _solve(monkeypatch, so, cparams, s):
    monkeypatch.setattr(emu, "build", lambda force=False: so)
    return emu.solve(cparams, s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], mu=s["mu"])


def _params(s, case=None):
    import biped_mpc_py_amd as bm
    mpc, biped = bm.MPC(), bm.Biped()
    mpc.h = H
    for mod, obj in zip(case or (None, None), (mpc, biped)):
        if mod:
            mod(obj)
    return bm.pack_params(mpc, biped, half=s["half"], solver_options=dict(path=1))


def _same(a, b, where):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (where, k, a[k], b[k])


@needs_clang
@pytest.mark.parametrize("turning", [False, True], ids=["standing", "turning"])
def test_no_form_moves_a_digit(emulations, monkeypatch, turning):
    s = util.synth_batch(B, H, 250, gait="mixed", vx_cmd=True, turn=True) if turning else util.synth_batch(B, H, 250, gait="standing")
    cp = _params(s)
    parent = _solve(monkeypatch, emulations["00"], cp, s)
    print("turning=%s: iters %s nfactor %s status %s" % (turning, parent["iters"], parent["nfactor"], parent["status"]))
    assert (parent["status"] == 0).all()
    # penalty moves were taken (what the kept move is about), and so were several factorisations (V overwritten in its layout)
    assert (parent["nfactor"] >= 2).all(), parent["nfactor"]
    for form in FORMS[1:]:
        _same(_solve(monkeypatch, emulations[form], cp, s), parent, form)


@needs_clang
def test_no_form_moves_a_digit_through_the_regularised_repeat(emulations, monkeypatch):
    s = util.synth_batch(B, H, 77 + H, gait="standing")
    cp = _params(s, util.WEIGHT_CASES["Q_x10"])
    parent = _solve(monkeypatch, emulations["00_repeat"], cp, s)
    plain = _solve(monkeypatch, emulations["00"], cp, s)
    print("Q x 10 through the repeat: iters %s (without it %s) status %s" % (parent["iters"], plain["iters"], parent["status"]))
    # the repeat was taken: the regularised inverse preconditions differently, the iterates differ from the plain sweep's
    assert not np.array_equal(parent["residuals"], plain["residuals"]) or not np.array_equal(parent["iters"], plain["iters"])
    for form in REPEAT_FORMS[1:]:
        _same(_solve(monkeypatch, emulations[form + "_repeat"], cp, s), parent, form)
