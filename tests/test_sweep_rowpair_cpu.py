"""The row-pair form of the symmetric sweep against the row-half form it replaces, on the CPU emulation (no GPU needed).

The row-pair form (bmpc_kernels.hip, factor(): a lane holds half the columns of TWO rows during the sweep) moves values and
changes no arithmetic: every entry of V sees the same FMAs with the same operands in the same order.  So the emulation built
with the form on (-DBMPC_ROWPAIR_HN=30) and off (-DBMPC_ROWPAIR_HN=0) must agree to the bit in everything a solve returns,
at every horizon that takes the form -- on a standing batch, on a turning one, and through the regularised repeat of a sweep
that met a lost pivot.  The repeat is rare (1 .. 2 instances in 16384 a decade off the reference's weights), so the third case also
raises the pivot floor at compile time (-DBMPC_PIV_MIN): every factorisation then takes the repeat, which shows in the result."""
import os
import subprocess

import numpy as np
import pytest

from tests import util
from tests.emu import emu

B = 3
KEYS = ("controls", "states", "residuals", "iters", "status", "nfactor")
# the dense horizons whose sweep takes the row-pair form at BMPC_ROWPAIR_HN = 30 (five steps fill a wave, 3 h <= 30)
ROWPAIR_HORIZONS = (10,)
needs_clang = pytest.mark.skipif(not os.path.exists(emu.CLANG), reason="host clang not available")


@pytest.fixture(scope="module")
def emulations(tmp_path_factory):
    """name -> the emulation library built with the extra defines of that name."""
    from biped_mpc_py_amd.synth import kernel_source_paths
    out = tmp_path_factory.mktemp("emu_rowpair")
    on, off, repeat = "-DBMPC_ROWPAIR_HN=30", "-DBMPC_ROWPAIR_HN=0", "-DBMPC_PIV_MIN=1.0e-2f"
    variants = {"on": [on], "off": [off], "on_repeat": [on, repeat], "off_repeat": [off, repeat]}
    assert kernel_source_paths()
    procs = {}
    for name, defs in variants.items():
        so = str(out / ("libbmpc_emu_%s.so" % name))
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


def _params(h, s, case=None):
    import biped_mpc_py_amd as bm
    mpc, biped = bm.MPC(), bm.Biped()
    mpc.h = h
    for mod, obj in zip(case or (None, None), (mpc, biped)):
        if mod:
            mod(obj)
    return bm.pack_params(mpc, biped, half=s["half"], solver_options=dict(path=1))


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


@needs_clang
@pytest.mark.parametrize("h", ROWPAIR_HORIZONS)
@pytest.mark.parametrize("turn", [False, True], ids=["standing", "turning"])
def test_rowpair_sweep_moves_no_digit(emulations, monkeypatch, h, turn):
    s = util.synth_batch(B, h, 240 + h, gait="standing", turn=turn)
    cp = _params(h, s)
    on, off = _solve(monkeypatch, emulations["on"], cp, s), _solve(monkeypatch, emulations["off"], cp, s)
    print("h=%d turn=%s: iters %s nfactor %s status %s" % (h, turn, on["iters"], on["nfactor"], on["status"]))
    assert (on["status"] == 0).all() and (on["nfactor"] >= 1).all()
    _same(on, off)


@needs_clang
@pytest.mark.parametrize("h", ROWPAIR_HORIZONS)
def test_rowpair_sweep_through_the_regularised_repeat(emulations, monkeypatch, h):
    s = util.synth_batch(B, h, 77 + h, gait="standing")
    cp = _params(h, s, util.WEIGHT_CASES["Q_x10"])
    on, off = _solve(monkeypatch, emulations["on_repeat"], cp, s), _solve(monkeypatch, emulations["off_repeat"], cp, s)
    plain = _solve(monkeypatch, emulations["on"], cp, s)
    print("h=%d Q x 10 through the repeat: iters %s (without it %s) status %s" % (h, on["iters"], plain["iters"], on["status"]))
    # the repeat was taken: the regularised inverse preconditions differently, the iterates differ from the plain sweep's
    assert not np.array_equal(on["residuals"], plain["residuals"]) or not np.array_equal(on["iters"], plain["iters"])
    _same(on, off)
