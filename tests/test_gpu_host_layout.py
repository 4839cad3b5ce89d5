"""The layout of the handle's page-locked I/O block (`bmpc_host_io`, include/bmpc.h), stated here on its own -- not read from the
C side's field table: which arrays there are, in which order, how wide, on which boundary."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import util

# (view, elements per instance as a function of h, bytes per element, the with_* flag it depends on or None), in block order
INPUTS = (("x_fb", lambda h: 12, 4, None), ("foot", lambda h: 6, 4, None), ("phase", lambda h: 1, 4, None),
          ("x_cmd", lambda h: 12, 4, "x_cmd"), ("mu", lambda h: 2 * h, 4, "mu"), ("contact", lambda h: 2 * h, 1, None))
OUTPUTS = (("controls", lambda h: 12 * h, 8, None), ("states", lambda h: 13 * h, 8, "states"), ("iters", lambda h: 1, 4, None),
           ("status", lambda h: 1, 4, None), ("nfactor", lambda h: 1, 4, None), ("residuals", lambda h: 2, 4, None))


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def layout_offsets(sol, B, flags):
    """{view: address, or None for a null view} of one bmpc_host_io call."""
    from biped_mpc_py_amd import _lib
    v = _lib.CHostViews()
    _lib.check(sol._lib.bmpc_host_io(sol._h, B, int(flags["x_cmd"]), int(flags["mu"]), int(flags["states"]), C.byref(v)))
    return {name: getattr(v, name) for name, _ in _lib.CHostViews._fields_}


@pytest.mark.gpu
def test_io_block_layout():
    """For h = 10 and h = 33, B = 5 and B = 1023 and all eight (with_x_cmd, with_mu, with_states): every view the layout holds lies
    on a 64-byte boundary; the inputs follow each other as x_fb, foot, phase, x_cmd, mu, contact and the outputs as controls,
    states, iters, status, nfactor, residuals; no two arrays overlap -- each ends, B x width x element size bytes on, at or before
    the start of the next --; a view the flags leave out is null."""
    import biped_mpc_py_amd as bm
    for h in (10, 33):
        mpc = bm.MPC()
        mpc.h = h
        sol = bm.BatchSolver(mpc=mpc, max_batch=1023)
        for B, (xc, mu, st) in itertools.product((5, 1023), itertools.product((False, True), repeat=3)):
            flags = dict(x_cmd=xc, mu=mu, states=st)
            a = layout_offsets(sol, B, flags)
            where = (h, B, flags)
            assert set(a) == {r[0] for r in INPUTS + OUTPUTS}, where
            for rows in (INPUTS, OUTPUTS):
                end = 0
                for name, width, elem, flag in rows:
                    if flag is not None and not flags[flag]:
                        assert a[name] is None, (where, name)
                        continue
                    assert a[name] is not None and a[name] % 64 == 0, (where, name)
                    assert a[name] >= end, (where, name)                      # the order, and no overlap with what came before
                    end = a[name] + B * width(h) * elem
            # the two blocks are separate allocations or disjoint ranges
            in_lo, in_hi = a["x_fb"], a["contact"] + B * 2 * h
            out_lo, out_hi = a["controls"], a["residuals"] + B * 2 * 4
            assert in_hi <= out_lo or out_hi <= in_lo, where
        sol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path,h", [(1, 10), (2, 26)])               # dense h = 10; stage h = 26, the smallest two-wave variant
def test_absolute_round_trip_solves_alike(path, h):
    """The block with penalty_mode ABSOLUTE and the five numbers of `bmpc_effective_penalties` written back
    (tests/test_host_logic.py: it resolves to the same kernel parameters) solves bit for bit like the SCALED block it came from:
    8 walking instances at Q x 10, each block on a fresh handle."""
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import _lib
    B = 8
    s = util.synth_batch(B, h, 7, gait="walking", vx_cmd=True)
    cp = util.case_params(util.WEIGHT_CASES["Q_x10"], h, path)
    cp.half = s["half"]
    eff = (C.c_double * 5)()
    _lib.check(_lib.load().bmpc_effective_penalties(C.byref(cp), eff))
    got = []
    for block in (cp, util.absolute_round_trip(cp, list(eff))):
        sol = bm.BatchSolver(cparams=block, max_batch=B)
        assert sol._lib.bmpc_solver_path(sol._h) == path
        x, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"])
        got.append(dict(controls=u, states=x, **{k: info[k] for k in ("iters", "nfactor", "status", "residuals")}))
        sol.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k
