"""CPU: S candidate plans per instance rolled out on the plant (csrc/bmpc_plant_rollout.hip) without a GPU -- the body of
plant_rollout_samples_kernel run as plain C++ (tests/emu/emu_plant_rollout.py) against the NumPy restatement
(tests/rollout_cases.py), the C ABI of the new entries and what they and the Python methods refuse before a device is needed.

Bounds (tests/rollout_cases.py `check`).  Every period is stepped by the model from the RECORDED state before it: 2 fp32 ulps, the
plant tests' bound.  Flags, the ground's reductions, the outcome and the footholds are rules on stored values: exact (a landed
coordinate within 1 fp32 ulp, since the target's fp64 expression may be associated differently; the figures are printed).  The cost
against a long-double recomputation from the stored states: (24 h + 4) 2^-52 relative; the score: sample_cases.SCORE_REL."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import rollout_cases as rc
from tests import util


def _cparams(h):
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    cp = _lib.CParams()
    assert _lib.load().bmpc_default_params(cp, h) == 0
    return cp


@pytest.fixture(scope="module")
def lib():
    _cparams(10)
    from biped_mpc_py_amd import _lib
    return _lib.load()


def _args(c, U, idx=slice(None)):
    return c["x_fb"][idx], c["foot"][idx], c["contact"][idx], U[idx]


def test_the_contact_tables_hold_every_kind():
    for h in (3, 10):
        t = rc.contact_tables(h)
        l = rc.landings(t)
        assert l[0, :, 0].sum() == 1 and not l[0, :, 1].any()            # leg 0 lands, once
        assert l[1, :, 1].sum() == 1 and not l[1, :, 0].any()            # leg 1 lands
        assert not l[2].any() and t[2, 0, 1] == 1 and t[2, -1, 1] == 0   # a lift-off
        assert t[3].all()                                               # double support throughout
        assert l[4, :, 0].any() or l[4, :, 1].any()                     # the walk
    assert not rc.landings(rc.contact_tables(1)).any()


@pytest.mark.parametrize("h,shape,integrator,substeps,name", [
    (10, (5, 13), "rk4", 4, "full"), (10, (5, 13), "euler", 1, "plain"), (3, (5, 67), "euler", 4, "full"), (3, (5, 13), "rk4", 1, "plain"),
    (1, (1, 1), "rk4", 4, "full"), (1, (5, 13), "euler", 4, "plain")])
def test_emulated_rollout_matches_the_restatement(h, shape, integrator, substeps, name):
    from tests.emu import emu_plant_rollout as er
    cp = _cparams(h)
    p = rc.params_of(cp)
    c = rc.case(h)
    B, S = shape
    idx = slice(0, B) if B > 1 else slice(2, 3)
    U = rc.plans(c, S)
    kw = dict(rc.take(rc.variant(c, name), idx), integrator=integrator, substeps=substeps, w_fall=rc.W_FALL, w_slip=rc.W_SLIP,
              w_unloaded=rc.W_UNLOADED, fall=(0.25, 0.3))
    if name == "full":
        kw["fz_floor"] = 20.0
    got = er.rollout(cp, *_args(c, U, idx), **kw)
    ref = rc.check(p, got, _args(c, U, idx), kw, (h, shape, integrator, substeps, name))
    assert np.isfinite(got["cost"]).all()
    if name == "full" and S > 1:
        assert ref["flags"].any() and ref["scaled"].any()


def test_emulated_rollout_moves_feet_only_when_asked_and_runs_free_like_the_restatement():
    from tests.emu import emu_plant_rollout as er
    cp = _cparams(10)
    p = rc.params_of(cp)
    c = rc.case(10)
    U = rc.plans(c, 3)
    args = _args(c, U)
    moved = er.rollout(cp, *args)
    stay = er.rollout(cp, *args, move_feet=False)
    rc.check(p, stay, args, dict(move_feet=False), "move_feet off")
    assert np.array_equal(stay["foot_end"], np.broadcast_to(c["foot"].astype(np.float32)[:, None], stay["foot_end"].shape))
    lands = rc.landings(c["contact"]).any(1)                            # (5, 2)
    changed = (moved["foot_end"] != stay["foot_end"]).reshape(5, 3, 2, 3).any(3)
    assert np.array_equal(changed.all(1), lands) and np.array_equal(changed.any(1), lands)
    # free-running, the restatement's stored states drift from the kernel's by roundings only
    free = rc.restate(p, *args)
    assert np.abs(free["x_traj"].astype(np.float64) - moved["x_traj"]).max() <= 1e-4
    assert np.allclose(free["cost"], moved["cost"], rtol=1e-5)


def test_emulated_bad_data_stays_with_its_sample_or_instance():
    from tests.emu import emu_plant_rollout as er
    cp = _cparams(10)
    c = rc.case(10)
    U = rc.plans(c, 5)
    kw = dict(rc.variant(c, "full"), fall=(np.inf, -np.inf))
    clean = er.rollout(cp, *_args(c, U), **kw)
    assert np.isfinite(clean["cost"]).all() and (clean["first_fall"] == -1).all()
    bad = U.copy()
    bad[1, 2, 2, 4] = np.nan
    got = er.rollout(cp, *_args(c, bad), **kw)
    assert got["first_fall"][1, 2] == 2 and np.isnan(got["cost"][1, 2]) and np.isnan(got["score"][1, 2])
    assert np.isnan(got["x_traj"][1, 2, 2:]).all() and np.array_equal(got["x_traj"][1, 2, :2], clean["x_traj"][1, 2, :2])
    keep = np.ones((5, 5), bool)
    keep[1, 2] = False
    for k in rc.PER_SAMPLE + rc.GROUND_ONLY:
        assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), k
    for what in ("mu", "m", "x_fb", "foot", "x_ref"):
        kb = dict(kw, body=dict(kw["body"]), ground=dict(kw["ground"]))
        x_fb, foot = c["x_fb"].copy(), c["foot"].copy()
        if what == "mu":
            kb["ground"]["mu"] = kw["ground"]["mu"].copy()
            kb["ground"]["mu"][3, 1] = np.nan
        elif what == "m":
            kb["body"]["m"] = kw["body"]["m"].copy()
            kb["body"]["m"][3] = 0.0
        elif what == "x_fb":
            x_fb[3, 7] = np.inf
        elif what == "foot":
            foot[3, 1] = np.nan
        else:
            kb["x_ref"] = kw["x_ref"].copy()
            kb["x_ref"][3, 0, 4] = np.nan
        got = er.rollout(cp, x_fb, foot, c["contact"], U, **kb)
        assert np.isnan(got["cost"][3]).all() and np.isnan(got["x_traj"][3]).all() and (got["first_fall"][3] == 0).all(), what
        keep = [0, 1, 2, 4]
        for k in rc.PER_SAMPLE + rc.GROUND_ONLY:
            assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), (what, k)


NEW = ("bmpc_plant_rollout_samples", "bmpc_plant_rollout_samples_device")


def test_new_symbols_are_exported_and_declared(lib):
    from biped_mpc_py_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(util.ROOT, "include", "bmpc.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(raw, name) and ("int " + name + "(") in header
        assert getattr(lib, name).argtypes is not None
    assert lib.bmpc_abi_version() == 13 and "#define BMPC_ABI_VERSION 13" in header


def test_rollout_struct_layouts_match_c(lib):
    from biped_mpc_py_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu", '
           'sizeof(bmpc_rollout_price), offsetof(bmpc_rollout_price, w_fall), offsetof(bmpc_rollout_price, fz_floor), '
           'sizeof(bmpc_rollout_out), offsetof(bmpc_rollout_out, first_slip), offsetof(bmpc_rollout_out, ess));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert sizes == [C.sizeof(_lib.CRolloutPrice), _lib.CRolloutPrice.w_fall.offset, _lib.CRolloutPrice.fz_floor.offset,
                     C.sizeof(_lib.CRolloutOut), _lib.CRolloutOut.first_slip.offset, _lib.CRolloutOut.ess.offset] == [64, 8, 56, 136, 64, 128]


def test_argument_checks_come_in_the_stated_order_without_a_device(lib):
    """The price block, then the plant block, then a ground-only output without a ground -- all before the handle is looked at --,
    then the handle, the required pointers, the outputs."""
    from biped_mpc_py_amd import _lib
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    ground = _lib.CPlantGround()
    good = dict(S=4, w_fall=1.0, w_slip=0.0, w_unloaded=2.0, temperature=np.inf, tilt_max=np.inf, z_min=-np.inf, fz_floor=0.0)

    def price(**kw):
        v = dict(good, **kw)
        return _lib.CRolloutPrice(v["S"], 0, v["w_fall"], v["w_slip"], v["w_unloaded"], v["temperature"], v["tilt_max"], v["z_min"], v["fz_floor"])

    def calls(pr, plant=None, gr=None, out=None, handle=None):
        a = (handle, 4, None, None, None, None, None, None, None, None if plant is None else C.byref(plant), None, gr,
             None if pr is None else C.byref(pr), None if out is None else C.byref(out))
        return lib.bmpc_plant_rollout_samples(*a), lib.bmpc_plant_rollout_samples_device(*a, None)

    def refused(rcs, word):
        for rc_ in rcs:
            assert rc_ == -1 and word in lib.bmpc_last_error(), (rcs, word, lib.bmpc_last_error())

    bad_plant = _lib.CPlant(1, 0, 1, 0, 0)
    ground_out = _lib.CRolloutOut(mu_demand=addr)
    refused(calls(None, bad_plant), b"null bmpc_rollout_price")
    for kw, word in ((dict(S=0), b"S = 0"), (dict(S=65537), b"S = 65537"), (dict(w_fall=np.nan), b"w_fall"), (dict(w_slip=-1.0), b"w_fall"),
                     (dict(w_unloaded=np.inf), b"w_fall"), (dict(temperature=0.0), b"temperature"), (dict(temperature=np.nan), b"temperature"),
                     (dict(tilt_max=np.nan), b"thresholds"), (dict(z_min=np.nan), b"thresholds"), (dict(fz_floor=np.nan), b"fz_floor"),
                     (dict(fz_floor=-1.0), b"fz_floor")):
        refused(calls(price(**kw), bad_plant, None, ground_out), word)          # the price block comes first
    # within the price block: S, the prices, the temperature, the thresholds, the floor
    refused(calls(price(S=0, w_fall=np.nan)), b"S = 0")
    refused(calls(price(w_fall=np.nan, temperature=0.0)), b"w_fall")
    refused(calls(price(temperature=0.0, tilt_max=np.nan)), b"temperature")
    refused(calls(price(tilt_max=np.nan, fz_floor=-1.0)), b"thresholds")
    # the plant block, as for bmpc_simulate_device, before the outputs that need a ground
    for field, value, word in (("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"), ("integrator", 2, b"integrator"),
                               ("push_from", -1, b"push"), ("push_steps", -1, b"push")):
        bad = _lib.CPlant(1, 4, 1, 0, 0)
        setattr(bad, field, value)
        refused(calls(price(), bad, None, ground_out), word)
    for name in rc.GROUND_ONLY:
        refused(calls(price(), None, None, _lib.CRolloutOut(**{name: addr})), b"need a ground")
    # then the handle, with and without a ground
    refused(calls(price(), None, None, _lib.CRolloutOut(cost=addr)), b"null handle")
    refused(calls(price(), None, C.byref(ground), ground_out), b"null handle")
    refused(calls(price(), None, None, None), b"null handle")


def test_python_keywords_are_checked_before_any_call():
    import biped_mpc_py_amd as bm
    s = object.__new__(bm.BatchSolver)                 # no handle: the checks come first
    s.h = 10
    x, f, c, u = np.zeros((3, 12)), np.zeros((3, 6)), np.ones((3, 10, 2)), np.zeros((3, 4, 10, 12))
    for kw in (dict(integrator="midpoint"), dict(substeps=0), dict(push_from=-1), dict(ground={"friction": 1.0}), dict(ground=0.5),
               dict(w_fall=-1.0), dict(w_slip=np.nan), dict(w_unloaded=np.inf), dict(temperature=0.0), dict(temperature=np.nan),
               dict(fall=(np.nan, 0.0)), dict(fall=0.3), dict(fz_floor=-1.0), dict(fz_floor=np.nan), dict(want=[]), dict(want=["states"]),
               dict(want=["mu_demand"]), dict(want=["cost", "first_slip"]), dict(body={"mass": np.ones(3)}),
               dict(body={"m": np.ones(3, np.float32)}), dict(ground={"mu": np.ones((3, 3))}), dict(x_cmd=np.zeros((3, 13))),
               dict(x_ref=np.zeros((3, 12, 10))), dict(push=np.zeros((2, 6)))):
        with pytest.raises(ValueError):
            s.plant_rollout_samples(x, f, c, u, **kw)
    for bad in (dict(controls=np.zeros((3, 10, 12))), dict(controls=np.zeros((3, 4, 9, 12))), dict(x_fb=np.zeros((2, 12))),
                dict(foot=np.zeros((3, 5))), dict(contact=np.ones((3, 9, 2))), dict(contact=np.full((3, 10, 2), 2))):
        a = dict(x_fb=x, foot=f, contact=c, controls=u)
        a.update(bad)
        with pytest.raises(ValueError):
            s.plant_rollout_samples(**a)
    import torch
    s.device = 0
    for kw, word in ((dict(integrator="midpoint"), "integrator"), (dict(temperature=0.0), "temperature"),
                     (dict(want=["mu_demand"]), "need a ground"), (dict(ground=0.5), "ground must be"), ({}, "must live on cuda")):
        with pytest.raises(ValueError, match=word):
            s.plant_rollout_samples_device(torch.zeros(3, 12), None, None, torch.zeros(3, 4, 10, 12), **kw)
