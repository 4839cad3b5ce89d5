"""CPU: the plant with a body per instance (csrc/bmpc_plant.hip: plant_body, plant_step_body, plant_outcome) without a GPU -- the
shared bodies of tests/body_cases.py against the model alone (conditioning, sensitivity), the per-instance functions run as plain
C++ (tests/emu/emu_plant_body.py) against the NumPy restatement (tests/plant_model.py), bad bodies, the fall outcome against its
restatement, and the C ABI of the new entries.

The 2-ulp bound is that of tests/test_plant_cpu.py and carries over: both sides compute in fp64; the one new source of error, the
inverse of I_b (adjugate over determinant here, a solve in the model), is bounded by cond(I_b) <= 48 times the fp64 rounding, about
nine orders below an fp32 ulp."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import body_cases as bc
from tests import plant_model as pm
from tests import util

B = 33
SUPPLIED = [(), ("m",), ("I",), ("g",), ("m", "I", "g")]


@pytest.fixture(scope="module")
def cparams():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    cp = _lib.CParams()
    assert _lib.load().bmpc_default_params(cp, 10) == 0
    return cp


@pytest.mark.parametrize("n", [33, 67, 257])
def test_bodies_are_well_conditioned_and_every_member_shows(n):
    """The model alone, on the batches the emulation (33) and the GPU tests (67, 257) use: cond(I) <= 48, and each of m, I, g supplied alone moves the model's next
    state by >= 100 x the 2-ulp bound on at least half of the instances (measured: m without wrench is the thinnest, about three
    quarters -- the instances with no leg in contact feel no force; every other combination shows on all of them)."""
    body = bc.bodies(n)
    assert (body["m"] >= 8).all() and (body["m"] <= 20).all() and (body["g"] >= 3.7).all() and (body["g"] <= 12).all()
    assert np.array_equal(body["I"], body["I"].transpose(0, 2, 1)) or np.abs(body["I"] - body["I"].transpose(0, 2, 1)).max() < 1e-15
    cond = np.linalg.cond(body["I"])
    print("cond(I) max", cond.max())
    assert cond.max() <= bc.COND_MAX
    x, u, foot, c, w = pm.batch(n)
    for integrator in ("euler", "rk4"):
        for wr in (w, None):
            base = pm.step_batch(x, u, foot, c, wr, integrator=integrator)
            for k in bc.MEMBERS:
                moved = bc.step_batch(x, u, foot, c, wr, body=bc.subset(body, (k,)), integrator=integrator)
                share = (pm.ulp_diff(moved.astype(np.float32), base).max(1) >= bc.SENSITIVITY * 2.0).mean()
                print(integrator, "wrench" if wr is not None else "none", k, "share %.2f" % share)
                assert share >= 0.5, (integrator, k, share)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("members", SUPPLIED, ids=lambda m: "+".join(m) or "none")
def test_emulation_matches_model_at_the_instances_body(cparams, integrator, substeps, members):
    from tests.emu import emu_plant_body
    x, u, foot, c, w = pm.batch(B)
    body = bc.subset(bc.bodies(B), members)
    got, ok = emu_plant_body.plant_step(cparams, x, u, foot, c, w, integrator, substeps, body=body)
    ref = bc.step_batch(x, u, foot, c, w, body=body, integrator=integrator, substeps=substeps)
    d = pm.ulp_diff(got, ref)
    print("max ulps", d.max())
    assert ok.all() and np.isfinite(ref).all() and d.max() <= 2.0, d.max()


def test_inertia_as_flat_rows_and_the_handles_inverse_bit_for_bit(cparams):
    """Without I the inverse is the handle's own, bit for bit (nothing is inverted); with I it is the inverse of the instance's."""
    from tests.emu import emu_plant_body
    body = bc.bodies(B)
    ok, P, hinv = emu_plant_body.plant_body(cparams, m=body["m"][3], g=body["g"][3])
    assert ok and np.array_equal(P["Ibinv"], hinv) and np.array_equal(P["Ib"], np.asarray(cparams.I))
    assert P["m"] == body["m"][3] and P["g"] == body["g"][3]
    ok, P, _ = emu_plant_body.plant_body(cparams, I=body["I"][3])
    assert ok and (P["m"], P["g"]) == (cparams.m, cparams.g) and np.array_equal(P["Ib"], body["I"][3].reshape(9))
    assert np.abs(P["Ibinv"].reshape(3, 3) @ body["I"][3] - np.eye(3)).max() <= 48 * 8 * np.finfo(float).eps


BAD = {"m_zero": ("m", 0.0), "m_negative": ("m", -1.0), "m_nan": ("m", np.nan), "g_inf": ("g", np.inf),
       "I_zero_row": ("I", "row"), "I_inf": ("I", "inf")}


@pytest.mark.parametrize("case", list(BAD))
def test_a_bad_body_is_all_nan_and_touches_no_neighbour(cparams, case):
    from tests.emu import emu_plant_body
    x, u, foot, c, w = (a[:5].copy() for a in pm.batch(B))
    good = {k: v[:5].copy() for k, v in bc.bodies(B).items()}
    body = {k: v.copy() for k, v in good.items()}
    member, value = BAD[case]
    if value == "row":
        body["I"][2, 1, :] = 0.0
    elif value == "inf":
        body["I"][2, 0, 0] = np.inf
    else:
        body[member][2] = value
    for members in ((member,), bc.MEMBERS):              # alone, and with the other members supplied too
        clean, ok = emu_plant_body.plant_step(cparams, x, u, foot, c, w, body=bc.subset(good, members))
        assert ok.all() and np.isfinite(clean).all()
        got, ok = emu_plant_body.plant_step(cparams, x, u, foot, c, w, body=bc.subset(body, members))
        assert np.isnan(got[2]).all() and not ok[2] and ok[[0, 1, 3, 4]].all()
        assert np.array_equal(got[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])


def _hand_made_states():
    """(steps 6, B 6): NaN in the middle, every period NaN, never fallen, fallen at period 0, a state exactly at both thresholds
    (not fallen), and one that falls by height late; thresholds (0.5, 0.25) are exact in fp32."""
    steps, n = 6, 6
    x = np.zeros((steps, n, 12), np.float32)
    x[:, :, 5] = 0.5
    x[:, :, 0] = np.linspace(0.05, 0.3, steps, dtype=np.float32)[:, None] * np.array([1, 1, -1, 1, 1, 1], np.float32)
    x[:, :, 1] = np.float32(-0.1)
    x[3, 0, :] = np.nan                              # NaN in the middle
    x[:, 1, :] = np.nan                              # every period NaN
    x[0, 3, 1] = np.float32(-0.75)                   # fallen at period 0 (by pitch)
    x[2, 4, 0] = np.float32(-0.5)                    # exactly tilt_max
    x[4, 4, 5] = np.float32(0.25)                    # exactly z_min
    x[4:, 5, 5] = np.float32(0.2)                    # falls by height at period 4
    return x, 0.5, 0.25


def test_fall_outcome_matches_its_restatement():
    from tests.emu import emu_plant_body
    x, tilt_max, z_min = _hand_made_states()
    first, mt, mz = emu_plant_body.outcome(x, tilt_max, z_min)
    rf, rt, rz = bc.outcome(x, tilt_max, z_min)
    assert first.dtype == np.int32 and mt.dtype == np.float32 and mz.dtype == np.float32
    assert np.array_equal(first, rf) and np.array_equal(mt, rt, equal_nan=True) and np.array_equal(mz, rz, equal_nan=True)
    assert list(first) == [3, 0, -1, 0, -1, 4]       # the cases are what they say
    assert np.isnan(mt[1]) and np.isnan(mz[1]) and not np.isnan(mt[0]) and mt[0] == np.float32(0.3) and mz[0] == np.float32(0.5)
    assert mt[4] == np.float32(0.5) and mz[4] == np.float32(0.25) and mz[5] == np.float32(0.2)
    # a threshold switched off by an infinity
    first, _, _ = emu_plant_body.outcome(x, np.inf, -np.inf)
    assert list(first) == [3, 0, -1, -1, -1, -1] and np.array_equal(first, bc.outcome(x, np.inf, -np.inf)[0])
    # no period at all
    first, mt, mz = emu_plant_body.outcome(x[:0], tilt_max, z_min)
    assert (first == -1).all() and np.isnan(mt).all() and np.isnan(mz).all()


def test_fall_thresholds_are_compared_in_fp64():
    """Thresholds that are no fp32 value, strictly between a stored state and its fp32 neighbour: the stored fp32 state is widened,
    the threshold is not rounded.  float32(0.3) lies above the fp64 0.3, and z_min lies a quarter of an fp32 ulp above the stored
    height: a comparison in fp32 would round both thresholds onto the states and call instance 0 upright."""
    from tests.emu import emu_plant_body
    x = np.zeros((2, 2, 12), np.float32)
    x[:, :, 5] = np.float32(0.4)
    x[1, 0, 0] = np.float32(0.3)                     # instance 0 exceeds tilt_max = 0.3 (fp64) by 1.2e-8 at period 1 only
    assert float(np.float32(0.3)) > 0.3 and np.float32(0.3) == np.float32(0.3 + 0.0)
    first, _, _ = emu_plant_body.outcome(x, 0.3, 0.0)
    assert list(first) == [1, -1] and np.array_equal(first, bc.outcome(x, 0.3, 0.0)[0])
    z = float(np.float32(0.4))
    z_min = z + 0.25 * float(np.spacing(np.float32(0.4)))
    assert np.float32(z_min) == np.float32(0.4) and z_min > z
    first, _, _ = emu_plant_body.outcome(x, 1.0, z_min)
    assert list(first) == [0, 0] and np.array_equal(first, bc.outcome(x, 1.0, z_min)[0])
    first, _, _ = emu_plant_body.outcome(x, 1.0, z)     # exactly the stored height: upright
    assert list(first) == [-1, -1]


def test_new_symbols_are_exported_and_declared(cparams):
    from biped_mpc_py_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(util.ROOT, "include", "bmpc.h")).read()
    for name in ("bmpc_plant_step_body", "bmpc_plant_step_body_device", "bmpc_simulate_body_device"):
        assert name in _lib.EXPORTS and hasattr(raw, name) and ("int " + name + "(") in header
        assert getattr(_lib.load(), name).argtypes is not None
    assert _lib.load().bmpc_abi_version() == 13


def test_body_struct_layouts_match_c(cparams):
    from biped_mpc_py_amd import _lib
    src = ('#include <stdio.h>\n#include "bmpc.h"\nint main(){printf("%zu %zu", sizeof(bmpc_plant_body), sizeof(bmpc_sim_outcome));'
           'return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert sizes == [C.sizeof(_lib.CPlantBody), C.sizeof(_lib.CSimOutcome)] == [24, 40]


def test_body_argument_validation(cparams):
    """What returns before a device is needed, in order: the plant block and a NaN threshold, then the handle."""
    from biped_mpc_py_amd import _lib
    lib = _lib.load()
    body = _lib.CPlantBody()

    def calls(p, outcome=None):
        ref = None if p is None else C.byref(p)
        return (lib.bmpc_plant_step_body(None, 4, ref, C.byref(body), None, None, None, None, None, None),
                lib.bmpc_plant_step_body_device(None, 4, ref, C.byref(body), None, None, None, None, None, None, None),
                lib.bmpc_simulate_body_device(None, 4, 3, ref, C.byref(body), None, None, None, None, None, None, None, None, None, None,
                                              None, None, outcome, None))

    for field, value, word in (("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"), ("integrator", 2, b"integrator"),
                               ("push_from", -1, b"push")):
        bad = _lib.CPlant(1, 4, 1, 0, 0)
        setattr(bad, field, value)
        for rc in calls(bad):
            assert rc == -1 and word in lib.bmpc_last_error(), (field, value, lib.bmpc_last_error())
    for tilt_max, z_min in ((np.nan, 0.3), (0.5, np.nan)):
        out = _lib.CSimOutcome(tilt_max, z_min, None, None, None)
        assert calls(None, C.byref(out))[2] == -1 and b"NaN" in lib.bmpc_last_error()
    # bad plant options come before a NaN threshold, a good block and good thresholds reach the handle
    assert calls(_lib.CPlant(1, 0, 1, 0, 0), C.byref(_lib.CSimOutcome(np.nan, 0.3, None, None, None)))[2] == -1
    assert b"substeps" in lib.bmpc_last_error()
    for out in (None, C.byref(_lib.CSimOutcome(np.inf, -np.inf, None, None, None))):
        for rc in calls(None, out):
            assert rc == -1 and b"null handle" in lib.bmpc_last_error()


def test_python_body_and_fall_are_checked_before_any_call():
    import biped_mpc_py_amd as bm
    s = object.__new__(bm.BatchSolver)                 # no handle: the checks come first
    z, f, c = np.zeros((3, 12)), np.zeros((3, 6)), np.ones((3, 2))
    for body in ({"m": np.ones(4)}, {"m": np.ones(3, np.float32)}, {"I": np.ones((3, 3, 2))}, {"I": np.ones((3, 8))},
                 {"g": np.ones((3, 1))}, {"mass": np.ones(3)}, [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            s.plant_step(z, z, f, c, body=body)
    for fall in ((np.nan, 0.3), (0.5, np.nan), 0.5, (0.5,), (0.5, 0.3, 0.1), ("a", "b")):
        with pytest.raises(ValueError):
            s.simulate_device(None, None, None, 3, fall=fall)
