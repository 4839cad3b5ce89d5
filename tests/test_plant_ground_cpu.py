"""CPU: the ground under the plant (csrc/bmpc_plant.hip: plant_ground, plant_step_ground, plant_ground_reduce) without a GPU -- the
per-instance functions run as plain C++ (tests/emu/emu_plant_ground.py) against the NumPy restatement of the rule
(tests/ground_cases.py) and of the plant (tests/plant_model.py), the exact cases of the rule, bad grounds, the reductions against
their restatement, and the C ABI and the Python keywords of the new entries.

Bounds.  What the ground does not scale is a copy or +0: equal to the bit.  A scaled entry is fx (lim / t) rounded to fp32 once;
the emulation is built without contraction and is expected to agree exactly, but the bound is the 1 fp32 ulp that a contracted
fx fx + fy fy may cost (tests/ground_cases.py assert_applied).  The next state is held to the plant's existing 2-ulp bound against
the model at u_applied (tests/test_plant_cpu.py: both sides compute in fp64, only the final rounding can differ)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import body_cases as bc
from tests import ground_cases as gc
from tests import plant_model as pm
from tests import util

B = 33


@pytest.fixture(scope="module")
def cparams():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    cp = _lib.CParams()
    assert _lib.load().bmpc_default_params(cp, 10) == 0
    return cp


def test_the_shared_controls_hold_every_kind_of_leg():
    """The model alone: swing, unloaded, holding, slipping legs and a leg on a mu of +inf all occur at the batch sizes the tests use,
    no loaded leg sits within 1e-6 of its cone (asserted inside controls()), and swing legs carry controls that are not zero."""
    for n in (33, 67, 257):
        mu = gc.grounds(n)
        u, c = gc.controls(n)
        assert ((mu >= 0.05) & (mu <= 1.0) | np.isinf(mu)).all() and np.isinf(mu).any(1).sum() == len(range(0, n, 8))
        ua, flags, demand, scaled = gc.transmit(u, c, mu)
        for bit in (1, 2, 4, 8):
            assert (flags & bit).any() and not (flags & bit).all(), (n, bit)
        assert (c == 0).any() and (np.abs(u[:, 0:3][c[:, 0] == 0]) > 0).all()
        holding = (c[:, 0] != 0) & (u[:, 2] > 0) & (flags & 1 == 0)
        assert holding.any() and np.isfinite(demand).any() and np.isnan(demand).any()
        assert scaled.any() and (ua[:, [2, 5]][(c != 0) & (u[:, [2, 5]] > 0)] > 0).all()


@pytest.mark.parametrize("given", ["mu", "handle"])
def test_emulated_ground_matches_the_rule(given):
    from tests.emu import emu_plant_ground as eg
    u, c = gc.controls(B)
    mu = gc.grounds(B) if given == "mu" else None
    for fz_floor in (0.0, 60.0):
        ua, flags, demand, ok = eg.ground(u, c, mu, mu_h=0.5, fz_floor=fz_floor)
        ref_ua, ref_flags, ref_demand, scaled = gc.transmit(u, c, np.full((B, 2), 0.5) if mu is None else mu, fz_floor)
        worst = gc.assert_applied(ua, flags, ref_ua, ref_flags, scaled, given)
        print(given, "fz_floor", fz_floor, "scaled entries", scaled.sum(), "max ulps", worst)
        assert ok.all() and scaled.sum() >= B // 2
        assert np.array_equal(demand, ref_demand, equal_nan=True)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("with_body", [False, True], ids=["handle_body", "bodies"])
def test_emulated_ground_step_is_the_model_at_u_applied(cparams, integrator, with_body):
    from tests.emu import emu_plant_body, emu_plant_ground as eg
    x, _, foot, _, w = pm.batch(B)
    u, c = gc.controls(B)
    mu = gc.grounds(B)
    body = bc.bodies(B) if with_body else {}
    got, ua, flags, ok = eg.plant_step(cparams, x, u, foot, c, w, integrator, 4, body=body, mu=mu)
    ref_ua, ref_flags, _, scaled = gc.transmit(u, c, mu)
    gc.assert_applied(ua, flags, ref_ua, ref_flags, scaled)
    ref = bc.step_batch(x, ua, foot, c, w, body=body, integrator=integrator, substeps=4)
    d = pm.ulp_diff(got, ref)
    print("max ulps", d.max())
    assert ok.all() and np.isfinite(ref).all() and d.max() <= 2.0, d.max()
    # a ground step is exactly the body step at u_applied
    plain, _ = emu_plant_body.plant_step(cparams, x, ua, foot, c, w, integrator, 4, body=body)
    assert np.array_equal(got, plain)
    # and the ground shows: the body step at the command differs on the instances with a flag
    cmd, _ = emu_plant_body.plant_step(cparams, x, u, foot, c, w, integrator, 4, body=body)
    assert (np.abs(cmd - got).max(1)[flags != 0] > 0).all() and np.array_equal(cmd[flags == 0], got[flags == 0])


def _one(f, m=(0.5, -0.25, 2.0), c=1, mu=0.5, fz_floor=0.0):
    """Leg 0 with force f and moment m under contact bit c and friction mu; leg 1 in swing with controls that are not zero."""
    from tests.emu import emu_plant_ground as eg
    u = np.array([[*f, 7.0, -8.0, 9.0, *m, 1.0, 2.0, 3.0]], np.float32)
    ua, flags, demand, ok = eg.ground(u, [[c, 0]], [[mu, 0.3]], fz_floor=fz_floor)
    ref = gc.transmit(u, [[c, 0]], [[mu, 0.3]], fz_floor)
    assert np.array_equal(ua.view(np.uint32), ref[0].view(np.uint32)) and flags[0] == ref[1][0] and ok[0]
    assert np.array_equal(demand, ref[2], equal_nan=True)
    swing = [3, 4, 5, 9, 10, 11]
    assert not ua[0, swing].any() and not np.signbit(ua[0, swing]).any()                  # the swing leg: six +0
    return ua[0], int(flags[0]), float(demand[0]), u[0]


def test_exact_cases_of_the_rule():
    # a tie holds: t = lim = 5 exactly, the controls pass with their bits
    ua, flags, demand, u = _one((3.0, 4.0, 10.0), mu=0.5)
    assert flags == 0 and np.array_equal(ua[[0, 1, 2, 6, 7, 8]], u[[0, 1, 2, 6, 7, 8]]) and demand == 0.5
    # half the friction: scaled onto the cone, exactly
    ua, flags, demand, u = _one((3.0, 4.0, 10.0), mu=0.25)
    assert flags == 1 and list(ua[0:3]) == [1.5, 2.0, 10.0] and np.array_equal(ua[6:9], u[6:9]) and demand == 0.5
    # the ground cannot pull, and passes no moment without load
    for fz in (0.0, -0.0, -10.0):
        ua, flags, demand, _ = _one((3.0, 4.0, fz))
        assert flags == 4 and not ua.any() and not np.signbit(ua).any() and np.isnan(demand)
    # no friction limit
    ua, flags, demand, u = _one((3000.0, -4000.0, 1.0), mu=np.inf)
    assert flags == 0 and np.array_equal(ua[[0, 1, 2, 6, 7, 8]], u[[0, 1, 2, 6, 7, 8]]) and demand == 5000.0
    # ice: fz and the moments only
    ua, flags, demand, u = _one((3.0, 4.0, 10.0), mu=0.0)
    assert flags == 1 and not ua[0:2].any() and ua[2] == 10.0 and np.array_equal(ua[6:9], u[6:9])
    ua, flags, _, u = _one((0.0, 0.0, 10.0), mu=0.0)                     # ... and nothing to scale: t = lim = 0 holds
    assert flags == 0 and ua[2] == 10.0
    # a swing leg is ignored, whatever it asks for: no flag, no demand
    ua, flags, demand, _ = _one((300.0, 400.0, -10.0), c=0)
    assert flags == 0 and not ua.any() and np.isnan(demand)


def test_fz_floor_keeps_a_light_leg_out_of_the_demand_but_not_out_of_the_flags():
    from tests.emu import emu_plant_ground as eg
    # leg 0 light (fz 2) and slipping badly, leg 1 heavy (fz 100) and holding at t / fz = 0.05
    u = np.array([[3.0, 4.0, 2.0, 3.0, 4.0, 100.0, 0, 0, 0, 0, 0, 0]], np.float32)
    for floor, want in ((0.0, 2.5), (2.0, 2.5), (2.5, 0.05), (100.0, 0.05), (101.0, np.nan)):
        ua, flags, demand, ok = eg.ground(u, [[1, 1]], [[0.5, 0.5]], fz_floor=floor)
        assert flags[0] == 1 and ok[0] and list(ua[0, 0:3]) == [np.float32(0.6), np.float32(0.8), 2.0]
        assert np.array_equal(demand, np.array([want], np.float32), equal_nan=True), (floor, demand)
        assert np.array_equal(demand, gc.transmit(u, [[1, 1]], [[0.5, 0.5]], floor)[2], equal_nan=True)


BAD = {"mu_nan": ("mu", np.nan), "mu_negative": ("mu", -1.0), "mu_nan_swing_leg": ("mu_swing", np.nan), "control_nan": ("u", np.nan),
       "control_inf_swing_leg": ("u_swing", np.inf)}


@pytest.mark.parametrize("case", list(BAD))
def test_a_bad_ground_is_all_nan_and_touches_no_neighbour(cparams, case):
    from tests.emu import emu_plant_ground as eg
    x, _, foot, _, w = (a[:5].copy() for a in pm.batch(B))
    u, c = (a[:5].copy() for a in gc.controls(B))
    mu = gc.grounds(B)[:5].copy()
    c[2] = (1, 0)
    clean, cua, cfl, ok = eg.plant_step(cparams, x, u, foot, c, w, mu=mu)
    assert ok.all() and np.isfinite(clean).all()
    what, value = BAD[case]
    if what.startswith("mu"):
        mu[2, 1 if what.endswith("swing") else 0] = value
    else:
        u[2, 4 if what.endswith("swing") else 7] = value
    got, ua, fl, ok = eg.plant_step(cparams, x, u, foot, c, w, mu=mu)
    assert np.isnan(got[2]).all() and np.isnan(ua[2]).all() and fl[2] == 0 and not ok[2] and ok[[0, 1, 3, 4]].all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(got[keep], clean[keep]) and np.array_equal(ua[keep].view(np.uint32), cua[keep].view(np.uint32))
    assert np.array_equal(fl[keep], cfl[keep])
    ref = gc.transmit(u, c, mu)
    assert np.isnan(ref[0][2]).all() and ref[1][2] == 0 and np.isnan(ref[2][2])
    _, _, demand, _ = eg.ground(u, c, mu)
    assert np.isnan(demand[2])


def _hand_made_flags():
    """(steps 6, B 7): never anything; slips at once; slips late on leg 1 only; unloaded throughout on leg 0, never slips; both legs
    slip in different periods; every bit in one period; a demand in a single period."""
    steps, n = 6, 7
    flags, demand = np.zeros((steps, n), np.uint8), np.full((steps, n), np.nan, np.float32)
    demand[:, 0] = np.float32(0.1)
    flags[:, 1] = 1
    demand[:, 1] = np.linspace(0.2, 0.7, steps, dtype=np.float32)[::-1]
    flags[4:, 2] = 2
    demand[2:, 2] = np.float32(0.3)
    flags[:, 3] = 4
    flags[1, 4], flags[3, 4], flags[5, 4] = 2, 1, 3
    demand[1, 4], demand[3, 4] = np.float32(0.9), np.float32(1.25)
    flags[2, 5] = 15
    demand[3, 6] = np.float32(0.05)
    return flags, demand


def test_reductions_match_their_restatement():
    from tests.emu import emu_plant_ground as eg
    flags, demand = _hand_made_flags()
    got, ref = eg.reduce(flags, demand), gc.reduce(flags, demand)
    for a, b, dt in zip(got, ref, (np.int32, np.int32, np.int32, np.float32)):
        assert a.dtype == dt and b.dtype == dt and np.array_equal(a, b, equal_nan=dt is np.float32)
    first, slip, unloaded, mu_demand = got
    assert list(first) == [-1, 0, 4, -1, 1, 2, -1]                    # the cases are what they say
    assert slip.tolist() == [[0, 0], [6, 0], [0, 2], [0, 0], [2, 2], [1, 1], [0, 0]]
    assert unloaded.tolist() == [[0, 0], [0, 0], [0, 0], [6, 0], [0, 0], [1, 1], [0, 0]]
    assert np.array_equal(mu_demand, np.array([0.1, 0.7, 0.3, np.nan, 1.25, np.nan, 0.05], np.float32), equal_nan=True)
    # no period at all: as initialised
    first, slip, unloaded, mu_demand = eg.reduce(flags[:0], demand[:0])
    assert (first == -1).all() and not slip.any() and not unloaded.any() and np.isnan(mu_demand).all()
    for a, b in zip((first, slip, unloaded, mu_demand), gc.reduce(flags[:0], demand[:0])):
        assert np.array_equal(a, b, equal_nan=True)


NEW = ("bmpc_plant_step_ground", "bmpc_plant_step_ground_device", "bmpc_simulate_ground_device")


def test_new_symbols_are_exported_and_declared(cparams):
    from biped_mpc_py_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(util.ROOT, "include", "bmpc.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(raw, name) and ("int " + name + "(") in header
        assert getattr(_lib.load(), name).argtypes is not None
    assert _lib.load().bmpc_abi_version() == 13 and "#define BMPC_ABI_VERSION 13" in header


def test_ground_struct_layouts_match_c(cparams):
    from biped_mpc_py_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(bmpc_plant_ground), '
           'sizeof(bmpc_ground_out), offsetof(bmpc_ground_out, u_applied), offsetof(bmpc_ground_out, mu_demand));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert sizes == [C.sizeof(_lib.CPlantGround), C.sizeof(_lib.CGroundOut), _lib.CGroundOut.u_applied.offset,
                     _lib.CGroundOut.mu_demand.offset] == [8, 56, 8, 48]


def test_ground_argument_validation(cparams):
    """What returns before a device is needed, in the order of the existing entries: the plant block, the outcome thresholds, fz_floor
    and outputs without a ground; then the handle."""
    from biped_mpc_py_amd import _lib
    lib = _lib.load()
    body, ground = _lib.CPlantBody(), _lib.CPlantGround()
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)

    def step_calls(p, gr, ua=None, fl=None):
        ref = None if p is None else C.byref(p)
        return (lib.bmpc_plant_step_ground(None, 4, ref, C.byref(body), gr, None, None, None, None, None, None, ua, fl),
                lib.bmpc_plant_step_ground_device(None, 4, ref, C.byref(body), gr, None, None, None, None, None, None, ua, fl, None))

    def sim_call(p, gr, outcome=None, gout=None):
        return lib.bmpc_simulate_ground_device(None, 4, 3, None if p is None else C.byref(p), C.byref(body), gr, None, None, None, None,
                                               None, None, None, None, None, None, None, None, outcome, gout, None)

    for field, value, word in (("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"), ("integrator", 2, b"integrator"),
                               ("push_from", -1, b"push")):
        bad = _lib.CPlant(1, 4, 1, 0, 0)
        setattr(bad, field, value)
        for rc in step_calls(bad, C.byref(ground)) + (sim_call(bad, C.byref(ground)),):
            assert rc == -1 and word in lib.bmpc_last_error(), (field, value, lib.bmpc_last_error())
    assert sim_call(None, C.byref(ground), C.byref(_lib.CSimOutcome(np.nan, 0.3, None, None, None))) == -1 and b"NaN" in lib.bmpc_last_error()
    for floor in (np.nan, -1.0, -np.inf):
        assert sim_call(None, C.byref(ground), None, C.byref(_lib.CGroundOut(floor))) == -1 and b"fz_floor" in lib.bmpc_last_error()
    # the plant block comes before fz_floor, the outcome thresholds too
    assert sim_call(_lib.CPlant(1, 0, 1, 0, 0), C.byref(ground), None, C.byref(_lib.CGroundOut(np.nan))) == -1
    assert b"substeps" in lib.bmpc_last_error()
    assert sim_call(None, C.byref(ground), C.byref(_lib.CSimOutcome(np.nan, 0.3, None, None, None)), C.byref(_lib.CGroundOut(np.nan))) == -1
    assert b"NaN" in lib.bmpc_last_error() and b"fz_floor" not in lib.bmpc_last_error()
    # outputs without a ground
    for rc in step_calls(None, None, ua=addr) + step_calls(None, None, fl=addr) + (sim_call(None, None, None, C.byref(_lib.CGroundOut(0.0))),):
        assert rc == -1 and b"need a ground" in lib.bmpc_last_error()
    # a good block reaches the handle, with and without a ground
    for gr in (None, C.byref(ground)):
        for rc in step_calls(None, gr) + (sim_call(None, gr),):
            assert rc == -1 and b"null handle" in lib.bmpc_last_error()
    for rc in step_calls(None, C.byref(ground), ua=addr, fl=addr) + (sim_call(None, C.byref(ground), None, C.byref(_lib.CGroundOut(np.inf))),):
        assert rc == -1 and b"null handle" in lib.bmpc_last_error()


def test_python_ground_is_checked_before_any_call():
    import biped_mpc_py_amd as bm
    s = object.__new__(bm.BatchSolver)                 # no handle: the checks come first
    z, f, c = np.zeros((3, 12)), np.zeros((3, 6)), np.ones((3, 2))
    for ground in ({"mu": np.ones((4, 2))}, {"mu": np.ones((3, 2), np.float32)}, {"mu": np.ones(3)}, {"mu": np.ones((3, 3))},
                   {"mu": 0.5}, {"friction": np.ones((3, 2))}, {"mu": np.ones((3, 2)), "g": np.ones(3)}, [0.5, 0.5], 0.5):
        with pytest.raises(ValueError):
            s.plant_step(z, z, f, c, ground=ground)
    with pytest.raises(ValueError):
        s.plant_step(z, z, f, c, want_applied=True)
    for kw in (dict(ground={"friction": 1.0}), dict(ground=0.5), dict(want_applied=True)):
        with pytest.raises(ValueError):
            s.plant_step_device(None, None, None, None, **kw)
    for kw in (dict(ground={"friction": 1.0}), dict(ground=[0.5]), dict(ground={}, fz_floor=np.nan), dict(ground={}, fz_floor=-1.0)):
        with pytest.raises(ValueError):
            s.simulate_device(None, None, None, 3, **kw)
