"""CPU: the plant of the closed-loop simulation (csrc/bmpc_plant.hip) without a GPU -- its per-instance function run as plain C++
(tests/emu/emu_plant.py) against the NumPy restatement of its definition (tests/plant_model.py), the anchor to the controller's
model at zero attitude, the physics of the restatement itself, the NaN rule, the landing rule, and the C ABI of the new entries.

The 2-ulp bound is derived, not measured: both sides compute in fp64, whose error is far below half an fp32 ulp, so only the final
rounding to fp32 can differ, by at most one ulp; the second ulp is margin.  1e-12 absolute covers entries that cancel to zero."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import plant_model as pm
from tests import util

B = 67


@pytest.fixture(scope="module")
def cparams():
    import __graft_entry__ as ge
    ge.build()
    from biped_mpc_py_amd import _lib
    cp = _lib.CParams()
    assert _lib.load().bmpc_default_params(cp, 10) == 0
    return cp


@pytest.fixture(scope="module")
def data():
    return pm.batch(B)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("substeps", [1, 4, 64])
def test_emulation_matches_model(cparams, data, integrator, substeps):
    from tests.emu import emu_plant
    x, u, foot, c, w = data
    got = emu_plant.plant_step(cparams, x, u, foot, c, w, integrator, substeps)
    ref = pm.step_batch(x, u, foot, c, w, integrator=integrator, substeps=substeps)
    d = pm.ulp_diff(got, ref)
    print("max ulps", d.max())
    assert np.isfinite(ref).all() and d.max() <= 2.0, d.max()


def test_euler_step_is_the_controllers_model_at_zero_attitude(cparams):
    """e = 0, w = 0, swing-leg controls exactly zero: Euler with one substep equals A_0 x + B_0 u of REF:165-184 at zero attitude
    (Rot = R_inv = identity, I = I_b), written out here."""
    from tests.emu import emu_plant
    x, u, foot, c, _ = pm.batch(B, seed=11)
    x[:, 0:3] = 0
    x[:, 6:9] = 0
    for g in range(2):
        u[c[:, g] == 0, 3 * g:3 * g + 3] = 0
        u[c[:, g] == 0, 6 + 3 * g:9 + 3 * g] = 0
    got = emu_plant.plant_step(cparams, x, u, foot, c, None, "euler", 1)
    dt, m, grav, Iinv = 0.04, 12.0, 9.81, np.linalg.inv(pm.I_BODY)
    xd, ud, fd = x.astype(np.float64), u.astype(np.float64), foot.astype(np.float64)
    ref = np.empty((B, 12))
    for b in range(B):
        tau = sum(np.cross(fd[b, 3 * g:3 * g + 3] - xd[b, 3:6], ud[b, 3 * g:3 * g + 3]) + ud[b, 6 + 3 * g:9 + 3 * g] for g in range(2))
        ref[b, 0:3] = xd[b, 0:3] + dt * xd[b, 6:9]
        ref[b, 3:6] = xd[b, 3:6] + dt * xd[b, 9:12]
        ref[b, 6:9] = xd[b, 6:9] + dt * (Iinv @ tau)
        ref[b, 9:12] = xd[b, 9:12] + dt * (ud[b, 0:3] + ud[b, 3:6]) / m + dt * np.array([0, 0, -grav])
    assert pm.ulp_diff(got, ref).max() <= 2.0


def test_model_conserves_momentum_and_energy_at_fourth_order():
    """Free flight (c = (0, 0), no wrench) of the MODEL, RK4 with n = 4 and 2n substeps over 10 periods: the drift of the world
    angular momentum I_w w and of the rotational energy falls by at least 8x (fourth order: 16x), and p_z follows the parabola."""
    x0 = np.array([0.2, -0.3, 0.4, 0.1, -0.2, 0.5, 6.0, -5.0, 4.0, 0.3, -0.1, 0.2])
    u, foot = np.full(12, 50.0), np.array([0.1, 0.1, 0, 0.1, -0.1, 0.0])

    def run(n):
        x = x0.copy()
        for _ in range(10):
            x = pm.step(x, u, foot, (0, 0), None, "rk4", n)
        R = pm.rot(x[0:3])
        L = R @ pm.I_BODY @ R.T @ x[6:9]
        return x, L, 0.5 * x[6:9] @ L

    R0 = pm.rot(x0[0:3])
    L0 = R0 @ pm.I_BODY @ R0.T @ x0[6:9]
    E0 = 0.5 * x0[6:9] @ L0
    (xa, La, Ea), (xb, Lb, Eb) = run(4), run(8)
    dL4, dL8, dE4, dE8 = np.abs(La - L0).max(), np.abs(Lb - L0).max(), abs(Ea - E0), abs(Eb - E0)
    print("drift L", dL4, dL8, "E", dE4, dE8)
    assert dL4 > 1e-11 and dE4 > 1e-11                 # well above rounding: the ratios below are not noise
    assert dL4 >= 8 * dL8 and dE4 >= 8 * dE8
    T = 0.4
    for x in (xa, xb):
        assert abs(x[5] - (x0[5] + x0[11] * T - 0.5 * 9.81 * T * T)) <= 8 * np.spacing(1.0)


def test_bad_instances_touch_only_themselves(cparams):
    from tests.emu import emu_plant
    x, u, foot, c, w = (a[:5].copy() for a in pm.batch(B))
    clean = emu_plant.plant_step(cparams, x, u, foot, c, w)
    x[1, 1] = np.float32(np.pi / 2)
    u[3, 2] = np.inf
    got = emu_plant.plant_step(cparams, x, u, foot, c, w)
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    assert np.array_equal(got[[0, 2, 4]], clean[[0, 2, 4]]) and np.isfinite(clean).all()
    ref = pm.step_batch(x, u, foot, c, w)
    assert np.isnan(ref[1]).all() and np.isnan(ref[3]).all()


@pytest.mark.parametrize("gait", [(10, (0, 5), (5, 5)), (7, (2, 5), (4, 3))])
def test_landing_rule_matches_model(cparams, gait):
    """All 20 phases of the default gait (the reference's table has 20 rows), and a custom (period, offset, duty)."""
    from tests.emu import emu_plant
    x, _, foot, _, _ = pm.batch(20, seed=3)
    k0 = np.arange(20)
    cmd = np.zeros((20, 12), np.float32)
    cmd[:, 3:5] = np.random.default_rng(1).uniform(-0.3, 0.3, (20, 2))
    for x_cmd in (None, cmd):
        got, lands = emu_plant.landing(cparams, gait, k0, k0 + 1, x, foot, x_cmd)
        n = 0
        for b in range(20):
            c = (0.0, 0.0) if x_cmd is None else cmd[b, 3:5].astype(np.float64)
            ref, rl = pm.landing(x[b].astype(np.float64), foot[b].astype(np.float64), int(k0[b]), int(k0[b]) + 1, gait[0], gait[1],
                                 gait[2], cmd=c)
            assert list(lands[b]) == rl
            assert pm.ulp_diff(got[b], ref, atol=0.0).max() <= 1.0
            for g in range(2):
                if not rl[g]:
                    assert np.array_equal(got[b, 3 * g:3 * g + 3], foot[b, 3 * g:3 * g + 3])
            n += sum(rl)
        assert n >= 2


def test_plant_struct_layout_matches_c(cparams):
    from biped_mpc_py_amd import _lib
    src = '#include <stdio.h>\n#include "bmpc.h"\nint main(){printf("%zu", sizeof(bmpc_plant));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), c, "-o", exe])
        size = int(subprocess.check_output([exe]).decode())
    assert size == C.sizeof(_lib.CPlant) == 20


def test_plant_argument_validation(cparams):
    """The BMPC_ERR_INVALID cases that return before a device is needed: the plant block is checked first, then the handle."""
    from biped_mpc_py_amd import _lib
    lib = _lib.load()
    pl = _lib.CPlant()
    assert lib.bmpc_plant_default(None) == -1
    assert lib.bmpc_plant_default(C.byref(pl)) == 0
    assert (pl.integrator, pl.substeps, pl.move_feet, pl.push_from, pl.push_steps) == (1, 4, 1, 0, 0)

    def calls(p):
        ref = None if p is None else C.byref(p)
        return (lib.bmpc_plant_step(None, 4, ref, None, None, None, None, None, None),
                lib.bmpc_plant_step_device(None, 4, ref, None, None, None, None, None, None, None),
                lib.bmpc_simulate_device(None, 4, 3, ref, None, None, None, None, None, None, None, None, None, None, None, None, None))

    for field, value, word in (("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"), ("integrator", 2, b"integrator"),
                               ("integrator", -1, b"integrator"), ("push_from", -1, b"push"), ("push_steps", -1, b"push")):
        bad = _lib.CPlant(1, 4, 1, 0, 0)
        setattr(bad, field, value)
        for rc in calls(bad):
            assert rc == -1 and word in lib.bmpc_last_error(), (field, value, lib.bmpc_last_error())
    for p in (None, pl):
        for rc in calls(p):
            assert rc == -1 and b"null handle" in lib.bmpc_last_error()


def test_python_arguments_are_checked_before_any_call():
    import biped_mpc_py_amd as bm
    s = object.__new__(bm.BatchSolver)                 # no handle: the checks come first
    z = np.zeros((3, 12))
    with pytest.raises(ValueError):
        s.plant_step(z, z, np.zeros((3, 6)), np.ones((3, 2)), integrator="heun")
    with pytest.raises(ValueError):
        s.plant_step(z, z, np.zeros((3, 6)), np.ones((3, 2)), substeps=65)
    with pytest.raises(ValueError):
        s.plant_step(np.zeros((3, 11)), z, np.zeros((3, 6)), np.ones((3, 2)))
    with pytest.raises(ValueError):
        s.plant_step(z, z, np.zeros((3, 5)), np.ones((3, 2)))
