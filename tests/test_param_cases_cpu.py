"""CPU: the parameter cases of tests/param_cases.py without a GPU.
  0. the extended yardsticks leave every existing group as it was (parameter blocks byte-equal);
  1. SENSITIVITY of every (case, entry) pair the GPU tests rely on, from the REFERENCE alone: a test that passes when the kernel
     ignores the parameter proves nothing, so the reference at the case and at the defaults, on the test's own inputs, must differ
     by at least 100 x the bound the GPU test applies on at least half of the instances;
  3. evaluate / evaluate_grad / certify: two instances per case and group through the kernels' sources on the CPU (tests/emu);
  4. the plant's per-instance function on the CPU at every plant case, and its angular momentum at a non-diagonal inertia;
  and that the gait and the start times of the closed-loop runs let both legs land."""
import functools
import os
import shutil

import numpy as np
import pytest

from tests import certify_cases as cc
from tests import eval_cases as ec
from tests import eval_grad_cases as gc
from tests import param_cases as pc
from tests import plant_model as pm
from tests import util


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


# ---- 0. the table, and the yardsticks that take it ----------------------------------------------------------------------------------

def test_the_table_takes_the_existing_cases_over_unchanged_and_every_struck_pair_has_its_reason():
    for table in (util.PARAM_CASES, util.WEIGHT_CASES):
        for k, v in table.items():
            assert pc.CASES[k] is v
    for name in ("kp_full", "kd_full", "hip_offset", "swingHeight_0.05", "h16", "xcmd_xy", "combined"):
        assert name in pc.LOWLEVEL_CASES
    assert not np.allclose(pc.KP_FULL, pc.KP_FULL.T) and not np.allclose(pc.KD_FULL, pc.KD_FULL.T)
    for entry, names in pc.ENTRIES.items():
        assert names and all(n in pc.CASES for n in names), entry
    for (entry, name), why in pc.STRUCK.items():
        assert entry in pc.ENTRIES and name in pc.CASES and name not in pc.ENTRIES[entry] and len(why) > 20


def test_a_case_applies_to_the_package_and_to_the_oracle_alike(built):
    import biped_mpc_py_amd as bm
    from oracle import bmpc_oracle as orc
    fields_m = ("h", "dt", "x_cmd", "Q", "R", "kv", "kp", "kd", "swingHeight")
    fields_b = ("m", "I", "lt", "lh", "g", "hip_offset", "mu", "f_max", "f_min", "tau_max", "tau_min")
    for name in pc.CASES:
        (ma, ba), (mb, bb) = pc.objects(bm, name, h=12), pc.objects(orc, name, h=12)
        for f in fields_m:
            assert np.array_equal(np.asarray(getattr(ma, f), float), np.asarray(getattr(mb, f), float)), (name, f)
        for f in fields_b:
            assert np.array_equal(np.asarray(getattr(ba, f), float), np.asarray(getattr(bb, f), float)), (name, f)
    m, b = pc.objects(orc, "combined")
    assert (m.dt, b.m, b.g) == (0.05, 20.0, 3.7) and b.I[0, 1] != 0
    assert pc.objects(orc, "h16", h=10)[0].h == 16 and tuple(pc.objects(orc, "xcmd_xy")[0].x_cmd[3:5]) == pc.XCMD_XY


def _cparams_before(g, path=0):
    """`eval_cases.cparams_of` as it was before it took modifications."""
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = g["h"]
    b = bm.Biped()
    for k in ("f_max", "f_min", "tau_max", "tau_min"):
        setattr(b, k, np.asarray(getattr(g["biped"], k), float).reshape(-1))
    return bm.pack_params(mpc, b, half=g["half"], solver_options=dict(path=path) if path else None)


def test_existing_groups_keep_their_parameter_blocks_and_yardsticks(built):
    from biped_mpc_py_amd.params import params_key
    groups = ec.ref_tracking_groups() + ec.ref_tracking_groups(breaking=True) + ec.generated_groups() + ec.horizon_groups() \
        + cc.optimum_groups() + [ec.bad_batch()[0], gc.batch_group(10)[0]]
    assert len(groups) >= 40
    for g in groups:
        assert "mods" not in g
        for path in (0, 2):
            assert params_key(ec.cparams_of(g, path)) == params_key(_cparams_before(g, path)), g["name"]
    # no modification: the yardstick takes the module constant and the group's own Biped object, as before; the defaults THROUGH
    # the modification path (dt from the MPC object, a copy of the Biped) give the same bits
    g = ec.generated_groups()[3]
    mpc, biped, dt = ec.oracle_objects(g, 0)
    assert biped is g["biped"] and dt is ec.DT
    a, b = ec.yardstick(g, 0), ec.yardstick(g, 0, pc.DEFAULT_MODS)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    a, b = gc.yardstick(g, 0), gc.yardstick(g, 0, pc.DEFAULT_MODS)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(cc.condensed(g, 0)[:4], cc.condensed(g, 0, pc.DEFAULT_MODS)[:4]):
        assert np.array_equal(x, y)


def test_a_modified_group_maps_to_the_block_of_its_case(built):
    from biped_mpc_py_amd.params import params_key
    for name in pc.SOLVE_CASES:
        g = pc.eval_group(10, name)
        want = util.case_params(pc.CASES[name], 10, 2)
        want.half = g["half"]
        assert params_key(ec.cparams_of(g, 2)) == params_key(want), name


def test_modifications_are_checked(built):
    """A case that changes the horizon cannot be an evaluation group's (its arrays have the group's h): refused by the yardsticks
    before anything is computed; an unknown case name is a KeyError; `mods` given explicitly wins over the group's own."""
    g = pc.eval_group(10, "m_20")
    for fn in (ec.yardstick, gc.yardstick, cc.condensed):
        with pytest.raises(AssertionError, match="horizon"):
            fn(g, 0, pc.mods("h16"))
    from oracle import bmpc_oracle as orc
    with pytest.raises(KeyError):
        pc.objects(orc, "m_21")
    assert ec.oracle_objects(g, 0)[1].m == 20.0 and ec.oracle_objects(g, 0, pc.DEFAULT_MODS)[1].m == 12
    assert ec.cparams_of(g).m == 20.0 and ec.cparams_of(g, mods=pc.DEFAULT_MODS).m == 12.0
    assert g["biped"].m == 12                             # (the group's own Biped is copied, never changed)


# ---- 1. sensitivity, from the reference alone ---------------------------------------------------------------------------------------

def _enough(dev, bound, where):
    """At least half of the instances differ by at least SENSITIVITY x bound."""
    dev = np.asarray(dev, float)
    n = int((dev >= pc.SENSITIVITY * bound).sum())
    print("sensitivity %-44s %3d of %3d instances >= %.1e (median %.2e)" % (where, n, dev.size, pc.SENSITIVITY * bound, np.median(dev)))
    assert 2 * n >= dev.size, (where, n, dev.size)


@pytest.fixture(scope="module")
def stage_fixture():
    return util.load("param_cases_stage")


@pytest.mark.parametrize("h", pc.STAGE_HORIZONS)
def test_sensitivity_of_the_solve(stage_fixture, h):
    """The oracle's optimum at the case against its optimum at the defaults, in the metric and against the bound of the GPU test
    (util.rel_err, util.REL_TOL).  The optima are the fixture's; the fixture belongs to today's inputs, and two of its solves are made
    again here."""
    f = stage_fixture
    s = pc.stage_batch(h)
    assert np.array_equal(f[f"h{h}/x_fb"], s["x_fb"])
    assert f[f"h{h}/kkt"].max() <= 1e-7                   # every instance of every case converged (tests/gen_param_cases.py)
    for name in pc.ENTRIES["solve_stage"]:
        _enough(util.rel_err(f[f"h{h}/{name}"], f[f"h{h}/default"]), util.REL_TOL, f"solve_stage h={h} {name}")
    if h <= 10:
        for name, i in (("I_nondiagonal", 1), ("kv_0.05", 6)):
            _, ct, info = pc.oracle_solve(s, i, h, name, return_info=True)
            assert info["polished"] and max(info["kkt"].values()) <= 1e-7
            assert np.abs(ct - f[f"h{h}/{name}"][i]).max() <= 1e-7 * max(1.0, np.abs(ct).max()), (name, i)


@functools.lru_cache(maxsize=None)
def _eval_refs_of(kind, name, h, default):
    g = pc.eval_group(h, name)
    if default:
        g = dict(g, mods=pc.DEFAULT_MODS)
    idx = pc.eval_indices(h)
    if kind == "evaluate":
        return ec.yardstick_group(g, idx)
    if kind == "evaluate_grad":
        return gc.yardstick_group(g, idx)
    return pc.certify_yardstick(g, idx)


_first_with_inputs = {}


def _eval_refs(kind, name, h, default):
    """The yardstick of `kind` for the checked instances of the group of case `name` at horizon h -- at the case, or (default) at the
    default parameters on the same inputs; cases that share their inputs share that one.  certify: (arrays, act_tol)."""
    if default:
        name = _first_with_inputs.setdefault(pc.eval_inputs_key(name), name)
    return _eval_refs_of(kind, name, h, default)


def _eval_deviation(kind, a, b):
    """Per instance: the largest of the entry's error metrics between two yardsticks."""
    if kind == "evaluate":
        return np.max(list(ec.metrics(a, b).values()), 0)
    if kind == "evaluate_grad":
        return np.max(list(gc.metrics(a, b).values()), 0)
    d = cc.deviations(a[0], dict(b[0], indep=a[0]["indep"] & b[0]["indep"]))
    return np.max([d[k] for k in ("resid", "stationarity", "primal_ineq", "grad_scale")], 0)


@pytest.mark.parametrize("kind", ["evaluate", "evaluate_grad", "certify"])
def test_sensitivity_of_the_evaluation_family(kind):
    """At every horizon of the GPU test (h = 10 serves both kernel families' handles).  The bound of the GPU tests is util.REL_TOL
    in the entry's own metrics.  The struck pairs of the gradient give the same bits at the case and at the defaults."""
    for h in sorted({h for h, _ in pc.EVAL_GROUPS}):
        for name in pc.ENTRIES[kind]:
            dev = _eval_deviation(kind, _eval_refs(kind, name, h, False), _eval_refs(kind, name, h, True))
            _enough(dev, util.REL_TOL, f"{kind} h={h} {name}")
    for (entry, name), _ in pc.STRUCK.items():
        if entry == kind == "evaluate_grad":
            a, b = _eval_refs(kind, name, 10, False), _eval_refs(kind, name, 10, True)
            assert all(np.array_equal(a[k], b[k]) for k in gc.KEYS), name


def _plant_runs():
    return [(i, n, w) for i in ("euler", "rk4") for n in (1, 4) for w in (True, False)]


def test_sensitivity_of_the_plant_step():
    """plant_model.step_batch at the case against the defaults; the GPU test's bound is 2 fp32 ulps (+ 1e-12)."""
    x, u, foot, c, w = pm.batch(67)
    for name in pc.ENTRIES["plant_step"]:
        kw = pc.plant_kw(name)
        for integrator, n, wr in _plant_runs():
            a = pm.step_batch(x, u, foot, c, w if wr else None, integrator=integrator, substeps=n, **kw)
            b = pm.step_batch(x, u, foot, c, w if wr else None, integrator=integrator, substeps=n)
            _enough(pm.ulp_diff(a.astype(np.float32), b).max(1), 2.0, f"plant_step {name} {integrator} {n} {'wrench' if wr else ''}")
    for (entry, name), why in pc.STRUCK.items():
        if entry == "plant_step":
            assert name == "kv_0.05"                      # (step_batch has no kv argument to vary: the model does not read it)


def test_sensitivity_of_the_low_level_kernels():
    """orc.getFootPositionWorld / orc.lowLevelControl at the case against the defaults on the case's own inputs; bounds 2e-6 and
    2e-5 max(1, max|tau|) as the GPU test applies them."""
    for name in pc.ENTRIES["foot_position_world"]:
        d = pc.lowlevel_batch(name)
        _enough(np.abs(pc.lowlevel_fk_ref(name, d) - pc.lowlevel_fk_ref("default", d)).max(1), pc.FK_TOL, f"foot_position_world {name}")
    for name in pc.ENTRIES["low_level_control"]:
        d = pc.lowlevel_batch(name)
        pf = pc.lowlevel_fk_ref(name, d)
        a, b = pc.lowlevel_tau_ref(name, d, pf), pc.lowlevel_tau_ref("default", d, pf)
        _enough(np.abs(a - b).max(1) / np.maximum(1.0, np.abs(a).max(1)), pc.TAU_TOL, f"low_level_control {name}")
    # the struck pairs really change nothing in the reference
    d = pc.lowlevel_batch("default")
    pf = pc.lowlevel_fk_ref("default", d)
    for (entry, name), _ in pc.STRUCK.items():
        if entry == "foot_position_world":
            assert np.array_equal(pc.lowlevel_fk_ref(name, d), pf), name
        if entry == "low_level_control":
            assert np.array_equal(pc.lowlevel_tau_ref(name, d, pf), pc.lowlevel_tau_ref("default", d, pf)), name


def test_the_low_level_batch_covers_negative_times_period_multiples_and_every_contact_pattern():
    for name in ("default", "h16", "combined"):
        d = pc.lowlevel_batch(name)
        Ts = d["Ts"]
        assert (d["t"] < 0).sum() >= 50 and d["t"].min() >= -8 * Ts - 1e-12 and d["t"].max() <= max(3.0, 15 * Ts)
        assert np.array_equal(d["t"][:24], np.arange(-8, 16) * Ts)
        for pat in ((1, 1), (1, 0), (0, 1), (0, 0)):
            sel = (d["contact0"] == pat).all(1)
            assert sel.sum() >= 60 and (d["t"][sel] < 0).any() and sel[:24].sum() >= 4
        assert np.abs(d["x_fb"][:, :3]).max() > 0.55


# ---- 3. evaluate / evaluate_grad / certify through the emulation ---------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_evaluation_family_in_the_emulation(built, name):
    """Two instances per case and group through the kernels' sources on the CPU, against the yardsticks at the case: a wrong mapping
    of a parameter fails here, without a GPU."""
    from tests.emu import emu_eval
    idx = list(pc.EMU_INSTANCES)
    for h, path in pc.EVAL_GROUPS:
        g = pc.eval_group(h, name)
        cp, a = ec.cparams_of(g, path), ec.kernel_args(g, idx)
        where = f"{g['name']}/path{path}"
        ec.check(emu_eval.evaluate(cp, **a), ec.yardstick_group(g, idx), where, reg_bound=pc.PARAM_REG_BOUND)
        gc.check(emu_eval.evaluate_grad(cp, **a), gc.yardstick_group(g, idx), where, reg_bound=pc.PARAM_GRAD_REG_BOUND)
        ref, tol = pc.certify_yardstick(g, idx)
        cc.check(emu_eval.certify(cp, **a, act_tol=tol), ref, where, bound=pc.PARAM_CERT_REL_BOUND)


# ---- 4. the plant ----------------------------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("name", pc.PLANT_CASES)
def test_plant_emulation_matches_the_model_at_the_case(built, name):
    """B = 67; Euler and RK4, 1 and 4 substeps, with and without a wrench, against plant_model.step_batch at the case's I_b, m, g
    and dt.  The bound is test_plant_cpu's derived 2 fp32 ulps + 1e-12: both sides compute in fp64 at any of these parameters."""
    from tests.emu import emu_plant
    cp = util.case_params(pc.CASES[name], 10, 0)
    x, u, foot, c, w = pm.batch(67)
    for integrator, n, wr in _plant_runs():
        got = emu_plant.plant_step(cp, x, u, foot, c, w if wr else None, integrator, n)
        ref = pm.step_batch(x, u, foot, c, w if wr else None, integrator=integrator, substeps=n, **pc.plant_kw(name))
        d = pm.ulp_diff(got, ref)
        print(name, integrator, n, "wrench" if wr else "none", "max ulps", d.max())
        assert np.isfinite(ref).all() and d.max() <= 2.0, (integrator, n, wr, d.max())


@needs_emu
def test_emulated_plant_keeps_the_world_angular_momentum_of_the_model_at_a_non_diagonal_inertia(built):
    """The twin of test_model_conserves_momentum_and_energy_at_fourth_order on the emulated KERNEL function at I_nondiagonal: free
    flight (c = (0, 0), no wrench) at a body rate of 9 rad/s, where the gyroscopic term w x I_w w is what turns the body.  Free
    flight has to go period by period through fp32 I/O, whose rounding swamps a drift ratio, so ONE period is asserted: the world
    angular momentum L = R I_b R' w of the emulation's state against that of the model's state, within what 2 fp32 ulps of each of
    the six entries L depends on (e, w) can move it -- sum_i |dL/dx_i| 2 ulp(x_i), the module's bound carried through L -- and the
    model itself keeps L over that period to 1e-6 relative (RK4, 4 substeps), so an L that is held is the right one."""
    from tests.emu import emu_plant
    name = "I_nondiagonal"
    kw = pc.plant_kw(name)
    Ib = kw["I_b"]
    cp = util.case_params(pc.CASES[name], 10, 0)
    rng = np.random.default_rng(4)
    x0 = np.array([[0.2, -0.3, 0.4, 0.1, -0.2, 0.5, 6.0, -5.0, 4.0, 0.3, -0.1, 0.2]] * 9)
    x0[1:, 0:3] += rng.uniform(-0.3, 0.3, (8, 3))
    x0[1:, 6:9] *= rng.uniform(0.5, 1.2, (8, 3))
    x0 = x0.astype(np.float32)
    u, foot = np.full((9, 12), 50.0, np.float32), np.tile(np.array([0.1, 0.1, 0, 0.1, -0.1, 0.0], np.float32), (9, 1))
    c = np.zeros((9, 2), np.uint8)
    got = emu_plant.plant_step(cp, x0, u, foot, c, None, "rk4", 4).astype(np.float64)
    ref = pm.step_batch(x0, u, foot, c, None, integrator="rk4", substeps=4, **kw)

    def L(x):
        R = pm.rot(x[0:3])
        return R @ Ib @ R.T @ x[6:9]

    for b in range(9):
        L0, Lg, Lr = L(x0[b].astype(np.float64)), L(got[b]), L(ref[b])
        assert np.abs(Lr - L0).max() <= 1e-6 * np.abs(L0).max()
        J = np.zeros((3, 12))
        for i in (0, 1, 2, 6, 7, 8):
            e = np.zeros(12)
            e[i] = 1e-6
            J[:, i] = (L(ref[b] + e) - L(ref[b] - e)) / 2e-6
        ulp = np.spacing(np.abs(ref[b]).astype(np.float32)).astype(np.float64)
        bound = np.abs(J) @ (2.0 * ulp) + 1e-12
        print("instance", b, "L", Lr, "deviation", np.abs(Lg - Lr), "bound", bound)
        assert (np.abs(Lg - Lr) <= bound).all(), (b, np.abs(Lg - Lr), bound)
        # and the bound is sharp enough to see the default inertia in I_b^-1's place, or a slip of an index in w x I_w w:
        assert np.abs(L(pm.step(x0[b], u[b], foot[b], (0, 0), None, "rk4", 4)) - Lr).max() > 1e3 * bound.max()


def test_the_closed_loop_runs_let_both_legs_land():
    """For every instance of both runs the gait and the start time give each leg a landing (swing at step k, stance at k + 1) within
    the 12 periods, whatever the states do."""
    from oracle import bmpc_oracle as orc
    for run, r in pc.CLOSED_LOOP_RUNS.items():
        mpc, _ = pc.objects(orc, r["case"], h=r["h"])
        x0, foot, t0, x_cmd = pc.closed_loop_start(run)
        period, offset, duty = r["gait"]
        assert x0.shape[0] == pc.CLOSED_LOOP_B == 33 and (x_cmd[:, 3:5] != 0).all()
        for b in range(x0.shape[0]):
            t = float(t0[b])
            lands = np.zeros(2, int)
            for _ in range(pc.CLOSED_LOOP_K):
                k0, k1 = orc.phase_index(t, mpc), orc.phase_index(t + mpc.dt, mpc)
                for leg in range(2):
                    lands[leg] += (not pm.stance(k0, offset[leg], period, duty[leg])) and pm.stance(k1, offset[leg], period, duty[leg])
                t += mpc.dt
            assert (lands >= 1).all(), (run, b, lands)
