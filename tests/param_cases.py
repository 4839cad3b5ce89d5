"""Parameter cases for every kernel (TEST INFRASTRUCTURE): ONE table of parameter blocks away from the reference's defaults, a helper that
applies a case to (bm.MPC, bm.Biped) and to (orc.MPC, orc.Biped) alike, and per entry the list of cases that apply to it.

A case is a pair (change of the MPC object or None, change of the Biped object or None), as in util.PARAM_CASES / util.WEIGHT_CASES,
which are taken over unchanged.  LOWLEVEL_CASES adds what only the low-level kernels and the plant read.

ENTRIES lists, per entry, the cases whose effect the tests of that entry rely on: each (case, entry) pair in it passes the sensitivity
condition of tests/test_param_cases_cpu.py -- the REFERENCE alone, at the case and at the defaults, on the test's own inputs, differs by
at least SENSITIVITY x the bound the GPU test applies, on at least half of the instances.  A pair that cannot pass it because the
entry does not read the parameter is in STRUCK, with the reason: the kernels still run at that case (it must change nothing)."""
import numpy as np

from tests import util

SENSITIVITY = 100.0

# full, NON-symmetric gain matrices: a transposed or mis-strided read shows
KP_FULL = np.array([[500.0, 140.0, -95.0], [-160.0, 450.0, 130.0], [75.0, -115.0, 550.0]])
KD_FULL = np.array([[10.0, 3.5, -2.8], [-4.0, 8.0, 3.2], [1.6, -3.1, 12.0]])
HIP_OFFSET = np.array([0.021, 0.083, -0.071])          # REF:43 is (-0.005, 0.047, -0.126)
XCMD_XY = (0.3, -0.2)


def _xcmd_xy(m):
    x = np.array(m.x_cmd, float)
    x[3:5] = XCMD_XY
    m.x_cmd = x


def _both(*mods):
    return lambda o: [m(o) for m in mods]


LOWLEVEL_CASES = {
    "kp_full": (lambda m: setattr(m, "kp", KP_FULL.copy()), None),
    "kd_full": (lambda m: setattr(m, "kd", KD_FULL.copy()), None),
    "hip_offset": (None, lambda b: setattr(b, "hip_offset", HIP_OFFSET.copy())),
    "swingHeight_0.05": (lambda m: setattr(m, "swingHeight", 0.05), None),
    "h16": (lambda m: setattr(m, "h", 16), None),
    "xcmd_xy": (_xcmd_xy, None),
    "combined": (util.PARAM_CASES["dt_0.05"][0],
                 _both(util.PARAM_CASES["m_20"][1], util.PARAM_CASES["I_nondiagonal"][1], util.PARAM_CASES["g_3.7"][1])),
}

CASES = {**util.PARAM_CASES, **util.WEIGHT_CASES, **LOWLEVEL_CASES}

SOLVE_CASES = [k for k in list(util.PARAM_CASES) + list(util.WEIGHT_CASES) if k != "default"]
PLANT_CASES = ["m_8", "m_20", "g_3.7", "I_nondiagonal", "dt_0.02", "dt_0.05", "combined"]

ENTRIES = {
    "solve_stage": list(SOLVE_CASES),
    "evaluate": list(SOLVE_CASES),
    "evaluate_grad": [k for k in SOLVE_CASES if k not in ("lt_lh", "f_max_150")],
    "certify": list(SOLVE_CASES),
    "plant_step": list(PLANT_CASES),
    "foot_position_world": ["hip_offset"],
    "low_level_control": ["kp_full", "kd_full", "swingHeight_0.05", "h16", "xcmd_xy", "combined"],
}

# (entry, case) -> why the pair is not in ENTRIES although the entry's tests run the case
STRUCK = {
    ("plant_step", "kv_0.05"): "the plant step does not read kv (only the landing rule of the closed loop does)",
    ("evaluate_grad", "lt_lh"): "the gradient of the cost reads no constraint row: the line-foot lengths do not enter it",
    ("evaluate_grad", "f_max_150"): "the gradient of the cost reads no constraint row: the force box does not enter it",
    ("foot_position_world", "kp_full"): "the forward kinematics read hip_offset alone of the parameter block",
    ("foot_position_world", "kd_full"): "the forward kinematics read hip_offset alone of the parameter block",
    ("foot_position_world", "swingHeight_0.05"): "the forward kinematics read hip_offset alone of the parameter block",
    ("foot_position_world", "h16"): "the forward kinematics read hip_offset alone of the parameter block",
    ("foot_position_world", "xcmd_xy"): "the forward kinematics read hip_offset alone of the parameter block",
    ("foot_position_world", "combined"): "the forward kinematics read hip_offset alone of the parameter block",
    ("low_level_control", "hip_offset"): "lowLevelControl takes the foot positions as an input (REF:444): hip_offset acts through the FK",
}


def apply(name, mpc, biped):
    """Applies case `name` to an (MPC, Biped) pair of either module, in place; returns the pair."""
    for mod, obj in zip(CASES[name], (mpc, biped)):
        if mod:
            mod(obj)
    return mpc, biped


def objects(module, name, h=None, x_cmd=None):
    """(MPC, Biped) of `module` (biped_mpc_py_amd or oracle.bmpc_oracle) at case `name`; h and x_cmd are set BEFORE the case is
    applied, so that a case that sets them (h16, xcmd_xy) keeps its value."""
    mpc, biped = module.MPC(), module.Biped()
    if h is not None:
        mpc.h = int(h)
    if x_cmd is not None:
        mpc.x_cmd = np.array(x_cmd, float)
    return apply(name, mpc, biped)


def mods(name):
    """The case as the `mods` argument of eval_cases.yardstick / cparams_of and certify_cases.condensed."""
    return CASES[name]


def plant_kw(name):
    """The keyword arguments of plant_model.step / step_batch at case `name`."""
    from oracle import bmpc_oracle as orc
    mpc, biped = objects(orc, name)
    return dict(I_b=np.asarray(biped.I, float).reshape(3, 3), m=float(biped.m), g=float(biped.g), dt=float(mpc.dt))


# ---- the stage family's inputs and the oracle's answers to them (tests/golden/param_cases_stage.npz, tests/gen_param_cases.py) -----
STAGE_HORIZONS = (7, 10, 26)
STAGE_B = 8
STAGE_SEEDS = {7: 707, 10: 62, 26: 726}


def stage_batch(h):
    """The B = 8 instances of the stage-family test at horizon h: mixed gait, commanded v_x, the half period fitted to the horizon
    as test_odd_and_short_horizons does (max(1, h // 2); the reference's 5 at h = 10)."""
    return util.synth_batch(STAGE_B, h, STAGE_SEEDS[h], gait="mixed", vx_cmd=True)


def oracle_solve(s, i, h, name, return_info=False):
    """`orc.solve_mpc` of instance i of synth batch s at case `name`, on the fp32-rounded inputs the GPU sees."""
    from oracle import bmpc_oracle as orc
    r32 = lambda a: np.asarray(a, float).astype(np.float32).astype(float)
    m, b = objects(orc, name, h=h, x_cmd=r32(s["x_cmd"][i]))
    mu = None if s["mu"] is None else r32(s["mu"][i])
    return orc.solve_mpc(r32(s["x_fb"][i]), (int(s["phase"][i]) + 0.5) * m.dt, r32(s["foot"][i]), m, b, s["contact"][i], half=s["half"],
                         mu_steps=mu, return_info=return_info)


# ---- evaluate / evaluate_grad / certify: the groups of a case -----------------------------------------------------------------------
EVAL_GROUPS = ((10, 1), (10, 2), (13, 2), (26, 2))        # (h, kernel family): dense and stage at 10, stage at 13, two waves at 26
EVAL_B = 16                                               # one instance per mask of eval_cases.breaking_controls
# the instances held to the yardstick (all 16 run): at h = 26 a yardstick takes 0.4 s per instance, so eight -- the four broken ones and
# four of the case's flavour -- are compared there
EVAL_CHECKED = {26: (0, 1, 2, 3, 5, 9, 12, 15)}
EMU_INSTANCES = (0, 9)                                    # the two that also run through the emulation: every class broken / the case's flavour


# Which controls make a case show (the sensitivity condition decides; tests/test_param_cases_cpu.py):
#   broken    `breaking_controls` of `seeded_controls`: the tracking cost of a plan that falls over dominates everything -- it shows
#             Q, dt, I, kv, and f_max through the force box;
#   internal  a plan that holds the body still (the weight shared at the case's m and g, every leg's torque about the body cancelled
#             by its moment, supplied references that stay at x_fb) with 250-400 N of INTERNAL force between the legs: the cost and
#             the gradient are the R term's, and they leave it as soon as m or g is not the case's;
#   line      1.3 x the seeded plan with 40 N m of pitch moment on the STANCE legs: the line-foot rows alone are violated, by an
#             amount that lt and lh set (on a swing leg, f_z = 0, the violation would be the moment itself whatever lt is).
# The first four instances of every group are broken ones (masks 15, 1, 2, 4 of breaking_controls), so that every violation class
# is non-zero and zero somewhere in every group.
FLAVOUR = {"R_div100": "internal", "R_x100": "internal", "R_x10": "internal", "R_div10": "internal", "R_mixed": "internal",
           "m_8": "internal", "m_20": "internal", "g_3.7": "internal", "lt_lh": "line"}
N_BROKEN = 4


def eval_group(h, name):
    """The evaluation group of case `name` at horizon h: 16 mixed-gait instances with a commanded v_x.  Flavour broken and line:
    GENERATED references, so that dt and kv act through the reference generators too; internal: supplied ones.  The group carries the
    case as its "mods"."""
    from oracle import bmpc_oracle as orc
    from tests import eval_cases as ec
    s = util.synth_batch(EVAL_B, h, 3100 + h, gait="mixed", vx_cmd=True)
    _, biped = objects(orc, name)
    m, grav = float(biped.m), float(biped.g)
    flavour = FLAVOUR.get(name, "broken")
    U0 = ec.seeded_controls(s["contact"], np.random.default_rng(3200 + h), m=m, g=grav)
    U = ec.breaking_controls(U0, 3300 + h)
    x_fb, x_cmd, x_ref, foot_ref = ec.r32(s["x_fb"]), s["x_cmd"], None, None
    rng = np.random.default_rng(3400 + h)
    if flavour == "line":
        d = np.zeros_like(U0)
        for leg in range(2):
            d[:, :, 6 + 3 * leg + 1] = s["contact"][:, :, leg] * (40.0 + rng.uniform(0, 4, U0.shape[:2]))
        U[N_BROKEN:] = ec.r32(1.3 * U0 + d)[N_BROKEN:]
    if flavour == "internal":
        x_fb[:, 6:12] = 0.0
        foot = ec.r32(s["foot"])
        x_ref = np.concatenate([np.repeat(x_fb[:, :, None], h, 2), np.ones((EVAL_B, 1, h))], 1)
        foot_ref = np.repeat(foot[:, :, None], h, 2)
        x_cmd = np.concatenate([x_fb[:, :6], np.zeros((EVAL_B, 6))], 1)
        F = rng.uniform(250.0, 400.0, (EVAL_B, h, 2)) * rng.choice([-1.0, 1.0], (EVAL_B, h, 2))
        V = np.zeros_like(U0)
        for leg, sgn in enumerate((1.0, -1.0)):
            f = np.concatenate([sgn * F, np.full((EVAL_B, h, 1), m * grav / 2)], 2)
            f = ec.r32(f)
            r = (foot[:, 3 * leg:3 * leg + 3] - x_fb[:, 3:6])[:, None, :]
            V[:, :, 3 * leg:3 * leg + 3] = f
            V[:, :, 6 + 3 * leg:9 + 3 * leg] = -np.cross(r, f)
        U[N_BROKEN:] = ec.r32(V)[N_BROKEN:]
    g = ec._group(h, s["half"], None, x_fb, s["foot"], s["contact"], s["phase"], x_cmd, U, x_ref=x_ref, foot_ref=foot_ref,
                  name=f"param_{name}_h{h}")
    g["mods"] = mods(name)
    return g


def eval_indices(h):
    return list(EVAL_CHECKED.get(h, range(EVAL_B)))


def eval_inputs_key(name):
    """Cases with the same key have the same evaluation groups but for their "mods"."""
    from oracle import bmpc_oracle as orc
    _, biped = objects(orc, name)
    return FLAVOUR.get(name, "broken"), float(biped.m), float(biped.g)


DEFAULT_MODS = (None, None)                               # the defaults THROUGH the modification path (dt from the MPC object)


def pick_act_tol(mats, U):
    """(act_tol, margin) for controls U (n,h,12) on the condensed problems `mats`: the first of certify_cases.ACT_TOL_CANDIDATES
    that keeps every positive slack a factor 2 from its threshold, else the one with the largest margin -- the rule of
    tests/gen_certify.py for plans that are not optima."""
    from tests import certify_cases as cc
    seen = []
    for tol in cc.ACT_TOL_CANDIDATES:
        m = min(cc.margin(mats[i], U[i], tol) for i in range(len(mats)))
        if m >= 2.0:
            return tol, m
        seen.append((m, tol))
    m, tol = max(seen)
    assert m >= cc.PERT_MIN_MARGIN, m
    return tol, m


def certify_yardstick(g, idx=None):
    """(yardstick arrays stacked over instances idx of group g -- at the group's case --, act_tol)."""
    from tests import certify_cases as cc
    idx = list(range(g["x_fb"].shape[0]) if idx is None else idx)
    mats = [cc.condensed(g, i) for i in idx]
    U = g["controls"][idx]
    tol, _ = pick_act_tol(mats, U)
    ys = [cc.yardstick(mats[k], U[k], tol) for k in range(len(idx))]
    return {k: np.stack([np.asarray(y[k]) for y in ys]) for k in ("lam", "resid", "summary", "n_active", "active", "indep")}, tol


# Regression bounds of the parameter cases, by the rule of eval_cases.REG_BOUND: 100 x the larger of the maxima measured in the
# emulation and on the MI355X over the new cases, against the yardstick (docs/history_r16.md has the measurements per metric and where
# each maximum sits).  The acceptance bound is util.REL_TOL; these are asserted in addition.  eval_cases.REG_BOUND,
# eval_grad_cases.REG_BOUND and certify_cases.REL_BOUND stay the bounds of the existing cases.
# Measured maxima (emulation / MI355X): states 4.442e-14 / 4.442e-14, cost 1.165e-15 / 1.750e-15, objective 1.165e-15 / 1.615e-15,
# violation 1.922e-16 / 7.849e-16.
PARAM_REG_BOUND = dict(states=4.45e-12, cost=1.75e-13, objective=1.62e-13, violation=7.85e-14)
# Measured maxima (emulation / MI355X): cost 8.856e-14 / 2.279e-13, grad_u 2.209e-11 / 2.209e-11, grad_x0 8.690e-11 / 1.201e-10 (the
# metric divides by max(1, max|ref|): on the plans that hold the body still the gradient is the R term's, below 1, and the figure is
# absolute).
PARAM_GRAD_REG_BOUND = dict(cost=2.28e-11, grad_u=2.21e-09, grad_x0=1.21e-08)
# Per quantity of certify_cases.deviations, relative to grad_scale.  Measured maxima (emulation / MI355X): resid 2.346e-08 / 6.465e-08,
# stationarity 1.196e-08 / 3.990e-08, complementarity 1.048e-07 / 1.388e-06, grad_scale 1.196e-08 / 6.205e-08, primal_ineq
# 1.922e-16 / 2.018e-16, lam 3.591e-09 / 2.031e-08 -- all but primal_ineq at R_div100, h = 26, on the plans that hold the body
# still: there the gradient is 2 R u with R = 1e-6, grad_scale is 1e-3, and the YARDSTICK forms it as Hc U + gc from dense matrices
# whose terms are of order 1e2 and cancel (the note at certify_cases.MEASURED_REL).  On those instances the emulation's gradient is
# 7e-9 grad_scale from the yardstick of eval_grad_cases, the two yardsticks 7e-8 from each other (docs/history_r16.md); the device
# entry sees eight instances there, the emulation two.  complementarity's 100 x lies above util.REL_TOL: for it the acceptance bound
# is the one that binds.
PARAM_CERT_REL_BOUND = dict(resid=6.47e-06, stationarity=3.99e-06, complementarity=1.39e-04, grad_scale=6.21e-06, primal_ineq=2.02e-14,
                            lam=2.04e-06)


# ---- low-level kernels --------------------------------------------------------------------------------------------------------------
LOWLEVEL_B = 300
FK_TOL, TAU_TOL = 2e-6, 2e-5                              # the tolerances of test_low_level_control_and_fk_on_device


def lowlevel_batch(name, B=LOWLEVEL_B, seed=17):
    """Inputs of the low-level test at case `name`, fp32-rounded: attitudes up to +-0.6 rad, t in [-1, 3] with the first 24 entries
    exact multiples k Ts, k = -8 .. 15, of the case's swing period, all four contact patterns in turn."""
    from oracle import bmpc_oracle as orc
    mpc, _ = objects(orc, name)
    Ts = mpc.dt * mpc.h / 2
    rng = np.random.default_rng(seed)
    r32 = lambda a: np.asarray(a, float).astype(np.float32).astype(float)
    x = np.concatenate([rng.uniform(-0.6, 0.6, (B, 3)), rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(0.45, 0.6, (B, 1)),
                        rng.uniform(-0.5, 0.5, (B, 6))], 1)
    t = rng.uniform(-1.0, 3.0, B)
    t[:min(24, B)] = (np.arange(-8, 16) * Ts)[:B]
    c0 = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], np.uint8)[(np.arange(B) + np.arange(B) // 4) % 4]
    return dict(x_fb=r32(x), q=r32(rng.uniform(-1, 1, (B, 10))), qd=r32(rng.uniform(-2, 2, (B, 10))), t=t, contact0=c0,
                u0=r32(rng.uniform(-50, 150, (B, 12))), Ts=Ts)


def lowlevel_fk_ref(name, d):
    """orc.getFootPositionWorld at case `name` on batch d: (B,6) fp64."""
    from oracle import bmpc_oracle as orc
    _, biped = objects(orc, name)
    return np.stack([orc.getFootPositionWorld(d["x_fb"][i], d["q"][i], biped).reshape(-1) for i in range(len(d["t"]))])


def lowlevel_tau_ref(name, d, pf):
    """orc.lowLevelControl at case `name` on batch d with foot positions pf (B,6) (rounded to fp32 here): (B,10) fp64."""
    from oracle import bmpc_oracle as orc
    mpc, biped = objects(orc, name)
    pf = np.asarray(pf, float).astype(np.float32).astype(float)
    return np.stack([orc.lowLevelControl(d["x_fb"][i], float(d["t"][i]), pf[i].reshape(6, 1), d["q"][i], d["qd"][i], mpc, biped,
                                         np.tile(d["contact0"][i].astype(int), (mpc.h, 1)), d["u0"][i].reshape(12, 1)).reshape(-1)
                     for i in range(len(d["t"]))])


# ---- closed loop on the plant -------------------------------------------------------------------------------------------------------
CLOSED_LOOP_B, CLOSED_LOOP_K = 33, 12
CLOSED_LOOP_RUNS = {
    "combined_h7_stage": dict(case="combined", h=7, path=2, gait=(7, (2, 5), (4, 3)), integrator="rk4", substeps=4),
    "euler_h10_dense": dict(case="I_nondiagonal", h=10, path=1, gait=(10, (0, 5), (5, 5)), integrator="euler", substeps=3),
}


def closed_loop_start(run, B=CLOSED_LOOP_B, seed=9):
    """(x0 (B,12) f32, foot (B,6) f32, t0 (B,), x_cmd (B,12) f32 with x_cmd[:, 3:5] != 0) of closed-loop run `run`: mixed schedule
    steps, away from the period boundaries at the run's dt."""
    from oracle import bmpc_oracle as orc
    r = CLOSED_LOOP_RUNS[run]
    mpc, _ = objects(orc, r["case"], h=r["h"])
    x0, foot, _ = util.closed_loop_start(B, seed)
    rng = np.random.default_rng(seed + 1)
    x0[:, 6:9] = rng.uniform(-0.1, 0.1, (B, 3))
    t0 = rng.integers(0, r["gait"][0], B) * mpc.dt + 0.25 * mpc.dt
    x_cmd = np.tile(np.asarray(mpc.x_cmd, np.float32), (B, 1))
    x_cmd[:, 3:5] = rng.uniform(0.02, 0.08, (B, 2)) * rng.choice([-1.0, 1.0], (B, 2))
    return x0, foot, t0, x_cmd
