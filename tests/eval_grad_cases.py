"""Yardstick, bounds and helpers of the cost-gradient tests (tests/test_evaluate_grad_cpu.py, tests/test_gpu_evaluate_grad.py).  The case
sets are those of tests/eval_cases.py, imported.

Yardstick: the oracle's matrices, not a QP solve and not finite differences.  For an instance and controls U (every input rounded to
fp32 first, as the entry takes them) `orc.build_sparse_qp` gives P, q, A = [A_x A_u], b of REF:187-297;
  X = solve(A_x, b - A_u U), z = [X; U], r = P z + q
  grad_u  = r_U - (A_x^-1 A_u)' r_X
  grad_x0 = (A_x^-1 db/dx_fb)' r_X, db/dx_fb column by column as b(x_fb + e_j) - b(x_fb) with the references pinned through
            `refs_cases.supplied` (b is affine in x_fb then); for generated references the oracle's own x_ref / foot_ref are
            taken first and pinned -- the convention of include/bmpc.h: references, lever arms and linearisation held fixed.
Error metric per instance and output: max|got - ref| / max(1, max|ref|)."""
import numpy as np

from tests import eval_cases as ec
from tests import refs_cases as rc
from tests import util

KEYS = ("cost", "grad_u", "grad_x0")

# Regression bounds per metric: 100 x the larger of the maxima measured over all cases of the new tests in the emulation and on the
# MI355X (the rule of eval_cases.REG_BOUND; docs/history_r10.md has the measurements).  The acceptance bound is util.REL_TOL; these
# are asserted in addition.
# Measured maxima (emulation / MI355X): cost 1.392e-13 / 1.392e-13, grad_u 3.018e-13 / 3.063e-13, grad_x0 1.576e-14 / 1.576e-14.
# (cost is the evaluation's, bit for bit; its figure here is the yardstick's own cancellation in objective + sum Q x_ref^2.)
REG_BOUND = dict(cost=1.40e-11, grad_u=3.07e-11, grad_x0=1.58e-12)

# CPU test 4 (gradient against differences of the merged evaluation's cost), relative to max(1, |cost|): the same rule.
# Measured maxima (emulation / MI355X): 4.013e-15 / 3.370e-15.
IDENTITY_BOUND = 4.02e-13

# CPU test 5: -(grad_u . U*) / max(1, cost) >= -OPT_TOL[h] on the reference's own optima (ref_tracking.npz).  u = 0 is feasible at the
# default bounds, so this is the variational inequality g . (V - U*) >= 0 with V = 0.  The yardstick itself gives worst values of
# -6.4e-7 (h = 10), -1.9e-6 (h = 16), -1.1e-5 (h = 20) on the fixture's fp32-rounded optima; the tolerance is 10 x that: the margin
# is for the fp32 rounding of U*.
OPT_YARDSTICK_WORST = {10: -6.4e-7, 16: -1.9e-6, 20: -1.1e-5}
OPT_TOL = {h: -10.0 * v for h, v in OPT_YARDSTICK_WORST.items()}

# GPU test 12: the same quantity on the SOLVER's own optima (4096-instance synth batches, both kernel families): OPT_TOL widened by
# the solver's stopping tolerance: the project accepts a solve whose controls are within util.REL_TOL (relative) of the optimum, q is
# itself a relative quantity (normalised by the cost), so the margin is util.REL_TOL.  Measured once on the MI355X
# (docs/history_r10.md): worst q over all 4096 instances and both families -4.5e-6 (h = 10), -1.2e-5 (h = 16), -1.8e-5 (h = 20),
# against -2.1e-7, -7.4e-7, -2.4e-6 for the oracle's optima of the same instances through the yardstick: the margin used is at
# most 1.6e-5.
OPT_SOLVER_MARGIN = util.REL_TOL
OPT_TOL_SOLVER = {h: v + OPT_SOLVER_MARGIN for h, v in OPT_TOL.items()}


def yardstick(g, i, mods=None):
    """dict(cost, grad_u (h,12), grad_x0 (12,)) of instance i of group g, fp64; `mods`: see eval_cases.oracle_objects."""
    from oracle import bmpc_oracle as orc
    h = g["h"]
    mpc, biped, dt = ec.oracle_objects(g, i, mods)
    mu = None if g["mu"] is None else ec.r32(g["mu"][i])
    U = ec.r32(g["controls"][i]).reshape(-1)
    t = (int(g["phase"][i]) + 0.5) * dt
    x_fb, foot, contact = ec.r32(g["x_fb"][i]), ec.r32(g["foot"][i]), np.asarray(g["contact"][i])
    build = lambda x: orc.build_sparse_qp(x, t, foot, mpc, biped, contact, half=g["half"], mu_steps=mu)
    xr = None if g["x_ref"] is None else np.vstack([ec.r32(g["x_ref"][i][:12]), np.ones((1, h))])
    fr = None if g["foot_ref"] is None else ec.r32(g["foot_ref"][i])
    if xr is None or fr is None:                 # generated: the oracle's own, pinned from here on
        with rc.supplied(orc, xr, fr):
            sp0 = build(x_fb)
        xr, fr = np.array(sp0["x_ref"], float), np.array(sp0["foot_ref"], float)
    with rc.supplied(orc, xr, fr):
        sp = build(x_fb)
        b0 = np.asarray(sp["b"], float).reshape(-1)
        db = np.stack([np.asarray(build(x_fb + np.eye(12)[j])["b"], float).reshape(-1) - b0 for j in range(12)], 1)
    A, P, q = np.asarray(sp["A"], float), np.asarray(sp["P"], float), np.asarray(sp["q"], float).reshape(-1)
    Ax, Au = A[:, :13 * h], A[:, 13 * h:]
    X = np.linalg.solve(Ax, b0 - Au @ U)
    z = np.concatenate([X, U])
    r = P @ z + q
    rX, rU = r[:13 * h], r[13 * h:]
    objective = float(z @ P @ z / 2 + q @ z)
    cost = objective + float(np.sum(np.asarray(mpc.Q, float)[:, None] * sp["x_ref"] ** 2))
    grad_u = rU - np.linalg.solve(Ax, Au).T @ rX
    grad_x0 = np.linalg.solve(Ax, db).T @ rX
    return dict(cost=cost, grad_u=grad_u.reshape(h, 12), grad_x0=grad_x0)


def yardstick_group(g, idx=None, mods=None):
    idx = range(g["x_fb"].shape[0]) if idx is None else idx
    ys = [yardstick(g, int(i), mods) for i in idx]
    return {k: np.stack([np.asarray(y[k]) for y in ys]) for k in KEYS}


def metrics(got, ref):
    """max|got - ref| / max(1, max|ref|) per instance and output."""
    n = ref["cost"].shape[0]
    out = {}
    for k in KEYS:
        a, b = np.asarray(got[k]).reshape(n, -1), np.asarray(ref[k]).reshape(n, -1)
        out[k] = np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b).max(1))
    return out


def check(got, ref, where, reg_bound=None):
    """Prints the maxima of the three metrics, then asserts the acceptance bound (util.REL_TOL) and the regression bound of each
    (REG_BOUND, or `reg_bound` for case sets that hold their own)."""
    reg_bound = REG_BOUND if reg_bound is None else reg_bound
    m = {k: float(v.max()) for k, v in metrics(got, ref).items()}
    print("evaluate_grad metrics", where, " ".join(f"{k}={v:.3e}" for k, v in m.items()),
          "|grad_u| %.3g |grad_x0| %.3g" % (np.abs(ref["grad_u"]).max(), np.abs(ref["grad_x0"]).max()))
    assert all(np.isfinite(got[k]).all() for k in KEYS), where
    for k, v in m.items():
        assert v <= util.REL_TOL, (where, k, v)
        assert v <= reg_bound[k], (where, k, v)
    return m


def all_groups():
    """The case sets of CPU test 1: ref_tracking (plain and breaking), generated references, every lane-group size."""
    return ec.ref_tracking_groups() + ec.ref_tracking_groups(breaking=True) + ec.generated_groups() + ec.horizon_groups()


def batch_group(h):
    """The batch of 200 of eval case 4 (tests/test_evaluate_cpu.py) and its permutation."""
    s = rc.make_batch(200, h, 31 + h, "abcde")
    rng = np.random.default_rng(h)
    g = ec._group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], ec.seeded_controls(s["contact"], rng),
                  x_ref=s["x_ref"], foot_ref=s["foot_ref"])
    return g, rng.permutation(200)


BATCH_POSITIONS = (0, 3, 77, 199)                # (first of a wave, inside a wave, last group of the last workgroup)


def grid_pair(g, seed):
    """(U, D) for the identity test: the group's controls rounded to the 2^-10 grid and a seeded direction on that grid with entries
    in [-2, 2], so that U + D and U - D are exact in fp32 (|U| < 2^13)."""
    rng = np.random.default_rng(seed)
    U = np.round(ec.r32(g["controls"]) * 1024.0) / 1024.0
    D = rng.integers(-2048, 2049, U.shape) / 1024.0
    assert np.abs(U).max() < 8192 - 2
    for a in (U, D, U + D, U - D):
        assert np.array_equal(a, ec.r32(a))
    return U, D


def check_identity(cost_of, grad_u, g, U, D, where):
    """(cost(U + D) - cost(U - D)) / 2 == grad_u(U) . D (exact for a quadratic) and cost(U + D) + cost(U - D) - 2 cost(U) >= 0
    (convexity), both relative to max(1, |cost(U)|).  `cost_of(controls)`: the merged evaluation's cost (B,)."""
    cp, cm, c0 = cost_of(U + D), cost_of(U - D), cost_of(U)
    lhs = (cp - cm) / 2
    rhs = np.sum(grad_u.reshape(D.shape[0], -1) * D.reshape(D.shape[0], -1), 1)
    scale = np.maximum(1.0, np.abs(c0))
    err = float((np.abs(lhs - rhs) / scale).max())
    curv = float(((cp + cm - 2 * c0) / scale).min())
    print("evaluate_grad identity", where, "err=%.3e" % err, "curvature min=%.3e" % curv, "|g.D| max %.3g cost max %.3g" % (np.abs(rhs).max(), c0.max()))
    assert err <= IDENTITY_BOUND, (where, err)
    assert curv >= 0.0, (where, curv)
    return err


def optimality(grad_u, controls, cost):
    """-(grad_u . U) / max(1, cost) per instance: >= 0 at an optimum U when u = 0 is feasible."""
    n = cost.shape[0]
    return -np.sum(np.asarray(grad_u).reshape(n, -1) * ec.r32(controls).reshape(n, -1), 1) / np.maximum(1.0, cost)
