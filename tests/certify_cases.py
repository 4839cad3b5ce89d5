"""Yardstick, case sets, bounds and helpers of the certificate tests (tests/test_certify_cpu.py, tests/test_gpu_certify.py) and of
the fixture generator tests/gen_certify.py.

Yardstick: the oracle's matrices and SciPy's NNLS, per instance, as `oracle.bmpc_oracle.certificate_from_primal` does it.  For an
instance and controls U (every input rounded to fp32 first, as the entry takes them) `orc.build_sparse_qp` -> `orc.condense` give
Hc, gc, C, d of the condensed problem;
  g = Hc U + gc,  slack = d - C U,  active = slack <= act_tol (1 + |d|),  lam[active] = nnls(C[active]', -g),  resid = g + C' lam.
The yardstick gets the SAME fp32-rounded controls and the same act_tol as the device.  The NNLS residual is unique, so resid, C' lam,
the summary and n_active compare on every case; lam itself only on the rows whose multiplier is unique: those not in the span of
the other active rows of their (step, leg) block (`indep`).  Expected values live in tests/golden/certify.npz and, for the four large
sets, in tests/golden/certify_<set>_<kind>.npz -- one file cannot hold every instance within the 1 MiB a committed file may have
(tests/gen_certify.py writes them; numeric arrays only), so that a machine without SciPy can run the comparison.

Case sets: EVERY instance of the oracle-solved golden sets cfg2, cfg4, cfg3_h16, cfg5_mu_h20, cfg_h32, cfg_h40, edge_cases_h10,
cfg_hodd and ref_tracking.  Each set comes twice: the fixture's optimum rounded to fp32 (`opt`) and that optimum with 1 % relative
noise clipped back into the box (`pert`), each a case set with ONE act_tol.  For `opt` (and the solver's own controls) it is the first
entry of ACT_TOL_CANDIDATES for which no slack of any instance of the set lies within a factor 2 of its threshold; the generator
asserts that one exists.  For `pert` that rule CANNOT hold on a whole set: a perturbed plan has positive slacks of every size (1 % of
entries that range from 1e-9 N to 500 N), and among the 92 160 rows of cfg_h40 some lie within a factor 2 of any threshold.  There
the generator takes the first candidate that keeps the factor 2 if one does, else the candidate with the LARGEST margin, records that
margin and asserts it is at least 1 + 1e-6: what the margin is for is that device and yardstick agree on which rows are active, and
their slacks agree to ~1e-15 relative, nine orders below that."""
import os

import numpy as np

from tests import eval_cases as ec
from tests import util

FIXTURE = os.path.join(util.GOLDEN, "certify.npz")
KEYS = ("lam", "resid", "summary", "n_active", "status")
SUMMARY = ("stationarity", "primal_ineq", "complementarity", "grad_scale")

# act_tol per case set, see above; the Python default 1e-4 comes first, the rest are half-decade steps either side of it
ACT_TOL_CANDIDATES = (1e-4, 3e-5, 3e-4, 1e-5, 1e-3, 3e-6, 3e-3, 1e-6)
PERT_MIN_MARGIN = 1.0 + 1e-6

# the sets whose arrays get files of their own, one per kind (1 MiB per committed file)
BIG_SETS = ("cfg2_standing_h10", "cfg4_walking_h10", "cfg_h32", "cfg_h40")

# Bound on |got - yardstick| / grad_scale per instance for resid (which is also C' lam: g is common), stationarity, complementarity,
# grad_scale and lam on its unique rows: 10 x the largest deviation of the EMULATION from the yardstick over all case sets (opt and
# pert).  `python -m tests.gen_certify --measure` prints the figure; per set: docs/history_r11.md.
# Measured maximum over every instance of every set: 3.630e-12 (resid of cfg2_standing_h10/opt; the yardstick forms g as Hc U + gc
# from the dense condensed matrices).
MEASURED_REL = 3.630e-12
REL_BOUND = 10.0 * MEASURED_REL
# duals_to_reference_order(lam) against solve_qp's lam on the unique rows, relative to grad_scale: the device's lam belongs to the
# optimum ROUNDED TO FP32, solve_qp's to its own fp64 optimum, so this measures the rounding of U through the Hessian, not arithmetic.
# Measured maximum over the opt sets, every instance (emulation): 3.450e-04 (cfg2_standing_h10; cfg3_trot_h16 2.137e-04, cfg4 9.344e-05);
# the bound is 10 x that.  The MI355X gives the same figures per set to all digits printed.
MEASURED_QP_REL = 3.450e-04
QP_REL_BOUND = 10.0 * MEASURED_QP_REL


def ref_index(h):
    """(h, 36) int: row of G at REF:273 of row r of step k -- friction 8k + r, box 8h + 24k + (r - 8), line foot 32h + 4k + (r - 32)."""
    k = np.arange(h)[:, None]
    r = np.arange(36)[None, :]
    return np.where(r < 8, 8 * k + r, np.where(r < 32, 8 * h + 24 * k + (r - 8), 32 * h + 4 * k + (r - 32)))


def leg_rows():
    """(2, 18) int: the rows of a step (0 .. 35) that touch leg g, in the kernel's candidate order -- 4 friction, 3 + 3 upper bounds
    (f, m), 3 + 3 lower bounds, 2 line foot."""
    out = []
    for g in range(2):
        out.append([4 * g + j for j in range(4)] + [8 + 3 * g + a for a in range(3)] + [14 + 3 * g + a for a in range(3)]
                   + [20 + 3 * g + a for a in range(3)] + [26 + 3 * g + a for a in range(3)] + [32 + 2 * g + j for j in range(2)])
    return np.array(out)


def leg_cols():
    """(2, 6) int: the controls of a step (0 .. 11) of leg g: f then m."""
    return np.array([[0, 1, 2, 6, 7, 8], [3, 4, 5, 9, 10, 11]])


def condensed(g, i, mods=None):
    """(Hc, gc, C, d, sparse dict) of instance i of group g: the condensed problem of the oracle on the fp32-rounded inputs; `mods`:
    see eval_cases.oracle_objects."""
    from oracle import bmpc_oracle as orc
    from tests import refs_cases as rc
    h = g["h"]
    mpc, biped, dt = ec.oracle_objects(g, i, mods)
    mu = None if g["mu"] is None else ec.r32(g["mu"][i])
    t = (int(g["phase"][i]) + 0.5) * dt
    xr = None if g["x_ref"] is None else np.vstack([ec.r32(g["x_ref"][i][:12]), np.ones((1, h))])
    fr = None if g["foot_ref"] is None else ec.r32(g["foot_ref"][i])
    with rc.supplied(orc, xr, fr):
        sp = orc.build_sparse_qp(ec.r32(g["x_fb"][i]), t, ec.r32(g["foot"][i]), mpc, biped, np.asarray(g["contact"][i]),
                                 half=g["half"], mu_steps=mu)
    assert orc.phase_index(t, mpc) == int(g["phase"][i])
    Hc, gc, C, d, _, _ = orc.condense(sp["P"], sp["q"], sp["G"], sp["h"], sp["A"], sp["b"], 13 * h)
    return Hc, gc, C, d, sp


def margin(mats, U, act_tol):
    """The smallest factor between a positive slack and its threshold act_tol (1 + |d|), either way round (>= 2 wanted)."""
    _, _, C, d, _ = mats
    slack = d - C @ ec.r32(U).reshape(-1)
    thr = act_tol * (1.0 + np.abs(d))
    pos = slack > 0
    return float(np.where(pos, np.maximum(slack / thr, thr / np.where(pos, slack, 1.0)), np.inf).min())


def yardstick(mats, U, act_tol):
    """The certificate of controls U (rounded to fp32 here) for the condensed problem `mats`, by the oracle's rule and
    scipy.optimize.nnls on the whole instance: dict(lam (h,36), resid (h,12), summary (4,), n_active, active (h,36) bool, indep (h,36)
    bool: active rows whose multiplier is unique -- the row is not in the span of the other active rows of its leg block)."""
    from scipy.optimize import nnls
    Hc, gc, C, d, _ = mats
    U = ec.r32(U).reshape(-1)
    h = len(U) // 12
    grad = Hc @ U + gc
    slack = d - C @ U
    act = slack <= act_tol * (1.0 + np.abs(d))
    lam = np.zeros(36 * h)
    if act.any():
        la, _ = nnls(C[act].T, -grad, maxiter=100 * len(U))
        lam[act] = la
    resid = grad + C.T @ lam
    ri, lr, lc = ref_index(h), leg_rows(), leg_cols()
    indep = np.zeros((h, 36), bool)
    for k in range(h):
        for leg in range(2):
            rows = [r for r in lr[leg] if act[ri[k][r]]]
            blk = C[ri[k][rows]][:, 12 * k + lc[leg]] if rows else np.zeros((0, 6))
            full = np.linalg.matrix_rank(blk) if rows else 0
            for n, r in enumerate(rows):
                rest = np.delete(blk, n, 0)                    # (no other active row: rank 0; matrix_rank refuses an empty array)
                indep[k, r] = (np.linalg.matrix_rank(rest) if rest.size else 0) == full - 1
    summary = np.array([np.abs(resid).max(), max(0.0, (-slack).max()), np.abs(lam * slack).max(), np.abs(grad).max()])
    return dict(lam=lam[ri], resid=resid.reshape(h, 12), summary=summary, n_active=int(act.sum()), active=act[ri], indep=indep,
                slack=slack[ri])


def qp_duals(mats):
    """`orc.solve_qp`'s multipliers of the same QP, in the reference's row order (36h,)."""
    from oracle import bmpc_oracle as orc
    sp = mats[4]
    h = sp["x_ref"].shape[1]
    return orc.solve_qp(sp["P"], sp["q"], sp["G"], sp["h"], sp["A"], sp["b"], 13 * h)[1]


def _hgroup(name, hkey=None):
    """A group of a batched golden set (every instance), or of horizon `hkey` of cfg_hodd (all four)."""
    d = util.load(name)
    if hkey is not None:
        f = {k: d["h%d_%s" % (hkey, k)] for k in ("x_fb", "t", "foot", "contact", "x_cmd", "mu_steps", "controls", "half")}
        h, half, n = hkey, int(f["half"][0]), f["x_fb"].shape[0]
        label = f"{name}_h{hkey}"
    else:
        f = {k: d[k] for k in d.files}
        h = f["contact"].shape[1]
        half = int(f["half"][0]) if "half" in f else util.BATCH_FIXTURES[name][1]
        n, label = f["x_fb"].shape[0], name
    mu = f.get("mu_steps")
    mu = None if mu is None or not np.asarray(mu).size else np.asarray(mu, float)[:n]
    return ec._group(h, half, None, f["x_fb"][:n], f["foot"][:n], f["contact"][:n], util.phases(f["t"][:n], ec.DT, h), f["x_cmd"][:n],
                     ec.r32(f["controls"][:n]), mu=mu, name=label)


def optimum_groups():
    """Case 1: the oracle's optima, rounded to fp32, of the golden sets the issue names."""
    out = [_hgroup(n) for n in ("cfg2_standing_h10", "cfg4_walking_h10", "cfg3_trot_h16", "cfg5_mu_h20", "cfg_h32", "cfg_h40",
                                "edge_cases_h10")]
    out += [_hgroup("cfg_hodd", h) for h in (1, 2, 3, 4, 5, 7, 9, 15, 21, 33)]
    for g in ec.ref_tracking_groups():
        g["controls"] = ec.r32(g["controls"])
        out.append(g)
    return out


def box_of(g):
    """(lb, ub) (n,h,12) of a group: the bounds of REF:235-251 scaled by contact."""
    b = g["biped"]
    c = np.asarray(g["contact"], float)
    v = lambda k: np.asarray(getattr(b, k), float).reshape(3)
    sc = np.concatenate([np.repeat(c[:, :, 0:1], 3, 2), np.repeat(c[:, :, 1:2], 3, 2)] * 2, 2)
    return sc * np.concatenate([v("f_min"), v("f_min"), v("tau_min"), v("tau_min")]), \
        sc * np.concatenate([v("f_max"), v("f_max"), v("tau_max"), v("tau_max")])


def perturbed(g, seed):
    """Case 3: the group's controls with 1 % relative noise, clipped back into the box, rounded to fp32."""
    rng = np.random.default_rng(seed)
    lb, ub = box_of(g)
    U = g["controls"] * (1.0 + 0.01 * rng.standard_normal(g["controls"].shape))
    return ec.r32(np.clip(ec.r32(np.clip(U, lb, ub)), lb, ub))


def assert_worse(g, U, cert_opt, cert_pert):
    """stationarity / grad_scale of the perturbed plan U is larger than the optimum's on EVERY instance that has a perturbed plan.
    Relative noise clipped into the box leaves an instance unchanged only if every control of it is pinned at 0 (no leg in contact
    over the whole horizon: edge_cases_h10[2]); its feasible set is that one point, there is no worse plan, and the check there is
    that the two certificates are identical bits."""
    same = np.all(ec.r32(U) == ec.r32(g["controls"]), axis=(1, 2))
    assert not np.any(same & (np.asarray(g["contact"]).reshape(same.shape[0], -1).max(1) > 0)), (g["name"], same)
    ra = cert_opt["summary"][:, 0] / cert_opt["summary"][:, 3]
    rb = cert_pert["summary"][:, 0] / cert_pert["summary"][:, 3]
    assert (rb[~same] > ra[~same]).all(), (g["name"], ra, rb)
    for k in ("lam", "resid", "summary", "n_active", "status"):
        assert np.array_equal(np.asarray(cert_opt[k])[same], np.asarray(cert_pert[k])[same]), (g["name"], k)


def pert_seed(name):
    return 7000 + sum(ord(c) for c in name)


def fixture_file(name, kind):
    """The file that holds case set `name`, kind `kind` ('opt', 'pert', 'solver_<family>')."""
    if name in BIG_SETS:
        return os.path.join(util.GOLDEN, f"certify_{name}_{kind}.npz")
    return FIXTURE


class Fixture:
    """All fixture files as one read-only mapping (keys "<set>/<kind>/<array>")."""

    def __init__(self):
        import glob
        self._files = [np.load(p) for p in sorted(glob.glob(os.path.join(util.GOLDEN, "certify*.npz")))]
        self.files = [k for f in self._files for k in f.files]

    def __getitem__(self, key):
        for f in self._files:
            if key in f.files:
                return f[key]
        raise KeyError(key)


def load_fixture():
    return Fixture()


def expected(fx, name, kind):
    """dict of the yardstick's arrays of case set `name`, kind 'opt' | 'pert' | 'solver<family>', from the fixture."""
    p = f"{name}/{kind}/"
    out = {k[len(p):]: fx[k] for k in fx.files if k.startswith(p)}
    out["act_tol"] = float(out["act_tol"])
    return out


def deviations(got, ref):
    """Per instance, relative to the yardstick's grad_scale: resid (which is also C' lam: g is common), stationarity,
    complementarity, and lam on the independent blocks."""
    n = ref["resid"].shape[0]
    gs = np.maximum(ref["summary"][:, 3], np.finfo(float).tiny)
    dl = np.where(ref["indep"], np.abs(got["lam"] - ref["lam"]), 0.0)
    comp = np.abs(got["summary"][:, 2] - ref["summary"][:, 2])
    if "slack" in ref:
        # complementarity max |lam_i slack_i| is only as unique as lam: a row whose multiplier is NOT unique and whose slack is not 0
        # (a solver's answer: a pinned force of 2e-8 N instead of 0) carries whatever share of the multiplier the NNLS gave it.  Found on
        # cfg4_walking_h10/solver_dense[6]: 1.2e-10 between two valid multiplier vectors.  So where the fixture brings the slacks (the
        # solver sets), the figure is held to (a) the device's own lam times those slacks and (b) the yardstick's on the unique rows.
        own = np.abs(got["lam"] * ref["slack"]).reshape(n, -1).max(1)
        uq = lambda lam: np.where(ref["indep"], np.abs(lam * ref["slack"]), 0.0).reshape(n, -1).max(1)
        comp = np.maximum(np.abs(got["summary"][:, 2] - own), np.abs(uq(got["lam"]) - uq(ref["lam"])))
    return dict(resid=np.abs(got["resid"] - ref["resid"]).reshape(n, -1).max(1) / gs,
                stationarity=np.abs(got["summary"][:, 0] - ref["summary"][:, 0]) / gs,
                complementarity=comp / gs,
                grad_scale=np.abs(got["summary"][:, 3] - ref["summary"][:, 3]) / gs,
                primal_ineq=np.abs(got["summary"][:, 1] - ref["summary"][:, 1]) / np.maximum(1.0, ref["summary"][:, 1]),
                lam=dl.reshape(n, -1).max(1) / gs)


def check(got, ref, where, bound=None):
    """Prints the largest deviation per quantity, then asserts the bound on each, n_active equal, status 0, lam >= 0 and exactly 0 on
    the rows the yardstick holds inactive (`ref['active']`).  `bound`: REL_BOUND, or a case set's own -- one figure, or a dict per
    quantity, which is then asserted IN ADDITION to the acceptance bound util.REL_TOL."""
    bound = REL_BOUND if bound is None else bound
    dev = {k: float(v.max()) for k, v in deviations(got, ref).items()}
    if isinstance(bound, dict):
        print("certify deviations", where, " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
        bound = {k: min(v, util.REL_TOL) for k, v in bound.items()}
    else:
        print("certify deviations", where, " ".join(f"{k}={v:.3e}" for k, v in dev.items()), "bound %.3e" % bound)
        bound = dict.fromkeys(dev, bound)
    assert np.isfinite(got["lam"]).all() and np.isfinite(got["resid"]).all() and np.isfinite(got["summary"]).all(), where
    assert np.array_equal(got["n_active"], ref["n_active"]), (where, got["n_active"], ref["n_active"])
    assert (got["status"] == 0).all(), (where, got["status"])
    assert (got["lam"] >= 0).all(), where
    assert not got["lam"][~ref["active"]].any(), where
    for k, v in dev.items():
        assert v <= bound[k], (where, k, v)
    return dev


def qp_deviation(lam, ref):
    """|duals_to_reference_order(lam) - solve_qp's lam| on independent blocks, relative to grad_scale, per instance."""
    import biped_mpc_py_amd as bm
    n, h = lam.shape[:2]
    flat = bm.duals_to_reference_order(lam)
    d = np.abs(flat - ref["lam_qp"])[:, ref_index(h)]
    return np.where(ref["indep"], d, 0.0).reshape(n, -1).max(1) / np.maximum(ref["summary"][:, 3], np.finfo(float).tiny)


def batch_group(h):
    """Case 4: the batch of 200 of the gradient's batch test and its permutation."""
    from tests import eval_grad_cases as gc
    return gc.batch_group(h)


BATCH_POSITIONS = (0, 3, 77, 199)
