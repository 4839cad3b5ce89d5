"""Stop cases (TEST INFRASTRUCTURE): the SOLVER's knobs, caps and self-report held to what include/bmpc.h says of them, as
tests/param_cases.py holds the model's parameters.  ONE table of cases for the CPU emulation (tests/test_stop_cases_cpu.py) and for
the device (tests/test_gpu_stop_cases.py).

The reference of a capped solve is the NumPy model of the product's algorithm, `oracle/ws_model.solve_batch(..., dtype=np.float32,
res_dtype=np.float64, iters=n)`, run on the parameter block through `model_params` -- the one adaptor from a `bmpc_params` block to
`ws.Params`.  The tolerance of a case comes from the reference ALONE (`cap_reference`): per instance 1/20 of the smaller of the
model's distances from its N-th iterate to its (N - 1)-th and (N + 1)-th (util.rel_err) -- a kernel one iteration off is 20 x the
bound away --, and the case is admissible only if that is at least 10 x the model's own distance between fp32 and fp64 factors at
N: what the number formats leave open is a tenth of the bound.  A knob case must also be able to FAIL: the model at the knob's
default and at its changed value differ by more than the bound on every instance (`knob_distance`)."""
import ctypes as C
import functools

import numpy as np

from tests import param_cases as pc
from tests import util

PATH_DENSE, PATH_STAGE = 1, 2
FAMILY = {PATH_DENSE: "dense", PATH_STAGE: "stage"}
TOL_FRACTION = 20.0                  # the bound: this fraction of the distance to the neighbouring iterate
ADMISSIBLE = 10.0                    # ... and at least this many times the model's fp32-against-fp64 distance
SLOW_GUARD = 1e-6                    # SLOW_TOL of the kernels (bmpc_host_params.hpp), `slow_guard` of the model

r32 = lambda a: None if a is None else np.asarray(a, float).astype(np.float32).astype(float)


def block(path, h, half, name="default", **opts):
    """The `bmpc_params` block of parameter case `name` (tests/param_cases.py) at horizon h on family `path` with solver options."""
    import biped_mpc_py_amd as bm
    mpc, biped = pc.objects(bm, name, h=h)
    return bm.pack_params(mpc, biped, half=half, solver_options=dict(path=path, **opts))


def effective(cp):
    """The five penalties (rho, rho_eq, rho_lo, rho_hi_f, rho_hi_m) block cp resolves to: `bmpc_effective_penalties` (host arithmetic)."""
    from biped_mpc_py_amd import _lib
    out = (C.c_double * 5)()
    _lib.check(_lib.load().bmpc_effective_penalties(C.byref(cp), out))
    return list(out)


def model_params(cp, eff=None, **over):
    """`ws.Params` of the block `cp`: the model's parameters from the block's fields, the five penalties as the library resolves them
    (`eff`: what `bmpc_effective_penalties` / `emu.dev_params` report; asked of the library if None), every solver knob, the third
    stopping test at the kernels' 1e-6, the Riccati factorisation on the stage family.  `over`: attributes set last (kernel_schedule)."""
    from oracle import ws_model as ws
    eff = effective(cp) if eff is None else list(eff)
    P = ws.Params(h=int(cp.h), half=int(cp.half))
    P.dt, P.kv, P.m, P.g, P.mu = float(cp.dt), float(cp.kv), float(cp.m), float(cp.g), float(cp.mu)
    P.x_cmd = np.array(cp.x_cmd[:12], float)
    P.Q = np.array(cp.Q[:12], float)
    P.R = np.array(cp.R[:12], float)
    P.I = np.array(cp.I[:9], float).reshape(3, 3)
    P.lt, P.lh = float(cp.lt) - 0.01, float(cp.lh) - 0.02           # REF:254-255, as make_dev_params applies them
    for k in ("f_max", "f_min", "tau_max", "tau_min"):
        setattr(P, k, np.array(getattr(cp, k)[:3], float))
    P.rho, P.rho_eq_scale, P.rho_lo, P.rho_hi_f, P.rho_hi_m = eff[0], eff[1] / eff[0], eff[2], eff[3], eff[4]
    for k in ("adapt_start", "adapt_every", "adapt_early", "adapt_late", "adapt_busy", "adapt_flips", "confirm_from", "max_iter",
              "check_every", "max_refactor"):
        setattr(P, k, int(getattr(cp, k)))
    for k in ("kappa", "kappa_confirm", "alpha", "eps_pri", "eps_dua"):
        setattr(P, k, float(getattr(cp, k)))
    P.accel = bool(cp.accel) and not no_accel(int(cp.path), int(cp.h))
    P.slow_guard = SLOW_GUARD
    P.want_residuals = True
    P.solver = "riccati" if int(cp.path) == PATH_STAGE else "dense"
    for k, v in over.items():
        setattr(P, k, v)
    return P


def no_accel(path, h):
    """The kernels that ignore `accel` (include/bmpc.h: no LDS / registers for it): the dense one of h = 12, the stage ones whose lanes
    own five steps (one wave, h = 21 .. 24)."""
    return (path == PATH_DENSE and h == 12) or (path == PATH_STAGE and 21 <= h <= 24)


def batch(h, B, seed):
    """B walking instances with a commanded v_x, rounded to the fp32 the ABI carries (the model reads what the kernel reads)."""
    s = util.synth_batch(B, h, seed, gait="walking", vx_cmd=True)
    return dict(s, x_fb=r32(s["x_fb"]), foot=r32(s["foot"]), x_cmd=r32(s["x_cmd"]), mu=r32(s["mu"]))


def model_solve(P, s, n=None, dtype=np.float32):
    """(states, controls, info) of the model on batch s: fp32 factors (or `dtype`), fp64 iterates; n iterations, or to convergence."""
    from oracle import ws_model as ws
    return ws.solve_batch(P, s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], mu=s["mu"], dtype=dtype,
                          res_dtype=np.float64, iters=n)


# ---- the cap returns the N-th iterate ------------------------------------------------------------------------------------------------
CAP_B = 3
# (family, h) -> the caps N.  The defaults re-classify at 5, 10, 15, 35 (h <= 12), 10, 20, 40 (h = 14 .. 18), 20, 40 (h = 20), 10, 20, 30
# (h > 20) and test every 5: the N lie before, at and after the first re-classifications, and most are no multiple of 5.
CAP_ROWS_CPU = {
    (PATH_DENSE, 10): (4, 5, 7, 12, 23), (PATH_DENSE, 16): (9, 13, 21), (PATH_DENSE, 20): (12, 20, 23),
    (PATH_STAGE, 7): (5, 13), (PATH_STAGE, 10): (4, 7, 10, 12, 23), (PATH_STAGE, 14): (10, 13), (PATH_STAGE, 22): (13,), (PATH_STAGE, 26): (12,),
}
# the device runs those and the variants the emulation does not build
CAP_ROWS_GPU_ONLY = {
    (PATH_DENSE, 12): (7, 16), (PATH_DENSE, 8): (5, 12), (PATH_DENSE, 18): (13, 21),
    (PATH_STAGE, 1): (3, 7), (PATH_STAGE, 33): (12,), (PATH_STAGE, 40): (11, 17),
}
# One knob at a time over dense h = 10 and stage h = 7: name -> (solver options, parameter case, N).  N is where the knob has acted:
# max_refactor = 2 withholds the factorisation of iteration 15 (the fourth), so N = 17; adapt_start = 3 moves every re-classification.
KNOBS = {
    "alpha_1.0": (dict(alpha=1.0), "default", 7),
    "adapt_every_0": (dict(adapt_every=0), "default", 12),
    "max_refactor_0": (dict(max_refactor=0), "default", 12),
    "max_refactor_2": (dict(max_refactor=2), "default", 17),
    "kappa_4": (dict(kappa=4.0), "default", 12),
    "adapt_start_3": (dict(adapt_start=3), "default", 7),
    "Q_x10": (dict(), "Q_x10", 12),                # an off-default block: the SCALED penalties pass through the adaptor
}
KNOB_ROWS = ((PATH_DENSE, 10), (PATH_STAGE, 7))
# check_every = 3 without the extrapolation moves no iterate (the tests only watch): the case runs -- N = 7 and 13 are no multiples of 3,
# iters and status must say so -- and the model at the default must give the SAME bits (asserted: tests/test_stop_cases_cpu.py)
WATCH_ONLY = {"check_every_3": (dict(check_every=3), "default", (7, 13))}


def cap_case(path, h, N, opts=None, name="default", accel=0, label=None):
    return dict(id="%s_h%d_N%d%s%s" % (FAMILY[path], h, N, "_accel" if accel else "", "_" + label if label else ""), path=path, h=h, N=N,
                opts=dict(opts or {}), name=name, accel=accel, label=label, B=CAP_B, seed=1900 + 10 * h + path)


def _rows(rows):
    return [cap_case(p, h, N) for (p, h), Ns in rows.items() for N in Ns]


def _knob_cases():
    out = [cap_case(p, h, N, opts, name, label=k) for (p, h) in KNOB_ROWS for k, (opts, name, N) in KNOBS.items()]
    return out + [cap_case(p, h, N, opts, name, label=k) for (p, h) in KNOB_ROWS for k, (opts, name, Ns) in WATCH_ONLY.items() for N in Ns]


CAP_CASES_CPU = _rows(CAP_ROWS_CPU) + _knob_cases()
CAP_CASES_GPU = CAP_CASES_CPU + _rows(CAP_ROWS_GPU_ONLY)


def case_block(c, **more):
    """The block of cap case c: its knobs, accel as the case says, max_iter = N; rescue off (a capped dense solve is the result)."""
    s = case_batch(c)
    return block(c["path"], c["h"], s["half"], c["name"], **{**dict(accel=c["accel"], max_iter=c["N"], rescue=0), **c["opts"], **more})


def case_batch(c):
    return batch(c["h"], c["B"], c["seed"])


@functools.lru_cache(maxsize=None)
def _cap_reference(key):
    c = _CASES_BY_ID[key]
    s, cp = case_batch(c), case_block(c)
    N = c["N"]
    sched = dict(kernel_schedule=True) if c["accel"] else {}
    run = lambda n, dtype=np.float32: model_solve(model_params(cp, max_iter=n, **sched), s, n, dtype)
    (_, um, im), (_, u, info), (_, up, ip) = run(N - 1), run(N), run(N + 1)
    _, u64, i64 = run(N, np.float64)
    near = np.minimum(util.rel_err(um, u), util.rel_err(up, u))
    # the residuals of the N-th iteration by the same rule, entry by entry: 1/20 of the distance to the neighbouring iterations',
    # admissible where that is 10 x the model's own fp32-against-fp64 distance (an entry at a turning point of its residual is not)
    res = info["residuals"]
    res_tol = np.minimum(np.abs(im["residuals"] - res), np.abs(ip["residuals"] - res)) / TOL_FRACTION
    res_ok = res_tol >= ADMISSIBLE * np.abs(i64["residuals"] - res)
    return dict(controls=u, n_factor=info["n_factor_used"].copy(), tol=near / TOL_FRACTION, near=near, own=util.rel_err(u64, u),
                residuals=res, res_tol=res_tol, res_ok=res_ok)


def cap_reference(c):
    """The model's N-th iterate of case c, its factorisation counts, and per instance: `near` (the smaller distance to the neighbouring
    iterates), `tol` = near / 20, `own` (fp64 factors against fp32 factors at N).  Computed once per case; nothing modifies it."""
    return _cap_reference(c["id"])


def admissible(c):
    r = cap_reference(c)
    return bool((r["tol"] >= ADMISSIBLE * r["own"]).all())


def knob_distance(c):
    """Per instance: util.rel_err between the model's N-th iterate at the case and at the knob's default (same inputs, same block
    otherwise; for a parameter case: the same block with the penalties the DEFAULT block resolves to -- what an adaptor that ignored
    the scaling would hand the model -- and, second, the default block altogether)."""
    s, N = case_batch(c), c["N"]
    sched = dict(kernel_schedule=True) if c["accel"] else {}
    if c["name"] != "default":
        cp = case_block(c)
        cd = case_block(dict(c, name="default"))
        a = model_solve(model_params(cp, eff=effective(cd)), s, N)[1]
        b = model_solve(model_params(cd), s, N)[1]
        ref = cap_reference(c)["controls"]
        return np.minimum(util.rel_err(a, ref), util.rel_err(b, ref))
    cd = case_block(dict(c, opts={}))
    return util.rel_err(model_solve(model_params(cd, **sched), s, N)[1], cap_reference(c)["controls"])


_CASES_BY_ID = {c["id"]: c for c in CAP_CASES_GPU}
assert len(_CASES_BY_ID) == len(CAP_CASES_GPU)


def check_cap(c, out, eval_states, where=""):
    """What a capped solve must report: status 1 and iters N on every instance, the model's factorisation counts, the model's N-th
    iterate within the case's tolerance, and states that are those of the returned controls (`eval_states`: `evaluate(...,
    want_states=True)` of them) to util.REL_TOL.  Prints the measured distances; returns the largest ratio distance / tolerance."""
    r = cap_reference(c)
    dist = util.rel_err(np.asarray(out["controls"], float), r["controls"])
    ds = util.rel_err(np.asarray(out["states"], float), np.asarray(eval_states, float))
    print("cap %-34s %s kernel-model %.2e  tol %.2e  (near %.2e, own %.2e)  ratio %.3f  states %.1e  nfactor %s" % (
        c["id"], where, dist.max(), r["tol"].min(), r["near"].min(), r["own"].max(), (dist / r["tol"]).max(), ds.max(), list(out["nfactor"])))
    assert (np.asarray(out["status"]) == 1).all(), out["status"]
    assert (np.asarray(out["iters"]) == c["N"]).all(), out["iters"]
    assert np.array_equal(np.asarray(out["nfactor"]), r["n_factor"]), (out["nfactor"], r["n_factor"])
    assert (dist <= r["tol"]).all(), (dist, r["tol"])
    assert ds.max() <= util.REL_TOL, ds
    # residuals[] are those of iteration N -- the test forced at the cap -- not of the last scheduled test before it
    dr = np.abs(np.asarray(out["residuals"], float) - r["residuals"])
    ok = r["res_ok"]
    print("    residuals: %d of %d entries admissible, largest distance / bound %.3f" % (ok.sum(), ok.size, (dr[ok] / r["res_tol"][ok]).max() if ok.any() else 0.0))
    assert (dr[ok] <= r["res_tol"][ok]).all(), (out["residuals"], r["residuals"], r["res_tol"])
    return float((dist / r["tol"]).max())


# ---- the extrapolation (accel = 1) against the model under the kernels' test schedule -------------------------------------------------
# The reference is the same model with `kernel_schedule` on (oracle/ws_model.py: first test of a cold start at 2 check_every, the FAR
# skip, the test forced at max_iter, no secant step on it; the stage family re-classifies on the extrapolated state).  The first
# secant step of a cold start is at the first test (iteration 10), so every N lies after it.  The kernels that ignore `accel`
# (`no_accel`) are rows of their own: there the model runs WITHOUT the step, and the case can fail because the model with it differs.
# STAGE FAMILY ONLY where a secant step is taken: the dense kernels sum the two secant sums over every lane, the lanes that clone a
# wave's last row included, so their gamma is not the model's <g - g', g> / |g - g'|^2 (dense h = 20, N = 12: 2.4e-3 from the model
# against a bound of 7e-4; docs/history_r19.md).  That disagreement is not closed, so no dense row that takes a secant step is here
# -- dense h = 12 (takes none, by documentation) and the dense `last_is_test` row (takes none, by the cap) are.
ACCEL_ROWS_CPU = {
    (PATH_STAGE, 7): (11, 13), (PATH_STAGE, 10): (13,), (PATH_STAGE, 14): (13,), (PATH_STAGE, 22): (13,), (PATH_STAGE, 26): (12,),
}
ACCEL_ROWS_GPU_ONLY = {
    (PATH_DENSE, 12): (13,), (PATH_STAGE, 24): (13,), (PATH_STAGE, 33): (12,), (PATH_STAGE, 40): (11,),
}
ACCEL_KNOBS = {"check_every_3": (dict(check_every=3), "default", 13)}        # tests at 6, 9, 12: other secant steps than at 10
ACCEL_KNOB_ROWS = ((PATH_STAGE, 7),)


def _accel_rows(rows):
    return [cap_case(p, h, N, accel=1) for (p, h), Ns in rows.items() for N in Ns]


# N = 10 is the first test of a cold start with a g' kept for it: the cap forbids the secant step there ("no secant step when
# it + 1 == max_iter"), and the case can fail because the model that takes it differs
LAST_IS_TEST = "last_is_test"
ACCEL_CASES_CPU = _accel_rows(ACCEL_ROWS_CPU) + [cap_case(p, h, N, opts, name, accel=1, label=k) for (p, h) in ACCEL_KNOB_ROWS
                                                 for k, (opts, name, N) in ACCEL_KNOBS.items()] \
    + [cap_case(p, h, 10, accel=1, label=LAST_IS_TEST) for (p, h) in KNOB_ROWS]
ACCEL_CASES_GPU = ACCEL_CASES_CPU + _accel_rows(ACCEL_ROWS_GPU_ONLY)
_CASES_BY_ID.update({c["id"]: c for c in ACCEL_CASES_GPU})


def accel_distance(c):
    """Per instance: util.rel_err between the model's N-th iterate of an accel = 1 case and what the OTHER answer to `accel` gives --
    the plain iterate where the kernel extrapolates, the extrapolated one where the kernel is documented to ignore the option."""
    s, cp, N = case_batch(c), case_block(c), c["N"]
    if c["label"] == LAST_IS_TEST:
        other = model_solve(model_params(cp, kernel_schedule=True, max_iter=N + 1), s, N)[1]       # (the step taken at iteration N)
    elif no_accel(c["path"], c["h"]):
        other = model_solve(model_params(cp, kernel_schedule=True, accel=True), s, N)[1]
    else:
        other = model_solve(model_params(cp, kernel_schedule=True, accel=False), s, N)[1]
    return util.rel_err(other, cap_reference(c)["controls"])


def assert_admissible_and_can_fail(c):
    """From the reference alone, per instance: the bound of case c (1/20 of the distance to the nearer neighbouring iterate) is at
    least 10 x the model's own fp32-against-fp64 distance, and at least one entry of `residuals` is admissible by the same rule; the
    knob of a knob case moves the model's iterate by more than the bound on every instance (a watch-only knob moves no bit, and its N
    is no multiple of its check_every); an accel case differs from the other answer to `accel` by more than the bound on at least one
    instance (the secant step of an instance can be small; check_cap holds EVERY instance to its bound, so one that moves fails)."""
    r = cap_reference(c)
    print("%-40s near %.2e tol %.2e own %.2e (tol / own %.0f), %d of %d residual entries admissible" % (
        c["id"], r["near"].min(), r["tol"].min(), r["own"].max(), (r["tol"] / r["own"]).min(), r["res_ok"].sum(), r["res_ok"].size))
    assert (r["tol"] > 0).all() and admissible(c), (r["tol"], r["own"])
    assert r["res_ok"].any(), (r["residuals"], r["res_tol"])
    assert c["N"] <= 40 and c["B"] <= 4
    if c["label"] in WATCH_ONLY and not c["accel"]:
        assert (knob_distance(c) == 0).all() and c["N"] % c["opts"]["check_every"] != 0
    elif c["label"] and c["label"] != LAST_IS_TEST:
        d = knob_distance(c)
        print("   knob moves the iterate by %.2e (%.0f x the bound)" % (d.min(), (d / r["tol"]).min()))
        assert (d > r["tol"]).all(), (d, r["tol"])
    if c["accel"]:
        d = accel_distance(c)
        print("   the other answer to accel is %.2e .. %.2e away (up to %.0f x the bound, %d of %d instances beyond it)" % (
            d.min(), d.max(), (d / r["tol"]).max(), (d > r["tol"]).sum(), d.size))
        assert (d > r["tol"]).any(), (d, r["tol"])


# ---- what a solve says about itself ---------------------------------------------------------------------------------------------------
REPORT_ROWS = ((PATH_DENSE, 10), (PATH_STAGE, 7))
EPS_SWAP = (1e-4, 1e-7)         # (loose, tight): chosen in the emulation, see test_swapped_tolerances_would_show
REPORT_CASES = {
    "defaults": dict(),
    "check_every_3": dict(check_every=3),
    "eps_pri_loose": dict(eps_pri=EPS_SWAP[0], eps_dua=EPS_SWAP[1]),
    "eps_dua_loose": dict(eps_pri=EPS_SWAP[1], eps_dua=EPS_SWAP[0]),
    "max_refactor_2": dict(max_refactor=2, max_iter=60),      # (plain ADMM once the budget is spent: some instances meet the cap)
    "alpha_1.0": dict(alpha=1.0),
    "capped_23": dict(max_iter=23),
    "capped_3": dict(max_iter=3),                      # below the first stopping test of a cold start: the forced one is the only one
    "adapt_every_0_capped": dict(adapt_every=0, max_iter=40),
    "max_refactor_0_capped": dict(max_refactor=0, max_iter=40),
}
REPORT_SEED = 4100


def report_batch(h, B):
    return batch(h, B, REPORT_SEED + h)


def report_block(path, h, half, name, **more):
    return block(path, h, half, rescue=0, **{**REPORT_CASES[name], **more})


def report_norms(cp, s, controls):
    """(||A u||_inf, ||u||_inf) per instance of returned controls (B,h,12): A of `ws.constraint_blocks` -- identity (box), friction,
    line-foot rows -- in fp64."""
    from oracle import ws_model as ws
    P = model_params(cp)
    u = np.asarray(controls, float)
    B, h = u.shape[0], int(cp.h)
    x = np.stack([np.concatenate([u[:, :, 3 * f:3 * f + 3], u[:, :, 6 + 3 * f:9 + 3 * f]], -1) for f in range(2)], 2)     # (B,h,2,6)
    mu = np.full((B, h, 2), P.mu) if s["mu"] is None else np.asarray(s["mu"], float)
    A, _, _ = ws.constraint_blocks(P, np.asarray(s["x_fb"], float), np.asarray(s["contact"]).reshape(B, h, 2), mu, np.float64)
    Au = np.einsum("bhfri,bhfi->bhfr", A, x)
    return np.abs(Au).reshape(B, -1).max(1), np.abs(x).reshape(B, -1).max(1)


def check_report(cp, s, out, where=""):
    """The contract of iters / nfactor / status / residuals (include/bmpc.h) on one solve.  Returns (ratio of the primal residual to
    its bound, of the step residual to its bound) per instance, bounds WITHOUT the 1 % -- for the swapped-eps condition."""
    it, nf, st = (np.asarray(out[k]).astype(int) for k in ("iters", "nfactor", "status"))
    res = np.asarray(out["residuals"], float)
    ce, mi, mr = int(cp.check_every), int(cp.max_iter), int(cp.max_refactor)
    nA, nu = report_norms(cp, s, out["controls"])
    bp, bd = float(cp.eps_pri) * np.maximum(1.0, nA), float(cp.eps_dua) * np.maximum(1.0, nu)
    print("report %-40s status %s iters %d..%d nfactor %d..%d ratio pri %.2f..%.2f dua %.2f..%.2f" % (
        where, np.bincount(st, minlength=3), it.min(), it.max(), nf.min(), nf.max(), (res[:, 0] / bp).min(), (res[:, 0] / bp).max(),
        (res[:, 1] / bd).min(), (res[:, 1] / bd).max()))
    assert np.isin(st, (0, 1)).all(), st
    assert (it >= 1).all() and (it <= mi).all(), it
    assert ((it % ce == 0) | (it == mi)).all(), (it, ce, mi)
    assert (nf >= 1).all() and (nf <= mr + 1).all(), (nf, mr)
    if int(cp.adapt_every) == 0 or mr == 0:
        assert (nf == 1).all(), nf
    ok = st == 0
    assert (res[ok, 0] <= 1.01 * bp[ok]).all() and (res[ok, 1] <= 1.01 * bd[ok]).all(), (res[ok], bp[ok], bd[ok])
    capped = st == 1
    assert ((it[capped] == mi) | (res[capped, 0] > 1.01 * bp[capped]) | (res[capped, 1] > 1.01 * bd[capped])).all()
    assert (it[capped] == mi).all()                    # (status 1 is the cap's alone)
    return res[:, 0] / bp, res[:, 1] / bd


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
BAD_B, BAD_I = 5, 2
BAD_ROWS = ((PATH_DENSE, 10), (PATH_STAGE, 7))
BAD_CASES = {"x_fb_nan": ("x_fb", (4,), np.nan), "x_fb_inf": ("x_fb", (7,), np.inf), "foot_nan": ("foot", (1,), np.nan),
             "foot_inf": ("foot", (3,), np.inf), "x_cmd_nan": ("x_cmd", (9,), np.nan), "mu_nan": ("mu", (0, 1), np.nan)}
OUT_KEYS = ("controls", "states", "iters", "nfactor", "residuals", "status")


def bad_batch(h):
    """The clean batch of 5 (walking, commanded v_x, per-step friction so that mu is an input)."""
    s = util.synth_batch(BAD_B, h, 5200 + h, gait="walking", vx_cmd=True, per_step_mu=True)
    return dict(s, x_fb=r32(s["x_fb"]), foot=r32(s["foot"]), x_cmd=r32(s["x_cmd"]), mu=r32(s["mu"]))


def poisoned(s, name):
    key, idx, val = BAD_CASES[name]
    t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    t[key][(BAD_I,) + idx] = val
    return t


def check_bad(clean, out, max_iter, where=""):
    st = np.asarray(out["status"])
    print("bad input %-28s status %s iters %s" % (where, list(st), list(np.asarray(out["iters"]))))
    assert st[BAD_I] == 2, st
    assert 0 <= int(out["iters"][BAD_I]) <= max_iter
    rest = [i for i in range(BAD_B) if i != BAD_I]
    assert (np.asarray(clean["status"])[rest] == 0).all()
    for k in OUT_KEYS:
        assert np.array_equal(np.asarray(out[k])[rest], np.asarray(clean[k])[rest]), (where, k)
