"""Case sets, references and bounds of the sampling tests (tests/test_evaluate_samples_cpu.py, tests/test_gpu_evaluate_samples.py),
built on tests/eval_cases.py: its groups, its `seeded_controls` and `breaking_controls`, its yardstick.

A sample set of a group g is an array (n,S,h,12): sample s of instance b is the group's controls plus seeded noise, rounded to fp32;
every fourth sample (s % 4 == 3) goes through `breaking_controls`, so that the violation prices matter.  A set for fewer instances
or samples is a slice of the (n, S_MAX) set: a reference computed for the large set serves the small ones."""
import numpy as np

from tests import eval_cases as ec
from tests import refs_cases as rc

HORIZONS = (1, 3, 10, 20, 33)          # lane groups of 16, 32 and 64, idle lanes past the horizon
W_VIOL = (1e3, 2e3, 5e2, 1.5e3)        # prices of the four violation classes in the tests that price them
# standard deviation of the noise relative to `seeded_controls`' own (8 N vertical, 6 N tangential, 1.5 N m).  Chosen on the
# REFERENCE's side: at the batch-median temperature the NumPy weights must have 1.5 <= ess <= S - 0.5 for every instance.
NOISE = 0.5

SCORE_REL = 2.0 ** -49                 # score against cost + sum w v recomputed: non-negative terms, at most eight roundings


def reduce_bound(S):
    """Relative bound of weights and ess (absolute, times max |controls|, of u_mean) against NumPy on the same scores: an exp within
    a couple of ulps and a sum of S non-negative terms in any order."""
    return (S + 8) * 2.0 ** -52


def horizon_group(h, supplied, n=5):
    """n instances (refs_cases.make_case kinds a-e) at horizon h with supplied or generated references and seeded controls, as
    eval_cases.horizon_groups builds them (h = 1: the first step of an h = 3 instance)."""
    rng = np.random.default_rng(900 + h)
    cases = [rc.make_case(k, max(h, 3), rng) for k in "abcde"[:n]]
    half = max(1, h // 2) if h > 1 else 1
    if h == 1:
        cases = [c | dict(contact=c["contact"][:1], x_ref=c["x_ref"][:, :1], foot_ref=c["foot_ref"][:, :1], phase=0) for c in cases]
    st = lambda k: np.stack([np.asarray(c[k]) for c in cases])
    U = ec.seeded_controls(st("contact"), rng)
    return ec._group(h, half, None, st("x_fb"), st("foot"), st("contact"), st("phase"), st("x_cmd"), U,
                     x_ref=st("x_ref") if supplied else None, foot_ref=st("foot_ref") if supplied else None,
                     name=f"samples_h{h}_" + ("supplied" if supplied else "generated"))


def mu_group(n=3):
    """The first n instances of eval_cases' per-step-mu walking batch (h = 20, generated references)."""
    g = ec.generated_groups()[-1]
    assert g["mu"] is not None and g["h"] == 20
    return take(g, range(n))


def take(g, idx):
    """Instances idx of group g, as a group."""
    idx = np.asarray(list(idx))
    out = dict(g)
    for k in ("x_fb", "foot", "contact", "phase", "x_cmd", "controls", "mu", "x_ref", "foot_ref"):
        out[k] = None if g[k] is None else np.asarray(g[k])[idx]
    return out


def sample_controls(g, S, seed=7, noise=NOISE):
    """(n,S,h,12) fp32 values in fp64: the group's controls plus seeded noise on the legs in stance (scaled as
    `seeded_controls` scales its own), every fourth sample through `breaking_controls`."""
    U = np.asarray(g["controls"], float)
    n, h, _ = U.shape
    c = np.asarray(g["contact"], float)
    out = np.empty((n, S, h, 12))
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        d = np.zeros_like(U)
        for leg in range(2):
            on = c[:, :, leg]
            d[:, :, 3 * leg + 2] = on * rng.normal(0, 8.0 * noise, (n, h))
            d[:, :, 3 * leg + 0] = on * rng.normal(0, 6.0 * noise, (n, h))
            d[:, :, 3 * leg + 1] = on * rng.normal(0, 6.0 * noise, (n, h))
            d[:, :, 6 + 3 * leg: 9 + 3 * leg] = on[:, :, None] * rng.normal(0, 1.5 * noise, (n, h, 3))
        Us = ec.r32(U + d)
        out[:, s] = ec.breaking_controls(Us, 1000 * seed + s) if s % 4 == 3 else Us
    return out


def replicated(g, controls):
    """The group of n S instances that holds instance b of g once per sample, with that sample's plan as its controls: what a caller
    without the operation has to build."""
    n, S = controls.shape[:2]
    out = dict(g)
    for k in ("x_fb", "foot", "contact", "phase", "x_cmd", "mu", "x_ref", "foot_ref"):
        out[k] = None if g[k] is None else np.repeat(np.asarray(g[k]), S, axis=0)
    out["controls"] = controls.reshape((n * S,) + controls.shape[2:])
    return out


def sample_args(g, controls, idx=None, unchecked=False):
    """The arguments of `BatchSolver.evaluate_samples` / `emu_samples.evaluate_samples` for (instances idx of) group g with the
    sample set `controls` (n,S,h,12); `unchecked`: references without the finiteness check (spoiled batches)."""
    a = ec.kernel_args_unchecked(g) if unchecked else ec.kernel_args(g)
    sl = slice(None) if idx is None else idx
    a = {k: None if v is None else v[sl] for k, v in a.items()}
    a["controls"] = controls[sl]
    return a


def as_instances(res):
    """cost (B,S) and violation (B,S,4) of a sampling result as the dict `eval_cases.check` takes for B S instances; the outputs
    the sampling operation does not have (objective, states) are taken from the reference by the caller."""
    return dict(cost=res["cost"].reshape(-1), violation=res["violation"].reshape(-1, 4))


def check_per_sample(res, ref, where):
    """`eval_cases.check` on cost and violation of B S plans (bounds util.REL_TOL and eval_cases.REG_BOUND); objective and states,
    which the sampling operation does not return, are compared with themselves."""
    got = as_instances(res)
    pick = {k: ref[k] for k in ("objective", "states")}
    return ec.check(dict(got, **pick), ref, where)


def score_reference(cost, violation, w_viol):
    s = np.array(cost, float)
    for c in range(4):
        s = s + w_viol[c] * violation[..., c]
    return s


def reduce_reference(score, controls, temperature):
    """NumPy's n_valid, best, weights, u_mean, ess of scores (B,S) and plans (B,S,h,12) by the rules of include/bmpc.h."""
    score = np.asarray(score, float)
    B, S = score.shape
    valid = np.isfinite(score)
    n_valid = valid.sum(1).astype(np.int32)
    masked = np.where(valid, score, np.inf)
    best = np.where(n_valid > 0, np.argmin(masked, 1), -1).astype(np.int32)
    m = np.where(n_valid > 0, masked.min(1), 0.0)
    with np.errstate(all="ignore"):
        e = np.where(valid, np.exp(-(np.where(valid, score, 0.0) - m[:, None]) / temperature), 0.0)
        tot = e.sum(1)
        w = np.where(valid, e / tot[:, None], 0.0)
        u = np.where(valid[:, :, None, None], np.asarray(controls, float), 0.0)
        u_mean = np.einsum("bs,bshi->bhi", w, u)
        ess = 1.0 / (w * w).sum(1)
    u_mean[n_valid == 0] = np.nan
    ess[n_valid == 0] = np.nan
    return dict(n_valid=n_valid, best=best, weights=w, u_mean=u_mean, ess=ess)


def check_reduced(res, controls, temperature, where):
    """The reduced outputs of `res` against NumPy on the kernel's own `score`: best and n_valid exact; weights and ess relative
    `reduce_bound(S)`; u_mean absolute that times the instance's largest finite |control|.  Prints the maxima first."""
    S = res["score"].shape[1]
    ref = reduce_reference(res["score"], controls, temperature)
    tol = reduce_bound(S)
    assert np.array_equal(res["n_valid"], ref["n_valid"]), (where, res["n_valid"], ref["n_valid"])
    assert np.array_equal(res["best"], ref["best"]), (where, res["best"], ref["best"])
    ok = ref["n_valid"] > 0
    with np.errstate(all="ignore"):
        dw = np.abs(res["weights"] - ref["weights"]) / np.where(ref["weights"] > 0, ref["weights"], 1.0)
        de = np.abs(res["ess"][ok] - ref["ess"][ok]) / ref["ess"][ok]
        umax = np.nanmax(np.where(np.isfinite(controls), np.abs(controls), np.nan).reshape(controls.shape[0], -1), 1)
        du = np.abs(res["u_mean"][ok] - ref["u_mean"][ok]).reshape(int(ok.sum()), -1).max(1) / umax[ok] if ok.any() else np.zeros(0)
    print("sample reductions", where, f"T={temperature:.3e} weights={dw.max():.3e} ess={de.max() if de.size else 0:.3e} "
          f"u_mean={du.max() if du.size else 0:.3e} bound={tol:.3e}")
    assert not np.signbit(res["weights"]).any() and (res["weights"][~np.isfinite(res["score"])] == 0).all(), where
    assert dw.max() <= tol and (de <= tol).all() and (du <= tol).all(), (where, dw.max(), de, du)
    assert np.isnan(res["ess"][~ok]).all() and np.isnan(res["u_mean"][~ok]).all(), where
    return ref


def temperatures(score):
    """The three temperatures of the reduction tests from scores (B,S): +inf, the batch median of (score - min over the instance's
    valid samples) over the valid samples, and 1e-6 of that median."""
    valid = np.isfinite(score)
    gap = score - np.where(valid, score, np.inf).min(1, keepdims=True)
    med = float(np.median(gap[valid]))
    assert med > 0
    return float("inf"), med, 1e-6 * med
