"""Cases, restatement and checks of the plant roll-out tests (TEST INFRASTRUCTURE: tests/test_plant_rollout_cpu.py,
tests/test_gpu_plant_rollout.py): S candidate plans per instance rolled out on the rigid body, restated in NumPy from
include/bmpc.h on tests/plant_model.py (`step`, the landing formula), tests/ground_cases.py (`transmit`, `reduce`) and
tests/body_cases.py (`outcome`), with the cost and the score.

A case is five instances at horizon h, one contact table of each kind -- leg 0 lands inside the horizon, leg 1 lands, a lift-off,
double support throughout, an alternating walk (both legs land and lift) -- with per-instance commands that take both branches of the
generated reference (a rate command that is zero, and one that is not), a push, a supplied reference, bodies and a ground.  The plans
are `sample_cases.sample_controls` around seeded controls: every fourth plan puts force on swing legs and pulls on the ground.

`restate(..., recorded=x_traj)` steps every period from the RECORDED fp32 state before it, with the footholds of the landing rule on
the recorded states, so that no error accumulates: the bound of a period is the plant tests' 2 fp32 ulps (both sides compute in fp64:
only the final rounding can differ, the second ulp is margin).  Everything that is a rule on stored values -- flags, ground
reductions, outcome, footholds -- is exact."""
import numpy as np

from tests import body_cases as bc
from tests import eval_cases as ec
from tests import ground_cases as gc
from tests import plant_model as pm
from tests import sample_cases as sc

N = 5                                  # (the tests run (B, S) = (1, 1), (5, 13) and (5, 67): 335 threads, a workgroup boundary inside an instance)
PUSH_FROM, PUSH_STEPS = 1, 2
W_FALL, W_SLIP, W_UNLOADED = 1e4, 2.5e2, 1e2
PER_SAMPLE = ("cost", "score", "x_end", "foot_end", "x_traj", "first_fall", "max_tilt", "min_z")
GROUND_ONLY = ("first_slip", "slip_periods", "unloaded_periods", "mu_demand")
REDUCED = ("best", "n_valid", "weights", "u_mean", "ess")


def contact_tables(h):
    """(5,h,2) uint8: leg 0 lands inside the horizon; leg 1 lands; leg 1 lifts off; double support; an alternating walk.  At h = 1
    there is no row to land in: the tables are their first rows."""
    k = np.arange(h)
    one = np.ones(h, bool)
    half = max(1, h // 3)
    walk = (k // half) % 2 == 0
    t = [(k >= max(1, h // 2), one), (one, k >= max(1, (h + 1) // 2)), (one, k < max(1, h // 3)), (one, one), (walk, ~walk)]
    return np.stack([np.stack(p, 1) for p in t]).astype(np.uint8)


def landings(contact):
    """(n,h,2) bool: leg g of the instance lands at the end of period k (bit 0 in row k, 1 in row k + 1; never in the last)."""
    c = np.asarray(contact) != 0
    out = np.zeros(c.shape, bool)
    out[:, :-1] = ~c[:, :-1] & c[:, 1:]
    return out


def case(h, seed=0):
    """The five instances at horizon h: dict(h, x_fb, foot, contact, x_cmd, controls (the nominal plan), push, x_ref, body, mu), fp32
    values in fp64 arrays where the entry takes fp32."""
    rng = np.random.default_rng(4100 + 10 * h + seed)
    r32 = ec.r32
    x_fb = r32(np.concatenate([rng.uniform(-0.1, 0.1, (N, 3)), rng.uniform(-0.5, 0.5, (N, 2)), rng.uniform(0.5, 0.6, (N, 1)),
                               rng.uniform(-0.3, 0.3, (N, 3)), rng.uniform(-0.3, 0.3, (N, 3))], 1))
    foot = np.zeros((N, 6))
    for g, sgn in enumerate((1.0, -1.0)):
        foot[:, 3 * g] = x_fb[:, 3] - 0.0195 + rng.uniform(-0.05, 0.05, N)
        foot[:, 3 * g + 1] = x_fb[:, 4] + sgn * (0.089 + rng.uniform(-0.03, 0.03, N))
    x_cmd = np.tile(np.array([0, 0, 0, 0, 0, 0.55, 0, 0, 0, 0, 0, 0.0]), (N, 1))
    x_cmd[:, 9] = rng.uniform(-0.5, 0.5, N)          # a velocity command: the x reference ramps
    x_cmd[::2, 8] = rng.uniform(-0.4, 0.4, len(x_cmd[::2]))        # a yaw rate on every other instance
    x_cmd[:, 3] = rng.uniform(-0.2, 0.2, N)          # (read by the landing rule)
    contact = contact_tables(h)
    controls = ec.seeded_controls(contact, rng)
    push = np.zeros((N, 6))
    push[::2, 1], push[::2, 3] = 40.0, 2.0
    x_ref = np.zeros((N, h, 12))
    x_ref[:, :, :] = x_fb[:, None, :]
    x_ref += rng.uniform(-0.05, 0.05, x_ref.shape)
    body = bc.bodies(N, seed=41 + h)
    mu = gc.grounds(N, seed=23 + h)
    return dict(h=h, x_fb=x_fb, foot=r32(foot), contact=contact, x_cmd=r32(x_cmd), controls=controls, push=r32(push), x_ref=r32(x_ref),
                body=body, mu=mu)


def plans(c, S, seed=7):
    """(5,S,h,12) fp32: `sample_cases.sample_controls` around the case's nominal plan."""
    return sc.sample_controls(c, S, seed).astype(np.float32)


def variant(c, name):
    """The keyword arguments of one of the variants the tests run -- `plain`: none of the options; `full`: per-instance commands, a
    push, bodies, a ground, supplied references -- beyond x_fb, foot, contact and controls."""
    if name == "plain":
        return {}
    assert name == "full"
    return dict(x_cmd=c["x_cmd"], x_ref=c["x_ref"], push=c["push"], push_from=PUSH_FROM, push_steps=PUSH_STEPS, body=c["body"],
                ground=dict(mu=c["mu"]))


def take(kw, idx):
    """The keyword arguments for instances idx alone."""
    out = {}
    for k, v in kw.items():
        if k == "body":
            out[k] = {m: np.ascontiguousarray(a[idx]) for m, a in v.items()}
        elif k == "ground":
            out[k] = {m: np.ascontiguousarray(a[idx]) for m, a in v.items()}
        elif isinstance(v, np.ndarray):
            out[k] = np.ascontiguousarray(v[idx])
        else:
            out[k] = v
    return out


def params_of(cp):
    """What the restatement reads of a `bmpc_params` block."""
    return dict(h=int(cp.h), dt=float(cp.dt), kv=float(cp.kv), Q=np.array(cp.Q[:12]), R=np.array(cp.R[:12]), x_cmd=np.array(cp.x_cmd[:12]),
                mu=float(cp.mu))


def references(p, x_fb, x_cmd=None, x_ref=None):
    """(n,h,12) fp64: the supplied rows (fp32 values), else generated by the rule of include/bmpc.h (REF:61-70) in fp64 without
    contraction: row 0 is x_fb; row k > 0 of entry i < 6 is x_fb[i] + x_cmd[i + 6] (k dt) where that rate is not zero, else
    x_cmd[i]; of entry i >= 6 it is x_cmd[i]."""
    if x_ref is not None:
        return np.asarray(x_ref, np.float32).astype(np.float64)
    x0 = np.asarray(x_fb, np.float32).astype(np.float64)
    n, h = x0.shape[0], p["h"]
    xc = np.tile(p["x_cmd"], (n, 1)) if x_cmd is None else np.asarray(x_cmd, np.float32).astype(np.float64)
    xr = np.empty((n, h, 12))
    for k in range(h):
        if k == 0:
            xr[:, 0] = x0
            continue
        xr[:, k, 6:] = xc[:, 6:]
        kdt = np.float64(k) * np.float64(p["dt"])
        xr[:, k, :6] = np.where(xc[:, 6:] != 0.0, x0[:, :6] + xc[:, 6:] * kdt, xc[:, :6])
    return xr


def land(p, x, foot, lands, cmd):
    """The footholds (6,) float32 after the landing rule of one period: the legs with `lands` set get `plant_model.landing`'s
    target at the stored state x (fp32, widened), rounded to fp32; the others stay.  (The model's rule is driven by a gait: a
    period-2 schedule in which step 1 is swing and step 0 stance for a leg with offset 0 -- it lands -- and a leg with offset 1 is in
    stance at step 1 -- it does not.)"""
    if not np.any(lands):
        return foot
    f2, _ = pm.landing(np.asarray(x, np.float32).astype(np.float64), foot, 1, 0, period=2, offset=tuple(0 if l else 1 for l in lands),
                       duty=(1, 1), h=p["h"], dt=p["dt"], kv=p["kv"], cmd=(cmd[3], cmd[4]))
    with np.errstate(invalid="ignore"):
        return f2.astype(np.float32)


def footholds(p, foot, contact, x_traj, x_cmd=None, move_feet=True):
    """(B,S,h,6) float32: the footholds every period of a recorded x_traj (B,S,h,12) STARTS with, by the landing rule on the recorded
    states."""
    B, S, h = x_traj.shape[:3]
    lands = landings(np.asarray(contact).reshape(B, h, 2))
    cmd = np.tile(p["x_cmd"], (B, 1)) if x_cmd is None else np.asarray(x_cmd, np.float32).astype(np.float64)
    out = np.empty((B, S, h, 6), np.float32)
    for b in range(B):
        for s in range(S):
            fs = np.asarray(foot, np.float32)[b]
            for k in range(h):
                out[b, s, k] = fs
                if move_feet:
                    fs = land(p, x_traj[b, s, k], fs, lands[b, k], cmd[b])
    return out


def spread_plans(c, S, seed=11):
    """(5,S,h,12) fp32 plans whose largest friction demand is spread over two orders of magnitude, so that a friction at half its
    median has plans on both sides: the nominal plan with its tangential forces taken out, plus `sample_cases.sample_controls`' noise
    at the levels 0.02, 0.1, 0.5 and 2.5 in turn (sample s at level s % 4)."""
    levels = (0.02, 0.1, 0.5, 2.5)
    nominal = np.array(c["controls"], float)
    nominal[:, :, [0, 1, 3, 4]] = 0.0
    sets = [sc.sample_controls(dict(c, controls=nominal), -(-S // 4), seed + i, noise=lv) for i, lv in enumerate(levels)]
    out = np.empty((N, S) + sets[0].shape[2:], np.float32)
    for s_ in range(S):
        out[:, s_] = sets[s_ % 4][:, s_ // 4]
    return out


def restate(p, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4", substeps=4,
            move_feet=True, body=None, ground=None, fall=(np.inf, -np.inf), fz_floor=0.0, w_fall=0.0, w_slip=0.0, w_unloaded=0.0,
            recorded=None):
    """The roll-out of include/bmpc.h in NumPy.  Free-running (every period from the restatement's own stored fp32 state), or with
    `recorded` = x_traj (B,S,h,12) float32 every period from the recorded state before it and the footholds of the rule on the
    recorded states.  Returns dict: x_model (B,S,h,12) fp64, what the model makes of each period BEFORE the rounding to fp32; x_traj
    (the states the periods started from, shifted: the recorded array, or the model's rounded); foot_end; u_applied (B,S,h,12),
    flags, demand (B,S,h) and `scaled`; the outcome and the ground's reductions of the x_traj / flags; cost (in long double from
    x_traj), score."""
    h, dt = p["h"], p["dt"]
    U = np.asarray(controls, np.float32)
    B, S = U.shape[:2]
    x_fb, foot = np.asarray(x_fb, np.float32), np.asarray(foot, np.float32)
    con = np.asarray(contact).reshape(B, h, 2) != 0
    lands = landings(con)
    mu = None if ground is None else (np.full((B, 2), p["mu"]) if ground.get("mu") is None else np.asarray(ground["mu"], np.float64))
    cmd = np.tile(p["x_cmd"], (B, 1)) if x_cmd is None else np.asarray(x_cmd, np.float32).astype(np.float64)
    body = body or {}
    xm = np.full((B, S, h, 12), np.nan)
    xt = np.empty((B, S, h, 12), np.float32)
    ua = np.empty((B, S, h, 12), np.float32)
    flags, demand = np.zeros((B, S, h), np.uint8), np.full((B, S, h), np.nan, np.float32)
    scaled = np.zeros((B, S, h, 12), bool)
    foot_end = np.empty((B, S, 6), np.float32)
    for b in range(B):
        kw = bc.plant_kw(body, b)
        for k in range(h):
            if mu is None:
                ua[b, :, k] = U[b, :, k]
            else:
                ua[b, :, k], flags[b, :, k], demand[b, :, k], scaled[b, :, k] = gc.transmit(U[b, :, k], np.tile(con[b, k], (S, 1)),
                                                                                           np.tile(mu[b], (S, 1)), fz_floor)
        for s in range(S):
            xs, fs = x_fb[b], foot[b].copy()
            for k in range(h):
                w = push[b] if push is not None and push_from <= k < push_from + push_steps else None
                xm[b, s, k] = pm.step(xs, ua[b, s, k], fs, con[b, k], w, integrator=integrator, substeps=substeps, dt=dt, **kw)
                xt[b, s, k] = xm[b, s, k].astype(np.float32) if recorded is None else recorded[b, s, k]
                xs = xt[b, s, k]
                if move_feet:
                    fs = land(p, xs, fs, lands[b, k], cmd[b])
            foot_end[b, s] = fs
    out = dict(x_model=xm, x_traj=xt, x_end=xt[:, :, -1], foot_end=foot_end, u_applied=ua, flags=flags, demand=demand, scaled=scaled)
    flat = xt.reshape(B * S, h, 12).transpose(1, 0, 2)
    first, mt, mz = bc.outcome(flat, fall[0], fall[1])
    out.update(first_fall=first.reshape(B, S), max_tilt=mt.reshape(B, S), min_z=mz.reshape(B, S))
    if mu is not None:
        fs_, sl, un, md = gc.reduce(flags.reshape(B * S, h).T, demand.reshape(B * S, h).T)
        out.update(first_slip=fs_.reshape(B, S), slip_periods=sl.reshape(B, S, 2), unloaded_periods=un.reshape(B, S, 2),
                   mu_demand=md.reshape(B, S))
    out["cost"] = cost_of(p, xt, U, references(p, x_fb, x_cmd, x_ref))
    out["score"] = score_of(out["cost"], out, w_fall, w_slip, w_unloaded)
    return out


def cost_of(p, x_traj, controls, xr):
    """sum_k sum_i Q_i (x - xr)^2 + R_i u^2 of stored states (B,S,h,12) fp32, commands (B,S,h,12) fp32 and reference rows (B,h,12)
    fp64, accumulated in long double (64 mantissa bits: its own error is 2^-11 of the fp64 bound's), returned as fp64."""
    L = np.longdouble
    e = x_traj.astype(L) - xr.astype(L)[:, None]
    u = np.asarray(controls, np.float32).astype(L)
    with np.errstate(all="ignore"):
        terms = p["Q"].astype(L) * e * e + p["R"].astype(L) * u * u
        return terms.reshape(terms.shape[0], terms.shape[1], -1).sum(2).astype(np.float64)


def cost_bound(h):
    """Relative bound of the kernel's fp64 cost against `cost_of`: non-negative terms added in a fixed order, 24 h + 4 roundings."""
    return (24 * h + 4) * 2.0 ** -52


def score_of(cost, res, w_fall, w_slip, w_unloaded):
    """cost + w_fall [first_fall >= 0] + w_slip (slips) + w_unloaded (unloaded), in that order; the ground's terms only with one."""
    s = np.asarray(cost, np.float64) + w_fall * (res["first_fall"] >= 0)
    if "slip_periods" in res and res["slip_periods"] is not None:
        s = s + w_slip * res["slip_periods"].sum(-1).astype(np.float64)
        s = s + w_unloaded * res["unloaded_periods"].sum(-1).astype(np.float64)
    return s


def check(p, res, args, kw, where, with_ground=None):
    """Everything per sample of a result `res` (NumPy arrays) against the restatement from its own recorded x_traj.  Prints the
    figures, then asserts: x_traj within 2 fp32 ulps of the model per period; foot_end, the outcome and the ground's reductions
    equal to their rules on the recorded values; cost within cost_bound(h); score within sample_cases.SCORE_REL.  Returns the
    restatement."""
    ref = restate(p, *args, **kw, recorded=res["x_traj"])
    good = np.isfinite(ref["x_model"]).all(-1)
    d = pm.ulp_diff(res["x_traj"], ref["x_model"])
    landed = ref["foot_end"] != np.asarray(args[1], np.float32)[:, None, :]
    same_foot = np.array_equal(res["foot_end"].view(np.uint32), ref["foot_end"].view(np.uint32))
    with np.errstate(all="ignore"):
        dfoot = np.abs(res["foot_end"].astype(np.float64) - ref["foot_end"]) / np.spacing(np.abs(ref["foot_end"])).astype(np.float64)
        dfoot = np.where(np.isnan(res["foot_end"]) & np.isnan(ref["foot_end"]), 0.0, dfoot)
        dcost = np.abs(res["cost"] - ref["cost"]) / np.abs(ref["cost"])
        dscore = np.abs(res["score"] - ref["score"]) / np.abs(ref["score"])
    fin = np.isfinite(ref["cost"])
    print("rollout", where, f"x_traj max ulps={d.max():.3f} foot_end bits equal={same_foot} (max ulps {np.nanmax(dfoot):.3f}, "
          f"{int(landed.sum())} landed coordinates) cost rel={dcost[fin].max() if fin.any() else 0:.3e} (bound {cost_bound(p['h']):.3e}) "
          f"score rel={dscore[fin].max() if fin.any() else 0:.3e} valid={int(fin.sum())}/{fin.size}")
    assert d.max() <= 2.0, (where, d.max())
    assert np.array_equal(np.isnan(res["x_traj"]).all(-1), ~good) and np.array_equal(np.isnan(res["x_traj"]).any(-1), ~good), where
    assert np.array_equal(res["x_end"].view(np.uint32), res["x_traj"][:, :, -1].view(np.uint32)), where
    assert (dfoot[~landed] == 0).all() and (dfoot <= 1.0).all(), (where, dfoot.max())
    for k in ("first_fall", "max_tilt", "min_z") + (GROUND_ONLY if "first_slip" in ref else ()):
        assert res[k].dtype == ref[k].dtype and np.array_equal(res[k], ref[k], equal_nan=True), (where, k)
    assert np.array_equal(np.isnan(res["cost"]), ~fin) and np.array_equal(np.isnan(res["score"]), ~fin), where
    assert (dcost[fin] <= cost_bound(p["h"])).all(), (where, dcost[fin].max())
    own = score_of(res["cost"], res, kw.get("w_fall", 0.0), kw.get("w_slip", 0.0), kw.get("w_unloaded", 0.0))
    with np.errstate(all="ignore"):
        down = np.abs(res["score"] - own) / np.abs(own)
    assert (down[fin] <= sc.SCORE_REL).all() and (dscore[fin] <= sc.SCORE_REL + cost_bound(p["h"])).all(), (where, down[fin].max())
    return ref
