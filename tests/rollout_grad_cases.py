"""Cases, reference and checks of the roll-out gradient tests (TEST INFRASTRUCTURE: tests/test_plant_rollout_grad_cpu.py,
tests/test_gpu_plant_rollout_grad.py), written from the definition in include/bmpc.h, NumPy only.

`jacobians`: for every (plan, period) the 12 x 30 Jacobian dPhi/d(x, ua, r) of one control period, by complex-step differentiation
(delta = 1e-30: the imaginary part carries the derivative without any subtraction, so there is no step-size error) of the integrator
`tests/plant_model.step` restates, restated here for a complex dtype on `plant_model.rate`, which accepts complex input as it is
(`cstep`, `period_jacobian`).  To keep the suite quick the thirty steps of a Jacobian are integrated side by side
(`period_jacobian_columns` on `rate_columns`, which is `rate` line for line for n points), and every fifth plan's Jacobian of one
period is held to `period_jacobian` within COLUMNS_REL wherever `jacobians` runs.
The linearisation point is what the kernel has: the recorded x_traj, the footholds of `rollout_cases.footholds` on it, and u_applied as
`ground_cases.transmit` gives it (fp32).  The ground's Jacobian is a complex step of the unrounded rule at the command, on the
branch the flags name.

`gradient`: the adjoint recursion of include/bmpc.h in fp64, with the landing fold.

`self_check`: a free-running, unrounded fp64 roll-out with its cost in complex arithmetic: Im cost(U + i delta D, x0 + i delta d0,
foot + i delta df) / delta against <gradient, (D, d0, df)>, the gradient linearised at that unrounded trajectory.  It holds the
recursion, landing fold included, to the derivative of the functional, independently of the kernel.

Bounds.  GRAD_REL and SELF_REL are 10 x the largest figure measured (docs/history_r26.md): both sides are fp64 evaluations of the same
sums in different association, and device and host sincos and division differ by ulps.  The figure, per plan and output, is
max |delta| / max |reference| of that output; where the reference output is identically zero the other side must be +-0."""
import numpy as np

from tests import body_cases as bc
from tests import ground_cases as gc
from tests import plant_model as pm
from tests import rollout_cases as rc

DELTA = 1e-30
GRAD_REL = 3.6e-11     # 10 x 3.55e-12, the largest figure of the emulation and of the device against `gradient` (docs/history_r26.md)
SELF_REL = 4.6e-14     # 10 x 4.6e-15, the largest figure of `self_check`
GRAD_REL_MAX, SELF_REL_MAX = 1e-9, 1e-10      # above these something is wrong and is to be found, not widened
OUTPUTS = ("cost", "grad_u", "grad_x0", "grad_foot", "x_traj", "first_bad")
GRADS = ("grad_u", "grad_x0", "grad_foot")
SWING_COMMAND = np.array([1.5, -2.5, 4.0, 0.5, -0.25, 0.125], np.float32)      # force and moment put on a swing leg


def plans(c, S, seed=7):
    """(5,S,h,12) fp32: `rollout_cases.plans`, with two kinds of plan added by construction, since those plans hold neither (checked
    at h in {1, 4, 10}, S in {3, 13, 67}: no unloaded stance leg occurs, and swing legs carry force only in every fourth plan, from
    s = 3 on).  Plan s with s % 4 == 1: the fz of one stance leg in one period becomes negative -- an unloaded stance leg.  Plan s
    with s % 4 == 2: in the first period an instance has a swing leg in, that leg carries SWING_COMMAND."""
    U = rc.plans(c, S, seed).copy()
    con = np.asarray(c["contact"]) != 0
    n, h = con.shape[:2]
    for s in range(S):
        for b in range(n):
            if s % 4 == 1:
                k = (b + s // 4) % h
                legs = np.flatnonzero(con[b, k])
                g = legs[(b + s) % len(legs)]
                U[b, s, k, 3 * g + 2] = -(abs(U[b, s, k, 3 * g + 2]) + np.float32(1.0))
            if s % 4 == 2:
                swing = np.argwhere(~con[b])
                if len(swing):
                    k, g = swing[0]
                    U[b, s, k, 3 * g:3 * g + 3] = SWING_COMMAND[:3]
                    U[b, s, k, 6 + 3 * g:9 + 3 * g] = SWING_COMMAND[3:]
    return U


def kinds(c, U):
    """What the plans U (5,S,h,12) hold, counted over all of them under the case's ground: dict of counts of leg-periods (slip, hold,
    unloaded, swing_command), of landings per leg and of periods inside the push window."""
    con = np.asarray(c["contact"]) != 0
    n, S, h = U.shape[:3]
    out = dict(slip=0, hold=0, unloaded=0, swing_command=0)
    for b in range(n):
        for k in range(h):
            _, fl, _, _ = gc.transmit(U[b, :, k], np.tile(con[b, k], (S, 1)), np.tile(c["mu"][b], (S, 1)))
            for g in range(2):
                f = U[b, :, k, 3 * g:3 * g + 3].astype(np.float64)
                if con[b, k, g]:
                    assert (f[:, 2] != 0).all(), "a stance leg with fz == 0"
                    loaded = f[:, 2] > 0
                    assert (np.hypot(f[loaded, 0], f[loaded, 1]) != c["mu"][b, g] * f[loaded, 2]).all(), "a leg exactly on the cone"
                    out["slip"] += int(((fl >> g) & 1).sum())
                    out["unloaded"] += int(((fl >> (2 + g)) & 1).sum())
                    out["hold"] += int((loaded & (((fl >> g) & 1) == 0)).sum())
                else:
                    out["swing_command"] += int((np.abs(U[b, :, k, [3 * g, 3 * g + 1, 3 * g + 2, 6 + 3 * g, 7 + 3 * g, 8 + 3 * g]]) > 0).any(0).sum())
    lands = rc.landings(c["contact"])
    out["landings"] = (int(lands[:, :, 0].sum()), int(lands[:, :, 1].sum()))
    out["pushed"] = len([k for k in range(h) if rc.PUSH_FROM <= k < rc.PUSH_FROM + rc.PUSH_STEPS])
    return out


def build(h, S):
    """(case, plans (5,S,h,12) fp32, counts): `rollout_cases.case(h)` with `plans`, holding every kind of leg-period the gradient
    treats differently (asserted; no plan is dropped to meet it).  A landing of each leg and a period inside the push window are
    asserted for h >= 3: at h = 1 there is no row to land in, and the push window (from period 1) lies beyond the horizon."""
    c = rc.case(h)
    U = plans(c, S)
    n = kinds(c, U)
    assert n["slip"] >= 1 and n["hold"] >= 1 and n["unloaded"] >= 1 and n["swing_command"] >= 1, n
    if h >= 3:
        assert n["landings"][0] >= 1 and n["landings"][1] >= 1 and n["pushed"] >= 1, n
    return c, U, n


# ---- the period map and its Jacobian

def cstep(x, u, foot, con, w, integrator, substeps, dt, **kw):
    """`plant_model.step` for a complex dtype: the same scheme on `plant_model.rate` (no bad-instance handling: finite plans only)."""
    x = np.asarray(x, complex)
    w = np.zeros(6) if w is None else np.asarray(w, float)
    hs = dt / substeps
    f = lambda y: pm.rate(y, u, foot, con, w, **kw)[0]
    for _ in range(substeps):
        if integrator == "euler":
            x = x + hs * f(x)
        else:
            k1 = f(x)
            k2 = f(x + hs / 2 * k1)
            k3 = f(x + hs / 2 * k2)
            k4 = f(x + hs * k3)
            x = x + hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def period_jacobian(x, ua, foot, con, w, integrator, substeps, dt, **kw):
    """(12,30): dPhi/d(x (12), ua (12), r (6)) at the fp64 point, one complex step per column."""
    z = np.concatenate([x, ua, foot]).astype(complex)
    J = np.empty((12, 30))
    for q in range(30):
        zq = z.copy()
        zq[q] += 1j * DELTA
        J[:, q] = cstep(zq[:12], zq[12:24], zq[24:], con, w, integrator, substeps, dt, **kw).imag / DELTA
    return J


def rate_columns(X, U, F, con, w, I_b=pm.I_BODY, m=pm.MASS, g=pm.GRAV):
    """`plant_model.rate`, line for line, for n points at once: X (n,12), U (n,12), F (n,6) complex -> dx/dt (n,12).  The thirty
    complex steps of a Jacobian are thirty points of one call instead of thirty calls; `check_columns` holds it to `rate` itself."""
    e, p, om, v = X[:, 0:3], X[:, 3:6], X[:, 6:9], X[:, 9:12]
    cr, sr, cp, sp, cy, sy = np.cos(e[:, 0]), np.sin(e[:, 0]), np.cos(e[:, 1]), np.sin(e[:, 1]), np.cos(e[:, 2]), np.sin(e[:, 2])
    z, o = np.zeros_like(cr), np.ones_like(cr)
    mat = lambda rows: np.array(rows).transpose(2, 0, 1)
    R = mat([[cy, -sy, z], [sy, cy, z], [z, z, o]]) @ mat([[cp, z, sp], [z, o, z], [-sp, z, cp]]) @ mat([[o, z, z], [z, cr, -sr], [z, sr, cr]])
    I_w = R @ I_b @ R.transpose(0, 2, 1)
    e0d = (cy * om[:, 0] + sy * om[:, 1]) / cp
    e1d = -sy * om[:, 0] + cy * om[:, 1]
    e2d = om[:, 2] + sp * e0d
    tau, f = np.tile(np.array(w[3:6], complex), (len(X), 1)), np.tile(np.array(w[0:3], complex), (len(X), 1))
    for g_ in range(2):
        if con[g_]:
            fg, mg = U[:, 3 * g_:3 * g_ + 3], U[:, 6 + 3 * g_:9 + 3 * g_]
            tau = tau + np.cross(F[:, 3 * g_:3 * g_ + 3] - p, fg) + mg
            f = f + fg
    omd = np.linalg.solve(I_w, (tau - np.cross(om, (I_w @ om[:, :, None])[:, :, 0]))[:, :, None])[:, :, 0]
    vd = f / m + np.array([0, 0, -g])
    return np.concatenate([np.stack([e0d, e1d, e2d], 1), v, omd, vd], 1)


def period_jacobian_columns(x, ua, foot, con, w, integrator, substeps, dt, **kw):
    """`period_jacobian`, its thirty complex steps integrated side by side (`cstep`'s scheme on `rate_columns`)."""
    Z = np.tile(np.concatenate([x, ua, foot]).astype(complex), (30, 1)) + 1j * DELTA * np.eye(30)
    X, U, F = Z[:, :12], Z[:, 12:24], Z[:, 24:]
    w = np.zeros(6) if w is None else np.asarray(w, float)
    hs = dt / substeps
    f = lambda Y: rate_columns(Y, U, F, con, w, **kw)
    for _ in range(substeps):
        if integrator == "euler":
            X = X + hs * f(X)
        else:
            k1 = f(X)
            k2 = f(X + hs / 2 * k1)
            k3 = f(X + hs / 2 * k2)
            k4 = f(X + hs * k3)
            X = X + hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return X.imag.T / DELTA


def check_columns(J, p, xs, ua, feet, con, pushes, opts, kw, periods):
    """The largest |J[k] - period_jacobian(k)| / max |period_jacobian(k)| over `periods`: the side-by-side Jacobians against the ones
    computed column by column on `plant_model.rate`."""
    worst = 0.0
    for k in periods:
        ref = period_jacobian(xs[k], ua[k], feet[k], con[k], pushes[k], dt=p["dt"], **opts, **kw)
        worst = max(worst, float(np.abs(J[k] - ref).max() / np.abs(ref).max()))
    return worst


COLUMNS_REL = 1e-13    # the two evaluate the same expressions; matrix products and solves may associate differently by ulps


def ground_rule(u, con, mu, flags):
    """What the ground transmits of u (12,) -- any dtype, unrounded -- on the branch `flags` names."""
    ua = np.zeros(12, np.asarray(u).dtype)
    for g in range(2):
        if not con[g] or (flags >> (2 + g)) & 1:
            continue
        ua[3 * g:3 * g + 3] = u[3 * g:3 * g + 3]
        ua[6 + 3 * g:9 + 3 * g] = u[6 + 3 * g:9 + 3 * g]
        if (flags >> g) & 1:
            fx, fy, fz = u[3 * g:3 * g + 3]
            sc = mu[g] * fz / np.sqrt(fx * fx + fy * fy)
            ua[3 * g], ua[3 * g + 1] = fx * sc, fy * sc
    return ua


def ground_jacobian(u, con, mu, flags):
    """(12,12): d u_applied / d u by a complex step of `ground_rule` at the command."""
    J = np.empty((12, 12))
    for q in range(12):
        uq = np.asarray(u, np.float64).astype(complex)
        uq[q] += 1j * DELTA
        J[:, q] = ground_rule(uq, con, mu, flags).imag / DELTA
    return J


def ground_flags(u, con, mu):
    """The flags of the rule on fp64 values (`ground_cases.transmit`'s, without the rounding)."""
    fl = 0
    for g in range(2):
        if not con[g]:
            continue
        fx, fy, fz = (float(v) for v in u[3 * g:3 * g + 3])
        if not fz > 0:
            fl |= gc.UNLOADED << g
        elif np.sqrt(fx * fx + fy * fy) > mu[g] * fz:
            fl |= gc.SLIP << g
    return fl


def plan_jacobians(p, xs, ua, feet, con, pushes, opts, kw):
    """(h,12,30): the Jacobian of every period of one plan at the point xs (h+1,12; row 0: the start), ua (h,12), feet (h,6), by
    `period_jacobian_columns`."""
    return np.stack([period_jacobian_columns(xs[k], ua[k], feet[k], con[k], pushes[k], dt=p["dt"], **opts, **kw) for k in range(p["h"])])


def adjoint(p, J, xs, U, flags, con, lands, xr, mu, move_feet):
    """The recursion for one plan: J (h,12,30) its Jacobians, xs (h+1,12) the states (row 0: the start), U (h,12) the commands,
    flags (h,) the ground's (None: no ground), lands (h,2), xr (h,12).  Returns (grad_u (h,12), grad_x0 (12,), grad_foot (6,))."""
    h = p["h"]
    Q, R = p["Q"][:12], p["R"][:12]
    tp, tv = 1.0 + p["kv"], (h / 2 * p["dt"]) / 2
    lam, mu_f = np.zeros(12), np.zeros(6)
    grad_u = np.empty((h, 12))
    for k in range(h - 1, -1, -1):
        lam = lam + 2.0 * Q * (xs[k + 1] - xr[k])
        if move_feet and k + 1 < h:
            for g in range(2):
                if lands[k, g]:
                    lam[3] += tp * mu_f[3 * g]
                    lam[9] += tv * mu_f[3 * g]
                    lam[4] += tp * mu_f[3 * g + 1]
                    lam[10] += tv * mu_f[3 * g + 1]
                    mu_f[3 * g:3 * g + 3] = 0.0
        g_ua = J[k][:, 12:24].T @ lam
        mu_f = mu_f + J[k][:, 24:].T @ lam
        lam = J[k][:, :12].T @ lam
        T = np.eye(12) if flags is None else ground_jacobian(U[k], con[k], mu, flags[k])
        grad_u[k] = T.T @ g_ua + 2.0 * R * U[k]
    return grad_u, lam, mu_f


def _common(p, x_fb, contact, x_cmd, x_ref, push, push_from, push_steps, body, ground, B):
    h = p["h"]
    con = np.asarray(contact).reshape(B, h, 2) != 0
    mu = None if ground is None else (np.full((B, 2), p["mu"]) if ground.get("mu") is None else np.asarray(ground["mu"], np.float64))
    xr = rc.references(p, x_fb, x_cmd, x_ref)
    pushes = [[np.asarray(push, np.float32).astype(np.float64)[b] if push is not None and push_from <= k < push_from + push_steps else None
               for k in range(h)] for b in range(B)]
    return con, rc.landings(con), mu, xr, pushes, body or {}


def _points(p, x_fb, foot, contact, controls, x_traj, x_cmd, x_ref, push, push_from, push_steps, move_feet, body, ground):
    """The linearisation point the kernel has, per finite plan: yields (b, s, xs (h+1,12), U (h,12), ua (h,12), feet (h,6), flags or
    None), and the common arrays."""
    U = np.asarray(controls, np.float32)
    B, S, h = U.shape[:3]
    com = _common(p, x_fb, contact, x_cmd, x_ref, push, push_from, push_steps, body, ground, B)
    con, mu = com[0], com[2]
    feet = rc.footholds(p, foot, contact, x_traj, x_cmd, move_feet).astype(np.float64)
    x0 = np.asarray(x_fb, np.float32).astype(np.float64)
    pts = []
    for b in range(B):
        for s in range(S):
            if not np.isfinite(x_traj[b, s]).all():
                continue
            if mu is None:
                ua, flags = U[b, s].astype(np.float64), None
            else:
                ua, flags, _, _ = gc.transmit(U[b, s], con[b], np.tile(mu[b], (h, 1)))
                ua = ua.astype(np.float64)
            pts.append((b, s, np.concatenate([x0[b][None], x_traj[b, s].astype(np.float64)]), U[b, s].astype(np.float64), ua, feet[b, s], flags))
    return pts, com


def jacobians(p, x_fb, foot, contact, controls, x_traj, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4",
              substeps=4, move_feet=True, body=None, ground=None):
    """(B,S,h,12,30): dPhi/d(x, ua, r) of every (plan, period) at the recorded x_traj (B,S,h,12) fp32, the footholds of
    `rollout_cases.footholds` on it and u_applied as `ground_cases.transmit` gives it; NaN for a plan whose recorded states are not
    all finite."""
    B, S, h = np.asarray(controls).shape[:3]
    pts, (con, _, _, _, pushes, body) = _points(p, x_fb, foot, contact, controls, x_traj, x_cmd, x_ref, push, push_from, push_steps,
                                                move_feet, body, ground)
    J = np.full((B, S, h, 12, 30), np.nan)
    opts = dict(integrator=integrator, substeps=substeps)
    for b, s, xs, _, ua, feet, _ in pts:
        J[b, s] = plan_jacobians(p, xs, ua, feet, con[b], pushes[b], opts, bc.plant_kw(body, b))
        if (b + s) % 5 == 0:
            # every fifth plan, one period each (the period moves with the plan): the side-by-side Jacobian against the one computed
            # column by column on `plant_model.rate`
            d = check_columns(J[b, s], p, xs, ua, feet, con[b], pushes[b], opts, bc.plant_kw(body, b), [(b + 2 * s) % h])
            assert d <= COLUMNS_REL, (b, s, d)
    return J


def gradient(p, x_fb, foot, contact, controls, x_traj, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4",
             substeps=4, move_feet=True, body=None, ground=None):
    """dict(grad_u (B,S,h,12), grad_x0 (B,S,12), grad_foot (B,S,6)) at the recorded x_traj (B,S,h,12) fp32; all NaN for a plan whose
    recorded states are not all finite (a bad plan: the kernel's are NaN too)."""
    B, S, h = np.asarray(controls).shape[:3]
    opt = dict(x_cmd=x_cmd, x_ref=x_ref, push=push, push_from=push_from, push_steps=push_steps, move_feet=move_feet, body=body, ground=ground)
    J = jacobians(p, x_fb, foot, contact, controls, x_traj, integrator=integrator, substeps=substeps, **opt)
    pts, (con, lands, mu, xr, _, _) = _points(p, x_fb, foot, contact, controls, x_traj, **opt)
    out = dict(grad_u=np.full((B, S, h, 12), np.nan), grad_x0=np.full((B, S, 12), np.nan), grad_foot=np.full((B, S, 6), np.nan))
    for b, s, xs, U, _, _, flags in pts:
        out["grad_u"][b, s], out["grad_x0"][b, s], out["grad_foot"][b, s] = adjoint(p, J[b, s], xs, U, flags, con[b], lands[b], xr[b],
                                                                                    None if mu is None else mu[b], move_feet)
    return out


def free_rollout(p, x0, foot, U, con, lands, xr, pushes, mu, cmd, opts, kw, move_feet, flags=None):
    """One plan free-running and unrounded, in complex arithmetic (no conjugate anywhere: the functional continued analytically):
    (cost, xs (h+1,12), ua (h,12), feet (h,6), flags (h,) or None), all complex but the flags.  `flags`: the branches to take
    (those of the real run); None: decided here on the real parts."""
    h = p["h"]
    Q, R = p["Q"][:12], p["R"][:12]
    x, fs, U = np.array(x0, complex), np.array(foot, complex), np.asarray(U, complex)
    xs, uas, feet, fls = [x], [], [], []
    cost = 0.0
    for k in range(h):
        feet.append(fs.copy())
        if mu is None:
            ua = U[k]
        else:
            fl = ground_flags(U[k].real, con[k], mu) if flags is None else flags[k]
            fls.append(fl)
            ua = ground_rule(U[k], con[k], mu, fl)
        uas.append(ua)
        x = cstep(x, ua, fs, con[k], pushes[k], dt=p["dt"], **opts, **kw)
        xs.append(x)
        cost = cost + np.sum(Q * (x - xr[k]) ** 2 + R * U[k] ** 2)
        if move_feet and k + 1 < h:
            for g, side in enumerate((1.0, -1.0)):
                if lands[k, g]:
                    fs = fs.copy()
                    fs[3 * g] = x[3] + x[9] * (h / 2 * p["dt"]) / 2 + p["kv"] * (x[3] - cmd[3])
                    fs[3 * g + 1] = x[4] + x[10] * (h / 2 * p["dt"]) / 2 + p["kv"] * (x[4] - cmd[4]) + 0.04 * side
                    fs[3 * g + 2] = 0.0
    return cost, np.array(xs), np.array(uas), np.array(feet), (np.array(fls) if mu is not None else None)


def self_check(p, x_fb, foot, contact, controls, pick, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4",
               substeps=4, move_feet=True, body=None, ground=None, directions=3, seed=5):
    """For the plans `pick` (pairs (b, s)): the largest |Im cost(. + i delta d) / delta - <gradient, d>| / max |either| over
    `directions` random directions d = (D, d0, df) each, the gradient linearised at the unrounded free-running trajectory."""
    U = np.asarray(controls, np.float32).astype(np.float64)
    B, S, h = U.shape[:3]
    con, lands, mu, xr, pushes, body = _common(p, x_fb, contact, x_cmd, x_ref, push, push_from, push_steps, body, ground, B)
    cmd = np.tile(p["x_cmd"], (B, 1)) if x_cmd is None else np.asarray(x_cmd, np.float32).astype(np.float64)
    x0, f0 = np.asarray(x_fb, np.float32).astype(np.float64), np.asarray(foot, np.float32).astype(np.float64)
    opts = dict(integrator=integrator, substeps=substeps)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for b, s in pick:
        kw = bc.plant_kw(body, b)
        mub = None if mu is None else mu[b]
        args = (con[b], lands[b], xr[b], pushes[b], mub, cmd[b], opts, kw, move_feet)
        _, xs, ua, feet, flags = free_rollout(p, x0[b], f0[b], U[b, s], *args)
        J = plan_jacobians(p, xs.real, ua.real, feet.real, con[b], pushes[b], opts, kw)
        gu, gx, gf = adjoint(p, J, xs.real, U[b, s], flags, con[b], lands[b], xr[b], mub, move_feet)
        for _ in range(directions):
            D, d0, df = rng.normal(size=(h, 12)), rng.normal(size=12), rng.normal(size=6)
            cz, *_ = free_rollout(p, x0[b] + 1j * DELTA * d0, f0[b] + 1j * DELTA * df, U[b, s] + 1j * DELTA * D, *args, flags=flags)
            dd, inner = cz.imag / DELTA, float((gu * D).sum() + gx @ d0 + gf @ df)
            worst = max(worst, abs(dd - inner) / max(abs(dd), abs(inner)))
    return worst


# ---- the figure and the checks

def figures(got, ref, finite=None):
    """{output: the largest figure over the plans}: per plan max |got - ref| / max |ref| of that output; where the reference output
    is identically zero `got` must be +-0 (asserted).  `finite` (B,S) bool: the plans whose state stays finite (default: all); every
    entry of another plan must be NaN (asserted)."""
    out = {}
    for k in GRADS:
        if k not in got:
            continue
        B, S = ref[k].shape[:2]
        g, r = got[k].reshape(B, S, -1), ref[k].reshape(B, S, -1)
        worst = 0.0
        for b in range(B):
            for s in range(S):
                if finite is not None and not finite[b, s]:
                    assert np.isnan(g[b, s]).all(), (k, b, s)
                    continue
                top = np.abs(r[b, s]).max()
                if top == 0.0:
                    assert (g[b, s] == 0.0).all(), (k, b, s)
                    continue
                worst = max(worst, float(np.abs(g[b, s] - r[b, s]).max() / top))
        out[k] = worst
    return out


def check_forward(p, got, args, kw, where):
    """x_traj, cost and first_bad of a result by `rollout_cases`' own rules: every period within 2 fp32 ulps of the model stepped from
    the recorded state before it, the cost within cost_bound(h) of the long-double recomputation, first_bad the first all-NaN period."""
    ref = rc.restate(p, *args, **kw, recorded=got["x_traj"])
    d = pm.ulp_diff(got["x_traj"], ref["x_model"])
    nan = np.isnan(got["x_traj"]).all(-1)
    first = np.where(nan.any(-1), nan.argmax(-1), -1).astype(np.int32)
    fin = np.isfinite(ref["cost"])
    with np.errstate(all="ignore"):
        dcost = np.abs(got["cost"] - ref["cost"]) / np.abs(ref["cost"])
    print("rollout_grad forward", where, f"x_traj max ulps={d.max():.3f} cost rel={dcost[fin].max() if fin.any() else 0:.3e} "
          f"(bound {rc.cost_bound(p['h']):.3e}) valid={int(fin.sum())}/{fin.size}")
    assert d.max() <= 2.0, (where, d.max())
    assert np.array_equal(np.isnan(got["x_traj"]).any(-1), nan), where
    assert got["first_bad"].dtype == np.int32 and np.array_equal(got["first_bad"], first), where
    assert np.array_equal(np.isnan(got["cost"]), ~fin) and (dcost[fin] <= rc.cost_bound(p["h"])).all(), (where, dcost[fin].max())
    return ref
