"""NumPy fp64 restatement of the plant of the closed-loop simulation and of its landing rule (TEST INFRASTRUCTURE), written from
the definition, not from the kernel: the nonlinear single rigid body with state x = [e(3), p(3), w(3), v(3)], e = [roll, pitch, yaw],
held controls u = [f1 f2 m1 m2], feet, contact bits and external wrench [F, M] over one control period."""
import numpy as np

SINGULAR = 2.0 ** -22
MASS, GRAV = 12.0, 9.81                                                # REF:36, 42
I_BODY = np.diag([0.932, 0.9420, 0.0711])                              # REF:37-39


def rot(e):
    """R = Rz(e2) Ry(e1) Rx(e0) (REF:124-138)."""
    cr, sr, cp, sp, cy, sy = np.cos(e[0]), np.sin(e[0]), np.cos(e[1]), np.sin(e[1]), np.cos(e[2]), np.sin(e[2])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def rate(x, u, foot, c, w, I_b=I_BODY, m=MASS, g=GRAV):
    """(dx/dt, singular) of one instance."""
    e, p, om, v = x[0:3], x[3:6], x[6:9], x[9:12]
    R = rot(e)
    I_w = R @ I_b @ R.T
    c1 = np.cos(e[1])
    with np.errstate(all="ignore"):
        e0d = (np.cos(e[2]) * om[0] + np.sin(e[2]) * om[1]) / c1
    e1d = -np.sin(e[2]) * om[0] + np.cos(e[2]) * om[1]
    e2d = om[2] + np.sin(e[1]) * e0d
    tau, f = np.array(w[3:6], float), np.array(w[0:3], float)
    for g_ in range(2):
        if c[g_]:
            fg, mg = u[3 * g_:3 * g_ + 3], u[6 + 3 * g_:9 + 3 * g_]
            tau = tau + np.cross(foot[3 * g_:3 * g_ + 3] - p, fg) + mg
            f = f + fg
    omd = np.linalg.solve(I_w, tau - np.cross(om, I_w @ om))
    vd = f / m + np.array([0, 0, -g])
    return np.concatenate([[e0d, e1d, e2d], v, omd, vd]), not (abs(c1) >= SINGULAR)


def step(x, u, foot, c, w=None, integrator="rk4", substeps=4, dt=0.04, **kw):
    """One control period of one instance (fp64 in, fp64 out); all NaN for a bad instance."""
    x, u, foot = np.asarray(x, float), np.asarray(u, float), np.asarray(foot, float)
    w = np.zeros(6) if w is None else np.asarray(w, float)
    bad = not (np.isfinite(x).all() and np.isfinite(u).all() and np.isfinite(foot).all() and np.isfinite(w).all())
    if bad:
        return np.full(12, np.nan)
    h = dt / substeps
    f = lambda y: rate(y, u, foot, c, w, **kw)
    for _ in range(substeps):
        if integrator == "euler":
            k1, s1 = f(x)
            x, bad = x + h * k1, bad or s1
        else:
            k1, s1 = f(x)
            k2, s2 = f(x + h / 2 * k1)
            k3, s3 = f(x + h / 2 * k2)
            k4, s4 = f(x + h * k3)
            x, bad = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4), bad or s1 or s2 or s3 or s4
    return np.full(12, np.nan) if bad else x


def step_batch(x, u, foot, c, w=None, **kw):
    return np.stack([step(x[b], u[b], foot[b], c[b], None if w is None else w[b], **kw) for b in range(len(x))])


def stance(step_, offset, period, duty):
    return ((step_ + offset) % period) < duty


def landing(x_new, foot, k0, k1, period=10, offset=(0, 5), duty=(5, 5), h=10, dt=0.04, kv=0.01, cmd=(0.0, 0.0)):
    """The footholds of one instance after the landing rule: a leg in swing at schedule step k0 and in stance at k1 gets the swing
    controller's target (REF:428-435) at the new state; every other foothold stays.  Returns (foot, lands[2])."""
    foot, lands = np.array(foot, float), [False, False]
    for g_, side in enumerate((1.0, -1.0)):
        if not stance(k0, offset[g_], period, duty[g_]) and stance(k1, offset[g_], period, duty[g_]):
            lands[g_] = True
            foot[3 * g_ + 0] = x_new[3] + x_new[9] * (h / 2 * dt) / 2 + kv * (x_new[3] - cmd[0])
            foot[3 * g_ + 1] = x_new[4] + x_new[10] * (h / 2 * dt) / 2 + kv * (x_new[4] - cmd[1]) + 0.04 * side
            foot[3 * g_ + 2] = 0.0
    return foot, lands


def ulp_diff(a, ref, atol=1e-12):
    """Per entry: how many fp32 ulps (of the reference's fp32 value) the fp32 array `a` is away from the fp64 reference, after
    `atol` absolute is taken off; NaN matches NaN."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    both_nan = np.isnan(a) & np.isnan(ref)
    ulp = np.spacing(np.abs(ref.astype(np.float32)).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.abs(a - ref) - atol, 0.0) / ulp
    d[both_nan] = 0.0
    d[np.isnan(d)] = np.inf
    return d


def batch(B, seed=7):
    """The test batch: attitudes up to +-0.6 rad, rates up to +-2 rad/s, single and double support, random wrench; fp32 values."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-0.6, 0.6, (B, 3)), rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(0.45, 0.6, (B, 1)),
                        rng.uniform(-2, 2, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))], 1).astype(np.float32)
    u = np.concatenate([rng.uniform(-30, 30, (B, 2)), rng.uniform(0, 150, (B, 1)), rng.uniform(-30, 30, (B, 2)), rng.uniform(0, 150, (B, 1)),
                        rng.uniform(-10, 10, (B, 6))], 1).astype(np.float32)
    foot = np.zeros((B, 6), np.float32)
    for g_, sgn in enumerate((1.0, -1.0)):
        foot[:, 3 * g_] = x[:, 3] + rng.uniform(-0.1, 0.1, B)
        foot[:, 3 * g_ + 1] = x[:, 4] + sgn * (0.09 + rng.uniform(-0.03, 0.03, B))
    c = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], np.uint8)[rng.integers(0, 4, B)]
    w = np.concatenate([rng.uniform(-40, 40, (B, 3)), rng.uniform(-5, 5, (B, 3))], 1).astype(np.float32)
    return x, u, foot, c, w
