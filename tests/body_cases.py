"""The per-instance bodies the plant tests share (TEST INFRASTRUCTURE): mass, gravity and body inertia of each instance, and what
the model (tests/plant_model.py) makes of them.  The inertia is the default diagonal scaled per axis and turned a little, so that
it is symmetric positive definite, not diagonal, and well conditioned: the default's axes are 13 : 1 apart and the scale factors add
at most 4 : 1, so a draw can reach 53.  What the default seed guarantees, and the tests assert: cond(I) <= COND_MAX = 48 at B = 33,
67 and 257 (tests/test_plant_body_cpu.py), and a closed loop of tests/test_gpu_plant_body.py in which every instance stays upright,
away from the pitch singularity.  At that conditioning the fp64 error of either way of inverting I (adjugate over determinant in
the kernel, a solve in the model) is about nine orders below an fp32 ulp, and the plant's 2-ulp bound carries over."""
import numpy as np

from tests import plant_model as pm

COND_MAX = 48.0
SENSITIVITY = 100.0                    # x the 2-ulp bound: what a member must move the model's next state by to count
MEMBERS = ("m", "I", "g")


def bodies(B, seed=41):
    """dict(m (B,) in [8, 20], I (B,3,3) = R0 diag(d) R0' with d the default diagonal x [0.5, 2] and R0 a rotation by up to 0.3 rad
    per axis, g (B,) in [3.7, 12]), float64."""
    rng = np.random.default_rng(seed)
    m, g = rng.uniform(8.0, 20.0, B), rng.uniform(3.7, 12.0, B)
    d = np.diag(pm.I_BODY) * rng.uniform(0.5, 2.0, (B, 3))
    ang = rng.uniform(-0.3, 0.3, (B, 3))
    I = np.stack([pm.rot(ang[b]) @ np.diag(d[b]) @ pm.rot(ang[b]).T for b in range(B)])
    return dict(m=m, I=np.ascontiguousarray(I), g=g)


def subset(body, members):
    """The body with only `members` supplied (the rest: the handle's)."""
    return {k: body[k] for k in members}


def plant_kw(body, b):
    """The model's keyword arguments of instance b for the supplied members."""
    names = {"m": "m", "I": "I_b", "g": "g"}
    return {names[k]: (np.asarray(v[b]).reshape(3, 3) if k == "I" else float(v[b])) for k, v in body.items()}


def step_batch(x, u, foot, c, w=None, body=None, **kw):
    """`plant_model.step_batch` with the body per instance (a bad body is not the model's business: finite ones only)."""
    body = body or {}
    return np.stack([pm.step(x[b], u[b], foot[b], c[b], None if w is None else w[b], **kw, **plant_kw(body, b)) for b in range(len(x))])


def outcome(x_traj, tilt_max, z_min):
    """The fall outcome of a recorded trajectory x_traj (steps, B, 12) float32, restated: (first_fall int32 (B,), max_tilt, min_z
    float32 (B,))."""
    x = np.asarray(x_traj, np.float32)
    tilt = np.fmax(np.abs(x[:, :, 0]), np.abs(x[:, :, 1]))
    with np.errstate(invalid="ignore"):
        up = (np.abs(x[:, :, 0].astype(np.float64)) <= tilt_max) & (np.abs(x[:, :, 1].astype(np.float64)) <= tilt_max) & \
             (x[:, :, 5].astype(np.float64) >= z_min)
    first = np.where((~up).any(0), (~up).argmax(0), -1).astype(np.int32)
    return first, np.fmax.reduce(tilt, 0), np.fmin.reduce(x[:, :, 5], 0)          # (fmax / fmin: NaN only where every period is)
