"""Reference-tracking instances (supplied x_ref / foot_ref, include/bmpc.h `bmpc_inputs`) and the oracle that solves them.

Every instance is built in fp32-representable values (what crosses the C ABI), in the reference's orientation: x_ref (13,h) with
its row of ones, foot_ref (6,h).  Kinds:
  a  turn in place, yaw rate ramping up
  b  crouch (or stand-up) height ramp with the matching v_z
  c  step-up: the footholds of the second touch-down at z = 0.1, the CoM height ramped by as much
  d  walking on a planner's footholds (not the REF:72-109 heuristic)
  e  x_fb rolled, pitched and yawed by ~0.2 rad, x_ref level: the body axes of the line-foot rows must be those of x_fb
  f  standing still, the supplied arrays ARE the generators' output (zero commanded velocity: exact copies)
"""
import contextlib

import numpy as np

KINDS = "abcdef"


def _r32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _walking_contact(h, half, phase):
    n = (phase + np.arange(h)) // half
    leg0 = n % 2 == 0
    return np.stack([leg0, ~leg0], 1).astype(np.uint8)


def make_case(kind, h, rng, dt=0.04):
    """One instance: dict(x_fb (12,), foot (6,), contact (h,2) uint8, phase, t, x_cmd (12,), x_ref (13,h), foot_ref (6,h), half, kind)."""
    from oracle import bmpc_oracle as orc
    half = h // 2
    x_cmd = np.array([0, 0, 0, 0, 0, 0.55, 0, 0, 0, 0, 0, 0], float)
    e = rng.uniform(-0.05, 0.05, 3)
    p = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.5, 0.58)])
    w = rng.uniform(-0.1, 0.1, 3)
    v = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05)])
    if kind == "e":
        e = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.17, 0.23, 3)
    x_fb = _r32(np.concatenate([e, p, w, v]))
    sy = 0.089 + rng.uniform(-0.02, 0.02)
    foot = _r32([p[0] - 0.0195, p[1] + sy, 0.0, p[0] - 0.0195, p[1] - sy, 0.0])
    if kind in "bef":
        contact, phase = np.ones((h, 2), np.uint8), 0
    else:
        phase = int(rng.integers(0, h))
        contact = _walking_contact(h, half, phase)
    if kind == "f":
        x_fb[6:] = 0.0                         # standing still: what the generators produce is then exactly fp32
    t = (phase + 0.5) * dt
    mpc = orc.MPC()
    mpc.h, mpc.x_cmd = h, _r32(x_cmd)
    x_ref = orc.get_reference_trajectory(x_fb, mpc)
    foot_ref = orc.get_reference_foot_trajectory(x_fb, t, foot, mpc, contact, half=half)
    tj = np.arange(h) * dt
    if kind == "a":                            # yaw (x[0] in REF:151) accelerating: rate a * t
        a = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
        x_ref[0] = x_fb[0] + 0.5 * a * tj ** 2
        x_ref[3:6] = x_fb[3:6, None]
        x_ref[3:6, 1:] = np.array([p[0], p[1], 0.55])[:, None]
        x_ref[8] = a * tj
    elif kind == "b":                          # crouch / stand-up ramp
        dz = rng.uniform(-0.12, 0.08)
        x_ref[5, 1:] = p[2] + dz * tj[1:] / tj[-1]
        x_ref[11, 1:] = dz / tj[-1]
    elif kind == "c":                          # step-up of 0.1
        late = np.arange(h) >= (h - (phase % half))
        late |= np.arange(h) >= half + (half - phase % half) // 2
        foot_ref[2, late] = 0.1
        foot_ref[5, late] = 0.1
        x_ref[5, 1:] = 0.55 + 0.1 * tj[1:] / tj[-1]
        x_ref[11, 1:] = 0.1 / tj[-1]
    elif kind == "d":                          # a footstep planner's footholds
        step = np.array([rng.uniform(0.02, 0.1), rng.uniform(-0.03, 0.03)])
        for j in range(h):
            n = (phase + j) // half
            for leg in range(2):
                if contact[j, leg] and n > phase // half:
                    foot_ref[3 * leg:3 * leg + 2, j] = foot[3 * leg:3 * leg + 2] + step * (n - phase // half) + rng.uniform(-0.01, 0.01, 2)
                    foot_ref[3 * leg + 2, j] = 0.0
        x_ref[9, 1:] = step[0] / (half * dt)
        x_ref[3, 1:] = x_fb[3] + x_ref[9, 1:] * tj[1:]
    elif kind == "e":                          # level reference, tilted body
        x_ref[0:3] = 0.0
        x_ref[6:9] = 0.0
    x_ref = np.vstack([_r32(x_ref[:12]), np.ones((1, h))])
    return dict(kind=kind, x_fb=x_fb, foot=foot, contact=contact, phase=phase, t=t, x_cmd=_r32(x_cmd), x_ref=x_ref,
                foot_ref=_r32(foot_ref), half=half)


def make_batch(B, h, seed, kinds="abcde"):
    """B instances cycling through `kinds`, stacked: arrays with a leading batch axis (x_ref (B,13,h), foot_ref (B,6,h))."""
    rng = np.random.default_rng(seed)
    cases = [make_case(kinds[i % len(kinds)], h, rng) for i in range(B)]
    out = {k: np.stack([c[k] for c in cases]) for k in ("x_fb", "foot", "contact", "x_cmd", "x_ref", "foot_ref", "t")}
    out["phase"] = np.array([c["phase"] for c in cases], np.int32)
    out["kind"] = np.array([c["kind"] for c in cases])
    out["half"] = cases[0]["half"]
    return out


@contextlib.contextmanager
def supplied(mod, x_ref, foot_ref):
    """`mod.get_reference_trajectory` / `mod.get_reference_foot_trajectory` (the oracle's, or the reference's own) replaced by
    functions that return the supplied arrays (None: left as it is)."""
    saved = mod.get_reference_trajectory, mod.get_reference_foot_trajectory
    try:
        if x_ref is not None:
            mod.get_reference_trajectory = lambda *a, **k: np.array(x_ref, float)
        if foot_ref is not None:
            mod.get_reference_foot_trajectory = lambda *a, **k: np.array(foot_ref, float)
        yield
    finally:
        mod.get_reference_trajectory, mod.get_reference_foot_trajectory = saved


def oracle_solve(c, h, x_ref=None, foot_ref=None, Q_scale=1.0):
    """Certified fp64 optimum of instance `c` (make_case's dict, or a row of a batch) tracking the supplied references
    (default: the instance's own).  Returns (controls (h,12), certified)."""
    from oracle import bmpc_oracle as orc
    mpc = orc.MPC()
    mpc.h, mpc.x_cmd = h, np.asarray(c["x_cmd"], float)
    mpc.Q = mpc.Q * Q_scale
    xr = c["x_ref"] if x_ref is None else x_ref
    fr = c["foot_ref"] if foot_ref is None else foot_ref
    with supplied(orc, xr, fr):
        _, ct, info = orc.solve_mpc(np.asarray(c["x_fb"], float), float(c["t"]), np.asarray(c["foot"], float), mpc, orc.Biped(),
                                    np.asarray(c["contact"]), half=int(c["half"]), mu_steps=c.get("mu"), return_info=True)
    k = info["kkt"]
    return ct, bool(info["polished"]) and max(k["stationarity"], k["primal_ineq"], k["complementarity"]) <= 1e-7


def _oracle_worker(a):
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1):
        return oracle_solve(*a)


def oracle_batch(s, idx, h, Q_scale=1.0, procs=16):
    """oracle_solve of instances `idx` of batch `s` in a process pool: (controls (n,h,12), certified (n,))."""
    import multiprocessing as mp
    import os
    rows = [({k: s[k][i] for k in ("x_fb", "foot", "contact", "x_cmd", "x_ref", "foot_ref", "t")}
             | {"half": s["half"], "mu": None if s.get("mu") is None else s["mu"][i]}, h, None, None, Q_scale) for i in idx]
    with mp.get_context("spawn").Pool(min(procs, os.cpu_count() or 1)) as pool:
        res = pool.map(_oracle_worker, rows, chunksize=8)
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res])
