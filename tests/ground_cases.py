"""The ground under the plant, restated (TEST INFRASTRUCTURE): what a flat floor with Coulomb friction transmits of the commanded
controls, in NumPy fp64 from the rule of include/bmpc.h, not from the kernel; the grounds and controls the tests share; and the
reduced outputs of the closed loop restated from the per-period flags and demands.

The rule, per leg g with contact bit c_g, commanded f = (fx, fy, fz), m and true friction mu_g: c_g == 0 transmits nothing (six
+0); c_g == 1 and not fz > 0 is UNLOADED (six +0, flag 4 << g); c_g == 1 and fz > 0 is LOADED: with t = sqrt(fx fx + fy fy) and
lim = mu_g fz the leg SLIPS if t > lim (fx, fy scaled by lim / t in fp64 and rounded to fp32 once each, flag 1 << g), else fx, fy
pass with their bits; fz and m always pass with their bits.  A mu that is NaN or negative, or a control that is not finite, is a bad
instance: everything NaN, flags 0.  Demand: the largest t / fz over the loaded legs with fz >= fz_floor, NaN if there is none."""
import numpy as np

SLIP, UNLOADED = 1, 4                  # flag bits of leg 0; leg 1: shifted left by one
BAND = 1e-6                            # no loaded leg of controls() has t / lim within 1 -+ BAND: slip or hold is never a rounding matter


def transmit(u, c, mu, fz_floor=0.0):
    """(u_applied (B,12) float32, flags (B,) uint8, demand (B,) float32, scaled (B,12) bool) of u (B,12) float32, contact bits c (B,2)
    and mu (B,2) float64.  `scaled`: the entries the rule multiplied (the only ones that are not copies or +0)."""
    u = np.asarray(u, np.float32)
    B = u.shape[0]
    c, mu = np.asarray(c).reshape(B, 2) != 0, np.asarray(mu, np.float64).reshape(B, 2)
    ua, flags = np.zeros((B, 12), np.float32), np.zeros(B, np.uint8)
    demand, scaled = np.full(B, np.nan, np.float32), np.zeros((B, 12), bool)
    for b in range(B):
        if not (np.isfinite(u[b]).all() and (mu[b] >= 0).all()):        # (a NaN mu compares false)
            ua[b] = np.nan
            continue
        worst = np.nan
        for g in range(2):
            fx, fy, fz = (np.float64(v) for v in u[b, 3 * g:3 * g + 3])
            if not c[b, g]:
                continue
            if not fz > 0:
                flags[b] |= UNLOADED << g
                continue
            ua[b, 3 * g:3 * g + 3] = u[b, 3 * g:3 * g + 3]
            ua[b, 6 + 3 * g:9 + 3 * g] = u[b, 6 + 3 * g:9 + 3 * g]
            t, lim = np.sqrt(fx * fx + fy * fy), mu[b, g] * fz
            if t > lim:
                ua[b, 3 * g], ua[b, 3 * g + 1] = np.float32(fx * (lim / t)), np.float32(fy * (lim / t))
                scaled[b, 3 * g:3 * g + 2] = True
                flags[b] |= SLIP << g
            if fz >= fz_floor:
                worst = np.fmax(worst, t / fz)
        demand[b] = np.float32(worst)
    return ua, flags, demand, scaled


def grounds(B, seed=23):
    """mu (B,2) float64 in [0.05, 1.0] per leg; every 8th instance has one leg at +inf."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.05, 1.0, (B, 2))
    mu[np.arange(0, B, 8), rng.integers(0, 2, len(range(0, B, 8)))] = np.inf
    return mu


def controls(B, seed=23):
    """(u (B,12) float32, c (B,2) uint8) against grounds(B, seed): per leg one of -- swing with controls that are not zero; stance
    and unloaded (fz = 0 or fz < 0); stance, loaded and holding (t = 0.1 .. 0.9 lim); stance, loaded and slipping (t = 1.1 .. 3 lim)
    -- with the instance index deciding, so that every pair of kinds meets.  Under a mu of +inf the tangential force is what a mu
    of 0.5 would give: it holds.  Every loaded leg has t / lim outside [1 - BAND, 1 + BAND] in the fp32 values (asserted)."""
    rng = np.random.default_rng(seed + 1)
    mu = grounds(B, seed)
    u = rng.uniform(-10, 10, (B, 12)).astype(np.float32)               # (the moments stay as drawn)
    c = np.ones((B, 2), np.uint8)
    kind = np.stack([np.arange(B) % 5, (np.arange(B) // 5) % 5], 1)    # 0 swing, 1 unloaded, 2 hold, 3 slip, 4 slip
    for b in range(B):
        for g in range(2):
            k = kind[b, g]
            fz = rng.uniform(5.0, 150.0)
            ratio = rng.uniform(0.1, 0.9) if k == 2 else rng.uniform(1.1, 3.0)
            t = ratio * (mu[b, g] if np.isfinite(mu[b, g]) else 0.5) * fz
            a = rng.uniform(0, 2 * np.pi)
            u[b, 3 * g:3 * g + 3] = (t * np.cos(a), t * np.sin(a), fz)
            if k == 0:
                c[b, g] = 0
            elif k == 1:
                u[b, 3 * g + 2] = 0.0 if rng.integers(0, 2) else -fz
    f = u.astype(np.float64)
    for g in range(2):
        loaded = (c[:, g] != 0) & (f[:, 3 * g + 2] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.hypot(f[:, 3 * g], f[:, 3 * g + 1]) / (mu[:, g] * f[:, 3 * g + 2])
        assert (np.abs(q[loaded] - 1.0) > BAND).all()
    return u, c


def reduce(flags, demand):
    """The reduced outputs of the closed loop from the per-period flags (steps,B) uint8 and demands (steps,B) float32:
    (first_slip (B,) int32, slip_periods (B,2) int32, unloaded_periods (B,2) int32, mu_demand (B,) float32)."""
    flags, demand = np.asarray(flags, np.uint8), np.asarray(demand, np.float32)
    B = flags.shape[1]
    slipped = (flags & (SLIP | SLIP << 1)) != 0
    first = np.array([int(np.flatnonzero(slipped[:, b])[0]) if slipped[:, b].any() else -1 for b in range(B)], np.int32)
    slip = np.stack([((flags >> g) & 1).sum(0) for g in range(2)], 1).astype(np.int32).reshape(B, 2)
    unloaded = np.stack([((flags >> (2 + g)) & 1).sum(0) for g in range(2)], 1).astype(np.int32).reshape(B, 2)
    mu_demand = np.fmax.reduce(demand, 0) if len(demand) else np.full(B, np.nan, np.float32)
    return first, slip, unloaded, mu_demand.astype(np.float32)


def assert_applied(ua, flags, ref_ua, ref_flags, scaled, where=""):
    """`ua`, `flags` against the model's: flags equal; entries the rule did not scale equal to the bit (the sign of a zero and NaN
    included); scaled entries within 1 fp32 ulp (a device may contract fx fx + fy fy: t, and with it the factor, moves by an fp64
    rounding, which the rounding to fp32 turns into at most one ulp).  Returns the largest deviation of a scaled entry in ulps."""
    ua, ref_ua = np.asarray(ua, np.float32), np.asarray(ref_ua, np.float32)
    assert np.array_equal(np.asarray(flags, np.uint8), ref_flags), where
    nan = np.isnan(ref_ua)
    assert np.array_equal(np.isnan(ua), nan), where
    same = ~scaled & ~nan
    assert np.array_equal(np.ascontiguousarray(ua).view(np.uint32)[same], np.ascontiguousarray(ref_ua).view(np.uint32)[same]), where
    if not scaled.any():
        return 0.0
    d = np.abs(ua[scaled].astype(np.float64) - ref_ua[scaled]) / np.spacing(np.abs(ref_ua[scaled])).astype(np.float64)
    assert d.max() <= 1.0, (where, d.max())
    return float(d.max())
