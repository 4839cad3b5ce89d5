"""Yardstick, case sets and bounds of the evaluation tests (tests/test_evaluate_cpu.py, tests/test_gpu_evaluate.py).

Yardstick: the oracle's matrices, not a QP solve.  For an instance and controls U (rounded to fp32, as the entry takes them)
`orc.build_sparse_qp` gives P, q, G, h, A, b of REF:187-297; X = solve(A[:, :13h], b - A[:, 13h:] U), z = [X; U],
objective = z'Pz/2 + q'z, cost = objective + sum Q x_ref^2, r = G z - h split by row class.  Every input is rounded to fp32 first:
both sides compute in fp64 on identical inputs.

A case group is a dict: h, half, biped (the oracle's Biped), x_fb (n,12), foot (n,6), contact (n,h,2), phase (n,), x_cmd (n,12),
mu (n,h,2) | None, x_ref (n,13,h) | None, foot_ref (n,6,h) | None (None: generated), controls (n,h,12)."""
import numpy as np

from tests import refs_cases as rc
from tests import util

DT = 0.04

# Regression bounds per metric: 100 x the larger of the maxima measured over all cases of the new tests in the emulation and on the
# MI355X (docs/history_r08.md has the measurements) -- room for another libm's sin / cos and another summation order, nothing more.
# The acceptance bound is util.REL_TOL; these are asserted in addition.
# Measured maxima (emulation / MI355X): states 4.69e-15 / 4.18e-15, cost 1.92e-15 / 2.23e-15, objective 1.92e-15 / 2.23e-15,
# violation 7.11e-15 / 3.69e-15.
REG_BOUND = dict(states=4.69e-13, cost=2.24e-13, objective=2.24e-13, violation=7.11e-13)


def r32(a):
    return None if a is None else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def oracle_objects(g, i, mods=None):
    """(orc.MPC, orc.Biped, dt) of instance i of group g.  `mods` (default: the group's own "mods" entry, else none) is a pair
    (change of the MPC object or None, of the Biped object or None) as in util.PARAM_CASES, applied to the MPC and to a copy of the
    group's Biped; dt is then the MPC's, else the module constant."""
    import copy
    from oracle import bmpc_oracle as orc
    mpc = orc.MPC()
    mpc.h, mpc.x_cmd = g["h"], r32(g["x_cmd"][i])
    mods = g.get("mods") if mods is None else mods
    if mods is None:
        return mpc, g["biped"], DT
    biped = copy.deepcopy(g["biped"])
    for mod, obj in zip(mods, (mpc, biped)):
        if mod:
            mod(obj)
    assert mpc.h == g["h"], "a case of an evaluation group must keep the horizon"
    return mpc, biped, float(mpc.dt)


def yardstick(g, i, mods=None):
    """dict(cost, objective, violation (4,), states (h,13)) of instance i of group g, fp64; `mods`: see oracle_objects."""
    from oracle import bmpc_oracle as orc
    h = g["h"]
    mpc, biped, dt = oracle_objects(g, i, mods)
    xr = None if g["x_ref"] is None else np.vstack([r32(g["x_ref"][i][:12]), np.ones((1, h))])
    fr = None if g["foot_ref"] is None else r32(g["foot_ref"][i])
    mu = None if g["mu"] is None else r32(g["mu"][i])
    U = r32(g["controls"][i]).reshape(-1)
    t = (int(g["phase"][i]) + 0.5) * dt
    with rc.supplied(orc, xr, fr):
        sp = orc.build_sparse_qp(r32(g["x_fb"][i]), t, r32(g["foot"][i]), mpc, biped, np.asarray(g["contact"][i]),
                                 half=g["half"], mu_steps=mu)
    assert orc.phase_index(t, mpc) == int(g["phase"][i])
    A, b = sp["A"], sp["b"]
    X = np.linalg.solve(A[:, :13 * h], b - A[:, 13 * h:] @ U)
    z = np.concatenate([X, U])
    objective = float(z @ sp["P"] @ z / 2 + sp["q"] @ z)
    cost = objective + float(np.sum(np.asarray(mpc.Q, float)[:, None] * sp["x_ref"] ** 2))
    r = np.maximum(sp["G"] @ z - sp["h"].reshape(-1), 0.0)
    box = r[8 * h:32 * h].reshape(h, 24)
    viol = np.array([r[:8 * h].max(), box[:, [0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17]].max(),
                     box[:, [6, 7, 8, 9, 10, 11, 18, 19, 20, 21, 22, 23]].max(), r[32 * h:].max()])
    return dict(cost=cost, objective=objective, violation=viol, states=X.reshape(h, 13))


def yardstick_group(g, idx=None, mods=None):
    idx = range(g["x_fb"].shape[0]) if idx is None else idx
    ys = [yardstick(g, int(i), mods) for i in idx]
    return {k: np.stack([np.asarray(y[k]) for y in ys]) for k in ("cost", "objective", "violation", "states")}


def metrics(got, ref):
    """The four error metrics |got - ref| / max(1, |ref|) per instance: states over the instance's h x 13 entries, cost and objective
    with |ref| the larger of the two magnitudes, violation per class (the largest of the four)."""
    n = ref["cost"].shape[0]
    st = np.abs(got["states"] - ref["states"]).reshape(n, -1).max(1) / np.maximum(1.0, np.abs(ref["states"]).reshape(n, -1).max(1))
    scale = np.maximum(1.0, np.maximum(np.abs(ref["cost"]), np.abs(ref["objective"])))
    vi = (np.abs(got["violation"] - ref["violation"]) / np.maximum(1.0, np.abs(ref["violation"]))).max(1)
    return dict(states=st, cost=np.abs(got["cost"] - ref["cost"]) / scale, objective=np.abs(got["objective"] - ref["objective"]) / scale,
                violation=vi)


def check(got, ref, where, reg_bound=None):
    """Prints the maxima of the four metrics, then asserts the acceptance bound (util.REL_TOL) and the regression bound of each
    (REG_BOUND, or `reg_bound` for case sets that hold their own)."""
    reg_bound = REG_BOUND if reg_bound is None else reg_bound
    m = {k: float(v.max()) for k, v in metrics(got, ref).items()}
    print("evaluate metrics", where, " ".join(f"{k}={v:.3e}" for k, v in m.items()))
    assert all(np.isfinite(got[k]).all() for k in ("cost", "objective", "violation", "states")), where
    for k, v in m.items():
        assert v <= util.REL_TOL, (where, k, v)
        assert v <= reg_bound[k], (where, k, v)
    return m


def seeded_controls(contact, rng, m=12.0, g=9.81):
    """Controls of the size of a solve's: f_z about m g shared by the stance legs plus noise, small tangential forces and moments."""
    c = np.asarray(contact, float)
    n, h, _ = c.shape
    nst = np.maximum(c.sum(2, keepdims=True), 1.0)
    u = np.zeros((n, h, 12))
    for leg in range(2):
        on = c[:, :, leg]
        u[:, :, 3 * leg + 2] = on * (m * g / nst[:, :, 0] + rng.normal(0, 8.0, (n, h)))
        u[:, :, 3 * leg + 0] = on * rng.normal(0, 6.0, (n, h))
        u[:, :, 3 * leg + 1] = on * rng.normal(0, 6.0, (n, h))
        u[:, :, 6 + 3 * leg: 9 + 3 * leg] = on[:, :, None] * rng.normal(0, 1.5, (n, h, 3))
    return r32(u)


def breaking_controls(U, seed):
    """U' = 1.3 U + d with a seeded d that, by the bits of a per-instance mask, puts force on every leg (swing legs included: force
    box), a roll moment (the tau_max[0] = 0 rows: moment box), tangential force outside the pyramid (friction) and a pitch moment
    beyond the line-foot rows."""
    rng = np.random.default_rng(seed)
    n, h, _ = U.shape
    masks = [15, 1, 2, 4, 8, 0, 3, 12, 5, 10, 6, 9, 7, 11, 13, 14]
    d = np.zeros_like(U)
    for i in range(n):
        mk = masks[i % len(masks)]
        for leg in range(2):
            if mk & 1:
                d[i, :, 3 * leg + 2] += 50.0 + rng.uniform(0, 5, h)
            if mk & 2:
                d[i, :, 6 + 3 * leg] += 5.0 + rng.uniform(0, 1, h)
            if mk & 4:
                d[i, :, 3 * leg] += 200.0 + rng.uniform(0, 20, h)
            if mk & 8:
                d[i, :, 6 + 3 * leg + 1] += 40.0 + rng.uniform(0, 4, h)
    return r32(1.3 * U + d)


def _group(h, half, biped, x_fb, foot, contact, phase, x_cmd, controls, mu=None, x_ref=None, foot_ref=None, name=""):
    from oracle import bmpc_oracle as orc
    return dict(name=name, h=h, half=half, biped=biped if biped is not None else orc.Biped(), x_fb=np.asarray(x_fb, float),
                foot=np.asarray(foot, float), contact=np.asarray(contact).astype(np.uint8), phase=np.asarray(phase, np.int32),
                x_cmd=np.asarray(x_cmd, float), controls=np.asarray(controls, float), mu=mu, x_ref=x_ref, foot_ref=foot_ref)


def ref_tracking_groups(breaking=False):
    """Cases 1 / 2: every instance of tests/golden/ref_tracking.npz (h = 10, 16, 20; kinds a-f; supplied references) with the
    fixture's own controls, or with `breaking_controls` of them.  Each group also carries the fixture's `states` and `q`."""
    d = util.load("ref_tracking")
    out = []
    for h in (10, 16, 20):
        p = f"h{h}_"
        f = {k[len(p):]: d[k] for k in d.files if k.startswith(p)}
        U = breaking_controls(f["controls"], 100 + h) if breaking else f["controls"]
        g = _group(h, int(f["half"]), None, f["x_fb"], f["foot"], f["contact"], f["phase"], f["x_cmd"], U, x_ref=f["x_ref"],
                   foot_ref=f["foot_ref"], name=f"ref_tracking_h{h}" + ("_broken" if breaking else ""))
        g["fix_states"], g["fix_q"], g["kind"] = f["states"], f["q"], f["kind"]
        out.append(g)
    return out


def generated_groups():
    """Case 3: generated references.  The fixtures' own controls on known_walking_t0, edge_cases_h10, cfg_cmd_h10 (tilted bodies,
    commanded rates), cfg_bounds_h10 (bounds off their defaults, one group per bounds set); seeded controls on a per-step-mu
    walking batch at h = 20."""
    out = []
    d = util.load("known_walking_t0")
    out.append(_group(10, 5, None, d["x_fb"][None], d["foot"][None], d["contact"][None], util.phases([float(d["t"])], DT, 10),
                      d["x_cmd"][None], d["controls"][None], name="known_walking_t0"))
    for name in ("edge_cases_h10", "cfg_cmd_h10", "cfg_bounds_h10"):
        d = util.load(name)
        h, half = util.BATCH_FIXTURES[name]
        ph = util.phases(d["t"], DT, h)
        for gi, (idx, biped) in enumerate(util.bounds_groups(d)):
            out.append(_group(h, half, biped, d["x_fb"][idx], d["foot"][idx], d["contact"][idx], ph[idx], d["x_cmd"][idx],
                              d["controls"][idx], name=f"{name}_{gi}"))
    s = util.synth_batch(24, 20, 5, gait="walking", per_step_mu=True)
    out.append(_group(20, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"],
                      seeded_controls(s["contact"], np.random.default_rng(55)), mu=s["mu"], name="synth_mu_h20"))
    return out


def horizon_groups():
    """h = 1, 3, 13, 33, 40 (lane groups of 16 / 32 / 64, idle lanes past the horizon) on refs_cases.make_case instances, each once
    with its supplied references and once with generated ones; seeded controls.  (h = 1: the first step of an h = 3 instance --
    make_case needs a half period of at least one step.)"""
    out = []
    for h in (1, 3, 13, 33, 40):
        rng = np.random.default_rng(900 + h)
        cases = [rc.make_case(k, max(h, 3), rng) for k in "abcde"]
        half = max(1, h // 2) if h > 1 else 1
        if h == 1:
            cases = [c | dict(contact=c["contact"][:1], x_ref=c["x_ref"][:, :1], foot_ref=c["foot_ref"][:, :1], phase=0) for c in cases]
        st = lambda k: np.stack([np.asarray(c[k]) for c in cases])
        U = seeded_controls(st("contact"), rng)
        for sup in (True, False):
            out.append(_group(h, half, None, st("x_fb"), st("foot"), st("contact"), st("phase"), st("x_cmd"), U,
                              x_ref=st("x_ref") if sup else None, foot_ref=st("foot_ref") if sup else None,
                              name=f"make_case_h{h}_" + ("supplied" if sup else "generated")))
    return out


def kernel_args(g, idx=None):
    """The arguments of `BatchSolver.evaluate` / `emu_eval.evaluate` for (instances idx of) group g: references in the kernel layout."""
    import biped_mpc_py_amd as bm
    sl = slice(None) if idx is None else idx
    xr, fr = bm.references_to_kernel_layout(None if g["x_ref"] is None else g["x_ref"][sl],
                                            None if g["foot_ref"] is None else g["foot_ref"][sl], g["h"])
    return dict(x_fb=g["x_fb"][sl], foot=g["foot"][sl], contact=g["contact"][sl], phase=g["phase"][sl], controls=g["controls"][sl],
                x_cmd=g["x_cmd"][sl], mu=None if g["mu"] is None else g["mu"][sl], x_ref=xr, foot_ref=fr)


def cparams_of(g, path=0, mods=None):
    """The parameter block of group g on kernel family `path`: the horizon, the half period and the four bound vectors of the group's
    Biped; `mods` (default: the group's own "mods" entry, else none; see oracle_objects) is then applied to the package's objects."""
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = g["h"]
    b = bm.Biped()
    for k in ("f_max", "f_min", "tau_max", "tau_min"):
        setattr(b, k, np.asarray(getattr(g["biped"], k), float).reshape(-1))
    mods = g.get("mods") if mods is None else mods
    for mod, obj in zip(mods or (), (mpc, b)):
        if mod:
            mod(obj)
    return bm.pack_params(mpc, b, half=g["half"], solver_options=dict(path=path) if path else None)


def bad_batch(h=10, seed=77):
    """Case 5: a batch of eight (supplied references) and its spoiled copy -- instance 1 with a NaN control entry, 4 with an Inf in
    x_ref, 6 with a reference pitch of 90 degrees (R_inv singular).  Returns (clean group, spoiled group, spoiled indices)."""
    s = rc.make_batch(8, h, seed, "abcde")
    U = seeded_controls(s["contact"], np.random.default_rng(seed + 1))
    clean = _group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], U, x_ref=s["x_ref"],
                   foot_ref=s["foot_ref"], name="bad_batch")
    bad = dict(clean)
    bad["controls"] = clean["controls"].copy()
    bad["x_ref"] = clean["x_ref"].copy()
    bad["controls"][1, h // 2, 7] = np.nan
    bad["x_ref"][4, 3, h - 1] = np.inf
    bad["x_ref"][6, 1, 2] = np.float32(np.pi / 2)
    return clean, bad, [1, 4, 6]


def kernel_args_unchecked(g):
    """kernel_args without the finiteness check of references_to_kernel_layout (the spoiled batch)."""
    a = kernel_args(dict(g, x_ref=None, foot_ref=None))
    a["x_ref"] = np.ascontiguousarray(np.swapaxes(g["x_ref"][:, :12, :], 1, 2))
    a["foot_ref"] = np.ascontiguousarray(np.swapaxes(g["foot_ref"], 1, 2))
    return a

