"""CPU: the gradient of the plant roll-out (csrc/bmpc_plant_rollout_grad.hip) without a GPU -- the body of plant_rollout_grad_kernel
run as plain C++ (tests/emu/emu_plant_rollout_grad.py) against the reference written from the definition
(tests/rollout_grad_cases.py): complex-step Jacobians of the NumPy plant model at the recorded trajectory, the adjoint recursion in
fp64 with the landing fold, and a self-check of that recursion against the complex-step derivative of the whole functional.

Bounds.  Forward: `rollout_cases`' own -- 2 fp32 ulps per period from the recorded state, cost_bound(h), first_bad the first all-NaN
period.  Gradient: per plan and output max |delta| / max |reference| <= GRAD_REL = 10 x the largest figure measured (both sides
are fp64 evaluations of the same sums in different association), held below 1e-9: evaluate_grad sits at 3e-13 and a missing term
shows at >= 1e-3.  Measured here (emulation): 3.55e-12 against `gradient`, on a force-breaking plan that tumbles through 230 rad
within the horizon (max |grad_u| 1.3e8: conditioning, not a term; plans that stay upright sit at 2e-15 and below); 4.6e-15 for the
self-check (bound 10 x, held below 1e-10).
The exact statements of include/bmpc.h are compared to the bit."""
import numpy as np
import pytest

from tests import ground_cases as gc
from tests import rollout_cases as rc
from tests import rollout_grad_cases as gcs

_CP = {}


def _cparams(h):
    if h not in _CP:
        import __graft_entry__ as ge
        ge.build()
        from biped_mpc_py_amd import _lib
        cp = _lib.CParams()
        assert _lib.load().bmpc_default_params(cp, h) == 0
        _CP[h] = cp
    return _CP[h]


def _args(c, U, idx=slice(None)):
    return c["x_fb"][idx], c["foot"][idx], c["contact"][idx], U[idx]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b, keep=None):
    for k in a:
        x, y = (a[k], b[k]) if keep is None else (a[k][keep], b[k][keep])
        assert x.dtype == y.dtype and np.array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y), k


@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("rk4", 4)])
@pytest.mark.parametrize("name", ["plain", "full"])
@pytest.mark.parametrize("h", [1, 3, 10])
def test_emulated_forward_and_gradient_match_the_reference(h, name, integrator, substeps):
    """1, 2: x_traj, cost and first_bad by rollout_cases' rules; grad_u, grad_x0, grad_foot against `gradient`."""
    from tests.emu import emu_plant_rollout_grad as eg
    cp = _cparams(h)
    p = rc.params_of(cp)
    c, U, counts = gcs.build(h, 13)
    kw = dict(rc.variant(c, name), integrator=integrator, substeps=substeps)
    got = eg.rollout_grad(cp, *_args(c, U), **kw)
    assert set(got) == set(gcs.OUTPUTS) and got["grad_u"].shape == (5, 13, h, 12) and got["grad_foot"].shape == (5, 13, 6)
    gcs.check_forward(p, got, _args(c, U), kw, (h, name, integrator, substeps))
    # (no plan is dropped: one of the force-breaking plans tumbles out of the fp32 range at h = 10 without a ground, and is held to
    # the rule for bad plans instead -- NaN cost and gradients from first_bad on)
    finite = np.isfinite(got["x_traj"]).all((2, 3))
    assert np.array_equal(got["first_bad"] == -1, finite) and np.array_equal(np.isfinite(got["cost"]), finite) and finite.sum() >= 64
    ref = gcs.gradient(p, *_args(c, U), got["x_traj"], **kw)
    fig = gcs.figures(got, ref, finite)
    print("rollout_grad emulation against the reference", (h, name, integrator, substeps), counts, fig, "GRAD_REL", gcs.GRAD_REL)
    assert gcs.GRAD_REL < gcs.GRAD_REL_MAX
    assert max(fig.values()) <= gcs.GRAD_REL, fig


def test_emulated_gradient_at_sixty_four_substeps():
    """2, once at h = 1 with 64 substeps, (B, S) = (1, 2): instance 4 (a swing leg) and its plans 0 and 1 (an unloaded stance leg)."""
    from tests.emu import emu_plant_rollout_grad as eg
    cp = _cparams(1)
    p = rc.params_of(cp)
    c, U, _ = gcs.build(1, 3)
    idx = slice(4, 5)
    kw = dict(rc.take(rc.variant(c, "full"), idx), integrator="rk4", substeps=64)
    args = _args(c, U[:, :2], idx)
    got = eg.rollout_grad(cp, *args, **kw)
    gcs.check_forward(p, got, args, kw, "64 substeps")
    fig = gcs.figures(got, gcs.gradient(p, *args, got["x_traj"], **kw))
    print("rollout_grad emulation against the reference, 64 substeps", fig)
    assert max(fig.values()) <= gcs.GRAD_REL, fig


@pytest.mark.parametrize("h", [3, 10])
def test_the_reference_recursion_is_the_derivative_of_the_functional(h):
    """3: directional derivatives of the free-running unrounded roll-out by complex step against <gradient, direction>."""
    cp = _cparams(h)
    p = rc.params_of(cp)
    c, U, _ = gcs.build(h, 13)
    worst = 0.0
    for name, integrator, substeps, pick in (("full", "rk4", 4, [(0, 0), (1, 1), (4, 3)]), ("plain", "euler", 1, [(2, 2), (4, 5)]),
                                             ("full", "euler", 2, [(0, 9), (1, 6), (3, 1), (4, 2)])):
        kw = dict(rc.variant(c, name), integrator=integrator, substeps=substeps)
        worst = max(worst, gcs.self_check(p, *_args(c, U), pick, **kw))
    off = gcs.self_check(p, *_args(c, U), [(0, 1), (4, 2)], **dict(rc.variant(c, "full"), integrator="euler", substeps=2, move_feet=False))
    print("rollout_grad reference self-check", h, worst, "move_feet off", off, "SELF_REL", gcs.SELF_REL)
    assert gcs.SELF_REL < gcs.SELF_REL_MAX
    assert max(worst, off) <= gcs.SELF_REL, (worst, off)


def test_exact_statements():
    """4: the 2.0 * R_i * u entries to the bit; grad_foot of a leg in swing until its first landing is +-0; move_feet off changes
    grad_foot and takes the landing term out of grad_x0, both against the reference with the same switch."""
    from tests.emu import emu_plant_rollout_grad as eg
    h = 3
    cp = _cparams(h)
    p = rc.params_of(cp)
    c, U, _ = gcs.build(h, 13)
    con = c["contact"] != 0
    own = 2.0 * p["R"][:12] * U.astype(np.float64)
    lands = rc.landings(c["contact"])
    for name in ("plain", "full"):
        kw = dict(rc.variant(c, name), integrator="rk4", substeps=2)
        got = eg.rollout_grad(cp, *_args(c, U), **kw)
        unseen = np.broadcast_to(~con[:, None], (5, 13, h, 2)).copy()
        if name == "full":
            for b in range(5):
                for k in range(h):
                    _, fl, _, _ = gc.transmit(U[b, :, k], np.tile(con[b, k], (13, 1)), np.tile(c["mu"][b], (13, 1)))
                    for g in range(2):
                        unseen[b, :, k, g] |= ((fl >> (2 + g)) & 1).astype(bool)
            assert (unseen & con[:, None]).any()                        # an unloaded stance leg
        entries = np.concatenate([np.repeat(unseen, 3, -1), np.repeat(unseen, 3, -1)], -1)      # [f1 f2 m1 m2] by leg
        assert entries.any() and (U[entries] != 0).any()
        assert np.array_equal(_bits(got["grad_u"][entries]), _bits(own[entries])), name
        assert not np.array_equal(_bits(got["grad_u"][~entries]), _bits(own[~entries]))
        swung = 0
        for b in range(5):
            for g in range(2):
                first = np.flatnonzero(lands[b, :, g])
                if len(first) and not con[b, :first[0] + 1, g].any():
                    assert (got["grad_foot"][b, :, 3 * g:3 * g + 3] == 0.0).all(), (name, b, g)
                    swung += 1
        assert swung >= 2
    idx = [0, 1, 4]
    args = _args(c, U[:, :3], idx)
    kw = dict(rc.take(rc.variant(c, "full"), idx), integrator="rk4", substeps=2)
    on, off = eg.rollout_grad(cp, *args, **kw), eg.rollout_grad(cp, *args, **kw, move_feet=False)
    assert not np.array_equal(on["grad_foot"], off["grad_foot"]) and not np.array_equal(on["grad_x0"], off["grad_x0"])
    for got, move in ((on, True), (off, False)):
        fig = gcs.figures(got, gcs.gradient(p, *args, got["x_traj"], **kw, move_feet=move))
        print("rollout_grad move_feet", move, fig)
        assert max(fig.values()) <= gcs.GRAD_REL, (move, fig)


def test_bad_data_stays_with_its_plan_or_instance():
    """5: a NaN control entry at period k of one plan; a pitch start at pi / 2 (the |cos e1| rule)."""
    from tests.emu import emu_plant_rollout_grad as eg
    h = 3
    cp = _cparams(h)
    p = rc.params_of(cp)
    c, U, _ = gcs.build(h, 13)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    clean = eg.rollout_grad(cp, *_args(c, U), **kw)
    assert (clean["first_bad"] == -1).all()
    bad = U.copy()
    bad[1, 5, 1, 7] = np.nan
    got = eg.rollout_grad(cp, *_args(c, bad), **kw)
    gcs.check_forward(p, got, _args(c, bad), kw, "NaN control")
    assert got["first_bad"][1, 5] == 1 and np.isnan(got["cost"][1, 5])
    for k in gcs.GRADS:
        assert np.isnan(got[k][1, 5]).all(), k
    keep = np.ones((5, 13), bool)
    keep[1, 5] = False
    _same(got, clean, keep)
    x_fb = c["x_fb"].copy()
    x_fb[2, 1] = np.float32(np.pi / 2)
    got = eg.rollout_grad(cp, x_fb, c["foot"], c["contact"], U, **kw)
    assert (got["first_bad"][2] == 0).all() and np.isnan(got["cost"][2]).all() and np.isnan(got["x_traj"][2]).all()
    for k in gcs.GRADS:
        assert np.isnan(got[k][2]).all(), k
    keep = np.ones((5, 13), bool)
    keep[2] = False
    _same(got, clean, keep)


def test_scratch_takes_the_place_of_x_traj():
    """`want` without x_traj: the recorded states live in the scratch, and every other output has the same bits."""
    from tests.emu import emu_plant_rollout_grad as eg
    cp = _cparams(3)
    c, U, _ = gcs.build(3, 3)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    full = eg.rollout_grad(cp, *_args(c, U), **kw)
    for k in gcs.OUTPUTS:
        one = eg.rollout_grad(cp, *_args(c, U), **kw, want=[k])
        assert set(one) == {k}
        _same(one, {k: full[k]})
