"""GPU: the gradient of the plant roll-out (`plant_rollout_grad`, `plant_rollout_grad_device`, `plant_cost_torch`) against the
reference written from the definition (tests/rollout_grad_cases.py) and against itself.

Bounds.  Forward: `rollout_cases`' own (2 fp32 ulps per period from the recorded state, cost_bound(h), first_bad the first all-NaN
period).  Gradient: per plan and output max |delta| / max |reference| <= rollout_grad_cases.GRAD_REL, 10 x the larger of the
emulation's and the device's largest figure (docs/history_r26.md), held below 1e-9.  Place independence and host against device: to
the bit.  Bit equality of cost / x_traj with `plant_rollout_samples` on the same inputs is printed, not asserted: a forward pass
compiled in another context may move a cost by an ulp (round 11).  The sizes are small because the reference's Python time
dominates: (B, S) = (5, 3) is at most 60 (plan, period) pairs a case."""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_cases as rc
from tests import rollout_grad_cases as gcs

pytestmark = pytest.mark.gpu
_SOLVERS = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()
    yield
    for s in _SOLVERS.values():
        s.close()
    _SOLVERS.clear()


def _solver(h):
    if h not in _SOLVERS:
        import biped_mpc_py_amd as bm
        mpc = bm.MPC()
        mpc.h = h
        _SOLVERS[h] = bm.BatchSolver(mpc=mpc, biped=bm.Biped(), max_batch=512)
    return _SOLVERS[h]


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _device_kw(kw):
    out = dict(kw)
    for k in ("x_cmd", "x_ref", "push"):
        if out.get(k) is not None:
            out[k] = _cuda(out[k], np.float32)
    for k in ("body", "ground"):
        if out.get(k) is not None:
            out[k] = {m: _cuda(v, np.float64) for m, v in out[k].items()}
    return out


def _device_args(args):
    x, f, c, u = args
    return _cuda(x, np.float32), _cuda(f, np.float32), _cuda(c, np.uint8), _cuda(u, np.float32)


def _device(s, args, kw):
    import torch
    r = s.plant_rollout_grad_device(*_device_args(args), **_device_kw(kw))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b, where=""):
    assert set(a) == set(b), where
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), (where, k)


def _args(c, U, idx=slice(None)):
    return c["x_fb"][idx], c["foot"][idx], c["contact"][idx], U[idx]


@pytest.mark.parametrize("h,integrator,substeps,name", [(4, "rk4", 3, "full"), (4, "euler", 1, "plain"), (1, "rk4", 4, "full"),
                                                        (3, "euler", 2, "full")])
def test_host_and_device_entries_match_the_reference(h, integrator, substeps, name):
    """1, 3: both entries against `gradient` and the forward rules, and against each other to the bit."""
    s = _solver(h)
    p = rc.params_of(s.cparams)
    c, U, counts = gcs.build(h, 3)
    kw = dict(rc.variant(c, name), integrator=integrator, substeps=substeps)
    args = _args(c, U)
    dev = _device(s, args, kw)
    host = s.plant_rollout_grad(*args, **kw)
    assert list(dev) == list(gcs.OUTPUTS)
    _same(host, dev, "host entry against device entry")
    gcs.check_forward(p, dev, args, kw, (h, name, integrator, substeps))
    assert (dev["first_bad"] == -1).all()
    fig = gcs.figures(dev, gcs.gradient(p, *args, dev["x_traj"], **kw))
    fwd = s.plant_rollout_samples(*args, **kw, want=["cost", "x_traj"])
    print("rollout_grad device against the reference", (h, name, integrator, substeps), counts, fig, "GRAD_REL", gcs.GRAD_REL,
          "| forward bits equal to plant_rollout_samples: cost", np.array_equal(_bits(fwd["cost"]), _bits(dev["cost"])),
          "x_traj", np.array_equal(_bits(fwd["x_traj"]), _bits(dev["x_traj"])))
    assert gcs.GRAD_REL < gcs.GRAD_REL_MAX
    assert max(fig.values()) <= gcs.GRAD_REL, fig


def test_a_plan_does_not_depend_on_its_place():
    """2: the (5, 67) launch -- 335 threads, a workgroup boundary inside an instance -- against (1, 1) launches of single plans and a
    (5, 3) launch of plans 0 .. 2, bit for bit."""
    h = 3
    s = _solver(h)
    c, U, _ = gcs.build(h, 67)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    big = _device(s, _args(c, U), kw)
    assert (big["first_bad"] == -1).all()
    for b, j in ((0, 0), (1, 66), (4, 33)):
        one = _device(s, _args(c, U[:, j:j + 1], [b]), rc.take(kw, [b]))
        _same(one, {k: v[b:b + 1, j:j + 1] for k, v in big.items()}, (b, j))
    few = _device(s, _args(c, U[:, :3]), kw)
    _same(few, {k: v[:, :3] for k, v in big.items()}, "plans 0 .. 2")


def test_every_output_alone_and_an_empty_batch():
    """4: `want` with one output at a time (without x_traj the recorded states live in the handle's scratch); B = 0."""
    import torch
    h = 3
    s = _solver(h)
    c, U, _ = gcs.build(h, 3)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    full = _device(s, _args(c, U), kw)
    for k in gcs.OUTPUTS:
        _same(_device(s, _args(c, U), dict(kw, want=[k])), {k: full[k]}, k)
        _same(s.plant_rollout_grad(*_args(c, U), **kw, want=[k]), {k: full[k]}, k)
    empty = s.plant_rollout_grad(c["x_fb"][:0], c["foot"][:0], c["contact"][:0], U[:0], **rc.take(kw, slice(0, 0)))
    assert empty["grad_u"].shape == (0, 3, h, 12) and empty["first_bad"].shape == (0, 3)
    empty = _device(s, _args(c, U, slice(0, 0)), rc.take(kw, slice(0, 0)))
    assert empty["x_traj"].shape == (0, 3, h, 12)
    from biped_mpc_py_amd import _lib
    one = torch.zeros(16, device="cuda")
    out = _lib.CRolloutGradOut(cost=one.data_ptr())
    a = [one.data_ptr()] * 3 + [None] * 3 + [one.data_ptr(), None, None, None]
    assert s._lib.bmpc_plant_rollout_grad_device(s._h, 0, 3, *a, C.byref(out), None) == 0
    assert s._lib.bmpc_plant_rollout_grad_device(s._h, 513, 3, *a, C.byref(out), None) == -1 and b"max_batch" in s._lib.bmpc_last_error()
    assert s._lib.bmpc_plant_rollout_grad_device(s._h, 0, 3, *a, C.byref(_lib.CRolloutGradOut()), None) == -1
    assert s._lib.bmpc_plant_rollout_grad_device(s._h, 1, 3, *a, None, None) == -1


def test_plant_cost_torch_hands_the_gradients_on_and_descends():
    """5: cost.sum().backward() gives controls.grad = grad_u cast, x_fb.grad and foot.grad the sums over s; ten plain gradient steps
    of size 1e-3 / max |grad_u| on one standing instance lower the device's own plant_rollout_samples cost monotonically."""
    import torch
    h = 3
    s = _solver(h)
    c, U, _ = gcs.build(h, 3)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    dkw = _device_kw(kw)
    x, f, con, u = _device_args(_args(c, U))
    ref = s.plant_rollout_grad_device(x, f, con, u, **dkw)
    x.requires_grad_(True)
    f.requires_grad_(True)
    u.requires_grad_(True)
    cost = s.plant_cost_torch(x, f, con, u, **dkw)
    assert cost.dtype == torch.float64 and tuple(cost.shape) == (5, 3) and torch.equal(cost, ref["cost"])
    cost.sum().backward()
    assert u.grad.dtype == torch.float32 and torch.equal(u.grad, ref["grad_u"].to(torch.float32))
    assert torch.equal(x.grad, ref["grad_x0"].sum(1).to(torch.float32)) and torch.equal(f.grad, ref["grad_foot"].sum(1).to(torch.float32))
    w = torch.tensor([[1.0, 0.0, -2.0]], dtype=torch.float64, device="cuda").expand(5, 3)
    u2 = u.detach().clone().requires_grad_(True)
    (s.plant_cost_torch(x.detach(), f.detach(), con, u2, **dkw) * w).sum().backward()
    assert torch.equal(u2.grad, (w[..., None, None] * ref["grad_u"]).to(torch.float32)) and not u2.grad[:, 1].any()
    # descent on one standing instance (double support throughout), its nominal plan
    b = [3]
    xs, fs, cs, us = _device_args(_args(c, U[:, :1], b))
    assert (c["contact"][3] != 0).all()
    costs = []
    for _ in range(11):
        costs.append(float(s.plant_rollout_samples_device(xs, fs, cs, us, want=["cost"])["cost"][0, 0]))
        us.requires_grad_(True)
        s.plant_cost_torch(xs, fs, cs, us).sum().backward()
        g = us.grad
        us = (us.detach() - (1e-3 / float(g.abs().max())) * g).contiguous()
    print("plant_cost_torch descent", costs)
    assert all(b_ < a_ for a_, b_ in zip(costs, costs[1:]))


def test_bad_data_stays_with_its_plan():
    """6: a NaN control entry at period 1 of one plan: its cost and gradients are NaN and its first_bad is 1; every other plan's
    outputs are bit-identical to the clean run."""
    h = 3
    s = _solver(h)
    p = rc.params_of(s.cparams)
    c, U, _ = gcs.build(h, 13)
    kw = dict(rc.variant(c, "full"), integrator="rk4", substeps=2)
    clean = _device(s, _args(c, U), kw)
    assert (clean["first_bad"] == -1).all()
    bad = U.copy()
    bad[1, 5, 1, 7] = np.nan
    got = _device(s, _args(c, bad), kw)
    gcs.check_forward(p, got, _args(c, bad), kw, "NaN control")
    assert got["first_bad"][1, 5] == 1 and np.isnan(got["cost"][1, 5])
    for k in gcs.GRADS:
        assert np.isnan(got[k][1, 5]).all(), k
    keep = np.ones((5, 13), bool)
    keep[1, 5] = False
    _same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()}, "the other plans")


def test_device_method_marshals_as_the_header_says():
    """The device half of tests/test_plant_rollout_grad_api_cpu.py: real tensors, the recording stand-in for the library."""
    import torch
    from tests.api_calls import HANDLE, H, S, At, Out, St, solver
    from biped_mpc_py_amd import _lib
    B = 3
    r = np.random.default_rng(6)
    f = lambda *shape: torch.from_numpy(r.normal(size=shape).astype(np.float32)).cuda()
    d = dict(x_fb=f(B, 12), foot=f(B, 6), contact=torch.ones((B, H, 2), dtype=torch.uint8, device="cuda"), samples=f(B, S, H, 12),
             x_cmd=f(B, 12), x_ref=f(B, H, 12), push=f(B, 6), g=torch.ones(B, dtype=torch.float64, device="cuda"),
             gmu=torch.ones((B, 2), dtype=torch.float64, device="cuda"))
    at = lambda t: At(t.data_ptr())
    shapes = dict(cost=(torch.float64,), grad_u=(torch.float64, H, 12), grad_x0=(torch.float64, 12), grad_foot=(torch.float64, 6),
                  x_traj=(torch.float32, H, 12), first_bad=(torch.int32,))
    out = lambda names: St(_lib.CRolloutGradOut, **{k: Out(k, shapes[k][0], (B, S) + shapes[k][1:]) for k in names})
    three = [at(d["x_fb"]), at(d["foot"]), at(d["contact"])]
    a = (d["x_fb"], d["foot"], d["contact"], d["samples"])
    entry = "bmpc_plant_rollout_grad_device"
    sv = solver([(entry, [HANDLE, B, S, *three, None, None, None, at(d["samples"]), St(_lib.CPlant, integrator=1, substeps=4, move_feet=1),
                          None, None, out(shapes), torch.cuda.current_stream().cuda_stream])], fill=False)
    sv._lib.check_outputs(sv.plant_rollout_grad_device(*a))
    sv = solver([(entry, [HANDLE, B, S, *three, at(d["x_cmd"]), at(d["x_ref"]), at(d["push"]), at(d["samples"]),
                          St(_lib.CPlant, integrator=0, substeps=2, move_feet=0, push_from=1, push_steps=3), St(_lib.CPlantBody, g=at(d["g"])),
                          St(_lib.CPlantGround, mu=at(d["gmu"])), out(["grad_u", "cost"]), 0x1234])], fill=False)
    sv._lib.check_outputs(sv.plant_rollout_grad_device(*a, x_cmd=d["x_cmd"], x_ref=d["x_ref"], push=d["push"], push_from=1, push_steps=3,
                                                       integrator="euler", substeps=2, move_feet=False, body=dict(g=d["g"]),
                                                       ground=dict(mu=d["gmu"]), want=["cost", "grad_u"], stream=0x1234))
