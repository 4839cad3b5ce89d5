"""What the device methods of `BatchSolver` hand the library, call by call (the device half of tests/test_api_calls_cpu.py): the
entry, B, steps, which pointers and struct members are NULL, every tensor's address, the scalar struct members, the trailing stream,
and that the tensors a method returns are the ones whose addresses it handed over.  Real tensors on cuda:0, but the library is the
recording stand-in of tests/api_calls.py: nothing of libbmpc is launched.  The expected calls are written by hand from
include/bmpc.h and the methods' docstrings."""
import numpy as np
import pytest

from tests.api_calls import GROUND_ONLY, HANDLE, ROLLOUT, H, S, STEPS, At, Out, St, solver
from biped_mpc_py_amd import _lib

pytestmark = pytest.mark.gpu
B = 3
inf = float("inf")
STREAM = 0x1234          # an explicit `stream=` is passed on as it is (nothing is launched on it here)


@pytest.fixture(scope="module")
def d():
    """Inputs of B instances as the device methods take them, every tensor with an address of its own."""
    import torch
    r = np.random.default_rng(6)
    f = lambda *shape: r.normal(size=shape).astype(np.float32)
    host = dict(x_fb=f(B, 12), foot=f(B, 6), contact=r.integers(0, 2, (B, H, 2)).astype(np.uint8), phase=r.integers(0, H, B).astype(np.int32),
                x_cmd=f(B, 12), mu=f(B, H, 2), x_ref=f(B, H, 12), foot_ref=f(B, H, 6), controls=f(B, H, 12), samples=f(B, S, H, 12),
                u0=f(B, 12), contact0=r.integers(0, 2, (B, 2)).astype(np.uint8), wrench=f(B, 6), push=f(B, 6), t=r.uniform(0, 3, B),
                m=r.uniform(20, 40, B), I=r.normal(size=(B, 3, 3)), g=r.uniform(9, 10, B), gmu=r.uniform(0.2, 0.9, (B, 2)))
    return {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items()}


def at(t):
    return None if t is None else At(t.data_ptr())


def default_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def inputs(d, **over):
    """`bmpc_inputs` of the four required tensors, plus the optional ones named in `over` (None: NULL)."""
    m = dict(x_fb=at(d["x_fb"]), foot=at(d["foot"]), contact=at(d["contact"]), phase=at(d["phase"]))
    m.update(over)
    return St(_lib.CInputs, **{k: v for k, v in m.items() if v is not None})


def run(rows, method, *args, given=(), names=None, **kw):
    """Call `method` of a stand-in solver that expects `rows`; the result as a dict (`names`: of a tuple), without the caller's own
    tensors `given` (which must come back as they went in), checked against the outputs handed over."""
    s = solver(rows, fill=False)
    res = getattr(s, method)(*args, **kw)
    if names is not None:
        res = dict(zip(names, res if isinstance(res, tuple) else (res,)))
    for k in given:
        assert res.pop(k) is kw[k]
    return s._lib.check_outputs(res)


def test_solve_device(d):
    import torch
    f32, i32 = torch.float32, torch.int32
    a = (d["x_fb"], d["foot"], d["contact"], d["phase"])
    four = [at(t) for t in a]
    names = ("controls", "states")
    res = run([("bmpc_solve_batch_device", [HANDLE, B, *four, None, None, Out("controls", f32, (B, H, 12)), None, None, None, None, None,
                                            default_stream()])], "solve_device", *a, names=names)
    assert res["states"] is None
    mine = dict(controls=torch.empty((B, H, 12), dtype=f32, device="cuda:0"), states=torch.empty((B, H, 13), dtype=f32, device="cuda:0"),
                iters=torch.empty(B, dtype=i32, device="cuda:0"), residuals=torch.empty((B, 2), dtype=f32, device="cuda:0"),
                status=torch.empty(B, dtype=i32, device="cuda:0"), nfactor=torch.empty(B, dtype=i32, device="cuda:0"))
    run([("bmpc_solve_batch_device", [HANDLE, B, *four, at(d["x_cmd"]), at(d["mu"]), *[at(t) for t in mine.values()], STREAM])],
        "solve_device", *a, x_cmd=d["x_cmd"], mu=d["mu"], stream=STREAM, names=names, given=names, **mine)
    # a reference switches the entry; `foot` may then be None
    run([("bmpc_solve_inputs_device", [HANDLE, B, inputs(d, mu=at(d["mu"]), x_ref=at(d["x_ref"]), foot_ref=at(d["foot_ref"])),
                                       Out("controls", f32, (B, H, 12)), None, None, None, None, None, default_stream()])],
        "solve_device", *a, mu=d["mu"], x_ref=d["x_ref"], foot_ref=d["foot_ref"], names=names)
    run([("bmpc_solve_inputs_device", [HANDLE, B, inputs(d, foot=None, foot_ref=at(d["foot_ref"])), Out("controls", f32, (B, H, 12)),
                                       at(mine["states"]), None, None, None, None, STREAM])],
        "solve_device", d["x_fb"], None, d["contact"], d["phase"], foot_ref=d["foot_ref"], states=mine["states"], stream=STREAM,
        names=names, given=("states",))


def test_evaluation_family_device(d):
    import torch
    f64, i32 = torch.float64, torch.int32
    a = (d["x_fb"], d["foot"], d["contact"], d["phase"], d["controls"])
    u = at(d["controls"])
    opt = {k: at(d[k]) for k in ("x_cmd", "mu", "x_ref", "foot_ref")}
    kw = {k: d[k] for k in opt}
    st = default_stream()
    ev = dict(cost=Out("cost", f64, (B,)), objective=Out("objective", f64, (B,)), violation=Out("violation", f64, (B, 4)))
    res = run([("bmpc_evaluate_device", [HANDLE, B, inputs(d), u, St(_lib.CEvalOut, **ev), st])], "evaluate_device", *a)
    assert res["states"] is None
    run([("bmpc_evaluate_device", [HANDLE, B, inputs(d, **opt), u, St(_lib.CEvalOut, states=Out("states", f64, (B, H, 13)), **ev), STREAM])],
        "evaluate_device", *a, want_states=True, stream=STREAM, **kw)
    cost, states = torch.empty(B, dtype=f64, device="cuda:0"), torch.empty((B, H, 13), dtype=f64, device="cuda:0")
    run([("bmpc_evaluate_device", [HANDLE, B, inputs(d, foot=None, foot_ref=opt["foot_ref"]), u,
                                   St(_lib.CEvalOut, **dict(ev, cost=at(cost), states=at(states))), st])],
        "evaluate_device", d["x_fb"], None, d["contact"], d["phase"], d["controls"], foot_ref=d["foot_ref"], cost=cost, states=states,
        given=("cost", "states"))

    gr = St(_lib.CGradOut, cost=Out("cost", f64, (B,)), grad_u=Out("grad_u", f64, (B, H, 12)), grad_x0=Out("grad_x0", f64, (B, 12)))
    run([("bmpc_evaluate_grad_device", [HANDLE, B, inputs(d), u, gr, st])], "evaluate_grad_device", *a)
    run([("bmpc_evaluate_grad_device", [HANDLE, B, inputs(d, **opt), u, gr, STREAM])], "evaluate_grad_device", *a, stream=STREAM, **kw)

    ce = St(_lib.CCertOut, lam=Out("lam", f64, (B, H, 36)), resid=Out("resid", f64, (B, H, 12)), summary=Out("summary", f64, (B, 4)),
            n_active=Out("n_active", i32, (B,)), status=Out("status", i32, (B,)))
    run([("bmpc_certify_device", [HANDLE, B, inputs(d), u, 1e-4, ce, st])], "certify_device", *a)
    run([("bmpc_certify_device", [HANDLE, B, inputs(d, **opt), u, 0.25, ce, STREAM])], "certify_device", *a, act_tol=0.25, stream=STREAM, **kw)


def test_evaluate_samples_device(d):
    import torch
    f64, i32 = torch.float64, torch.int32
    a = (d["x_fb"], d["foot"], d["contact"], d["phase"], d["samples"])
    us = at(d["samples"])
    outs = dict(cost=Out("cost", f64, (B, S)), violation=Out("violation", f64, (B, S, 4)), score=Out("score", f64, (B, S)),
                best=Out("best", i32, (B,)), n_valid=Out("n_valid", i32, (B,)), weights=Out("weights", f64, (B, S)),
                u_mean=Out("u_mean", f64, (B, H, 12)), ess=Out("ess", f64, (B,)))
    plain = St(_lib.CSamples, S=S, w_viol=[0.0, 0.0, 0.0, 0.0], temperature=inf)
    run([("bmpc_evaluate_samples_device", [HANDLE, B, inputs(d), us, plain, St(_lib.CSamplesOut, **outs), default_stream()])],
        "evaluate_samples_device", *a)
    res = run([("bmpc_evaluate_samples_device",
                [HANDLE, B, inputs(d, x_cmd=at(d["x_cmd"]), x_ref=at(d["x_ref"])), us, St(_lib.CSamples, S=S, w_viol=[1.0, 2.0, 0.5, 0.0],
                                                                                     temperature=0.75),
                 St(_lib.CSamplesOut, cost=outs["cost"], best=outs["best"]), STREAM])],
              "evaluate_samples_device", *a, x_cmd=d["x_cmd"], x_ref=d["x_ref"], w_viol=(1, 2, 0.5, 0), temperature=0.75,
              want=["best", "cost"], stream=STREAM)
    assert sorted(res) == sorted(outs) and res["score"] is None and res["u_mean"] is None
    weights = torch.empty((B, S), dtype=f64, device="cuda:0")
    run([("bmpc_evaluate_samples_device", [HANDLE, B, inputs(d), us, plain, St(_lib.CSamplesOut, score=outs["score"], weights=at(weights)),
                                           default_stream()])],
        "evaluate_samples_device", *a, want=("score",), weights=weights, given=("weights",))


def test_contact_sequence_and_rollout_device(d):
    import torch
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    names = ("phase", "contact")
    outs = [Out("phase", i32, (B,)), Out("contact", u8, (B, H, 2))]
    run([("bmpc_contact_sequence_device", [HANDLE, B, at(d["t"]), None, *outs, default_stream()])], "contact_sequence_device", d["t"],
        names=names)
    default = ("bmpc_gait_default", [St(_lib.CGait), 5])          # (fetched for this solver's half period; the stand-in leaves it zero)
    gait = St(_lib.CGait, period=12, offset=[0, 6], duty=[7, 5])
    phase = torch.empty(B, dtype=i32, device="cuda:0")
    run([default, ("bmpc_contact_sequence_device", [HANDLE, B, at(d["t"]), gait, at(phase), outs[1], STREAM])], "contact_sequence_device",
        d["t"], phase=phase, period=12, offset=(0, 6), duty=(7, 5), stream=STREAM, names=names, given=("phase",))

    traj = lambda iters=True: [Out("u0", f32, (STEPS, B, 12)), Out("x", f32, (STEPS, B, 12)), Out("iters", i32, (STEPS, B)) if iters else None,
                               Out("status_any", i32, (B,))]
    three = [at(d["x_fb"]), at(d["foot"]), at(d["t"])]
    run([("bmpc_rollout_device", [HANDLE, B, STEPS, *three, None, None, None, *traj(), default_stream()])],
        "rollout_device", d["x_fb"], d["foot"], d["t"], STEPS)
    res = run([default, ("bmpc_rollout_device", [HANDLE, B, STEPS, *three, St(_lib.CGait, period=8), at(d["x_cmd"]), at(d["mu"]), *traj(False),
                                                 STREAM])],
              "rollout_device", d["x_fb"], d["foot"], d["t"], STEPS, x_cmd=d["x_cmd"], mu=d["mu"], period=8, want_iters=False, stream=STREAM)
    assert res["iters"] is None


PLANT = St(_lib.CPlant, integrator=1, substeps=4, move_feet=1)


def test_plant_step_device(d):
    import torch
    f32, u8 = torch.float32, torch.uint8
    a = (d["x_fb"], d["u0"], d["foot"], d["contact0"])
    five = lambda wrench=None: [*[at(t) for t in a], at(wrench)]
    x_next = Out("x_next", f32, (B, 12))
    body = St(_lib.CPlantBody, m=at(d["m"]), I=at(d["I"]))
    st = default_stream()
    one, three = ("x_next",), ("x_next", "u_applied", "flags")
    run([("bmpc_plant_step_device", [HANDLE, B, PLANT, *five(), x_next, st])], "plant_step_device", *a, names=one)
    mine = torch.empty((B, 12), dtype=f32, device="cuda:0")
    run([("bmpc_plant_step_device", [HANDLE, B, St(_lib.CPlant, integrator=0, substeps=7, move_feet=1), *five(d["wrench"]), at(mine), STREAM])],
        "plant_step_device", *a, wrench=d["wrench"], integrator="euler", substeps=7, x_next=mine, stream=STREAM, names=one, given=one)
    run([("bmpc_plant_step_body_device", [HANDLE, B, PLANT, body, *five(), x_next, st])], "plant_step_device", *a,
        body=dict(m=d["m"], I=d["I"]), names=one)
    run([("bmpc_plant_step_body_device", [HANDLE, B, PLANT, St(_lib.CPlantBody, I=at(d["I"]), g=at(d["g"])), *five(), x_next, STREAM])],
        "plant_step_device", *a, body=dict(I=d["I"].reshape(B, 9), g=d["g"]), stream=STREAM, names=one)
    run([("bmpc_plant_step_ground_device", [HANDLE, B, PLANT, None, St(_lib.CPlantGround), *five(), x_next, None, None, st])],
        "plant_step_device", *a, ground={}, names=one)
    run([("bmpc_plant_step_ground_device", [HANDLE, B, PLANT, body, St(_lib.CPlantGround, mu=at(d["gmu"])), *five(d["wrench"]), x_next,
                                            Out("u_applied", f32, (B, 12)), Out("flags", u8, (B,)), STREAM])],
        "plant_step_device", *a, ground=dict(mu=d["gmu"]), body=dict(m=d["m"], I=d["I"]), wrench=d["wrench"], want_applied=True,
        stream=STREAM, names=three)
    run([("bmpc_plant_step_ground_device", [HANDLE, B, PLANT, None, St(_lib.CPlantGround, mu=at(d["gmu"])), *five(), x_next, None, None, st])],
        "plant_step_device", *a, ground=dict(mu=d["gmu"]), names=one)


def test_simulate_device(d):
    import torch
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    a = (d["x_fb"], d["foot"], d["t"], STEPS)
    three = [at(d["x_fb"]), at(d["foot"]), at(d["t"])]
    traj = lambda iters=True: [Out("u0", f32, (STEPS, B, 12)), Out("x", f32, (STEPS, B, 12)), Out("foot", f32, (STEPS, B, 6)),
                               Out("iters", i32, (STEPS, B)) if iters else None, Out("status_any", i32, (B,))]
    st = default_stream()
    run([("bmpc_simulate_device", [HANDLE, B, STEPS, PLANT, *three, None, None, None, None, *traj(), st])], "simulate_device", *a)
    pushed = St(_lib.CPlant, integrator=0, substeps=2, move_feet=0, push_from=1, push_steps=3)
    opts = dict(integrator="euler", substeps=2, move_feet=False, push_from=1, push_steps=3)
    run([("bmpc_gait_default", [St(_lib.CGait), 5]),
         ("bmpc_simulate_device", [HANDLE, B, STEPS, pushed, *three, St(_lib.CGait, period=8), at(d["x_cmd"]), at(d["mu"]), at(d["push"]),
                                   *traj(False), STREAM])],
        "simulate_device", *a, x_cmd=d["x_cmd"], mu=d["mu"], push=d["push"], period=8, want_iters=False, stream=STREAM, **opts)
    body = St(_lib.CPlantBody, m=at(d["m"]), g=at(d["g"]))
    run([("bmpc_simulate_body_device", [HANDLE, B, STEPS, PLANT, body, *three, None, None, None, None, *traj(), None, st])],
        "simulate_device", *a, body=dict(m=d["m"], g=d["g"]))
    outcome = St(_lib.CSimOutcome, tilt_max=0.6, z_min=0.2, first_fall=Out("first_fall", i32, (B,)), max_tilt=Out("max_tilt", f32, (B,)),
                 min_z=Out("min_z", f32, (B,)))
    run([("bmpc_simulate_body_device", [HANDLE, B, STEPS, PLANT, None, *three, None, None, None, at(d["push"]), *traj(), outcome, STREAM])],
        "simulate_device", *a, push=d["push"], fall=(0.6, 0.2), stream=STREAM)
    ground_out = lambda floor: St(_lib.CGroundOut, **dict(
        {} if floor == 0.0 else dict(fz_floor=floor), u_applied=Out("u_applied", f32, (STEPS, B, 12)), flags=Out("contact_flags", u8, (STEPS, B)),
        first_slip=Out("first_slip", i32, (B,)), slip_periods=Out("slip_periods", i32, (B, 2)),
        unloaded_periods=Out("unloaded_periods", i32, (B, 2)), mu_demand=Out("mu_demand", f32, (B,))))
    run([("bmpc_simulate_ground_device", [HANDLE, B, STEPS, PLANT, None, St(_lib.CPlantGround), *three, None, None, None, None, *traj(),
                                          None, ground_out(0.0), st])], "simulate_device", *a, ground={})
    run([("bmpc_simulate_ground_device", [HANDLE, B, STEPS, PLANT, body, St(_lib.CPlantGround, mu=at(d["gmu"])), *three, None, None,
                                          at(d["mu"]), None, *traj(), outcome, ground_out(5.0), STREAM])],
        "simulate_device", *a, mu=d["mu"], body=dict(m=d["m"], g=d["g"]), fall=(0.6, 0.2), ground=dict(mu=d["gmu"]), fz_floor=5.0,
        stream=STREAM)


def test_plant_rollout_samples_device(d):
    import torch
    a = (d["x_fb"], d["foot"], d["contact"], d["samples"])
    three = [at(d["x_fb"]), at(d["foot"]), at(d["contact"])]
    us = at(d["samples"])
    tdt = lambda dt: getattr(torch, np.dtype(dt).name)
    lead = {"B": (B,), "BS": (B, S)}
    out = lambda names: St(_lib.CRolloutOut, **{k: Out(k, tdt(ROLLOUT[k][0]), lead[ROLLOUT[k][1]] + ROLLOUT[k][2:]) for k in names})
    price = St(_lib.CRolloutPrice, S=S, temperature=inf, tilt_max=inf, z_min=-inf)
    entry = "bmpc_plant_rollout_samples_device"
    run([(entry, [HANDLE, B, *three, None, None, None, us, PLANT, None, None, price, out([k for k in ROLLOUT if k not in GROUND_ONLY]),
                  default_stream()])], "plant_rollout_samples_device", *a)
    priced = St(_lib.CRolloutPrice, S=S, w_fall=100.0, w_slip=2.0, w_unloaded=3.0, temperature=0.5, tilt_max=0.6, z_min=0.2, fz_floor=5.0)
    run([(entry, [HANDLE, B, *three, at(d["x_cmd"]), at(d["x_ref"]), at(d["push"]), us,
                  St(_lib.CPlant, integrator=0, substeps=2, move_feet=0, push_from=1, push_steps=3), St(_lib.CPlantBody, g=at(d["g"])),
                  St(_lib.CPlantGround, mu=at(d["gmu"])), priced, out(ROLLOUT), STREAM])],
        "plant_rollout_samples_device", *a, x_cmd=d["x_cmd"], x_ref=d["x_ref"], push=d["push"], push_from=1, push_steps=3,
        integrator="euler", substeps=2, move_feet=False, body=dict(g=d["g"]), ground=dict(mu=d["gmu"]), fall=(0.6, 0.2), fz_floor=5.0,
        w_fall=100.0, w_slip=2.0, w_unloaded=3.0, temperature=0.5, stream=STREAM)
    run([(entry, [HANDLE, B, *three, None, None, None, us, PLANT, None, St(_lib.CPlantGround), price, out(["score", "mu_demand", "best"]),
                  default_stream()])], "plant_rollout_samples_device", *a, ground={}, want=["best", "score", "mu_demand"])
    # B = 0: the outputs come back empty, of their shapes, and the library is not called
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda:0")
    s = solver([], fill=False)
    res = s.plant_rollout_samples_device(e(0, 12), e(0, 6), e(0, H, 2, dt=torch.uint8), e(0, S, H, 12), want=["cost", "x_traj", "best"])
    s._lib.check_outputs({})
    assert {k: (v.dtype, tuple(v.shape)) for k, v in res.items()} == {
        "cost": (torch.float64, (0, S)), "x_traj": (torch.float32, (0, S, H, 12)), "best": (torch.int32, (0,))}
