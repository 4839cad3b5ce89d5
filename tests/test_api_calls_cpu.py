"""What the host methods of `BatchSolver` hand the library, call by call: the entry, B, which pointers and struct members are NULL,
the bytes behind every input pointer, the scalar struct members, and that the arrays a method returns are the ones whose addresses
it handed over.  No library and no device: the solver has no handle and its `_lib` is the recording stand-in of tests/api_calls.py.
The expected calls below are written by hand from include/bmpc.h and the methods' docstrings."""
import numpy as np
import pytest

from tests.api_calls import GROUND_ONLY, HANDLE, ROLLOUT, H, S, In, Out, St, solver
from biped_mpc_py_amd import _lib

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
inf = float("inf")


def data(B):
    """Inputs of B instances in the dtypes a caller has them in (fp64, Python ints), every array with values of its own."""
    r = np.random.default_rng(5)
    d = dict(x_fb=r.normal(size=(B, 12)), foot=r.normal(size=(B, 6)), contact=r.integers(0, 2, (B, H, 2)), phase=r.integers(0, H, B),
             x_cmd=r.normal(size=(B, 12)), mu=r.uniform(0.3, 1.0, (B, H, 2)), x_ref=r.normal(size=(B, H, 12)),
             foot_ref=r.normal(size=(B, H, 6)), controls=r.normal(size=(B, H, 12)), samples=r.normal(size=(B, S, H, 12)),
             u0=r.normal(size=(B, 12)), contact0=r.integers(0, 2, (B, 2)), wrench=r.normal(size=(B, 6)), push=r.normal(size=(B, 6)),
             m=r.uniform(20, 40, B), I=r.normal(size=(B, 3, 3)), g=r.uniform(9, 10, B), gmu=r.uniform(0.2, 0.9, (B, 2)),
             t=r.uniform(0, 3, B), q=r.normal(size=(B, 10)), qd=r.normal(size=(B, 10)), pf_w=r.normal(size=(B, 6)))
    return d


def inputs(d, **over):
    """`bmpc_inputs` of the four required arrays, plus the optional ones named in `over` (None: NULL)."""
    m = dict(x_fb=In(d["x_fb"], f32), foot=In(d["foot"], f32), contact=In(d["contact"], u8), phase=In(d["phase"], i32))
    m.update(over)
    return St(_lib.CInputs, **{k: v for k, v in m.items() if v is not None})


def run(rows, method, *args, extra=(), **kw):
    """Call `method` of a stand-in solver that expects `rows`; the result as a dict, checked against the outputs handed over."""
    s = solver(rows)
    res = getattr(s, method)(*args, **kw)
    extra = {k: res.pop(k) for k in extra}
    s._lib.check_outputs(res)
    return res, extra


def as_dict(names):
    return lambda t: dict(zip(names, t))


SOLVE_OUT = lambda B, states=True: [Out("controls", f64, (B, H, 12)), Out("states", f64, (B, H, 13)) if states else None,
                                    Out("iters", i32, (B,)), Out("residuals", f32, (B, 2)), Out("status", i32, (B,)),
                                    Out("nfactor", i32, (B,))]


def solve(rows, d, *a, **kw):
    s = solver(rows)
    states, controls, info = s.solve(d["x_fb"], *a, **kw)
    assert sorted(info) == ["iters", "nfactor", "residuals", "status"]
    s._lib.check_outputs(dict(states=states, controls=controls, **info))
    return states, controls


@pytest.mark.parametrize("B", [3, 0])
def test_solve(B):
    d = data(B)
    four = [In(d["x_fb"], f32), In(d["foot"], f32), In(d["contact"], u8), In(d["phase"], i32)]
    solve([("bmpc_solve_batch_f64", [HANDLE, B, *four, None, None, *SOLVE_OUT(B)])], d, d["foot"], d["contact"], d["phase"])
    states, _ = solve([("bmpc_solve_batch_f64", [HANDLE, B, *four, In(d["x_cmd"], f32), In(d["mu"], f32), *SOLVE_OUT(B, False)])],
                      d, d["foot"], d["contact"], d["phase"], x_cmd=d["x_cmd"], mu=d["mu"], want_states=False)
    assert states is None
    # a reference switches the entry; both, one, and `foot` None with `foot_ref`
    xr, fr = In(d["x_ref"], f32), In(d["foot_ref"], f32)
    solve([("bmpc_solve_inputs_f64", [HANDLE, B, inputs(d, x_ref=xr, foot_ref=fr, mu=In(d["mu"], f32)), *SOLVE_OUT(B)])],
          d, d["foot"], d["contact"], d["phase"], mu=d["mu"], x_ref=d["x_ref"], foot_ref=d["foot_ref"])
    solve([("bmpc_solve_inputs_f64", [HANDLE, B, inputs(d, x_ref=xr), *SOLVE_OUT(B)])],
          d, d["foot"], d["contact"], d["phase"], x_ref=d["x_ref"])
    solve([("bmpc_solve_inputs_f64", [HANDLE, B, inputs(d, foot=None, foot_ref=fr), *SOLVE_OUT(B, False)])],
          d, None, d["contact"], d["phase"], foot_ref=d["foot_ref"], want_states=False)
    # out=: the caller's arrays are the ones handed over and returned
    mine = (np.empty((B, H, 13)), np.empty((B, H, 12)))
    states, controls = solve([("bmpc_solve_batch_f64", [HANDLE, B, *four, None, None, *SOLVE_OUT(B)])],
                             d, d["foot"], d["contact"], d["phase"], out=mine)
    assert states is mine[0] and controls is mine[1]
    states, controls = solve([("bmpc_solve_batch_f64", [HANDLE, B, *four, None, None, *SOLVE_OUT(B, False)])],
                             d, d["foot"], d["contact"], d["phase"], out=(None, mine[1]))
    assert states is None and controls is mine[1]
    states, controls = solve([("bmpc_solve_batch_f64", [HANDLE, B, *four, None, None, *SOLVE_OUT(B, False)])],
                             d, d["foot"], d["contact"], d["phase"], out=mine, want_states=False)
    assert states is None and controls is mine[1]


@pytest.mark.parametrize("B", [3, 0])
def test_evaluation_family(B):
    d = data(B)
    a = (d["x_fb"], d["foot"], d["contact"], d["phase"], d["controls"])
    u = In(d["controls"], f32)
    opt = dict(x_cmd=In(d["x_cmd"], f32), mu=In(d["mu"], f32), x_ref=In(d["x_ref"], f32), foot_ref=In(d["foot_ref"], f32))
    kw = {k: d[k] for k in opt}
    ev = dict(cost=Out("cost", f64, (B,)), objective=Out("objective", f64, (B,)), violation=Out("violation", f64, (B, 4)))
    res, _ = run([("bmpc_evaluate", [HANDLE, B, inputs(d), u, St(_lib.CEvalOut, **ev)])], "evaluate", *a)
    assert res["states"] is None
    run([("bmpc_evaluate", [HANDLE, B, inputs(d, **opt), u, St(_lib.CEvalOut, states=Out("states", f64, (B, H, 13)), **ev)])],
        "evaluate", *a, want_states=True, **kw)
    run([("bmpc_evaluate", [HANDLE, B, inputs(d, foot=None, foot_ref=opt["foot_ref"]), u, St(_lib.CEvalOut, **ev)])],
        "evaluate", d["x_fb"], None, d["contact"], d["phase"], d["controls"], foot_ref=d["foot_ref"])

    gr = St(_lib.CGradOut, cost=Out("cost", f64, (B,)), grad_u=Out("grad_u", f64, (B, H, 12)), grad_x0=Out("grad_x0", f64, (B, 12)))
    run([("bmpc_evaluate_grad", [HANDLE, B, inputs(d), u, gr])], "evaluate_grad", *a)
    run([("bmpc_evaluate_grad", [HANDLE, B, inputs(d, **opt), u, gr])], "evaluate_grad", *a, **kw)

    ce = St(_lib.CCertOut, lam=Out("lam", f64, (B, H, 36)), resid=Out("resid", f64, (B, H, 12)), summary=Out("summary", f64, (B, 4)),
            n_active=Out("n_active", i32, (B,)), status=Out("status", i32, (B,)))
    columns = ("stationarity", "primal_ineq", "complementarity", "grad_scale")
    for tol, more, ins in ((1e-4, {}, inputs(d)), (0.25, dict(act_tol=0.25, **kw), inputs(d, **opt))):
        res, cols = run([("bmpc_certify", [HANDLE, B, ins, u, tol, ce])], "certify", *a, extra=columns, **more)
        for i, k in enumerate(columns):
            assert np.array_equal(cols[k], res["summary"][:, i])

    a = (d["x_fb"], d["foot"], d["contact"], d["phase"], d["samples"])
    us = In(d["samples"], f32)
    so = St(_lib.CSamplesOut, cost=Out("cost", f64, (B, S)), violation=Out("violation", f64, (B, S, 4)), score=Out("score", f64, (B, S)),
            best=Out("best", i32, (B,)), n_valid=Out("n_valid", i32, (B,)), weights=Out("weights", f64, (B, S)),
            u_mean=Out("u_mean", f64, (B, H, 12)), ess=Out("ess", f64, (B,)))
    run([("bmpc_evaluate_samples", [HANDLE, B, inputs(d), us, St(_lib.CSamples, S=S, w_viol=[0.0, 0.0, 0.0, 0.0], temperature=inf), so])],
        "evaluate_samples", *a)
    run([("bmpc_evaluate_samples", [HANDLE, B, inputs(d, **opt), us, St(_lib.CSamples, S=S, w_viol=[1.0, 2.0, 0.5, 0.0], temperature=0.75),
                                    so])], "evaluate_samples", *a, w_viol=(1, 2, 0.5, 0), temperature=0.75, **kw)


@pytest.mark.parametrize("B", [3, 0])
def test_assemble(B):
    d = data(B)
    a = (d["x_fb"], d["foot"], d["contact"], d["phase"])
    four = [In(d["x_fb"], f32), In(d["foot"], f32), In(d["contact"], u8), In(d["phase"], i32)]
    outs = lambda matrices=True: [Out("x_ref", f64, (B, H, 12)), Out("foot_ref", f64, (B, H, 6)),
                                  Out("Gt", f64, (B, 6 * H, 6 * H)) if matrices else None, Out("qt", f64, (B, 6 * H)) if matrices else None]
    names = as_dict(("x_ref", "foot_ref", "Gt", "qt"))
    for rows, args, kw in (
            ([("bmpc_debug_assemble", [HANDLE, B, *four, None, None, *outs()])], a, {}),
            ([("bmpc_debug_assemble", [HANDLE, B, *four, In(d["x_cmd"], f32), In(d["mu"], f32), *outs(False)])], a,
             dict(x_cmd=d["x_cmd"], mu=d["mu"], want_matrices=False)),
            ([("bmpc_debug_assemble_inputs", [HANDLE, B, inputs(d, x_ref=In(d["x_ref"], f32)), *outs()])], a, dict(x_ref=d["x_ref"])),
            ([("bmpc_debug_assemble_inputs", [HANDLE, B, inputs(d, foot=None, foot_ref=In(d["foot_ref"], f32)), *outs(False)])],
             (d["x_fb"], None, d["contact"], d["phase"]), dict(foot_ref=d["foot_ref"], want_matrices=False))):
        s = solver(rows)
        s._lib.check_outputs(names(s.assemble(*args, **kw)))


PLANT = St(_lib.CPlant, integrator=1, substeps=4, move_feet=1)


@pytest.mark.parametrize("B", [3, 0])
def test_plant_step(B):
    d = data(B)
    five = lambda wrench=None: [In(d["x_fb"], f32), In(d["u0"], f32), In(d["foot"], f32), In(d["contact0"] != 0, u8), wrench]
    x_next = Out("x_next", f32, (B, 12), returned=f64)
    a = (d["x_fb"], d["u0"], d["foot"], d["contact0"])
    one = lambda x: dict(x_next=x)
    body = St(_lib.CPlantBody, m=In(d["m"], f64), I=In(d["I"], f64))
    for rows, kw, names in (
            ([("bmpc_plant_step", [HANDLE, B, PLANT, *five(), x_next])], {}, one),
            ([("bmpc_plant_step", [HANDLE, B, St(_lib.CPlant, integrator=0, substeps=7, move_feet=1), *five(In(d["wrench"], f32)), x_next])],
             dict(wrench=d["wrench"], integrator="euler", substeps=7), one),
            ([("bmpc_plant_step_body", [HANDLE, B, PLANT, body, *five(), x_next])], dict(body=dict(m=d["m"], I=d["I"])), one),
            ([("bmpc_plant_step_body", [HANDLE, B, PLANT, St(_lib.CPlantBody, I=In(d["I"], f64), g=In(d["g"], f64)), *five(), x_next])],
             dict(body=dict(I=d["I"].reshape(B, 9), g=d["g"])), one),
            ([("bmpc_plant_step_ground", [HANDLE, B, PLANT, None, St(_lib.CPlantGround), *five(), x_next, None, None])],
             dict(ground={}), one),
            ([("bmpc_plant_step_ground", [HANDLE, B, PLANT, body, St(_lib.CPlantGround, mu=In(d["gmu"], f64)), *five(In(d["wrench"], f32)),
                                          x_next, Out("u_applied", f32, (B, 12)), Out("flags", u8, (B,))])],
             dict(ground=dict(mu=d["gmu"]), body=dict(m=d["m"], I=d["I"]), wrench=d["wrench"], want_applied=True),
             as_dict(("x_next", "u_applied", "flags"))),
            ([("bmpc_plant_step_ground", [HANDLE, B, PLANT, None, St(_lib.CPlantGround, mu=In(d["gmu"], f64)), *five(), x_next, None, None])],
             dict(ground=dict(mu=d["gmu"])), one)):
        s = solver(rows)
        s._lib.check_outputs(names(s.plant_step(*a, **kw)))


def rollout_out(B, names):
    """`bmpc_rollout_out` with the outputs `names`, each of its documented dtype and shape."""
    lead = {"B": (B,), "BS": (B, S)}
    return St(_lib.CRolloutOut, **{k: Out(k, ROLLOUT[k][0], lead[ROLLOUT[k][1]] + ROLLOUT[k][2:]) for k in names})


@pytest.mark.parametrize("B", [3, 0])
def test_plant_rollout_samples(B):
    d = data(B)
    a = (d["x_fb"], d["foot"], d["contact"], d["samples"])
    three = [In(d["x_fb"], f32), In(d["foot"], f32), In(d["contact"], u8)]
    us = In(d["samples"], f32)
    price = St(_lib.CRolloutPrice, S=S, temperature=inf, tilt_max=inf, z_min=-inf)
    run([("bmpc_plant_rollout_samples", [HANDLE, B, *three, None, None, None, us, PLANT, None, None, price,
                                         rollout_out(B, [k for k in ROLLOUT if k not in GROUND_ONLY])])], "plant_rollout_samples", *a)
    priced = St(_lib.CRolloutPrice, S=S, w_fall=100.0, w_slip=2.0, w_unloaded=3.0, temperature=0.5, tilt_max=0.6, z_min=0.2, fz_floor=5.0)
    run([("bmpc_plant_rollout_samples",
          [HANDLE, B, *three, In(d["x_cmd"], f32), In(d["x_ref"], f32), In(d["push"], f32), us,
           St(_lib.CPlant, integrator=0, substeps=2, move_feet=0, push_from=1, push_steps=3), St(_lib.CPlantBody, g=In(d["g"], f64)),
           St(_lib.CPlantGround, mu=In(d["gmu"], f64)), priced, rollout_out(B, ROLLOUT)])],
        "plant_rollout_samples", *a, x_cmd=d["x_cmd"], x_ref=d["x_ref"], push=d["push"], push_from=1, push_steps=3, integrator="euler",
        substeps=2, move_feet=False, body=dict(g=d["g"]), ground=dict(mu=d["gmu"]), fall=(0.6, 0.2), fz_floor=5.0, w_fall=100.0,
        w_slip=2.0, w_unloaded=3.0, temperature=0.5)
    run([("bmpc_plant_rollout_samples", [HANDLE, B, *three, None, None, None, us, PLANT, None, St(_lib.CPlantGround), price,
                                         rollout_out(B, ["score", "mu_demand", "best"])])],
        "plant_rollout_samples", *a, ground={}, want=["best", "score", "mu_demand"])
    run([("bmpc_plant_rollout_samples", [HANDLE, B, *three, None, None, None, us, PLANT, None, None, price, rollout_out(B, ["x_end"])])],
        "plant_rollout_samples", *a, want=("x_end",))


@pytest.mark.parametrize("B", [3, 0])
def test_contact_sequence(B):
    d = data(B)
    names = as_dict(("phase", "contact"))
    outs = [Out("phase", i32, (B,)), Out("contact", u8, (B, H, 2))]
    s = solver([("bmpc_contact_sequence", [HANDLE, B, In(d["t"], f64), None, *outs])])
    s._lib.check_outputs(names(s.contact_sequence(d["t"])))
    s = solver([("bmpc_contact_sequence", [HANDLE, B, In(d["t"], f64), None, outs[0], None])])
    s._lib.check_outputs(names(s.contact_sequence(d["t"], want_contact=False)))
    # a gait keyword: the default schedule is fetched for this solver's half period (the stand-in leaves it zero), then overridden
    default = ("bmpc_gait_default", [St(_lib.CGait), 5])
    s = solver([default, ("bmpc_contact_sequence", [HANDLE, B, In(d["t"], f64), St(_lib.CGait, period=8), *outs])])
    s._lib.check_outputs(names(s.contact_sequence(d["t"], period=8)))
    s = solver([default, ("bmpc_contact_sequence", [HANDLE, B, In(d["t"], f64), St(_lib.CGait, period=12, offset=[0, 6], duty=[7, 5]),
                                                    *outs])])
    s._lib.check_outputs(names(s.contact_sequence(d["t"], period=12, offset=(0, 6), duty=(7, 5))))


@pytest.mark.parametrize("B", [3, 0])
def test_foot_position_and_low_level_control(B):
    d = data(B)
    s = solver([("bmpc_foot_position_world", [HANDLE, B, In(d["x_fb"], f32), In(d["q"], f32), Out("pf_w", f32, (B, 6), returned=f64)])])
    s._lib.check_outputs(dict(pf_w=s.foot_position_world(d["x_fb"], d["q"])))
    s = solver([("bmpc_low_level_control", [HANDLE, B, In(d["x_fb"], f32), In(d["t"], f64), In(d["pf_w"], f32), In(d["q"], f32),
                                            In(d["qd"], f32), In(d["contact0"], u8), In(d["u0"], f32),
                                            Out("tau", f32, (B, 10), returned=f64)])])
    s._lib.check_outputs(dict(tau=s.low_level_control(d["x_fb"], d["t"], d["pf_w"], d["q"], d["qd"], d["contact0"], d["u0"])))
