"""GPU: the solver's knobs, caps and self-report (tests/stop_cases.py).  The self-report and non-finite-input cases, and the cap cases
of the variants the emulation builds, run through the emulation first (tests/test_stop_cases_cpu.py); the admissibility and the
ability to fail of EVERY cap case, the device-only ones included, are tests there.
  3. `max_iter = N` returns the model's N-th iterate, says so, and its states are those of its controls -- every kernel variant the
     emulation builds and those it does not (dense h = 8, 12, 18; stage h = 1, 24, 33, 40), plain and -- stage family -- with the
     extrapolation;
  4. what a solve says about itself: iters, nfactor, status, residuals;
  5. the rescue pass hands over instance by instance;
  6. a non-finite input ends its instance with status 2 and touches no other."""
import numpy as np
import pytest

from tests import param_cases as pc
from tests import stop_cases as sc
from tests import util
from tests.gpu_common import built as _built  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu


def _solver(cp, B):
    import biped_mpc_py_amd as bm
    sol = bm.BatchSolver(cparams=cp, max_batch=max(16, B))
    assert sol._lib.bmpc_solver_path(sol._h) == int(cp.path)
    return sol


def _solve(cp, s, states_of_controls=False):
    """`BatchSolver.solve` of batch s on a fresh handle: dict of the six outputs (and `eval_states`: `evaluate(..., want_states=True)`
    of the returned controls)."""
    B = s["x_fb"].shape[0]
    sol = _solver(cp, B)
    states, controls, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], mu=s["mu"])
    out = dict(info, controls=controls, states=states)
    if states_of_controls:
        out["eval_states"] = sol.evaluate(s["x_fb"], s["foot"], s["contact"], s["phase"], controls, x_cmd=s["x_cmd"], mu=s["mu"],
                                          want_states=True)["states"]
    sol.close()
    return out


def _solve_device(cp, s):
    """The same through `solve_device`: every output a tensor of the caller's."""
    import torch
    B, h = s["x_fb"].shape[0], int(cp.h)
    cuda = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()
    o = dict(controls=torch.empty((B, h, 12), dtype=torch.float32, device="cuda"), states=torch.empty((B, h, 13), dtype=torch.float32, device="cuda"),
             iters=torch.empty(B, dtype=torch.int32, device="cuda"), residuals=torch.empty((B, 2), dtype=torch.float32, device="cuda"),
             status=torch.empty(B, dtype=torch.int32, device="cuda"), nfactor=torch.empty(B, dtype=torch.int32, device="cuda"))
    sol = _solver(cp, B)
    sol.solve_device(cuda(s["x_fb"], np.float32), cuda(s["foot"], np.float32), cuda(np.asarray(s["contact"]).reshape(B, h, 2), np.uint8),
                     cuda(s["phase"], np.int32), x_cmd=cuda(s["x_cmd"], np.float32), mu=cuda(s["mu"], np.float32), **o)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    sol.close()
    return out


# ---- 3. the cap returns the N-th iterate ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c["id"] for c in sc.CAP_CASES_GPU + sc.ACCEL_CASES_GPU])
def test_the_cap_returns_the_models_nth_iterate(cid):
    """status 1, iters N, the model's factorisation count, the model's N-th iterate within the case's own bound (from the reference
    alone: stop_cases.cap_reference), and states that `evaluate` confirms for the returned controls: the exit at the cap rebuilds."""
    c = sc._CASES_BY_ID[cid]
    s, cp = sc.case_batch(c), sc.case_block(c)
    assert sc.admissible(c)
    out = _solve(cp, s, states_of_controls=True)
    sc.check_cap(c, out, out["eval_states"], "MI355X")


# ---- 4. what a solve says about itself --------------------------------------------------------------------------------------------------
REPORT_B, REPORT_WIDE = 4, 64            # the emulation's batch, with its assertions; a wider one held to the contract alone
_reports = {}


def _report(path, h, name, B=REPORT_B):
    key = (path, h, name, B)
    if key not in _reports:
        s = sc.report_batch(h, B)
        cp = sc.report_block(path, h, s["half"], name)
        out = _solve(cp, s)
        _reports[key] = (cp, s, out, sc.check_report(cp, s, out, "%s h=%d %s B=%d" % (sc.FAMILY[path], h, name, B)))
    return _reports[key]


@pytest.mark.parametrize("name", list(sc.REPORT_CASES))
@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_a_solve_reports_itself_truthfully(path, h, name):
    cp, s, out, _ = _report(path, h, name)
    st = out["status"]
    if "capped" in name:
        assert (st == 1).all() and (out["iters"] == cp.max_iter).all()
    elif name == "max_refactor_2":
        assert (out["nfactor"] == 3).any() and (st == 0).any()
    else:
        assert (st == 0).all(), st
    if name == "capped_3":
        assert (out["nfactor"] == 1).all() and np.abs(out["residuals"]).min() > 0
    _, _, wide, _ = _report(path, h, name, REPORT_WIDE)          # (check_report asserts the contract on all 64)
    if name == "max_refactor_2":
        assert (wide["nfactor"] == 3).any()


@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_swapped_tolerances_would_show(path, h):
    """As in the emulation (tests/test_stop_cases_cpu.py has the reasoning): the eps_dua-loose run ends with step residuals above the
    tight bound, which is what a kernel with the two fields swapped would return for the eps_pri-loose case."""
    loose, tight = sc.EPS_SWAP
    for B in (REPORT_B, REPORT_WIDE):
        rp_a, rd_a = _report(path, h, "eps_pri_loose", B)[3]
        rp_b, rd_b = _report(path, h, "eps_dua_loose", B)[3]
        other_a = (rp_a * loose > 1.01 * tight) | (rd_a * tight > 1.01 * loose)
        other_b = (rp_b * tight > 1.01 * loose) | (rd_b * loose > 1.01 * tight)
        print("B=%d instances beyond the other pairing's bounds: eps_pri loose %d, eps_dua loose %d" % (B, other_a.sum(), other_b.sum()))
        assert other_b.any()


@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_status_0_means_the_optimum_at_the_default_tolerances(path, h):
    cp, s, out, _ = _report(path, h, "defaults")
    ref = np.stack([pc.oracle_solve(s, i, h, "default")[1] for i in range(REPORT_B)])
    err = util.rel_err(out["controls"], ref)
    print("status 0 against the oracle:", err)
    assert (out["status"] == 0).all() and err.max() <= util.REL_TOL


# ---- 5. the rescue pass, instance by instance -------------------------------------------------------------------------------------------
RESCUE_B, RESCUE_MAX_ITER, RESCUE_SEED = 256, 38, 6100       # (emulation: 64 % of these need more than 35 iterations, 31 % more than 40)


@pytest.mark.parametrize("entry", ["solve", "solve_device"])
def test_rescue_hands_over_instance_by_instance(entry):
    """Dense h = 10 at the reference's weights with an iteration cap near the median count, so that the dense pass leaves a good
    share of the batch unsolved.  With rescue ON every instance the dense pass solved keeps every output bit of the rescue-OFF run,
    and every other instance has the bits of a stage-family handle with the same options (whose penalties resolve alike)."""
    run = _solve if entry == "solve" else _solve_device
    s = sc.batch(10, RESCUE_B, RESCUE_SEED)
    opts = dict(max_iter=RESCUE_MAX_ITER)
    off = run(sc.block(sc.PATH_DENSE, 10, s["half"], rescue=0, **opts), s)
    on = run(sc.block(sc.PATH_DENSE, 10, s["half"], rescue=1, **opts), s)
    cs = sc.block(sc.PATH_STAGE, 10, s["half"], rescue=1, **opts)
    assert sc.effective(cs) == sc.effective(sc.block(sc.PATH_DENSE, 10, s["half"], rescue=1, **opts))
    stage = run(cs, s)
    lost = off["status"] != 0
    print("rescue (%s): %d of %d instances left unsolved by the dense pass at max_iter %d; %d still unsolved after the rescue" % (
        entry, lost.sum(), RESCUE_B, RESCUE_MAX_ITER, (on["status"] != 0).sum()))
    assert 0.2 * RESCUE_B <= lost.sum() <= 0.8 * RESCUE_B
    assert (off["status"][lost] == 1).all() and (off["iters"][lost] == RESCUE_MAX_ITER).all()
    for k in sc.OUT_KEYS:
        assert np.array_equal(on[k][~lost], off[k][~lost]), ("solved by the dense pass", k)
        assert np.array_equal(on[k][lost], stage[k][lost]), ("rescued", k)
    assert not np.array_equal(on["controls"][lost], off["controls"][lost])


# ---- 6. non-finite inputs -------------------------------------------------------------------------------------------------------------
BAD_ROWS_GPU = sc.BAD_ROWS                # (exactly the rows the emulation runs first)
_clean = {}


def _clean_solve(path, h):
    if (path, h) not in _clean:
        s = sc.bad_batch(h)
        cp = sc.block(path, h, s["half"], rescue=0)
        _clean[(path, h)] = (cp, s, _solve(cp, s))
    return _clean[(path, h)]


@pytest.mark.parametrize("name", list(sc.BAD_CASES))
@pytest.mark.parametrize("path,h", BAD_ROWS_GPU)
def test_a_non_finite_input_ends_its_instance_alone(path, h, name):
    cp, s, clean = _clean_solve(path, h)
    out = _solve(cp, sc.poisoned(s, name))
    sc.check_bad(clean, out, int(cp.max_iter), "%s h=%d %s" % (sc.FAMILY[path], h, name))
