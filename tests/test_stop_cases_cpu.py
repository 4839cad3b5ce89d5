"""CPU: the solver's knobs, caps and self-report (tests/stop_cases.py) without a GPU -- the kernels' sources through tests/emu.
  1. the adaptor from a `bmpc_params` block to the model's parameters;
  2. every cap case is admissible and can fail, from the REFERENCE alone;
  3. `max_iter = N` returns the model's N-th iterate, says so, and its states are those of its controls -- plain, and with the
     extrapolation against the model under the kernels' test schedule;
  4. what a solve says about itself: iters, nfactor, status, residuals;
  6. a non-finite input ends its instance with status 2 and touches no other."""
import os
import shutil

import numpy as np
import pytest

from tests import param_cases as pc
from tests import stop_cases as sc
from tests import util


def _emu_available():
    from tests.emu import emu
    return os.path.exists(emu.CLANG) or shutil.which(emu.CLANG)


needs_emu = pytest.mark.skipif(not _emu_available(), reason="host clang (ROCm) not available")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _emu_solve(cp, s):
    from tests.emu import emu
    return emu.solve(cp, s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], mu=s["mu"])


def _emu_states(cp, s, controls):
    from tests.emu import emu_eval
    return emu_eval.evaluate(cp, s["x_fb"], s["foot"], s["contact"], s["phase"], controls, x_cmd=s["x_cmd"], mu=s["mu"])["states"]


# ---- 1. the adaptor -------------------------------------------------------------------------------------------------------------------

@needs_emu
def test_the_adaptor_hands_the_model_what_the_kernels_get():
    """Every field of the model's parameters against the block and against the `bmpc::DevParams` the emulation resolves it to: the five
    penalties are the library's (equal to the emulation's), off their defaults at a scaled block; every knob arrives; the kernels
    that ignore `accel` are modelled without it."""
    from tests.emu import emu
    for path, h, name in ((sc.PATH_DENSE, 10, "default"), (sc.PATH_STAGE, 7, "Q_x10"), (sc.PATH_STAGE, 26, "R_div10"), (sc.PATH_DENSE, 20, "m_20")):
        opts = dict(alpha=1.3, check_every=3, adapt_start=4, adapt_every=7, adapt_early=2, adapt_late=9, adapt_busy=6, adapt_flips=2,
                    confirm_from=1, kappa=7.0, kappa_confirm=50.0, max_refactor=5, eps_pri=3e-6, eps_dua=2e-5, max_iter=77, accel=1)
        cp = sc.block(path, h, 3, name, **opts)
        _, eff = emu.dev_params(cp)
        assert eff == sc.effective(cp)
        P = sc.model_params(cp)
        for k, v in opts.items():
            assert getattr(P, k) == v, (k, getattr(P, k))
        assert (P.h, P.half, P.slow_guard, P.solver) == (h, 3, 1e-6, "riccati" if path == sc.PATH_STAGE else "dense")
        assert [P.rho, P.rho * P.rho_eq_scale, P.rho_lo, P.rho_hi_f, P.rho_hi_m] == pytest.approx(eff, rel=1e-14)
        assert (P.dt, P.kv, P.m, P.g, P.mu) == (cp.dt, cp.kv, cp.m, cp.g, cp.mu) and (P.lt, P.lh) == (cp.lt - 0.01, cp.lh - 0.02)
        assert np.array_equal(P.Q, cp.Q[:12]) and np.array_equal(P.R, cp.R[:12]) and np.array_equal(P.I.reshape(-1), cp.I[:9])
        assert np.array_equal(P.f_max, cp.f_max[:3]) and np.array_equal(P.tau_min, cp.tau_min[:3])
        if name != "default":
            assert eff != sc.effective(sc.block(path, h, 3, "default", **opts))
    assert sc.model_params(sc.block(sc.PATH_DENSE, 12, 6)).accel is False and sc.model_params(sc.block(sc.PATH_STAGE, 22, 11)).accel is False
    assert sc.model_params(sc.block(sc.PATH_STAGE, 12, 6)).accel is True and not sc.model_params(sc.block(sc.PATH_DENSE, 10, 5, accel=0)).accel


def test_the_model_schedule_option_is_off_by_default_and_changes_nothing_without_the_extrapolation():
    """`kernel_schedule` moves the stopping tests, and a test without the secant step moves no iterate: with accel = 0 the option
    gives the same bits; with accel = 1 and the option off the model is the one it was (tests at every check_every from the start:
    a secant step at iteration 5, which the kernels never take)."""
    c = sc.cap_case(sc.PATH_DENSE, 10, 13)
    s, cp = sc.case_batch(c), sc.case_block(c)
    a = sc.model_solve(sc.model_params(cp), s, 13)
    b = sc.model_solve(sc.model_params(cp, kernel_schedule=True), s, 13)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2]["n_factor"], b[2]["n_factor"])
    cp1 = sc.case_block(dict(c, accel=1))
    old7 = sc.model_solve(sc.model_params(cp1, max_iter=7), s, 7)[1]
    new7 = sc.model_solve(sc.model_params(cp1, max_iter=7, kernel_schedule=True), s, 7)[1]
    plain7 = sc.model_solve(sc.model_params(cp, max_iter=7), s, 7)[1]
    assert np.array_equal(new7, plain7) and util.rel_err(old7, plain7).min() > 1e-3


# ---- 2. admissible, and able to fail: from the reference alone ------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c["id"] for c in sc.CAP_CASES_GPU + sc.ACCEL_CASES_GPU])
def test_a_cap_case_is_admissible_and_can_fail(cid):
    """The conditions are the case module's own (stop_cases.assert_admissible_and_can_fail), for the device-only cases too."""
    sc.assert_admissible_and_can_fail(sc._CASES_BY_ID[cid])


def test_the_cap_cases_cover_what_the_issue_names():
    rows = {(c["path"], c["h"]) for c in sc.CAP_CASES_CPU if not c["label"]}
    assert rows == {(1, 10), (1, 16), (1, 20), (2, 7), (2, 10), (2, 14), (2, 22), (2, 26)}
    gpu = {(c["path"], c["h"]) for c in sc.CAP_CASES_GPU if not c["label"]} - rows
    assert gpu == {(1, 12), (1, 8), (1, 18), (2, 1), (2, 33), (2, 40)}
    for p, h in sc.KNOB_ROWS:
        labels = {c["label"] for c in sc.CAP_CASES_CPU if c["label"] and (c["path"], c["h"]) == (p, h)}
        assert labels == {"alpha_1.0", "check_every_3", "adapt_every_0", "max_refactor_0", "max_refactor_2", "kappa_4", "adapt_start_3", "Q_x10"}
    for (p, h), Ns in {**sc.CAP_ROWS_CPU, **sc.CAP_ROWS_GPU_ONLY}.items():
        assert any(N % 5 for N in Ns)
    # before, at and after the first re-classifications (5, 10, 15 at h = 10)
    assert {4, 5, 7, 12}.issubset(sc.CAP_ROWS_CPU[(1, 10)]) and {4, 10, 12}.issubset(sc.CAP_ROWS_CPU[(2, 10)])
    # the extrapolation: the documented exceptions are rows
    acc = {(c["path"], c["h"]) for c in sc.ACCEL_CASES_GPU}
    assert {(1, 12), (2, 22), (2, 24)}.issubset(acc) and not {(1, 10), (1, 16), (1, 20), (1, 8), (1, 18)} & {(c['path'], c['h']) for c in sc.ACCEL_CASES_GPU if c['label'] != sc.LAST_IS_TEST} and all(sc.no_accel(p, h) for p, h in ((1, 12), (2, 22), (2, 24)))


# ---- 3. the cap returns the N-th iterate ------------------------------------------------------------------------------------------------

@needs_emu
@pytest.mark.parametrize("cid", [c["id"] for c in sc.CAP_CASES_CPU + sc.ACCEL_CASES_CPU])
def test_the_cap_returns_the_models_nth_iterate_in_the_emulation(cid):
    c = sc._CASES_BY_ID[cid]
    s, cp = sc.case_batch(c), sc.case_block(c)
    out = _emu_solve(cp, s)
    sc.check_cap(c, out, _emu_states(cp, s, out["controls"]), "emulation")


# ---- 4. what a solve says about itself --------------------------------------------------------------------------------------------------
REPORT_B = 4
_reports = {}


def _report(path, h, name):
    key = (path, h, name)
    if key not in _reports:
        s = sc.report_batch(h, REPORT_B)
        cp = sc.report_block(path, h, s["half"], name)
        out = _emu_solve(cp, s)
        _reports[key] = (cp, s, out, sc.check_report(cp, s, out, "%s h=%d %s" % (sc.FAMILY[path], h, name)))
    return _reports[key]


@needs_emu
@pytest.mark.parametrize("name", list(sc.REPORT_CASES))
@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_a_solve_reports_itself_truthfully_in_the_emulation(path, h, name):
    cp, s, out, _ = _report(path, h, name)
    st = out["status"]
    if "capped" in name:
        assert (st == 1).all() and (out["iters"] == cp.max_iter).all()
    elif name == "max_refactor_2":
        assert (out["nfactor"] == 3).any() and (st == 0).any()      # (the bound is reached; with the budget spent, not every instance converges in time)
    else:
        assert (st == 0).all(), st
    if name == "capped_3":
        assert (out["nfactor"] == 1).all() and np.abs(out["residuals"]).min() > 0       # (the forced test wrote them)


@needs_emu
@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_swapped_tolerances_would_show(path, h):
    """A swap of eps_pri and eps_dua in the parameter mapping must fail test_a_solve_reports_itself_truthfully.  It does if, in the
    two swapped-eps cases, some instance's residuals violate the bounds of the OTHER pairing: the swapped kernel's run of one case IS
    the true kernel's run of the other.  With (loose, tight) = (1e-4, 1e-7), chosen in the emulation: in the eps_dua-loose run the
    step residual of 3 of 4 (dense) / 1 of 4 (stage) instances ends above the tight bound -- that run is what a swapped kernel
    returns for the eps_pri-loose case, whose bound on residuals[:, 1] it fails.  The converse cannot be had with any pair (scanned:
    tight 2e-8 .. 1e-5 against 1e-4, and 2e-7 .. 1e-6 against 1e-7): in this method the primal residual passes any level before the
    step residual does, so the eps_pri-loose run never ends with a primal residual above the tight bound; its count is printed."""
    loose, tight = sc.EPS_SWAP
    rp_a, rd_a = _report(path, h, "eps_pri_loose")[3]
    rp_b, rd_b = _report(path, h, "eps_dua_loose")[3]
    other_a = (rp_a * loose > 1.01 * tight) | (rd_a * tight > 1.01 * loose)      # eps_pri-loose run against (pri tight, dua loose)
    other_b = (rp_b * tight > 1.01 * loose) | (rd_b * loose > 1.01 * tight)      # eps_dua-loose run against (pri loose, dua tight)
    print("instances beyond the other pairing's bounds: eps_pri loose %s, eps_dua loose %s" % (other_a.astype(int), other_b.astype(int)))
    assert other_b.any()


@needs_emu
@pytest.mark.parametrize("path,h", sc.REPORT_ROWS)
def test_status_0_means_the_optimum_at_the_default_tolerances(path, h):
    cp, s, out, _ = _report(path, h, "defaults")
    ref = np.stack([pc.oracle_solve(s, i, h, "default")[1] for i in range(REPORT_B)])
    err = util.rel_err(out["controls"].astype(float), ref)
    print("status 0 against the oracle:", err)
    assert (out["status"] == 0).all() and err.max() <= util.REL_TOL


# ---- 6. non-finite inputs -------------------------------------------------------------------------------------------------------------
_clean = {}


def _clean_solve(path, h):
    if (path, h) not in _clean:
        s = sc.bad_batch(h)
        cp = sc.block(path, h, s["half"], rescue=0)
        _clean[(path, h)] = (cp, s, _emu_solve(cp, s))
    return _clean[(path, h)]


@needs_emu
@pytest.mark.parametrize("name", list(sc.BAD_CASES))
@pytest.mark.parametrize("path,h", sc.BAD_ROWS)
def test_a_non_finite_input_ends_its_instance_alone_in_the_emulation(path, h, name):
    cp, s, clean = _clean_solve(path, h)
    out = _emu_solve(cp, sc.poisoned(s, name))
    sc.check_bad(clean, out, int(cp.max_iter), "%s h=%d %s" % (sc.FAMILY[path], h, name))
