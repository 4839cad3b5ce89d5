"""GPU: reference tracking -- caller-supplied x_ref / foot_ref (include/bmpc.h `bmpc_inputs`, ABI 12) through both kernel families,
the C ABI and the Python API, against the reference's own solve_mpc with its generators replaced (tests/golden/ref_tracking.npz) and
the oracle the same way (tests/refs_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import refs_cases as rc
from tests import util

pytestmark = pytest.mark.gpu

PATH_DENSE, PATH_STAGE = 1, 2


def _solver(h, path=PATH_DENSE, half=None, max_batch=4096, mod=None, **opts):
    import biped_mpc_py_amd as bm
    mpc = bm.MPC()
    mpc.h = h
    if mod is not None:
        mod(mpc)
    return bm.BatchSolver(mpc=mpc, half=half if half is not None else h // 2, max_batch=max_batch,
                          solver_options=dict(path=path, **opts))


def _kernel(s, h):
    import biped_mpc_py_amd as bm
    return bm.references_to_kernel_layout(s["x_ref"], s["foot_ref"], h)


def _same(a, b, keys=("iters", "nfactor", "status")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("path", [PATH_DENSE, PATH_STAGE])
def test_new_entries_without_references_are_the_abi11_entries(path):
    """1. Nothing supplied, through bmpc_solve_inputs_f64 / _device: bit-identical to bmpc_solve_batch_f64 / _device."""
    import torch
    from biped_mpc_py_amd import _lib
    from biped_mpc_py_amd.api import _ptr
    B, h = 4096, 10
    s = util.synth_batch(B, h, 5, gait="walking", vx_cmd=True)
    sol = _solver(h, path, half=s["half"])
    lib = sol._lib
    x = np.ascontiguousarray(s["x_fb"], np.float32); f = np.ascontiguousarray(s["foot"], np.float32)
    con = np.ascontiguousarray(s["contact"], np.uint8); ph = np.ascontiguousarray(s["phase"], np.int32)
    xc = np.ascontiguousarray(s["x_cmd"], np.float32)

    def host(fn, *pre):
        u = np.empty((B, h, 12)); st = np.empty((B, h, 13))
        o = dict(iters=np.empty(B, np.int32), status=np.empty(B, np.int32), nfactor=np.empty(B, np.int32), res=np.empty((B, 2), np.float32))
        _lib.check(fn(sol._h, B, *pre, _ptr(u), _ptr(st), _ptr(o["iters"]), _ptr(o["res"]), _ptr(o["status"]), _ptr(o["nfactor"])))
        return u, st, o

    inp = _lib.CInputs(_ptr(x), _ptr(f), _ptr(con), _ptr(ph), _ptr(xc), None, None, None)
    u0, s0, o0 = host(lib.bmpc_solve_batch_f64, _ptr(x), _ptr(f), _ptr(con), _ptr(ph), _ptr(xc), None)
    u1, s1, o1 = host(lib.bmpc_solve_inputs_f64, C.byref(inp))
    assert np.array_equal(u0, u1) and np.array_equal(s0, s1)
    _same(o0, o1)
    assert (o0["status"] == 0).all()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(a).to(dev)
    tx, tf, tc, tp, txc = T(x), T(f), T(con), T(ph), T(xc)

    def device(with_inputs):
        u = torch.empty((B, h, 12), dtype=torch.float32, device=dev); st = torch.empty((B, h, 13), dtype=torch.float32, device=dev)
        o = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in ("iters", "status", "nfactor")}
        if with_inputs:
            di = _lib.CInputs(tx.data_ptr(), tf.data_ptr(), tc.data_ptr(), tp.data_ptr(), txc.data_ptr(), None, None, None)
            _lib.check(lib.bmpc_solve_inputs_device(sol._h, B, C.byref(di), u.data_ptr(), st.data_ptr(), o["iters"].data_ptr(), None,
                                                    o["status"].data_ptr(), o["nfactor"].data_ptr(), None))
        else:
            _lib.check(lib.bmpc_solve_batch_device(sol._h, B, tx.data_ptr(), tf.data_ptr(), tc.data_ptr(), tp.data_ptr(), txc.data_ptr(),
                                                   None, u.data_ptr(), st.data_ptr(), o["iters"].data_ptr(), None, o["status"].data_ptr(),
                                                   o["nfactor"].data_ptr(), None))
        torch.cuda.synchronize()
        return u.cpu().numpy(), st.cpu().numpy(), {k: v.cpu().numpy() for k, v in o.items()}

    d0, ds0, do0 = device(False)
    d1, ds1, do1 = device(True)
    assert np.array_equal(d0, d1) and np.array_equal(ds0, ds1)
    _same(do0, do1)
    assert np.array_equal(d0.astype(np.float64), u0)
    sol.close()


@pytest.mark.parametrize("path", [PATH_DENSE, PATH_STAGE])
def test_generator_output_fed_back_is_the_generated_solve(path):
    """2. The generators' own output (reference_trajectories_batch) supplied back, standing with zero commanded velocity: the same
    bits as the generated path.  (x_cmd is passed per instance, i.e. in fp32: from the parameter block the generator would take
    the commanded height 0.55 in fp64, which no fp32 reference holds.)"""
    import biped_mpc_py_amd as bm
    B, h = 1024, 10
    s = util.synth_batch(B, h, 21, gait="standing")
    x_fb = s["x_fb"].astype(np.float32).astype(float)
    x_fb[:, 6:] = 0.0
    mpc = bm.MPC()
    x_cmd = np.tile(np.asarray(mpc.x_cmd, np.float32), (B, 1))
    xr, fr = bm.reference_trajectories_batch(x_fb, None, s["foot"], s["contact"], mpc=mpc, x_cmd=x_cmd, phase=s["phase"])
    sol = _solver(h, path, half=s["half"], max_batch=B)
    st0, u0, i0 = sol.solve(x_fb, s["foot"], s["contact"], s["phase"], x_cmd=x_cmd)
    xk, fk = bm.references_to_kernel_layout(xr, fr, h)
    st1, u1, i1 = sol.solve(x_fb, s["foot"], s["contact"], s["phase"], x_cmd=x_cmd, x_ref=xk, foot_ref=fk)
    st2, u2, i2 = sol.solve(x_fb, None, s["contact"], s["phase"], x_cmd=x_cmd, x_ref=xk, foot_ref=fk)     # foot unused with foot_ref
    assert np.array_equal(u0, u1) and np.array_equal(st0, st1) and np.array_equal(u1, u2) and np.array_equal(st1, st2)
    _same(i0, i1)
    sol.close()


@pytest.mark.parametrize("path", [PATH_DENSE, PATH_STAGE])
@pytest.mark.parametrize("h", [10, 16, 20])
def test_fixture_instances_match_the_reference(path, h):
    """3. Every instance of ref_tracking.npz (the reference's own solve_mpc, generators replaced) within REL_TOL, status 0."""
    d = util.load("ref_tracking")
    s = {k[len(f"h{h}_"):]: d[k] for k in d.files if k.startswith(f"h{h}_")}
    xr, fr = _kernel(s, h)
    sol = _solver(h, path, half=int(s["half"]), max_batch=64)
    st, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
    sol.close()
    e = util.rel_err(u, s["controls"])
    print("h=%d path %d: max err %.2e (kind %s), iterations %.1f" % (h, path, e.max(), s["kind"][e.argmax()], info["iters"].mean()))
    assert (info["status"] == 0).all()
    assert e.max() <= util.REL_TOL
    assert util.rel_err(st, s["states"]).max() <= util.REL_TOL


_SCALE = [(10, PATH_DENSE, 41), (20, PATH_DENSE, 42), (20, PATH_STAGE, 43), (13, PATH_STAGE, 44), (32, PATH_STAGE, 45)]


@pytest.mark.parametrize("h,path,seed", _SCALE)
def test_tracking_at_scale_against_the_oracle(h, path, seed):
    """4. 4096 seeded instances mixing kinds a-e: every status 0; 256 sampled against the oracle with its generators replaced."""
    B = 4096
    s = rc.make_batch(B, h, seed, kinds="abcde")
    xr, fr = _kernel(s, h)
    sol = _solver(h, path, half=s["half"], max_batch=B)
    _, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr, want_states=False)
    sol.close()
    assert (info["status"] == 0).all(), np.flatnonzero(info["status"])[:8]
    idx = np.random.default_rng(seed).choice(B, 256, replace=False)
    ref, ok = rc.oracle_batch(s, idx, h)
    assert ok.mean() > 0.99
    e, e0 = util.rel_err(u[idx], ref)[ok], util.u0_err(u[idx], ref)[ok]
    print("h=%d path %d: all controls max %.2e | u0 max %.2e | iterations %.2f (max %d), factorisations %.2f" % (
        h, path, e.max(), e0.max(), info["iters"].mean(), info["iters"].max(), info["nfactor"].mean()))
    assert e.max() <= util.REL_TOL and e0.max() <= util.REL_TOL
    # the regression bounds of test_parity_against_the_oracle_at_scale (measured on MI355X: maxima 1.2e-6 / 1.2e-6 over these cases)
    assert e.max() <= 5e-6 and e0.max() <= 1e-5, (e.max(), e0.max())


def test_assembly_returns_the_supplied_references_and_their_qp():
    """5. assemble(x_ref=, foot_ref=) hands the supplied arrays back (fp64) and builds Gt / qt from them: against
    orc.build_condensed_qp with the generators replaced, within the assembly test's 2e-6."""
    from oracle import bmpc_oracle as orc
    h = 10
    d = util.load("ref_tracking")
    s = {k[4:]: d[k] for k in d.files if k.startswith("h10_")}
    xr, fr = _kernel(s, h)
    sol = _solver(h, PATH_DENSE, half=int(s["half"]), max_batch=64)
    x_ref, foot_ref, Gt, qt = sol.assemble(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
    sol.close()
    assert np.array_equal(x_ref, xr.astype(np.float32).astype(float)) and np.array_equal(foot_ref, fr.astype(np.float32).astype(float))
    for i in range(len(s["kind"])):
        m = orc.MPC()
        m.h, m.x_cmd = h, s["x_cmd"][i].astype(float)
        with rc.supplied(orc, s["x_ref"][i], s["foot_ref"][i]):
            c = orc.build_condensed_qp(s["x_fb"][i].astype(float), float(s["t"][i]), s["foot"][i].astype(float), m, orc.Biped(),
                                       s["contact"][i], half=int(s["half"]))
        # Hc = Wbar' Gt Wbar + 2 Rbar, gc = Wbar' qt from what the assembly returns (test_assembly_is_the_condensed_qp_of_the_oracle)
        r = foot_ref[i].reshape(h, 2, 3) - x_ref[i][:, None, 3:6]
        W = util.wrench_map(r)
        Hc = W.T @ Gt[i] @ W + 2 * np.kron(np.eye(h), np.diag(np.asarray(m.R, float)))
        gc = W.T @ qt[i]
        eh = np.abs(Hc - c["Hc"]).max() / np.abs(c["Hc"]).max()
        eg = np.abs(gc - c["gc"]).max() / max(1.0, np.abs(c["gc"]).max())
        print(i, s["kind"][i], "Hc rel err %.2e gc rel err %.2e" % (eh, eg))
        assert eh <= 2e-6 and eg <= 2e-6, (i, s["kind"][i])


def test_solve_device_with_references_is_solve():
    """6. solve_device with torch tensors: bit-identical to solve with the same references."""
    import torch
    h, B = 10, 512
    s = rc.make_batch(B, h, 61)
    xr, fr = _kernel(s, h)
    for path in (PATH_DENSE, PATH_STAGE):
        sol = _solver(h, path, half=s["half"], max_batch=B)
        st, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
        dev = torch.device("cuda:0")
        T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
        sd = torch.empty((B, h, 13), dtype=torch.float32, device=dev)
        it = torch.empty(B, dtype=torch.int32, device=dev)
        uc, _ = sol.solve_device(T(s["x_fb"]), None, T(s["contact"], torch.uint8), T(s["phase"], torch.int32), x_cmd=T(s["x_cmd"]),
                                 states=sd, iters=it, x_ref=T(xr), foot_ref=T(fr))
        torch.cuda.synchronize()
        assert np.array_equal(uc.cpu().numpy().astype(float), u) and np.array_equal(sd.cpu().numpy().astype(float), st)
        assert np.array_equal(it.cpu().numpy(), info["iters"])
        sol.close()


def test_rescue_pass_solves_against_the_supplied_references():
    """7. The existing rescue configuration (h = 20, Q x 10, uncapped ceilings): with references far from the generated ones the
    dense family alone loses instances, the rescue pass solves them -- to the oracle's optimum FOR THE SUPPLIED references."""
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd.params import RESCUE_OFF, RESCUE_ON
    h, B = 20, 16384
    s = util.synth_batch(B, h, 97, gait="standing", per_step_mu=True)
    s = dict(s)
    s["x_cmd"] = np.tile(bm.MPC().x_cmd.astype(np.float32).astype(float), (B, 1))
    s["t"] = (s["phase"] + 0.5) * 0.04
    xr, fr = bm.reference_trajectories_batch(s["x_fb"], None, s["foot"], s["contact"], phase=s["phase"], mpc=_mpc(h))
    tj = np.arange(h) * 0.04
    xr = xr.copy()
    xr[:, 5, 1:] -= 0.08 * tj[1:] / tj[-1]              # a crouch ...
    xr[:, 11, 1:] = -0.08 / tj[-1]
    xr[:, 0, 1:] += 0.3 * tj[1:]                        # ... while turning
    xr[:, 8, 1:] = 0.3
    xr = xr.astype(np.float32).astype(float); xr[:, 12] = 1.0
    fr = fr.astype(np.float32).astype(float)
    s["x_ref"], s["foot_ref"] = xr, fr
    xk, fk = bm.references_to_kernel_layout(xr, fr, h)
    bad = dict(penalty_mode=1, rho=0.1423, rho_eq_scale=300.0 / 0.1423, rho_hi_f=10.0, rho_hi_m=500.0)
    q10 = lambda m: setattr(m, "Q", np.asarray(m.Q, float) * 10.0)

    def run(mode):
        sol = _solver(h, PATH_DENSE, half=s["half"], max_batch=B, mod=q10, rescue=mode, **bad)
        _, u, info = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], mu=s["mu"], x_ref=xk, foot_ref=fk, want_states=False)
        sol.close()
        return u, info

    u0, i0 = run(RESCUE_OFF)
    u1, i1 = run(RESCUE_ON)
    lost = np.flatnonzero(i0["status"])
    print("h=20 Q_x10, supplied references: dense path alone loses %d %s" % (len(lost), lost[:6]))
    assert len(lost) >= 1                               # (seed 97: 2 of 16384 on MI355X)
    assert (i1["status"] == 0).all()
    keep = np.setdiff1d(np.arange(B), lost)
    assert np.array_equal(u1[keep], u0[keep])
    pick = lost[:4]
    ref, ok = rc.oracle_batch(s, pick, h, Q_scale=10.0)
    gen = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    gx, gf = bm.reference_trajectories_batch(s["x_fb"][pick], None, s["foot"][pick], s["contact"][pick], phase=s["phase"][pick], mpc=_mpc(h))
    gen["x_ref"] = np.zeros_like(s["x_ref"]); gen["foot_ref"] = np.zeros_like(s["foot_ref"])
    gen["x_ref"][pick], gen["foot_ref"][pick] = gx, gf
    ref_gen, _ = rc.oracle_batch(gen, pick, h, Q_scale=10.0)
    e = util.rel_err(u1[pick], ref)
    print("rescued: err %.2e; supplied vs generated optimum differ by %.2e" % (e.max(), util.rel_err(ref_gen, ref).min()))
    assert ok.all() and e.max() <= util.REL_TOL
    assert util.rel_err(ref_gen, ref).min() > 100 * util.REL_TOL


def _mpc(h):
    import biped_mpc_py_amd as bm
    m = bm.MPC()
    m.h = h
    return m


def test_warm_start_with_references_reaches_the_cold_optimum():
    """8. Warm start (shift = 0) with supplied references ends at the cold solve's optimum."""
    h, B = 10, 1024
    s = rc.make_batch(B, h, 81)
    xr, fr = _kernel(s, h)
    for path in (PATH_DENSE, PATH_STAGE):
        sol = _solver(h, path, half=s["half"], max_batch=B)
        _, uc, ic = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
        sol.set_warm_start(True, shift=0)
        sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
        _, uw, iw = sol.solve(s["x_fb"], s["foot"], s["contact"], s["phase"], x_cmd=s["x_cmd"], x_ref=xr, foot_ref=fr)
        sol.close()
        assert (iw["status"] == 0).all()
        print("path %d: cold %.1f iterations, warm %.1f" % (path, ic["iters"].mean(), iw["iters"].mean()))
        assert util.rel_err(uw, uc).max() <= util.REL_TOL


def test_drop_in_generate_edit_pass_back():
    """9. bm.solve_mpc with an edited get_reference_trajectory / get_reference_foot_trajectory: the oracle's optimum for the
    edited references, and row 0 of the batch call bit for bit."""
    import biped_mpc_py_amd as bm
    d = util.load("known_walking_t0")
    mpc, biped = bm.MPC(), bm.Biped()
    x_fb, foot, t, contact = d["x_fb"].astype(float), d["foot"].astype(float), float(d["t"]), d["contact"]
    xr = bm.get_reference_trajectory(x_fb, mpc)
    fr = bm.get_reference_foot_trajectory(x_fb, t, foot, mpc, contact)
    xr[5, 1:] -= 0.05                                    # crouch a little
    fr[2, 5:] = fr[5, 5:] = 0.05                         # and step up
    xr = xr.astype(np.float32).astype(float); fr = fr.astype(np.float32).astype(float)
    st, u = bm.solve_mpc(x_fb, t, foot, mpc, biped, contact, x_ref=xr, foot_ref=fr)
    sb, ub = bm.solve_mpc_batch(x_fb[None], [t], foot[None], np.asarray(contact)[None, :mpc.h], mpc=mpc, biped=biped,
                                x_ref=xr[None], foot_ref=fr[None])
    assert np.array_equal(u, ub[0]) and np.array_equal(st, sb[0])
    c = dict(x_fb=x_fb.astype(np.float32).astype(float), foot=foot.astype(np.float32).astype(float), t=t, contact=np.asarray(contact)[:mpc.h],
             x_cmd=np.asarray(mpc.x_cmd, float), x_ref=xr, foot_ref=fr, half=5)
    ref, ok = rc.oracle_solve(c, mpc.h)
    assert ok and util.rel_err(u[None], ref[None]).max() <= util.REL_TOL
    _, u_gen = bm.solve_mpc(x_fb, t, foot, mpc, biped, contact)
    assert util.rel_err(u_gen[None], ref[None]).max() > 10 * util.REL_TOL      # (the edit matters)
