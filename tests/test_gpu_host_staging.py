"""The staging of the synchronous host entries: every one of them lays its host inputs out in one block of the handle and its
outputs and scratch in one other (bmpc_capi.hip).  Here nine entries share ONE handle, interleaved, so that the two blocks grow, are
reused at a smaller size and are reused by an entry with another row table: every result has to have the bits a fresh handle
gives.  And the three low-level host entries against their _device twins, bit for bit."""
import numpy as np
import pytest

from tests import body_cases as bc
from tests import eval_cases as ec
from tests import ground_cases as gc
from tests import rollout_cases as rc
from tests import util

H = 10
MAX_BATCH = 300
REDUCED_ONLY = ("cost", "violation", "score", "weights")      # skipped: the scores and weights of the reductions live in scratch


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def low_level_inputs(B):
    """The random part of test_gpu_parity.py::test_low_level_control_and_fk_on_device at batch B."""
    rng = np.random.default_rng(7)
    xs = np.stack([util.synth_batch(1, H, 100 + i)["x_fb"][0] for i in range(B)])
    q = rng.uniform(-1, 1, (B, 10)); qd = rng.uniform(-2, 2, (B, 10)); t = rng.uniform(0, 2, B)
    u0 = rng.uniform(-50, 150, (B, 12)); c0 = rng.integers(0, 2, (B, 2))
    return xs, q, qd, t, u0, c0


def calls():
    """[(name, f(solver) -> dict of arrays)], in the order of the shared handle's first pass.  B = 257 crosses a 256-thread block and
    a 256-byte boundary for every width involved; B = 1 and B = 3 leave slices shorter than the alignment."""
    xs, q, qd, t, u0, c0 = low_level_inputs(257)
    rng = np.random.default_rng(11)
    step = util.synth_batch(257, H, 31)
    pf = (step["foot"] + rng.uniform(-0.02, 0.02, (257, 6))).astype(np.float32)       # (any footholds will do for the torque map)
    body, mu = bc.bodies(257, seed=5), gc.grounds(257, seed=6)
    ev = util.synth_batch(67, H, 32, gait="walking", per_step_mu=True)
    U = ec.seeded_controls(ev["contact"], rng)
    ev_args = (ev["x_fb"], ev["foot"], ev["contact"], ev["phase"], U)
    sm = util.synth_batch(3, H, 33, gait="walking", vx_cmd=True)
    Us = (ec.seeded_controls(sm["contact"], rng)[:, None] + rng.normal(0, 5.0, (3, 5, H, 12))).astype(np.float32)
    c = rc.case(H)
    ro_kw = dict(rc.take(rc.variant(c, "full"), slice(0, 3)), w_fall=rc.W_FALL, w_slip=rc.W_SLIP, w_unloaded=rc.W_UNLOADED, temperature=50.0,
                 fall=(0.6, 0.3))
    ro_U = rc.plans(c, 5)[:3]
    asm = util.synth_batch(3, H, 34, gait="walking", vx_cmd=True)

    def named(names, values):
        return dict(zip(names, values))

    return [
        ("plant_step", lambda s: named(("x_next", "u_applied", "flags"), s.plant_step(
            step["x_fb"], u0, step["foot"], c0, wrench=None, body=body, ground=dict(mu=mu), want_applied=True))),
        ("foot_position_world", lambda s: dict(pf_w=s.foot_position_world(xs[:3], q[:3]))),
        ("evaluate", lambda s: s.evaluate(*ev_args, x_cmd=None, mu=ev["mu"], want_states=True)),
        ("low_level_control", lambda s: dict(tau=s.low_level_control(xs, t, pf, q, qd, c0, u0))),
        ("contact_sequence", lambda s: named(("phase", "contact"), s.contact_sequence(t[:1]))),
        ("plant_rollout_samples", lambda s: s.plant_rollout_samples(c["x_fb"][:3], c["foot"][:3], c["contact"][:3], ro_U, **ro_kw)),
        ("certify", lambda s: s.certify(*ev_args, x_cmd=None, mu=ev["mu"])),
        ("evaluate_samples", lambda s: s._samples_host(sm["x_fb"], sm["foot"], sm["contact"], sm["phase"], Us, sm["x_cmd"], None, None, None,
                                                       (1e3, 2e3, 5e2, 1.5e3), 25.0, skip=REDUCED_ONLY)),
        ("assemble", lambda s: named(("x_ref", "foot_ref", "Gt", "qt"), s.assemble(
            asm["x_fb"], asm["foot"], asm["contact"], asm["phase"], x_cmd=asm["x_cmd"]))),
    ]


def same(got, want, where):
    assert set(got) == set(want), where
    for k, v in want.items():
        if v is None:
            assert got[k] is None, (where, k)
            continue
        g = got[k]
        assert g.dtype == v.dtype and g.shape == v.shape, (where, k)
        assert np.array_equal(g, v, equal_nan=v.dtype.kind == "f"), (where, k)


@pytest.mark.gpu
def test_one_handle_many_entries_interleaved():
    """Nine host entries -- plant_step (B = 257: ground, body, want_applied, no wrench), foot_position_world (3), evaluate (67, every
    output, no x_cmd), low_level_control (257), contact_sequence (1), plant_rollout_samples (3 x 5, every output, ground and
    body), certify (67), evaluate_samples (3 x 5, reduced outputs only), assemble (3) -- each on a fresh handle of its own, then all
    of them on one shared handle in that order, then once more in reverse order: every array of every result is bit-equal to
    the fresh handle's."""
    import biped_mpc_py_amd as bm
    todo = calls()
    assert len(todo) == 9
    fresh = {}
    for name, f in todo:
        s = bm.BatchSolver(max_batch=MAX_BATCH)
        fresh[name] = f(s)
        s.close()
    assert fresh["evaluate"]["states"] is not None and fresh["assemble"]["Gt"] is not None
    assert set(fresh["evaluate_samples"]) >= {"best", "n_valid", "u_mean", "ess"} and fresh["evaluate_samples"]["score"] is None
    assert len(fresh["plant_rollout_samples"]) == 17
    shared = bm.BatchSolver(max_batch=MAX_BATCH)
    for order, run in (("forward", todo), ("reverse", todo[::-1])):
        for name, f in run:
            same(f(shared), fresh[name], (order, name))
    shared.close()


@pytest.mark.gpu
def test_low_level_host_entries_equal_their_device_twins():
    """bmpc_foot_position_world, bmpc_low_level_control and bmpc_contact_sequence against their _device twins on torch tensors and
    the current stream, bit for bit, at B = 257."""
    import torch
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import _lib
    B = 257
    xs, q, qd, t, u0, c0 = low_level_inputs(B)
    s = bm.BatchSolver(max_batch=MAX_BATCH)
    dev = torch.device("cuda", s.device)
    st = torch.cuda.current_stream(dev).cuda_stream
    cuda = lambda a, dt: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt)), device=dev)
    d_x, d_q, d_qd, d_u0 = (cuda(a, np.float32) for a in (xs, q, qd, u0))
    d_t, d_c0 = cuda(t, np.float64), cuda(c0, np.uint8)

    pf = s.foot_position_world(xs, q)
    d_pf = torch.empty((B, 6), dtype=torch.float32, device=dev)
    _lib.check(s._lib.bmpc_foot_position_world_device(s._h, B, d_x.data_ptr(), d_q.data_ptr(), d_pf.data_ptr(), st))
    torch.cuda.synchronize(dev)
    assert np.array_equal(pf, d_pf.cpu().numpy().astype(np.float64))

    tau = s.low_level_control(xs, t, pf, q, qd, c0, u0)
    d_tau = torch.empty((B, 10), dtype=torch.float32, device=dev)
    _lib.check(s._lib.bmpc_low_level_control_device(s._h, B, d_x.data_ptr(), d_t.data_ptr(), d_pf.data_ptr(), d_q.data_ptr(),
                                                    d_qd.data_ptr(), d_c0.data_ptr(), d_u0.data_ptr(), d_tau.data_ptr(), st))
    torch.cuda.synchronize(dev)
    assert np.array_equal(tau, d_tau.cpu().numpy().astype(np.float64))

    phase, contact = s.contact_sequence(t)
    d_phase, d_contact = s.contact_sequence_device(d_t)
    torch.cuda.synchronize(dev)
    assert phase.dtype == np.int32 and contact.shape == (B, H, 2)
    assert np.array_equal(phase, d_phase.cpu().numpy()) and np.array_equal(contact, d_contact.cpu().numpy())
    assert len(np.unique(phase)) > 1 and 0 < contact.mean() < 1                      # (not a comparison of constants)
    s.close()
