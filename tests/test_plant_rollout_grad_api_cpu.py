"""What `BatchSolver.plant_rollout_grad` hands the library and what both gradient methods and both C entries refuse before a device is
needed: the marshalling against the recording stand-in of tests/api_calls.py (argument order, NULLs for absent options, `want`), the
struct layout against the C compiler, the symbols, and the refusals of include/bmpc.h in their stated order.  The device method's
marshalling needs device tensors: tests/test_gpu_plant_rollout_grad.py holds it to the same rows."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import util
from tests.api_calls import HANDLE, H, S, In, Out, St, solver
from biped_mpc_py_amd import _lib

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
PLANT = St(_lib.CPlant, integrator=1, substeps=4, move_feet=1)
GRAD = dict(cost=(f64,), grad_u=(f64, H, 12), grad_x0=(f64, 12), grad_foot=(f64, 6), x_traj=(f32, H, 12), first_bad=(i32,))
NEW = ("bmpc_plant_rollout_grad", "bmpc_plant_rollout_grad_device")


def data(B):
    r = np.random.default_rng(9)
    return dict(x_fb=r.normal(size=(B, 12)), foot=r.normal(size=(B, 6)), contact=r.integers(0, 2, (B, H, 2)), x_cmd=r.normal(size=(B, 12)),
                x_ref=r.normal(size=(B, H, 12)), push=r.normal(size=(B, 6)), samples=r.normal(size=(B, S, H, 12)), g=r.uniform(9, 10, B),
                I=r.normal(size=(B, 3, 3)), gmu=r.uniform(0.2, 0.9, (B, 2)))


def grad_out(B, names):
    return St(_lib.CRolloutGradOut, **{k: Out(k, GRAD[k][0], (B, S) + GRAD[k][1:]) for k in names})


def run(rows, *args, **kw):
    s = solver(rows)
    res = s.plant_rollout_grad(*args, **kw)
    s._lib.check_outputs(res)
    return res


@pytest.mark.parametrize("B", [3, 0])
def test_plant_rollout_grad_marshals_as_the_header_says(B):
    d = data(B)
    a = (d["x_fb"], d["foot"], d["contact"], d["samples"])
    three = [In(d["x_fb"], f32), In(d["foot"], f32), In(d["contact"], u8)]
    us = In(d["samples"], f32)
    entry = "bmpc_plant_rollout_grad"
    res = run([(entry, [HANDLE, B, S, *three, None, None, None, us, PLANT, None, None, grad_out(B, GRAD)])], *a)
    assert list(res) == list(GRAD)
    run([(entry, [HANDLE, B, S, *three, In(d["x_cmd"], f32), In(d["x_ref"], f32), In(d["push"], f32), us,
                  St(_lib.CPlant, integrator=0, substeps=2, move_feet=0, push_from=1, push_steps=3),
                  St(_lib.CPlantBody, I=In(d["I"], f64), g=In(d["g"], f64)), St(_lib.CPlantGround, mu=In(d["gmu"], f64)), grad_out(B, GRAD)])],
        *a, x_cmd=d["x_cmd"], x_ref=d["x_ref"], push=d["push"], push_from=1, push_steps=3, integrator="euler", substeps=2, move_feet=False,
        body=dict(I=d["I"], g=d["g"]), ground=dict(mu=d["gmu"]))
    run([(entry, [HANDLE, B, S, *three, None, None, None, us, PLANT, None, St(_lib.CPlantGround), grad_out(B, ["grad_u", "first_bad"])])],
        *a, ground={}, want=["first_bad", "grad_u"])
    for k in GRAD:
        run([(entry, [HANDLE, B, S, *three, None, None, None, us, PLANT, None, None, grad_out(B, [k])])], *a, want=(k,))


def test_python_keywords_are_checked_before_any_call():
    import biped_mpc_py_amd as bm
    s = object.__new__(bm.BatchSolver)                 # no handle: the checks come first
    s.h = 10
    x, f, c, u = np.zeros((3, 12)), np.zeros((3, 6)), np.ones((3, 10, 2)), np.zeros((3, 4, 10, 12))
    for kw in (dict(integrator="midpoint"), dict(substeps=0), dict(substeps=65), dict(push_from=-1), dict(push_steps=-1),
               dict(ground={"friction": 1.0}), dict(ground=0.5), dict(want=[]), dict(want=["score"]), dict(want=["cost", "states"]),
               dict(body={"mass": np.ones(3)}), dict(body={"m": np.ones(3, np.float32)}), dict(ground={"mu": np.ones((3, 3))}),
               dict(x_cmd=np.zeros((3, 13))), dict(x_ref=np.zeros((3, 12, 10))), dict(push=np.zeros((2, 6)))):
        with pytest.raises(ValueError):
            s.plant_rollout_grad(x, f, c, u, **kw)
    for bad in (dict(controls=np.zeros((3, 10, 12))), dict(controls=np.zeros((3, 4, 9, 12))), dict(x_fb=np.zeros((2, 12))),
                dict(foot=np.zeros((3, 5))), dict(contact=np.ones((3, 9, 2))), dict(contact=np.full((3, 10, 2), 2))):
        a = dict(x_fb=x, foot=f, contact=c, controls=u)
        a.update(bad)
        with pytest.raises(ValueError):
            s.plant_rollout_grad(**a)
    import torch
    s.device = 0
    for kw, word in ((dict(integrator="midpoint"), "integrator"), (dict(want=["score"]), "want names"), (dict(ground=0.5), "ground must be"),
                     ({}, "must live on cuda")):
        with pytest.raises(ValueError, match=word):
            s.plant_rollout_grad_device(torch.zeros(3, 12), None, None, torch.zeros(3, 4, 10, 12), **kw)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_new_symbols_are_exported_and_declared(lib):
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(util.ROOT, "include", "bmpc.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(raw, name) and ("int " + name + "(") in header
        assert getattr(lib, name).argtypes is not None
    assert lib.bmpc_abi_version() == 13 and "#define BMPC_ABI_VERSION 13" in header


def test_struct_layout_matches_c(lib):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(bmpc_rollout_grad_out), '
           'offsetof(bmpc_rollout_grad_out, grad_foot), offsetof(bmpc_rollout_grad_out, x_traj), '
           'offsetof(bmpc_rollout_grad_out, first_bad));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    G = _lib.CRolloutGradOut
    assert sizes == [C.sizeof(G), G.grad_foot.offset, G.x_traj.offset, G.first_bad.offset] == [48, 24, 32, 40]


def test_argument_checks_come_in_the_stated_order_without_a_device(lib):
    """S, then the plant block -- both before the handle is looked at --, then the handle, the required pointers, the outputs."""
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)

    def calls(S_, plant=None, out=None, handle=None, ptr=None):
        a = (handle, 4, S_, ptr, ptr, ptr, None, None, None, ptr, None if plant is None else C.byref(plant), None, None,
             None if out is None else C.byref(out))
        return lib.bmpc_plant_rollout_grad(*a), lib.bmpc_plant_rollout_grad_device(*a, None)

    def refused(rcs, word):
        for rc_ in rcs:
            assert rc_ == -1 and word in lib.bmpc_last_error(), (rcs, word, lib.bmpc_last_error())

    bad_plant = _lib.CPlant(1, 0, 1, 0, 0)
    for S_ in (0, -1, 65537):
        refused(calls(S_, bad_plant), b"S = ")                         # S comes first
    for field, value, word in (("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"), ("integrator", 2, b"integrator"),
                               ("push_from", -1, b"push"), ("push_steps", -1, b"push")):
        bad = _lib.CPlant(1, 4, 1, 0, 0)
        setattr(bad, field, value)
        refused(calls(4, bad), word)                                    # then the plant block, before the handle
    refused(calls(4, None, _lib.CRolloutGradOut(cost=addr)), b"null handle")
    refused(calls(65536, None, None), b"null handle")
