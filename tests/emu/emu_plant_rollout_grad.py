"""ctypes driver of tests/emu/bmpc_emu_plant_rollout_grad.cpp (TEST INFRASTRUCTURE): the body of plant_rollout_grad_kernel
(csrc/bmpc_plant_rollout_grad.hip) on the CPU, in a small shared library of its own, built on first use like
`emu_plant_rollout.build`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu
from tests.emu.emu_plant import INTEGRATORS
from tests.emu.emu_plant_rollout import RolloutIn

SO = os.path.join(emu.HERE, "libbmpc_emu_plant_rollout_grad.so")

# (name, dtype, shape per plan) of the outputs, in the member order of bmpc::RolloutGradOut
OUTPUTS = (("cost", np.float64, ()), ("grad_u", np.float64, ("h", 12)), ("grad_x0", np.float64, (12,)), ("grad_foot", np.float64, (6,)),
           ("x_traj", np.float32, ("h", 12)), ("first_bad", np.int32, ()))


class RolloutGradOut(C.Structure):
    """`bmpc::RolloutGradOut`."""
    _fields_ = [(n, C.c_void_p) for n, _, _ in OUTPUTS]


class RolloutGradScratch(C.Structure):
    """`bmpc::RolloutGradScratch`."""
    _fields_ = [("x_rec", C.c_void_p), ("foot_rec", C.c_void_p), ("sub", C.c_void_p), ("plans", C.c_size_t)]


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_plant_rollout_grad.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def rollout_grad(cparams, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4",
                 substeps=4, move_feet=True, body=None, ground=None, want=None):
    """Marshals like `BatchSolver.plant_rollout_grad`; returns the dict of the wanted outputs (None: all)."""
    from biped_mpc_py_amd import _lib
    lib = C.CDLL(build())
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    lib.bmpc_emu_plant_rollout_grad_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(RolloutIn), C.sizeof(RolloutGradOut), C.sizeof(RolloutGradScratch))
    f32 = lambda v, shape: None if v is None else np.ascontiguousarray(np.asarray(v, np.float32).reshape(shape))
    f64 = lambda v, shape: None if v is None else np.ascontiguousarray(np.asarray(v, np.float64).reshape(shape))
    u = np.ascontiguousarray(np.asarray(controls, np.float32))
    B, S, h, _ = u.shape
    assert h == cparams.h
    body = body or {}
    keep = [f32(x_fb, (B, 12)), f32(foot, (B, 6)), np.ascontiguousarray((np.asarray(contact).reshape(B, h, 2) != 0).astype(np.uint8)),
            f32(x_cmd, (B, 12)), f32(x_ref, (B, h, 12)), f32(push, (B, 6)), u, f64(body.get("m"), (B,)), f64(body.get("I"), (B, 9)),
            f64(body.get("g"), (B,)), None if ground is None else f64(ground.get("mu"), (B, 2))]
    cin = RolloutIn(*[emu._ptr(v) for v in keep], 0.0, 0 if ground is None else 1, 0, 0, 0)
    names = [k for k, _, _ in OUTPUTS]
    want = names if want is None else list(want)
    assert want and set(want) <= set(names)
    res = {k: np.empty((B, S) + tuple(h if d == "h" else d for d in shp), dt) for k, dt, shp in OUTPUTS if k in want}
    cout = RolloutGradOut(**{k: emu._ptr(v) for k, v in res.items()})
    # the scratch, the test's own arrays, filled with NaN: what the kernel reads of it, it has written
    x_rec = None if "x_traj" in res else np.full((B * S, h, 12), np.nan, np.float32)
    foot_rec, sub = np.full((h, 6, B * S), np.nan, np.float32), np.full((int(substeps), 6, B * S), np.nan)
    scratch = RolloutGradScratch(emu._ptr(x_rec), emu._ptr(foot_rec), emu._ptr(sub), B * S)
    plant = _lib.CPlant(INTEGRATORS[integrator], int(substeps), 1 if move_feet else 0, int(push_from), int(push_steps))
    lib.bmpc_emu_plant_rollout_grad.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    if lib.bmpc_emu_plant_rollout_grad(C.byref(cparams), B, S, C.byref(plant), C.byref(cin), C.byref(cout), C.byref(scratch)) != 0:
        raise RuntimeError("bmpc_emu_plant_rollout_grad refused the arguments")
    return res
