"""ctypes driver of tests/emu/bmpc_emu_plant_rollout.cpp (TEST INFRASTRUCTURE): the body of plant_rollout_samples_kernel
(csrc/bmpc_plant_rollout.hip) on the CPU, in a small shared library of its own, built on first use with the flags of
`emu_plant.build`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu
from tests.emu.emu_plant import INTEGRATORS

SO = os.path.join(emu.HERE, "libbmpc_emu_plant_rollout.so")

# (name, dtype, shape per plan) of the per-sample outputs, in the member order of bmpc::RolloutOut
OUTPUTS = (("cost", np.float64, ()), ("score", np.float64, ()), ("x_end", np.float32, (12,)), ("foot_end", np.float32, (6,)),
           ("x_traj", np.float32, ("h", 12)), ("first_fall", np.int32, ()), ("max_tilt", np.float32, ()), ("min_z", np.float32, ()),
           ("first_slip", np.int32, ()), ("slip_periods", np.int32, (2,)), ("unloaded_periods", np.int32, (2,)),
           ("mu_demand", np.float32, ()))
GROUND_ONLY = ("first_slip", "slip_periods", "unloaded_periods", "mu_demand")


class RolloutIn(C.Structure):
    """`bmpc::RolloutIn` (the members the entry fills from the plant block and the handle are left zero here)."""
    _fields_ = [(n, C.c_void_p) for n in ("x_fb", "foot", "contact", "x_cmd", "x_ref", "push", "controls", "m", "I", "g", "mu")] + \
               [("mu_h", C.c_double)] + [(n, C.c_int) for n in ("ground", "move_feet", "push_from", "push_steps")]


class RolloutOut(C.Structure):
    """`bmpc::RolloutOut`."""
    _fields_ = [(n, C.c_void_p) for n, _, _ in OUTPUTS]


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_plant_rollout.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def rollout(cparams, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0, integrator="rk4",
            substeps=4, move_feet=True, body=None, ground=None, fall=(np.inf, -np.inf), fz_floor=0.0, w_fall=0.0, w_slip=0.0,
            w_unloaded=0.0):
    """Marshals like `BatchSolver.plant_rollout_samples`; returns the dict of its per-sample outputs (the ground's four only with a
    ground)."""
    from biped_mpc_py_amd import _lib
    lib = C.CDLL(build())
    a, b = C.c_int(), C.c_int()
    lib.bmpc_emu_plant_rollout_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(RolloutIn), C.sizeof(RolloutOut))
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
    res = {k: np.empty((B, S) + tuple(h if d == "h" else d for d in shp), dt) for k, dt, shp in OUTPUTS
           if ground is not None or k not in GROUND_ONLY}
    cout = RolloutOut(**{k: emu._ptr(v) for k, v in res.items()})
    plant = _lib.CPlant(INTEGRATORS[integrator], int(substeps), 1 if move_feet else 0, int(push_from), int(push_steps))
    price = _lib.CRolloutPrice(S, 0, float(w_fall), float(w_slip), float(w_unloaded), np.inf, float(fall[0]), float(fall[1]), float(fz_floor))
    lib.bmpc_emu_plant_rollout.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    if lib.bmpc_emu_plant_rollout(C.byref(cparams), B, C.byref(plant), C.byref(price), C.byref(cin), C.byref(cout)) != 0:
        raise RuntimeError("bmpc_emu_plant_rollout refused the arguments")
    return res
