"""ctypes driver of tests/emu/bmpc_emu_plant_body.cpp (TEST INFRASTRUCTURE): the per-instance body and the fall outcome of
csrc/bmpc_plant.hip on the CPU, in a small shared library of their own, built on first use with the flags of `emu_plant.build`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu
from tests.emu.emu_plant import INTEGRATORS

SO = os.path.join(emu.HERE, "libbmpc_emu_plant_body.so")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_plant_body.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def _f64(a, shape):
    return None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def plant_step(cparams, x_fb, u0, foot, contact0, wrench=None, integrator="rk4", substeps=4, body=None):
    """Marshals like `BatchSolver.plant_step(..., body=body)`; returns (x_next (B,12) float32, ok (B,) bool)."""
    lib = C.CDLL(build())
    f32 = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, n))
    x, u, r, w = f32(x_fb, 12), f32(u0, 12), f32(foot, 6), f32(wrench, 6)
    B = x.shape[0]
    body = body or {}
    m, I, g = _f64(body.get("m"), (B,)), _f64(body.get("I"), (B, 9)), _f64(body.get("g"), (B,))
    c = np.ascontiguousarray((np.asarray(contact0).reshape(B, 2) != 0).astype(np.uint8))
    out, ok = np.empty((B, 12), np.float32), np.zeros(B, np.uint8)
    lib.bmpc_emu_plant_step_body.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10
    rc = lib.bmpc_emu_plant_step_body(C.byref(cparams), B, INTEGRATORS[integrator], int(substeps),
                                      *[emu._ptr(a) for a in (m, I, g, x, u, r, c, w, out, ok)])
    if rc != 0:
        raise RuntimeError("bmpc_emu_plant_step_body refused the arguments")
    return out, ok.astype(bool)


def plant_body(cparams, m=None, I=None, g=None):
    """`plant_body` of one instance: (ok, dict(m, g, Ib (9,), Ibinv (9,)), the handle's I_b^-1 (9,))."""
    lib = C.CDLL(build())
    m, I, g = _f64(m, (1,)), _f64(I, (9,)), _f64(g, (1,))
    hinv, out = np.empty(9), np.empty(20)
    lib.bmpc_emu_plant_body.argtypes = [C.c_void_p] * 6
    rc = lib.bmpc_emu_plant_body(C.byref(cparams), *[emu._ptr(a) for a in (m, I, g, hinv, out)])
    if rc < 0:
        raise RuntimeError("bmpc_emu_plant_body refused the arguments")
    return bool(rc), dict(m=out[0], g=out[1], Ib=out[2:11].copy(), Ibinv=out[11:20].copy()), hinv


def outcome(x_traj, tilt_max, z_min):
    """(first_fall int32 (B,), max_tilt, min_z float32 (B,)) of x_traj (steps,B,12) float32, as the closed loop reduces them."""
    lib = C.CDLL(build())
    x = np.ascontiguousarray(np.asarray(x_traj, np.float32))
    steps, B = x.shape[:2]
    first, mt, mz = np.empty(B, np.int32), np.empty(B, np.float32), np.empty(B, np.float32)
    lib.bmpc_emu_plant_outcome.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 3
    lib.bmpc_emu_plant_outcome.restype = None
    lib.bmpc_emu_plant_outcome(steps, B, emu._ptr(x), float(tilt_max), float(z_min), *[emu._ptr(a) for a in (first, mt, mz)])
    return first, mt, mz
