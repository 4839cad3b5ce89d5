"""ctypes driver of tests/emu/bmpc_emu_plant.cpp (TEST INFRASTRUCTURE): the per-instance functions of csrc/bmpc_plant.hip on the CPU,
in a small shared library of their own, built on first use with the flags of `emu.build`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_plant.so")
INTEGRATORS = {"euler": 0, "rk4": 1}


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_plant.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def plant_step(cparams, x_fb, u0, foot, contact0, wrench=None, integrator="rk4", substeps=4):
    """Marshals like `BatchSolver.plant_step`; returns x_next (B,12) float32."""
    lib = C.CDLL(build())
    f32 = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, n))
    x, u, r, w = f32(x_fb, 12), f32(u0, 12), f32(foot, 6), f32(wrench, 6)
    B = x.shape[0]
    c = np.ascontiguousarray((np.asarray(contact0).reshape(B, 2) != 0).astype(np.uint8))
    out = np.empty((B, 12), np.float32)
    lib.bmpc_emu_plant_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    rc = lib.bmpc_emu_plant_step(C.byref(cparams), B, INTEGRATORS[integrator], int(substeps), *[emu._ptr(a) for a in (x, u, r, c, w, out)])
    if rc != 0:
        raise RuntimeError("bmpc_emu_plant_step refused the arguments")
    return out


def landing(cparams, gait, k0, k1, x_new, foot, x_cmd=None):
    """(foot after the landing rule (B,6) float32, lands (B,2) bool); gait = (period, offset, duty)."""
    from biped_mpc_py_amd import _lib
    lib = C.CDLL(build())
    g = _lib.CGait(int(gait[0]), (C.c_int32 * 2)(*gait[1]), (C.c_int32 * 2)(*gait[2]))
    x = np.ascontiguousarray(np.asarray(x_new, np.float32).reshape(-1, 12))
    B = x.shape[0]
    k0, k1 = (np.ascontiguousarray(np.asarray(k, np.int32).reshape(B)) for k in (k0, k1))
    r = np.ascontiguousarray(np.asarray(foot, np.float32).reshape(B, 6)).copy()
    cmd = None if x_cmd is None else np.ascontiguousarray(np.asarray(x_cmd, np.float32).reshape(B, 12))
    lands = np.zeros((B, 2), np.uint8)
    lib.bmpc_emu_plant_landing.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    if lib.bmpc_emu_plant_landing(C.byref(cparams), C.byref(g), B, *[emu._ptr(a) for a in (k0, k1, x, cmd, r, lands)]) != 0:
        raise RuntimeError("bmpc_emu_plant_landing refused the arguments")
    return r, lands.astype(bool)
