"""ctypes driver of tests/emu/bmpc_emu_plant_ground.cpp (TEST INFRASTRUCTURE): the ground under the plant of csrc/bmpc_plant.hip on
the CPU, in a small shared library of its own, built on first use with the flags of `emu_plant.build`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu
from tests.emu.emu_plant import INTEGRATORS

SO = os.path.join(emu.HERE, "libbmpc_emu_plant_ground.so")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_plant_ground.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def _f64(a, shape):
    return None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def _u_c(u0, contact0):
    u = np.ascontiguousarray(np.asarray(u0, np.float32).reshape(-1, 12))
    return u, np.ascontiguousarray((np.asarray(contact0).reshape(u.shape[0], 2) != 0).astype(np.uint8))


def ground(u0, contact0, mu=None, mu_h=0.5, fz_floor=0.0):
    """`plant_ground` of every instance: (u_applied (B,12) float32, flags (B,) uint8, demand (B,) float32, ok (B,) bool); mu (B,2)
    or None: mu_h for both legs."""
    lib = C.CDLL(build())
    u, c = _u_c(u0, contact0)
    B = u.shape[0]
    mu = _f64(mu, (B, 2))
    ua, fl, dem, ok = np.empty((B, 12), np.float32), np.empty(B, np.uint8), np.empty(B, np.float32), np.empty(B, np.uint8)
    lib.bmpc_emu_plant_ground.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_double, C.c_double] + [C.c_void_p] * 4
    lib.bmpc_emu_plant_ground.restype = None
    lib.bmpc_emu_plant_ground(B, emu._ptr(u), emu._ptr(c), emu._ptr(mu), float(mu_h), float(fz_floor),
                              *[emu._ptr(a) for a in (ua, fl, dem, ok)])
    return ua, fl, dem, ok.astype(bool)


def plant_step(cparams, x_fb, u0, foot, contact0, wrench=None, integrator="rk4", substeps=4, body=None, mu=None):
    """Marshals like `BatchSolver.plant_step(..., body=body, ground=dict(mu=mu), want_applied=True)` (mu None: the handle's); returns
    (x_next (B,12) float32, u_applied (B,12) float32, flags (B,) uint8, ok (B,) bool)."""
    lib = C.CDLL(build())
    f32 = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, n))
    x, r, w = f32(x_fb, 12), f32(foot, 6), f32(wrench, 6)
    u, c = _u_c(u0, contact0)
    B = x.shape[0]
    body = body or {}
    m, I, g, mu = _f64(body.get("m"), (B,)), _f64(body.get("I"), (B, 9)), _f64(body.get("g"), (B,)), _f64(mu, (B, 2))
    out, ua, fl, ok = np.empty((B, 12), np.float32), np.empty((B, 12), np.float32), np.empty(B, np.uint8), np.empty(B, np.uint8)
    lib.bmpc_emu_plant_step_ground.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13
    rc = lib.bmpc_emu_plant_step_ground(C.byref(cparams), B, INTEGRATORS[integrator], int(substeps),
                                        *[emu._ptr(a) for a in (m, I, g, mu, x, u, r, c, w, out, ua, fl, ok)])
    if rc != 0:
        raise RuntimeError("bmpc_emu_plant_step_ground refused the arguments")
    return out, ua, fl, ok.astype(bool)


def reduce(flags, demand):
    """(first_slip (B,) int32, slip_periods (B,2) int32, unloaded_periods (B,2) int32, mu_demand (B,) float32) of flags (steps,B)
    uint8 and demand (steps,B) float32, as the closed loop reduces them."""
    lib = C.CDLL(build())
    fl = np.ascontiguousarray(np.asarray(flags, np.uint8))
    dem = np.ascontiguousarray(np.asarray(demand, np.float32))
    steps, B = fl.shape
    first, sl, un, md = np.empty(B, np.int32), np.empty((B, 2), np.int32), np.empty((B, 2), np.int32), np.empty(B, np.float32)
    lib.bmpc_emu_ground_reduce.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.bmpc_emu_ground_reduce.restype = None
    lib.bmpc_emu_ground_reduce(steps, B, *[emu._ptr(a) for a in (fl, dem, first, sl, un, md)])
    return first, sl, un, md
