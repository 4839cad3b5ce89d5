"""ctypes driver of tests/emu/bmpc_emu_refs.cpp (TEST INFRASTRUCTURE): the kernels' source on the CPU, as tests/emu/emu.py, with
supplied references (bmpc::WarmArgs::x_ref / foot_ref).  Same marshalling as emu.solve."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_refs.so")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_refs.cpp"), os.path.join(emu.HERE, "bmpc_emu.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-I" + emu.HERE, "-x", "c++", srcs[0],
                               "-o", SO])
    return SO


def solve(cparams, x_fb, foot, contact, phase, x_cmd=None, x_ref=None, foot_ref=None, assemble_only=False):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict as emu.solve."""
    lib = C.CDLL(build())
    from biped_mpc_py_amd import _lib as _bl
    eff = (C.c_double * 5)()
    _bl.check(_bl.load().bmpc_effective_penalties(C.byref(cparams), eff))
    cp2 = type(cparams)()
    C.memmove(C.byref(cp2), C.byref(cparams), C.sizeof(cparams))
    cp2.rho, cp2.rho_eq_scale, cp2.rho_lo, cp2.rho_hi_f, cp2.rho_hi_m, cp2.penalty_mode = eff[0], eff[1] / eff[0], eff[2], eff[3], eff[4], 1
    h = int(cp2.h)
    f32 = lambda a, shp: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shp))
    x_fb = f32(x_fb, (-1, 12))
    B = x_fb.shape[0]
    foot = f32(foot, (B, 6))
    contact = np.ascontiguousarray(np.asarray(contact).reshape(B, h, 2).astype(np.uint8))
    phase = np.ascontiguousarray(np.asarray(phase, np.int32).reshape(B))
    x_cmd, x_ref, foot_ref = f32(x_cmd, (B, 12)), f32(x_ref, (B, h, 12)), f32(foot_ref, (B, h, 6))
    out = dict(controls=np.zeros((B, h, 12), np.float32), states=np.zeros((B, h, 13), np.float32),
               iters=np.zeros(B, np.int32), residuals=np.zeros((B, 2), np.float32), status=np.zeros(B, np.int32),
               nfactor=np.zeros(B, np.int32), x_ref=np.zeros((B, h, 12)), foot_ref=np.zeros((B, h, 6)))
    p = emu._ptr
    lib.bmpc_emu_solve_refs.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 16 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                                   C.c_double, C.c_void_p, C.c_void_p]
    rc = lib.bmpc_emu_solve_refs(C.byref(cp2), B, p(x_fb), p(foot), p(contact), p(phase), p(x_cmd), None,
                                 p(out["controls"]), p(out["states"]), p(out["iters"]), p(out["residuals"]), p(out["status"]),
                                 p(out["nfactor"]), p(out["x_ref"]), p(out["foot_ref"]), None, None, 1 if assemble_only else 0,
                                 None, 0, 0, 0, 0.5, p(x_ref), p(foot_ref))
    if rc != 0:
        raise RuntimeError("bmpc_emu_solve_refs failed")
    return out
