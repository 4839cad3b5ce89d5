"""ctypes driver of tests/emu/bmpc_emu_certify.cpp (TEST INFRASTRUCTURE): the certificate kernel's source (csrc/bmpc_certify.hip) on
the CPU.  Same marshalling and the same result dict as `BatchSolver.certify`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_certify.so")
KEYS = ("lam", "resid", "summary", "n_active", "status")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, n) for n in ("bmpc_emu_certify.cpp", "bmpc_emu_eval_grad.cpp", "bmpc_emu_eval.cpp", "bmpc_emu.cpp")] \
        + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-I" + emu.HERE, "-x", "c++", srcs[0],
                               "-o", SO])
    return SO


def certify(cparams, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, act_tol=1e-4, want=KEYS):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict(lam (B,h,36), resid (B,h,12),
    summary (B,4) fp64, n_active (B,), status (B,) int32); an output not named in `want` is passed as NULL and comes back as None."""
    from biped_mpc_py_amd import _lib as _bl
    lib = C.CDLL(build())
    h = int(cparams.h)
    f32 = lambda a, shp: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shp))
    x_fb = f32(x_fb, (-1, 12))
    B = x_fb.shape[0]
    foot = f32(foot, (B, 6))
    contact = np.ascontiguousarray(np.asarray(contact).reshape(B, h, 2).astype(np.uint8))
    phase = np.ascontiguousarray(np.asarray(phase, np.int32).reshape(B))
    controls = f32(controls, (B, h, 12))
    x_cmd, mu, x_ref, foot_ref = f32(x_cmd, (B, 12)), f32(mu, (B, h, 2)), f32(x_ref, (B, h, 12)), f32(foot_ref, (B, h, 6))
    shapes = dict(lam=(B, h, 36), resid=(B, h, 12), summary=(B, 4), n_active=(B,), status=(B,))
    out = {k: (np.full(shp, -7.0) if k in ("lam", "resid", "summary") else np.full(shp, -7, np.int32)) if k in want else None
           for k, shp in shapes.items()}
    p = lambda a: None if a is None else a.ctypes.data
    inp = _bl.CInputs(p(x_fb), p(foot), p(contact), p(phase), p(x_cmd), p(mu), p(x_ref), p(foot_ref))
    co = _bl.CCertOut(*[p(out[k]) for k in KEYS])
    lib.bmpc_emu_certify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    if lib.bmpc_emu_certify(C.byref(cparams), B, C.byref(inp), p(controls), float(act_tol), C.byref(co)) != 0:
        raise RuntimeError("bmpc_emu_certify failed")
    return out
