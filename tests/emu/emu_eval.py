"""ctypes driver of tests/emu/bmpc_emu_eval.cpp (TEST INFRASTRUCTURE): the evaluation kernel's source (csrc/bmpc_evaluate.hip) on the
CPU.  Same marshalling and the same result dict as `BatchSolver.evaluate`."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_eval.so")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_eval.cpp"), os.path.join(emu.HERE, "bmpc_emu.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-I" + emu.HERE, "-x", "c++", srcs[0],
                               "-o", SO])
    return SO


def evaluate(cparams, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, want_states=True):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict(cost (B,), objective (B,),
    violation (B,4), states (B,h,13) | None), fp64."""
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
    out = dict(cost=np.full(B, -7.0), objective=np.full(B, -7.0), violation=np.full((B, 4), -7.0),
               states=np.full((B, h, 13), -7.0) if want_states else None)
    p = lambda a: None if a is None else a.ctypes.data
    inp = _bl.CInputs(p(x_fb), p(foot), p(contact), p(phase), p(x_cmd), p(mu), p(x_ref), p(foot_ref))
    eo = _bl.CEvalOut(p(out["cost"]), p(out["objective"]), p(out["states"]), p(out["violation"]))
    lib.bmpc_emu_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if lib.bmpc_emu_evaluate(C.byref(cparams), B, C.byref(inp), p(controls), C.byref(eo)) != 0:
        raise RuntimeError("bmpc_emu_evaluate failed")
    return out


def lanes(h):
    return int(C.CDLL(build()).bmpc_emu_eval_lanes(int(h)))
