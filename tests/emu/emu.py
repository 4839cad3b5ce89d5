"""ctypes driver of tests/emu/bmpc_emu.cpp (TEST INFRASTRUCTURE): the kernels' sources executed on the CPU, one thread per
lane -- both solve families here, the evaluation family in emu_eval.py, all in one shared library.  Builds it on first use
(host clang from ROCm: the kernel source uses clang vector extensions)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SO = os.path.join(HERE, "libbmpc_emu.so")
CLANG = os.environ.get("BMPC_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(HERE, "bmpc_emu.cpp"), os.path.join(HERE, "bmpc_emu_harness.hpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-x", "c++", srcs[0], "-o", SO])
    return SO


def threads(h):
    lib = C.CDLL(build())
    return int(lib.bmpc_emu_threads(int(h)))


def warm_buffer(cparams, B, fill=np.nan):
    """A warm-start buffer of the shape the kernel family of `cparams` addresses, every entry `fill`: dense (B, NT, 6) -- one
    lane per slot --, stage (B, HS, 12, 6) -- step slot, state coordinate n = 2 c + f."""
    lib = C.CDLL(build())
    h = int(cparams.h)
    if int(cparams.path) == 2:
        return np.full((B, int(lib.bmpc_emu_stage_hs(h)), 12, 6), fill, np.float64)
    return np.full((B, threads(h), 6), fill, np.float64)


def warm_slots(cparams):
    """Where the buffer of `warm_buffer` keeps variable (step j, component c, foot f): an int array (h, 6, 2) of indices into the
    buffer of one instance flattened to (slots, 6).  Slots no entry names belong to no variable (phantom steps, spare lanes)."""
    lib = C.CDLL(build())
    h = int(cparams.h)
    idx = np.empty((h, 6, 2), np.int64)
    for j in range(h):
        for c in range(6):
            for f in range(2):
                idx[j, c, f] = (j * 12 + 2 * c + f) if int(cparams.path) == 2 else int(lib.bmpc_emu_lane_of(h, 6 * j + c, f))
    assert idx.min() >= 0 and len(np.unique(idx)) == idx.size
    return idx


def _ptr(a):
    return None if a is None else a.ctypes.data


def inputs(h, x_fb, foot, contact, phase, x_cmd=None, mu=None, x_ref=None, foot_ref=None, controls=None):
    """The arrays of a solve or an evaluation as the `BatchSolver` methods marshal them: (B, arrays by name -- contiguous, of the
    ABI's dtypes, None where absent --, the `bmpc_inputs` descriptor over them).  The arrays have to outlive the descriptor's use."""
    from biped_mpc_py_amd import _lib as _bl
    f32 = lambda a, shp: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shp))
    x_fb = f32(x_fb, (-1, 12))
    B = x_fb.shape[0]
    a = dict(x_fb=x_fb, foot=f32(foot, (B, 6)), contact=np.ascontiguousarray(np.asarray(contact).reshape(B, h, 2).astype(np.uint8)),
             phase=np.ascontiguousarray(np.asarray(phase, np.int32).reshape(B)), x_cmd=f32(x_cmd, (B, 12)), mu=f32(mu, (B, h, 2)),
             x_ref=f32(x_ref, (B, h, 12)), foot_ref=f32(foot_ref, (B, h, 6)), controls=f32(controls, (B, h, 12)))
    desc = _bl.CInputs(*[_ptr(a[k]) for k in ("x_fb", "foot", "contact", "phase", "x_cmd", "mu", "x_ref", "foot_ref")])
    return B, a, desc


class _Out(C.Structure):                         # bmpc_emu_out
    _fields_ = [(k, C.c_void_p) for k in ("controls", "states", "iters", "residuals", "status", "nfactor", "x_ref", "foot_ref", "Gt", "qt")]


class _Warm(C.Structure):                        # bmpc_emu_warm
    _fields_ = [("buf", C.c_void_p), ("load", C.c_int), ("store", C.c_int), ("shift", C.c_int), ("theta", C.c_double)]


def dev_params(cparams):
    """What the library's own `make_dev_params`, compiled into the emulation from the same header, resolves `cparams` to: (the
    bytes of the `bmpc::DevParams`, the five penalties as `bmpc_effective_penalties` reports them); RuntimeError with the library's
    message where it refuses the block."""
    lib = C.CDLL(build())
    buf, eff = C.create_string_buffer(4096), (C.c_double * 5)()
    n = lib.bmpc_emu_dev_params(C.byref(cparams), buf, len(buf), eff)
    if n <= 0:
        lib.bmpc_emu_last_error.restype = C.c_char_p
        raise RuntimeError(lib.bmpc_emu_last_error().decode())
    return buf.raw[:n], list(eff)


def solve(cparams, x_fb, foot, contact, phase, x_cmd=None, mu=None, assemble_only=False, warm=None, warm_load=False,
          warm_shift=0, warm_theta=0.5, x_ref=None, foot_ref=None):
    """Same marshalling as BatchSolver.solve / assemble; x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None
    (generated).  Returns dict.  `warm`: None, or a float64 array of the shape `warm_buffer` gives (dense: (B, threads(h), 6)) that
    receives the final solver state and, with warm_load, provides the start."""
    lib = C.CDLL(build())
    h = int(cparams.h)
    B, _keep, inp = inputs(h, x_fb, foot, contact, phase, x_cmd, mu, x_ref, foot_ref)
    if warm is not None:
        need = warm_buffer(cparams, B, 0.0)
        assert warm.dtype == np.float64 and warm.flags.c_contiguous and warm.size >= need.size, "warm: see warm_buffer"
    out = dict(controls=np.zeros((B, h, 12), np.float32), states=np.zeros((B, h, 13), np.float32),
               iters=np.zeros(B, np.int32), residuals=np.zeros((B, 2), np.float32), status=np.zeros(B, np.int32),
               nfactor=np.zeros(B, np.int32), x_ref=np.zeros((B, h, 12)), foot_ref=np.zeros((B, h, 6)),
               Gt=np.zeros((B, 6 * h, 6 * h)), qt=np.zeros((B, 6 * h)))
    w = _Warm(_ptr(warm), 1 if warm_load else 0, 0 if warm is None else 1, int(warm_shift), float(warm_theta))
    lib.bmpc_emu_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if lib.bmpc_emu_solve(C.byref(cparams), B, C.byref(inp), C.byref(_Out(**{k: _ptr(v) for k, v in out.items()})),
                          1 if assemble_only else 0, C.byref(w)) != 0:
        lib.bmpc_emu_last_error.restype = C.c_char_p
        raise RuntimeError("bmpc_emu_solve failed: " + lib.bmpc_emu_last_error().decode())
    return out
