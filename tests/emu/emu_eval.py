"""ctypes driver of tests/emu/bmpc_emu_eval.cpp (TEST INFRASTRUCTURE): the sources of the evaluation family's kernels
(csrc/bmpc_evaluate.hip, bmpc_evaluate_grad.hip, bmpc_certify.hip) on the CPU, in one shared library.  `evaluate`, `evaluate_grad` and
`certify` marshal like the `BatchSolver` methods of those names and return the same result dicts."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_eval.so")
CERT_KEYS = ("lam", "resid", "summary", "n_active", "status")


def build(force=False):
    from biped_mpc_py_amd.synth import kernel_source_paths
    srcs = [os.path.join(emu.HERE, "bmpc_emu_eval.cpp"), os.path.join(emu.HERE, "bmpc_emu.cpp")] + kernel_source_paths()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-pthread", "-fPIC", "-shared", "-D_GNU_SOURCE",
                               "-ffp-contract=off", "-I" + os.path.join(emu.ROOT, "include"), "-I" + emu.HERE, "-x", "c++", srcs[0],
                               "-o", SO])
    return SO


def _run(kind, want, cparams, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, act_tol=None):
    """Entry bmpc_emu_<kind> of the library for row `kind` of the package's table of the family (`api._EVAL_OPS`: descriptor, outputs,
    whether there is an `act_tol`): inputs marshalled as the `BatchSolver` methods do; an output not named in `want` is passed as NULL
    and comes back as None, the others start at -7."""
    from biped_mpc_py_amd import _lib as _bl
    from biped_mpc_py_amd import api
    struct, _, _, takes_tol, outputs = api._EVAL_OPS[kind]
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
    out = {k: np.full(api._shape(shp, B, h), -7, dtype) if k in want else None for k, dtype, shp in outputs}
    p = lambda a: None if a is None else a.ctypes.data
    inp = _bl.CInputs(p(x_fb), p(foot), p(contact), p(phase), p(x_cmd), p(mu), p(x_ref), p(foot_ref))
    so = struct(**{k: p(v) for k, v in out.items()})
    tol = (float(act_tol),) if takes_tol else ()
    fn = getattr(lib, "bmpc_emu_" + kind)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * len(tol) + [C.c_void_p]
    if fn(C.byref(cparams), B, C.byref(inp), p(controls), *tol, C.byref(so)) != 0:
        raise RuntimeError(f"bmpc_emu_{kind} failed")
    return out


def evaluate(cparams, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, want_states=True):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict(cost (B,), objective (B,),
    violation (B,4), states (B,h,13) | None), fp64."""
    want = ("cost", "objective", "violation") + (("states",) if want_states else ())
    return _run("evaluate", want, cparams, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref)


def evaluate_grad(cparams, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                  want=("cost", "grad_u", "grad_x0")):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict(cost (B,), grad_u (B,h,12),
    grad_x0 (B,12)), fp64; an output not named in `want` is passed as NULL and comes back as None."""
    return _run("evaluate_grad", want, cparams, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref)


def certify(cparams, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, act_tol=1e-4, want=CERT_KEYS):
    """x_ref (B,h,12) / foot_ref (B,h,6) in the kernel layout, or None (generated).  Returns dict(lam (B,h,36), resid (B,h,12),
    summary (B,4) fp64, n_active (B,), status (B,) int32); an output not named in `want` is passed as NULL and comes back as None."""
    return _run("certify", want, cparams, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, act_tol=act_tol)


def lanes(h):
    return int(C.CDLL(build()).bmpc_emu_eval_lanes(int(h)))
