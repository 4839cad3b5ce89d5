"""ctypes driver of the evaluation family's entries of tests/emu/bmpc_emu.cpp (TEST INFRASTRUCTURE): the sources of
csrc/bmpc_evaluate.hip, bmpc_evaluate_grad.hip and bmpc_certify.hip on the CPU, in the one library `emu.build` makes.  `evaluate`,
`evaluate_grad` and `certify` marshal like the `BatchSolver` methods of those names and return the same result dicts."""
import ctypes as C

import numpy as np

from tests.emu import emu

CERT_KEYS = ("lam", "resid", "summary", "n_active", "status")


def _run(kind, want, cparams, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, act_tol=None):
    """Entry bmpc_emu_<kind> of the library for row `kind` of the package's table of the family (`api._EVAL_OPS`: descriptor, outputs,
    whether there is an `act_tol`): inputs marshalled as the `BatchSolver` methods do; an output not named in `want` is passed as NULL
    and comes back as None, the others start at -7."""
    from biped_mpc_py_amd import api
    struct, _, _, takes_tol, outputs = api._EVAL_OPS[kind]
    lib = C.CDLL(emu.build())
    h = int(cparams.h)
    B, arr, inp = emu.inputs(h, x_fb, foot, contact, phase, x_cmd, mu, x_ref, foot_ref, controls)
    out = {k: np.full(api._shape(shp, B, h), -7, dtype) if k in want else None for k, dtype, shp in outputs}
    p = emu._ptr
    so = struct(**{k: p(v) for k, v in out.items()})
    tol = (float(act_tol),) if takes_tol else ()
    fn = getattr(lib, "bmpc_emu_" + kind)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * len(tol) + [C.c_void_p]
    if fn(C.byref(cparams), B, C.byref(inp), p(arr["controls"]), *tol, C.byref(so)) != 0:
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
    return int(C.CDLL(emu.build()).bmpc_emu_eval_lanes(int(h)))
