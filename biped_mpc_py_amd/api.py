"""Host side of the drop-in: the reference's `solve_mpc` call surface over libbmpc.so.

    states, controls = solve_mpc(x_fb, t, foot, mpc, biped, contact)        # REF:187, 304, 487

returns new fp64 arrays `states (h,13)`, `controls (h,12)` exactly like the reference, so
`u0 = controls[0, :].reshape(-1, 1)` -> `lowLevelControl(...)` (REF:493-494) keeps working.  The
three prints of REF:190-192 are not reproduced.  `solve_mpc_batch` is the same for B instances.
All arithmetic happens in the HIP kernels; this module only marshals arrays.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .params import MPC, pack_params, params_key


def phase_index(t, mpc_or_dt, h=None):
    """k = int(t // dt) % h, evaluated in fp64 on the host exactly as REF:56-57 / REF:99-100."""
    if h is None:
        dt, h = mpc_or_dt.dt, mpc_or_dt.h
    else:
        dt = mpc_or_dt
    return int(t // dt) % int(h)


def phase_indices(t, dt, h):
    """`phase_index` for an array of times: np.floor_divide on float64 has CPython's `//` semantics (the quotient is
    corrected by the fmod remainder, REF:56-57 / 99-100 rely on exactly that at step boundaries), so this is the
    same arithmetic without a Python loop (tests/test_host_logic.py holds it to `phase_index` on and next to 3000
    step boundaries).  t: array of seconds (>= 0) -> int32 array."""
    tt = np.asarray(t, np.float64).reshape(-1)
    k = np.floor_divide(tt, np.float64(dt))
    return (k.astype(np.int64) % int(h)).astype(np.int32)


def _contact_u8(contact, B, h):
    """(B, h, 2) uint8 contact table with entries in {0, 1}.  uint8 / bool input takes one pass (a max), anything
    else is checked value by value."""
    c = np.asarray(contact)
    if c.shape[-1] != 2 or c.size != B * h * 2:
        raise ValueError(f"contact must have shape (B, {h}, 2)")
    if c.dtype == np.uint8 or c.dtype == np.bool_:
        c8 = c.view(np.uint8) if c.dtype == np.bool_ else c
        if c8.size and c8.max() > 1:
            raise ValueError("contact entries must be 0 or 1")
    else:
        c8 = c.astype(np.uint8)
        if not np.array_equal(c8, c) or (c8.size and c8.max() > 1):
            raise ValueError("contact entries must be 0 or 1")
    return np.ascontiguousarray(c8.reshape(B, h, 2))


def get_contact_sequence(t, mpc, half=None):
    """REF:50-59.  Default: the reference's 20x2 table of 5-on/5-off, rows k..k+9 (ten rows whatever
    `mpc.h` is -- reference quirk).  With `half` given: the same schedule with that half period, continued
    periodically, rows k..k+h-1 (what `BatchSolver.contact_sequence` computes on the device)."""
    if half is None:
        half_, nrow = 5, 10
    else:
        half_, nrow = int(half), int(mpc.h)
    k = phase_index(t, mpc)
    leg0 = ((k + np.arange(nrow)) // half_) % 2 == 0
    return np.stack([leg0, ~leg0], axis=1).astype(int)


def _kernel_refs(x_ref, foot_ref, B, h, finite=True):
    """Supplied references in the kernel layout -- x_ref (B,h,12), foot_ref (B,h,6), each or None -- as C-contiguous fp32 arrays
    (what `bmpc_inputs` takes).  Raises ValueError on a wrong shape or a non-finite value: a bad reference is the caller's
    mistake, caught before the call (on the device it would only show as status 2 of that instance).  `finite=False` (the
    evaluation, whose answer for such an instance is defined: NaN) leaves the values unchecked."""
    out = []
    for name, a, w in (("x_ref", x_ref, 12), ("foot_ref", foot_ref, 6)):
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a)
        if a.shape != (B, h, w):
            raise ValueError(f"{name} must have shape ({B}, {h}, {w}) (kernel layout: row j = step j), got {a.shape}")
        if finite and not np.all(np.isfinite(a)):
            raise ValueError(f"{name} holds non-finite values")
        out.append(np.ascontiguousarray(a, np.float32))
    return out[0], out[1]


def references_to_kernel_layout(x_ref=None, foot_ref=None, h=None):
    """The reference's orientation -> the kernel layout, exactly (a transpose): x_ref (...,13,h) or (...,12,h) as
    `get_reference_trajectory` / `reference_trajectories_batch` return it -> (...,h,12); foot_ref (...,6,h) -> (...,h,6).
    A 13th row must be all ones (REF:62): anything else would silently change what Q[12] weighs, so it raises ValueError, as do
    a wrong shape and non-finite values.  Values stay fp64 here; the solve takes them in fp32."""
    xr = fr = None
    if x_ref is not None:
        a = np.asarray(x_ref, np.float64)
        if a.ndim < 2 or a.shape[-2] not in (12, 13) or (h is not None and a.shape[-1] != h):
            raise ValueError(f"x_ref must have shape (..., 13, h) or (..., 12, h){'' if h is None else f' with h = {h}'}, got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError("x_ref holds non-finite values")
        if a.shape[-2] == 13:
            if not np.all(a[..., 12, :] == 1.0):
                raise ValueError("row 12 of x_ref (the row of ones, REF:62) must be all ones")
            a = a[..., :12, :]
        xr = np.ascontiguousarray(np.swapaxes(a, -1, -2))
    if foot_ref is not None:
        a = np.asarray(foot_ref, np.float64)
        if a.ndim < 2 or a.shape[-2] != 6 or (h is not None and a.shape[-1] != h):
            raise ValueError(f"foot_ref must have shape (..., 6, h){'' if h is None else f' with h = {h}'}, got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError("foot_ref holds non-finite values")
        fr = np.ascontiguousarray(np.swapaxes(a, -1, -2))
    return xr, fr


def _controls_f32(controls, h, B=None):
    """A control sequence as the evaluation takes it: (B,h,12) of any float dtype -> C-contiguous fp32.  Shape checked here
    (ValueError), before any call."""
    c = np.asarray(controls)
    if c.ndim != 3 or c.shape[1:] != (h, 12) or (B is not None and c.shape[0] != B) or not np.issubdtype(c.dtype, np.floating):
        raise ValueError(f"controls must be a float array of shape ({'B' if B is None else B}, {h}, 12) (row k = [f1 f2 m1 m2]), "
                         f"got {c.dtype} {c.shape}")
    return np.ascontiguousarray(c, np.float32)


ACT_TOL = 1e-4          # default activity tolerance of `certify`: the tolerance the solver's controls are held to against the oracle


def duals_to_reference_order(lam):
    """Multipliers as `certify` returns them, (..., h, 36) in the order of a step's rows, -> (..., 36h) in the row order of G at
    REF:273: friction row 8k + r (r < 8), box rows 8h + 24k + (r - 8), line-foot rows 32h + 4k + (r - 32)."""
    lam = np.asarray(lam)
    if lam.ndim < 2 or lam.shape[-1] != 36:
        raise ValueError(f"lam must have shape (..., h, 36), got {lam.shape}")
    h = lam.shape[-2]
    lead = lam.shape[:-2]
    return np.concatenate([lam[..., 0:8].reshape(lead + (8 * h,)), lam[..., 8:32].reshape(lead + (24 * h,)),
                           lam[..., 32:36].reshape(lead + (4 * h,))], -1)


# The evaluation family (`bmpc_evaluate`, `bmpc_evaluate_grad`, `bmpc_certify`, `bmpc_evaluate_samples` and their _device twins):
# per operation the ctypes output descriptor, the host entry (the device entry is the same name + "_device"), the shape of
# `controls` -- with an "S" in it the entries take a `bmpc_samples` descriptor --, whether the entries take `act_tol`, and the
# outputs in the order of the result dict: (name, dtype, shape).  Shapes are in terms of "B", "h" and "S".  `BatchSolver._eval` is
# the one body of all four rows, for host arrays and device tensors alike (`_Host` / `_Device`); `_eval_host` does a host call's
# lenient conversions before it.
_EVAL_OPS = {
    "evaluate": (_lib.CEvalOut, "bmpc_evaluate", ("B", "h", 12), False,
                 (("cost", "float64", ("B",)), ("objective", "float64", ("B",)), ("violation", "float64", ("B", 4)),
                  ("states", "float64", ("B", "h", 13)))),
    "evaluate_grad": (_lib.CGradOut, "bmpc_evaluate_grad", ("B", "h", 12), False,
                      (("cost", "float64", ("B",)), ("grad_u", "float64", ("B", "h", 12)), ("grad_x0", "float64", ("B", 12)))),
    "certify": (_lib.CCertOut, "bmpc_certify", ("B", "h", 12), True,
                (("lam", "float64", ("B", "h", 36)), ("resid", "float64", ("B", "h", 12)), ("summary", "float64", ("B", 4)),
                 ("n_active", "int32", ("B",)), ("status", "int32", ("B",)))),
    "evaluate_samples": (_lib.CSamplesOut, "bmpc_evaluate_samples", ("B", "S", "h", 12), False,
                         (("cost", "float64", ("B", "S")), ("violation", "float64", ("B", "S", 4)), ("score", "float64", ("B", "S")),
                          ("best", "int32", ("B",)), ("n_valid", "int32", ("B",)), ("weights", "float64", ("B", "S")),
                          ("u_mean", "float64", ("B", "h", 12)), ("ess", "float64", ("B",)))),
}

# The arguments of the entry families as rows (name, dtype, shape), in the order of the entries' argument lists, each table a
# function of the call's dimensions (a device call forms the rows once; a host call, whose arrays are exact already, never does).
def _input_rows(B, h, S=None):
    """The members of `bmpc_inputs` in its order, then the `controls` of the evaluation family ((B,S,h,12) with S plans each)."""
    return (("x_fb", "float32", (B, 12)), ("foot", "float32", (B, 6)), ("contact", "uint8", (B, h, 2)), ("phase", "int32", (B,)),
            ("x_cmd", "float32", (B, 12)), ("mu", "float32", (B, h, 2)), ("x_ref", "float32", (B, h, 12)),
            ("foot_ref", "float32", (B, h, 6)), ("controls", "float32", (B, h, 12) if S is None else (B, S, h, 12)))


def _solve_output_rows(B, h, S=None):
    return (("controls", "float32", (B, h, 12)), ("states", "float32", (B, h, 13)), ("iters", "int32", (B,)),
            ("residuals", "float32", (B, 2)), ("status", "int32", (B,)), ("nfactor", "int32", (B,)))


def _loop_rows(B, h, S=None):
    """What the closed loops (`rollout_device`, `simulate_device`) advance in place, then their optional inputs."""
    return (("x_fb", "float32", (B, 12)), ("foot", "float32", (B, 6)), ("t", "float64", (B,)),
            ("x_cmd", "float32", (B, 12)), ("mu", "float32", (B, h, 2)), ("push", "float32", (B, 6)))


def _step_rows(B, h=None, S=None):
    return (("x_fb", "float32", (B, 12)), ("u0", "float32", (B, 12)), ("foot", "float32", (B, 6)), ("contact0", "uint8", (B, 2)),
            ("wrench", "float32", (B, 6)), ("x_next", "float32", (B, 12)))


def _rollout_input_rows(B, h, S):
    return (("x_fb", "float32", (B, 12)), ("foot", "float32", (B, 6)), ("contact", "uint8", (B, h, 2)), ("x_cmd", "float32", (B, 12)),
            ("x_ref", "float32", (B, h, 12)), ("push", "float32", (B, 6)), ("controls", "float32", (B, S, h, 12)))


SAMPLES_MAX = 65536     # samples per instance `evaluate_samples` takes (include/bmpc.h)


def _shape(spec, B, h, S=None):
    return tuple(B if d == "B" else h if d == "h" else S if d == "S" else d for d in spec)


def _samples_f32(controls, h, B=None):
    """Candidate plans as `evaluate_samples` takes them: (B,S,h,12) of any float dtype -> C-contiguous fp32.  Shape checked here
    (ValueError), before any call."""
    c = np.asarray(controls)
    if c.ndim != 4 or c.shape[2:] != (h, 12) or (B is not None and c.shape[0] != B) or not np.issubdtype(c.dtype, np.floating) \
            or not 1 <= c.shape[1] <= SAMPLES_MAX:
        raise ValueError(f"controls must be a float array of shape ({'B' if B is None else B}, S, {h}, 12) with 1 <= S <= {SAMPLES_MAX} "
                         f"(plan s of instance b, row k = [f1 f2 m1 m2]), got {c.dtype} {c.shape}")
    return np.ascontiguousarray(c, np.float32)


def _samples_desc(S, w_viol, temperature):
    """`bmpc_samples` from the Python arguments, checked as the library checks it (ValueError)."""
    w = np.asarray(w_viol, np.float64).reshape(-1)
    if w.shape != (4,) or not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("w_viol must be four finite prices >= 0 (friction, force box, moment box, line foot)")
    return _lib.CSamples(int(S), 0, (C.c_double * 4)(*w), _temperature(temperature))


# The scalar options more than one entry family takes, each checked as the library checks it (ValueError) and returned as a float.
def _temperature(temperature):
    T = float(temperature)
    if not T > 0.0:
        raise ValueError("temperature must be > 0 (inf: uniform weights)")
    return T


def _fall(fall):
    try:
        tilt_max, z_min = (float(v) for v in fall)
    except (TypeError, ValueError):
        raise ValueError("fall must be a (tilt_max, z_min) pair") from None
    if tilt_max != tilt_max or z_min != z_min:
        raise ValueError("fall thresholds must not be NaN")
    return tilt_max, z_min


def _fz_floor(fz_floor):
    floor = float(fz_floor)
    if not floor >= 0.0:
        raise ValueError("fz_floor must be >= 0 and not NaN")
    return floor


def _act_tol(act_tol):
    tol = float(act_tol)
    if tol != tol:
        raise ValueError("act_tol must not be NaN")
    return tol


def _ptr(a):
    """Address of a NumPy array as an integer (what a `c_void_p` parameter takes; building a ctypes pointer object per argument
    costs ~2 us each, fourteen of them per solve)."""
    return None if a is None else a.__array_interface__["data"][0]


# Where the arrays of a call live.  Past a host method's conversions a host call and a device call are the same thing -- exactly-typed
# arrays in a space -- and the body of an entry family is written once over these operations:
#   ptrs(rows, values, B, h, S)        the addresses of a method's arguments, one per row of the table `rows(B, h, S)`.  On the
#                                      device each tensor is held to its row (`ptr`); on the host the method's own conversions have
#                                      just made every array exact, and the addresses are taken as they are;
#   ptr(name, value, dtype, *shapes)   the address of an array the CALLER supplies as it is: exactly of `dtype` (a name: "float32")
#                                      and of one of `shapes` (None for None), or ValueError naming the argument;
#   empty(dtype, shape), address(a)    an uninitialised output, and the address of an array the binding made itself;
#   suffix, tail, empty_is_null        what the entry's name and its argument list end in, and whether an array without elements
#                                      has no address to hand over.
class _Host:
    """NumPy arrays.  A copy that `ptr` had to make (a list, a non-contiguous array) is kept until the space goes, past the call."""
    suffix, tail, empty_is_null, keep = "", (), False, ()
    address = staticmethod(_ptr)

    @staticmethod
    def ptrs(rows, values, B, h=None, S=None):
        return [None if a is None else a.__array_interface__["data"][0] for a in values]

    def ptr(self, name, value, dtype, *shapes):
        if value is None:
            return None
        a = np.asarray(value)
        if a.dtype != dtype or a.shape not in shapes:
            raise ValueError(f"{name} must be {dtype} of shape {' or '.join(map(str, shapes))}, not {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        if a is not value:
            self.keep += (a,)
        return a.__array_interface__["data"][0]

    @staticmethod
    def empty(dtype, shape):
        return np.empty(shape, dtype)


class _Device:
    """Contiguous torch tensors on the solver's device `index`, which `dev` (the device of the call's first tensor) must be; the
    call is asynchronous on `stream`, a raw hipStream_t value (None: torch's current stream)."""
    suffix, empty_is_null = "_device", True

    def __init__(self, index, dev, stream):
        import torch
        if dev.type != "cuda" or dev.index != index:
            raise ValueError(f"tensors must live on cuda:{index}")
        self.torch, self.dev = torch, dev
        self.tail = (torch.cuda.current_stream(dev).cuda_stream if stream is None else stream,)

    def ptrs(self, rows, values, B, h=None, S=None):
        return [None if t is None else self.ptr(name, t, dtype, shape) for (name, dtype, shape), t in zip(rows(B, h, S), values)]

    def ptr(self, name, value, dtype, *shapes):
        if value is None:
            return None
        t = value
        if not isinstance(t, self.torch.Tensor) or t.device != self.dev or t.dtype != getattr(self.torch, dtype) \
                or not t.is_contiguous() or tuple(t.shape) not in shapes:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {' or '.join(map(str, shapes))} on {self.dev}")
        return t.data_ptr()

    def empty(self, dtype, shape):
        return self.torch.empty(shape, dtype=getattr(self.torch, dtype), device=self.dev)

    @staticmethod
    def address(t):
        return t.data_ptr()


def _host_array(name, value, shape, dtype=np.float32, required=True):
    """An argument of the strict host methods: any array of exactly `shape` (ValueError naming the argument), converted to
    C-contiguous `dtype`; None stays None unless `required`."""
    if value is None:
        if required:
            raise ValueError(f"{name} is required")
        return None
    a = np.asarray(value)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, not {a.shape}")
    return np.ascontiguousarray(a, dtype)


class _HandleOwner:
    """The native handle's lifetime as a Python object: `bmpc_destroy` runs when the LAST reference goes -- the solver's own, or
    that of an array `solve_inplace` returned.  Those arrays are views of the handle's page-locked I/O block, which
    `bmpc_destroy` frees; every view keeps this object alive through the buffer it is built on, so closing (or losing) the
    solver while results are still held defers the destruction instead of leaving them pointing at freed memory."""

    def __init__(self, lib, value):
        self._lib, self._value = lib, value

    def __del__(self):
        try:
            if self._value:
                self._lib.bmpc_destroy(C.c_void_p(self._value))
                self._value = None
        except Exception:
            pass


_COST_FUNCTION = None


def _cost_function():
    """The `torch.autograd.Function` behind `BatchSolver.cost_torch`, built on first use (the package imports without torch)."""
    global _COST_FUNCTION
    if _COST_FUNCTION is not None:
        return _COST_FUNCTION.apply
    import torch
    from torch.autograd.function import once_differentiable

    class _Cost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref):
            r = solver.evaluate_grad_device(x_fb, foot, contact, phase, controls, x_cmd=x_cmd, mu=mu, x_ref=x_ref, foot_ref=foot_ref)
            ctx.save_for_backward(r["grad_u"], r["grad_x0"])
            return r["cost"]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            grad_u, grad_x0 = ctx.saved_tensors
            g_x = (grad_output[:, None] * grad_x0).to(torch.float32) if ctx.needs_input_grad[1] else None
            g_u = (grad_output[:, None, None] * grad_u).to(torch.float32) if ctx.needs_input_grad[5] else None
            return None, g_x, None, None, None, g_u, None, None, None, None

    _COST_FUNCTION = _Cost
    return _Cost.apply


_PLANT_COST_FUNCTION = None


def _plant_cost_function():
    """The `torch.autograd.Function` behind `BatchSolver.plant_cost_torch`, built on first use like `_cost_function`."""
    global _PLANT_COST_FUNCTION
    if _PLANT_COST_FUNCTION is not None:
        return _PLANT_COST_FUNCTION.apply
    import torch
    from torch.autograd.function import once_differentiable

    class _PlantCost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, x_fb, foot, contact, controls, x_cmd, x_ref, push, opts):
            want = ["cost", "grad_u"] + (["grad_x0"] if ctx.needs_input_grad[1] else []) + (["grad_foot"] if ctx.needs_input_grad[2] else [])
            r = solver.plant_rollout_grad_device(x_fb.detach(), foot.detach(), contact, controls.detach().to(torch.float32).contiguous(),
                                                 x_cmd=x_cmd, x_ref=x_ref, push=push, want=want, **opts)
            ctx.dtypes = (x_fb.dtype, foot.dtype, controls.dtype)
            ctx.has = ("grad_x0" in r, "grad_foot" in r)
            ctx.save_for_backward(r["grad_u"], *[r[k] for k in ("grad_x0", "grad_foot") if k in r])
            return r["cost"]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            grad_u, *rest = ctx.saved_tensors
            grad_x0 = rest.pop(0) if ctx.has[0] else None
            grad_foot = rest.pop(0) if ctx.has[1] else None
            g_x = (grad_output[..., None] * grad_x0).sum(1).to(ctx.dtypes[0]) if grad_x0 is not None and ctx.needs_input_grad[1] else None
            g_f = (grad_output[..., None] * grad_foot).sum(1).to(ctx.dtypes[1]) if grad_foot is not None and ctx.needs_input_grad[2] else None
            g_u = (grad_output[..., None, None] * grad_u).to(ctx.dtypes[2]) if ctx.needs_input_grad[4] else None
            return None, g_x, g_f, None, g_u, None, None, None, None

    _PLANT_COST_FUNCTION = _PlantCost
    return _PlantCost.apply


class BatchSolver:
    """Owns one `bmpc_handle` (device memory + stream) for a fixed parameter block."""

    def __init__(self, mpc=None, biped=None, half=None, device=0, max_batch=65536, solver_options=None,
                 cparams=None):
        self._lib = _lib.load()
        self.cparams = cparams if cparams is not None else pack_params(mpc, biped, half, solver_options)
        self.h = int(self.cparams.h)
        self.device = int(device)
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        _lib.check(self._lib.bmpc_create(C.byref(self._h), C.byref(self.cparams), self.device, self.max_batch))
        self._owner = _HandleOwner(self._lib, self._h.value)
        self._io, self._io_key = None, None

    def set_params(self, cparams):
        """Replace the parameter block of this handle (same horizon): `bmpc_set_params`."""
        _lib.check(self._lib.bmpc_set_params(self._h, C.byref(cparams)))
        self.cparams = cparams

    def close(self):
        """Give the handle up.  It is destroyed at once unless arrays returned by `solve_inplace` are still alive: those are views
        of the handle's page-locked block, and the native handle (device memory included) then lives until the last of them goes
        -- copy what must outlive the solver if the memory is to come back now."""
        self._io, self._io_key = None, None
        self._owner = None                         # (the last reference unless views are alive: _HandleOwner.__del__ destroys)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host arrays --------------------------------------------------------------------------
    def _marshal(self, x_fb, foot, contact, phase, x_cmd, mu):
        h = self.h
        x_fb = np.ascontiguousarray(np.asarray(x_fb, np.float32).reshape(-1, 12))
        B = x_fb.shape[0]
        foot = None if foot is None else np.ascontiguousarray(np.asarray(foot, np.float32).reshape(B, 6))
        contact = _contact_u8(contact, B, h)
        phase = np.ascontiguousarray(np.asarray(phase, np.int32).reshape(B))
        if x_cmd is not None:
            x_cmd = np.ascontiguousarray(np.asarray(x_cmd, np.float32).reshape(B, 12))
        if mu is not None:
            mu = np.ascontiguousarray(np.asarray(mu, np.float32).reshape(B, h, 2))
        return B, x_fb, foot, contact, phase, x_cmd, mu

    def solve(self, x_fb, foot, contact, phase, x_cmd=None, mu=None, want_states=True, out=None, x_ref=None, foot_ref=None,
              evaluate=False, certify=False, act_tol=ACT_TOL):
        """Host arrays in, host arrays out (fp32 over PCIe, fp64 returned -- the reference's dtype, REF:300-304; the
        widening happens inside `bmpc_solve_batch_f64` while the results are unpacked, overlapped with the solve).  Returns
        (states (B,h,13) | None, controls (B,h,12), info).  `out`: optional (states | None, controls) fp64 C-contiguous
        arrays of those shapes to write into (a control loop reuses its buffers instead of allocating 8 MB per call).
        `x_ref` (B,h,12) / `foot_ref` (B,h,6): references to track instead of the generated ones (`bmpc_solve_inputs_f64`,
        include/bmpc.h; kernel layout, row j = step j); `foot` may then be None if `foot_ref` is given.
        `evaluate=True`: `info` gains `cost` (B,), `objective` (B,), `violation` (B,4) of the returned controls (those of the rescue
        pass where it ran), as `evaluate` gives them; by default `info` keeps exactly its four keys.
        `certify=True`: `info` gains `kkt`, the KKT certificate of the returned controls as `certify` gives it under `act_tol`:
        dict(stationarity, primal_ineq, complementarity, grad_scale (B,) each, n_active (B,), status (B,), lam (B,h,36))."""
        B, x_fb, foot, contact, phase, x_cmd, mu = self._marshal(x_fb, foot, contact, phase, x_cmd, mu)
        x_ref, foot_ref = _kernel_refs(x_ref, foot_ref, B, self.h)
        if foot is None and foot_ref is None:
            raise ValueError("foot is required unless foot_ref is given")
        h = self.h
        if out is not None:
            states, controls = out
            for a, shp in ((states, (B, h, 13)), (controls, (B, h, 12))):
                if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shp):
                    raise ValueError(f"out arrays must be C-contiguous float64 of shape {shp}")
            if controls is None:
                raise ValueError("out = (states | None, controls): controls is required")
            if not want_states:
                states = None
        else:
            controls = np.empty((B, h, 12), np.float64)
            states = np.empty((B, h, 13), np.float64) if want_states else None
        iters = np.empty(B, np.int32)
        status = np.empty(B, np.int32)
        nfactor = np.empty(B, np.int32)
        resid = np.empty((B, 2), np.float32)
        if x_ref is None and foot_ref is None:
            _lib.check(self._lib.bmpc_solve_batch_f64(
                self._h, B, _ptr(x_fb), _ptr(foot), _ptr(contact), _ptr(phase), _ptr(x_cmd), _ptr(mu),
                _ptr(controls), _ptr(states), _ptr(iters), _ptr(resid), _ptr(status), _ptr(nfactor)))
        else:
            inp = _lib.CInputs(_ptr(x_fb), _ptr(foot), _ptr(contact), _ptr(phase), _ptr(x_cmd), _ptr(mu), _ptr(x_ref), _ptr(foot_ref))
            _lib.check(self._lib.bmpc_solve_inputs_f64(
                self._h, B, C.byref(inp), _ptr(controls), _ptr(states), _ptr(iters), _ptr(resid), _ptr(status), _ptr(nfactor)))
        info = dict(iters=iters, status=status, nfactor=nfactor, residuals=resid)
        if evaluate:
            ev = self.evaluate(x_fb, foot, contact, phase, controls, x_cmd=x_cmd, mu=mu, x_ref=x_ref, foot_ref=foot_ref)
            info.update(cost=ev["cost"], objective=ev["objective"], violation=ev["violation"])
        if certify:
            ce = self.certify(x_fb, foot, contact, phase, controls, x_cmd=x_cmd, mu=mu, x_ref=x_ref, foot_ref=foot_ref, act_tol=act_tol)
            info["kkt"] = {k: ce[k] for k in ("stationarity", "primal_ineq", "complementarity", "grad_scale", "n_active", "status", "lam")}
        return states, controls, info

    def evaluate(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, want_states=False):
        """What the MPC's own model makes of GIVEN control sequences (`bmpc_evaluate`, include/bmpc.h): inputs as `solve` takes
        them (references in the kernel layout, generated where None) and `controls` (B,h,12), row k = [f1 f2 m1 m2] -- the
        solver's own, a warm-start guess, a policy's output, another solver's answer.  Returns dict(cost (B,), objective (B,),
        violation (B,4), states (B,h,13) | None), NumPy fp64: the cost REF:278-286 minimises completed to a sum of squares (>= 0: the
        number to rank samples by), the value 1/2 z'Pz + q'z the reference hands its solver, the largest violation per row class
        [friction pyramid, force box, moment box, line foot] (0: the class holds) and the predicted states X(U).
        `controls` may have any float dtype and is converted to fp32, which is what the kernel reads; a solve's fp64 `controls` ARE
        fp32 values (widened exactly), so they pass through unchanged.  Its shape is checked before the call (ValueError).  An
        instance with a non-finite entry anywhere, or a reference pitch of +-90 degrees, gets NaN in all its outputs (reference
        values are therefore not checked here); no other instance is touched."""
        return self._eval_host("evaluate", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, skip=() if want_states else ("states",))

    def evaluate_grad(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None):
        """Gradient of `evaluate`'s cost (`bmpc_evaluate_grad`, include/bmpc.h): arguments as `evaluate` takes them.  Returns
        dict(cost (B,), grad_u (B,h,12), grad_x0 (B,12)), NumPy fp64: `cost` with the bits `evaluate` gives, d cost / d controls, and
        d cost / d x_fb through the initial condition only -- the references, lever arms and linearisation are held fixed whether
        they were supplied or generated (generated references depend on x_fb; that dependence is not differentiated).  The cost is
        an exact quadratic in the controls: `grad_u` at U + D minus `grad_u` at U is the Hessian times D.  Bad instances as in
        `evaluate`: NaN in all their outputs."""
        return self._eval_host("evaluate_grad", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref)

    def certify(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None, act_tol=ACT_TOL):
        """KKT certificate of GIVEN control sequences (`bmpc_certify`, include/bmpc.h): arguments as `evaluate_grad` takes them, and
        `act_tol`: an inequality row with slack = b - C u is active iff slack <= act_tol (1 + |b|); only active rows may carry a
        multiplier.  Returns NumPy arrays: lam (B,h,36) fp64, the multipliers >= 0 in the row order of a step (0..7 friction, 8..19
        upper bounds, 20..31 lower bounds, 32..35 line foot; `duals_to_reference_order` gives the reference's order); resid (B,h,12),
        `evaluate_grad`'s grad_u + C' lam; summary (B,4) and its columns stationarity = max |resid|, primal_ineq = the largest
        violation (the maximum of `evaluate`'s four, same bits), complementarity = max |lam_i slack_i|, grad_scale = max |grad_u|
        (stationarity / grad_scale is the relative figure); n_active (B,) int32; status (B,) int32: 0 converged, 1 an iteration cap
        was reached (the residuals are valid, only not the smallest), 2 bad instance (NaN in the fp64 outputs, n_active -1)."""
        res = self._eval_host("certify", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, act_tol=act_tol)
        for i, k in enumerate(("stationarity", "primal_ineq", "complementarity", "grad_scale")):
            res[k] = res["summary"][:, i]
        return res

    def evaluate_samples(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                         w_viol=(0, 0, 0, 0), temperature=float("inf")):
        """S candidate plans per instance scored, ranked and blended in one call (`bmpc_evaluate_samples`, include/bmpc.h): inputs of
        B instances as `evaluate` takes them -- nothing is replicated -- and `controls` (B,S,h,12), plan s of instance b.  Returns
        NumPy arrays: cost (B,S), violation (B,S,4) as `evaluate` gives them for each plan; score (B,S) = cost + sum_c w_viol[c]
        violation[..., c]; n_valid (B,) int32, the number of samples with a finite score; best (B,) int32, the lowest index of the
        smallest valid score (-1: none); weights (B,S), the softmin weights exp(-(score - min) / temperature) normalised over the
        valid samples (invalid ones exactly 0; temperature inf: uniform); u_mean (B,h,12), the weighted mean plan (MPPI's update;
        at a small temperature the best plan); ess (B,), the effective sample size 1 / sum weights^2.  A sample with a non-finite
        control gets NaN cost, violation and score and weight 0 and touches no other; an instance without a valid sample gets
        best -1 and NaN u_mean and ess.  `max_batch` bounds B, not B S."""
        return self._samples_host(x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, w_viol, temperature)

    def _samples_host(self, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, w_viol, temperature, skip=()):
        """The host entry of row "evaluate_samples" of `_EVAL_OPS`: `_eval_host` with S plans per instance."""
        return self._eval_host("evaluate_samples", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref,
                               samples=(w_viol, temperature), skip=skip)

    def _eval_host(self, kind, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, act_tol=None, samples=None, skip=()):
        """The host entry of row `kind` of `_EVAL_OPS`: host arrays marshalled as `solve` does, then `_eval`."""
        per_sample = "S" in _EVAL_OPS[kind][2]
        c32 = (_samples_f32 if per_sample else _controls_f32)(controls, self.h)
        B, x_fb, foot, contact, phase, x_cmd, mu = self._marshal(x_fb, foot, contact, phase, x_cmd, mu)
        if c32.shape[0] != B:
            raise ValueError(f"controls must have shape ({B}, {'S, ' if per_sample else ''}{self.h}, 12), got {c32.shape}")
        x_ref, foot_ref = _kernel_refs(x_ref, foot_ref, B, self.h, finite=False)
        if foot is None and foot_ref is None:
            raise ValueError("foot is required unless foot_ref is given")
        return self._eval(_Host(), kind, B, (x_fb, foot, contact, phase, x_cmd, mu, x_ref, foot_ref, c32), {}, act_tol, samples, skip)

    def _eval(self, space, kind, B, inputs, given, act_tol=None, samples=None, skip=()):
        """Row `kind` of `_EVAL_OPS` on exactly-typed arrays in `space`: `inputs` are the members of `bmpc_inputs` in its order and
        `controls`, `given` maps outputs to the caller's arrays (the others are allocated here, unless named in `skip`: those stay
        None and are not computed), `samples` is (w_viol, temperature) for the row with S plans per instance.  One call; returns
        the dict of outputs."""
        struct, entry, u_shape, takes_tol, outputs = _EVAL_OPS[kind]
        h, S, mid = self.h, None, ()
        if takes_tol:
            mid += (_act_tol(act_tol),)
        if "S" in u_shape:
            controls = inputs[-1]
            if len(controls.shape) != 4 or not 1 <= controls.shape[1] <= SAMPLES_MAX:
                raise ValueError(f"controls must have shape ({B}, S, {h}, 12) with 1 <= S <= {SAMPLES_MAX}, got {tuple(controls.shape)}")
            S = int(controls.shape[1])
            mid += (C.byref(_samples_desc(S, *samples)),)
        res, out = {}, struct()
        for k, dtype, shape in outputs:
            a = res[k] = given.get(k)
            if a is not None:
                setattr(out, k, space.ptr(k, a, dtype, _shape(shape, B, h, S)))
            elif k not in skip:
                a = res[k] = space.empty(dtype, _shape(shape, B, h, S))
                setattr(out, k, space.address(a))
        *inp, u = space.ptrs(_input_rows, inputs, B, h, S)
        _lib.check(getattr(self._lib, entry + space.suffix)(self._h, B, C.byref(_lib.CInputs(*inp)), u, *mid, C.byref(out), *space.tail))
        return res

    def _io_views(self, B, with_x_cmd, with_mu, with_states):
        """NumPy views of the handle's page-locked I/O block laid out for batches of B (`bmpc_host_io`); cached per layout."""
        # (the key carries the C side's layout generation: a raw bmpc_host_io on this handle, or one that failed part-way,
        #  moves it, and the cached views -- whose offsets belong to the layout they were made for -- are not trusted any more)
        key = (B, bool(with_x_cmd), bool(with_mu), bool(with_states), int(self._lib.bmpc_host_io_generation(self._h)))
        if self._io_key == key:
            return self._io
        self._io, self._io_key = None, None
        v = _lib.CHostViews()
        _lib.check(self._lib.bmpc_host_io(self._h, B, int(key[1]), int(key[2]), int(key[3]), C.byref(v)))
        key = key[:4] + (int(self._lib.bmpc_host_io_generation(self._h)),)
        h = self.h
        owner = self._owner

        def view(addr, dtype, shape):
            if not addr:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            buf = (C.c_char * n).from_address(addr)
            buf._owner = owner                     # the array's base: keeps the native handle alive as long as the view is
            return np.frombuffer(buf, dtype=dtype).reshape(shape)

        self._io = dict(x_fb=view(v.x_fb, np.float32, (B, 12)), foot=view(v.foot, np.float32, (B, 6)),
                        contact=view(v.contact, np.uint8, (B, h, 2)), phase=view(v.phase, np.int32, (B,)),
                        x_cmd=view(v.x_cmd, np.float32, (B, 12)), mu=view(v.mu, np.float32, (B, h, 2)),
                        controls=view(v.controls, np.float64, (B, h, 12)), states=view(v.states, np.float64, (B, h, 13)),
                        iters=view(v.iters, np.int32, (B,)), residuals=view(v.residuals, np.float32, (B, 2)),
                        status=view(v.status, np.int32, (B,)), nfactor=view(v.nfactor, np.int32, (B,)))
        self._io_key = key
        return self._io

    def solve_inplace(self, x_fb, foot, contact, phase, x_cmd=None, mu=None, want_states=True):
        """Host arrays in, results IN the solver's own buffers: what a control loop that keeps its arrays wants.  The inputs are
        converted (fp32) straight into the handle's page-locked I/O block and cross PCIe in one copy; the batch goes out in up to
        three chunked launches on prioritised streams; the kernels' epilogues widen to the reference's fp64 (REF:300-304) and store
        `controls` and the per-instance counters straight into the block's host arrays, `states` are stored in HBM and follow by
        copy engine chunk by chunk -- except the last chunk's, which go the way of the controls -- so there is no unpacking pass
        (`bmpc_host_io` / `bmpc_solve_batch_io`, include/bmpc.h).  Returns (states | None, controls, info) as VIEWS of that block:
        their CONTENT is valid until the next `solve_inplace` of this solver (copy what must outlive it); the MEMORY stays valid
        as long as a view is held -- the views keep the native handle alive past `close()` / garbage collection of the solver
        (`_HandleOwner`).  Same values as `solve`, bit for bit."""
        h = self.h
        xf = np.asarray(x_fb)
        B = xf.size // 12
        io = self._io_views(B, x_cmd is not None, mu is not None, want_states)
        np.copyto(io["x_fb"], xf.reshape(B, 12), casting="same_kind")
        np.copyto(io["foot"], np.asarray(foot).reshape(B, 6), casting="same_kind")
        cc = np.asarray(contact)
        if cc.dtype == np.uint8 and cc.size == B * h * 2:          # (the fast path: one pass for the 0 / 1 check, one for the copy)
            if cc.size and cc.max() > 1:
                raise ValueError("contact entries must be 0 or 1")
            np.copyto(io["contact"], cc.reshape(B, h, 2))
        else:
            np.copyto(io["contact"], _contact_u8(cc, B, h))
        np.copyto(io["phase"], np.asarray(phase).reshape(B), casting="same_kind")
        if x_cmd is not None:
            np.copyto(io["x_cmd"], np.asarray(x_cmd).reshape(B, 12), casting="same_kind")
        if mu is not None:
            np.copyto(io["mu"], np.asarray(mu).reshape(B, h, 2), casting="same_kind")
        rc = self._lib.bmpc_solve_batch_io(self._h, B)
        if rc != 0:
            self._io, self._io_key = None, None    # (whatever went wrong: the next call lays the block out afresh)
            _lib.check(rc)
        info = dict(iters=io["iters"], status=io["status"], nfactor=io["nfactor"], residuals=io["residuals"])
        return io["states"], io["controls"], info

    def assemble(self, x_fb, foot, contact, phase, x_cmd=None, mu=None, want_matrices=True, x_ref=None, foot_ref=None):
        """Assembly stage only (parity tests, reference generators): x_ref (B,h,12), foot_ref (B,h,6) and -- with
        `want_matrices`, dense family only (h <= 20) -- Gt (B,6h,6h), qt (B,6h), else None for both.  Without them the
        launch runs on the handle's own kernel family at every supported horizon and nothing of size (6h)^2 is allocated.
        Supplied `x_ref` / `foot_ref` (kernel layout, as `solve`) are what the assembly is built from and come back widened."""
        B, x_fb, foot, contact, phase, x_cmd, mu = self._marshal(x_fb, foot, contact, phase, x_cmd, mu)
        xr_in, fr_in = _kernel_refs(x_ref, foot_ref, B, self.h)
        if foot is None and fr_in is None:
            raise ValueError("foot is required unless foot_ref is given")
        h = self.h
        x_ref = np.zeros((B, h, 12)); foot_ref = np.zeros((B, h, 6))
        Gt = np.zeros((B, 6 * h, 6 * h)) if want_matrices else None
        qt = np.zeros((B, 6 * h)) if want_matrices else None
        if xr_in is None and fr_in is None:
            _lib.check(self._lib.bmpc_debug_assemble(
                self._h, B, _ptr(x_fb), _ptr(foot), _ptr(contact), _ptr(phase), _ptr(x_cmd), _ptr(mu),
                _ptr(x_ref), _ptr(foot_ref), _ptr(Gt), _ptr(qt)))
        else:
            inp = _lib.CInputs(_ptr(x_fb), _ptr(foot), _ptr(contact), _ptr(phase), _ptr(x_cmd), _ptr(mu), _ptr(xr_in), _ptr(fr_in))
            _lib.check(self._lib.bmpc_debug_assemble_inputs(self._h, B, C.byref(inp), _ptr(x_ref), _ptr(foot_ref), _ptr(Gt), _ptr(qt)))
        return x_ref, foot_ref, Gt, qt

    # ---- device-resident (torch tensors are only a way to own HBM and a stream) ----------------
    def solve_device(self, x_fb, foot, contact, phase, x_cmd=None, mu=None, controls=None, states=None,
                     iters=None, residuals=None, status=None, nfactor=None, stream=None, x_ref=None, foot_ref=None):
        """Inputs/outputs are CUDA(HIP) torch tensors on this solver's device (fp32 / uint8 / int32,
        contiguous).  Asynchronous on `stream` (default: torch's current stream).  Returns the
        output tensors; nothing crosses PCIe.  `stream` is a raw hipStream_t value; torch's default stream
        is HIP's null stream (value 0) and is passed on as such, so the launch is ordered against the
        surrounding torch work like any torch kernel.  `x_ref` (B,h,12) / `foot_ref` (B,h,6) float32 tensors: references to track
        (`bmpc_solve_inputs_device`); `foot` may then be None if `foot_ref` is given.  Their values are not checked here (that
        would synchronise): a non-finite one shows as status 2 of its instance."""
        space = _Device(self.device, x_fb.device, stream)
        B = x_fb.shape[0]
        h = self.h
        if controls is None:
            controls = space.empty("float32", (B, h, 12))
        inp = space.ptrs(_input_rows, (x_fb, foot, contact, phase, x_cmd, mu, x_ref, foot_ref), B, h)
        out = space.ptrs(_solve_output_rows, (controls, states, iters, residuals, status, nfactor), B, h)
        if x_ref is not None or foot_ref is not None:
            _lib.check(self._lib.bmpc_solve_inputs_device(self._h, B, C.byref(_lib.CInputs(*inp)), *out, *space.tail))
        else:
            _lib.check(self._lib.bmpc_solve_batch_device(self._h, B, *inp[:6], *out, *space.tail))
        return controls, states

    def evaluate_device(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                        cost=None, objective=None, violation=None, states=None, want_states=False, stream=None):
        """`evaluate` on CUDA(HIP) torch tensors of this solver's device (`bmpc_evaluate_device`): inputs as `solve_device` takes
        them, `controls` (B,h,12) float32 -- e.g. the tensor a `solve_device` on the same stream has just been asked to fill: no
        synchronisation is needed in between.  Outputs are float64 tensors cost (B,), objective (B,), violation (B,4) and -- if
        passed, or with `want_states` -- states (B,h,13), allocated where not passed.  Asynchronous on `stream` (default: torch's
        current stream); nothing crosses PCIe.  Returns dict(cost, objective, violation, states | None)."""
        return self._eval_device("evaluate", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref,
                                 dict(cost=cost, objective=objective, violation=violation, states=states),
                                 skip=() if want_states else ("states",), stream=stream)

    def evaluate_grad_device(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                             cost=None, grad_u=None, grad_x0=None, stream=None):
        """`evaluate_grad` on CUDA(HIP) torch tensors of this solver's device (`bmpc_evaluate_grad_device`): inputs as
        `evaluate_device` takes them.  Outputs are float64 tensors cost (B,), grad_u (B,h,12), grad_x0 (B,12), allocated where not
        passed.  Asynchronous on `stream` (default: torch's current stream); nothing crosses PCIe.  Returns dict(cost, grad_u,
        grad_x0)."""
        return self._eval_device("evaluate_grad", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref,
                                 dict(cost=cost, grad_u=grad_u, grad_x0=grad_x0), stream=stream)

    def certify_device(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                       lam=None, resid=None, summary=None, n_active=None, status=None, act_tol=ACT_TOL, stream=None):
        """`certify` on CUDA(HIP) torch tensors of this solver's device (`bmpc_certify_device`): inputs as `evaluate_grad_device`
        takes them -- e.g. the `controls` tensor a `solve_device` on the same stream has just been asked to fill: no synchronisation
        is needed in between.  Outputs are tensors lam (B,h,36), resid (B,h,12), summary (B,4) float64, n_active (B,), status (B,)
        int32, allocated where not passed.  Asynchronous on `stream` (default: torch's current stream); nothing crosses PCIe.
        Returns dict(lam, resid, summary, n_active, status)."""
        return self._eval_device("certify", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref,
                                 dict(lam=lam, resid=resid, summary=summary, n_active=n_active, status=status), act_tol=act_tol,
                                 stream=stream)

    def evaluate_samples_device(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None,
                                w_viol=(0, 0, 0, 0), temperature=float("inf"), want=None, cost=None, violation=None, score=None,
                                best=None, n_valid=None, weights=None, u_mean=None, ess=None, stream=None):
        """`evaluate_samples` on CUDA(HIP) torch tensors of this solver's device (`bmpc_evaluate_samples_device`): inputs as
        `evaluate_device` takes them, `controls` (B,S,h,12) float32.  Outputs are tensors cost (B,S), violation (B,S,4), score (B,S),
        weights (B,S), u_mean (B,h,12), ess (B,) float64 and best (B,), n_valid (B,) int32: the caller's where passed, else allocated
        -- all of them, or with `want` (names) only those named or passed; the others stay None and are not computed (a call that
        wants no reduced output is one launch, else two).  Asynchronous on `stream` (default: torch's current stream) unless the
        handle's scratch has to grow (include/bmpc.h); nothing crosses PCIe.  Returns the dict of outputs."""
        given = dict(cost=cost, violation=violation, score=score, best=best, n_valid=n_valid, weights=weights, u_mean=u_mean, ess=ess)
        if want is not None and not set(want) <= set(given):
            raise ValueError(f"want names outputs among {sorted(given)}")
        return self._eval_device("evaluate_samples", x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, given,
                                 samples=(w_viol, temperature), skip=() if want is None else set(given) - set(want), stream=stream)

    def _eval_device(self, kind, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref, given, act_tol=None, samples=None,
                     skip=(), stream=None):
        """The device entry of row `kind` of `_EVAL_OPS` on CUDA(HIP) torch tensors: `_eval` on this solver's device and `stream`."""
        return self._eval(_Device(self.device, x_fb.device, stream), kind, x_fb.shape[0],
                          (x_fb, foot, contact, phase, x_cmd, mu, x_ref, foot_ref, controls), given, act_tol, samples, skip)

    def cost_torch(self, x_fb, foot, contact, phase, controls, x_cmd=None, mu=None, x_ref=None, foot_ref=None):
        """`evaluate`'s cost as a differentiable torch value: float64 tensor (B,) on the device, with gradients to `controls` (B,h,12)
        and `x_fb` (B,12), both float32 CUDA tensors; every other argument is non-differentiable.  The forward is ONE
        `bmpc_evaluate_grad_device` launch on torch's current stream, which also leaves `grad_u` / `grad_x0` behind; the backward
        scales them by the incoming gradient per instance and casts to float32 -- no second launch, no synchronisation, no second
        derivative (`once_differentiable`).
        `x_fb.grad` follows the fixed-references convention of `evaluate_grad`: it is d cost / d x_fb through the initial condition
        only, with the references, lever arms and linearisation held fixed whether they were supplied or generated.  With supplied
        references that is the full derivative; generated references move with x_fb, and that dependence is not differentiated."""
        return _cost_function()(self, x_fb, foot, contact, phase, controls, x_cmd, mu, x_ref, foot_ref)

    # ---- the step either side of the solve ------------------------------------
    def foot_position_world(self, x_fb, q):
        """Batched REF:406-424 `getFootPositionWorld`: x_fb (B,12), q (B,10) -> pf_w (B,6) fp64."""
        x_fb = np.ascontiguousarray(np.asarray(x_fb, np.float32).reshape(-1, 12))
        B = x_fb.shape[0]
        q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(B, 10))
        pf = np.empty((B, 6), np.float32)
        _lib.check(self._lib.bmpc_foot_position_world(self._h, B, _ptr(x_fb), _ptr(q), _ptr(pf)))
        return pf.astype(np.float64)

    def low_level_control(self, x_fb, t, pf_w, q, qd, contact0, u0):
        """Batched REF:444-470 `lowLevelControl`: contact0 (B,2) = contact[0, 0:2], u0 (B,12) = controls[0]
        -> tau (B,10) fp64."""
        x_fb = np.ascontiguousarray(np.asarray(x_fb, np.float32).reshape(-1, 12))
        B = x_fb.shape[0]
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(B))
        pf_w = np.ascontiguousarray(np.asarray(pf_w, np.float32).reshape(B, 6))
        q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(B, 10))
        qd = np.ascontiguousarray(np.asarray(qd, np.float32).reshape(B, 10))
        c0 = _contact_u8(np.asarray(contact0).reshape(B, 1, 2), B, 1).reshape(B, 2)
        u0 = np.ascontiguousarray(np.asarray(u0, np.float32).reshape(B, 12))
        tau = np.empty((B, 10), np.float32)
        _lib.check(self._lib.bmpc_low_level_control(self._h, B, _ptr(x_fb), _ptr(t), _ptr(pf_w), _ptr(q), _ptr(qd),
                                                    _ptr(c0), _ptr(u0), _ptr(tau)))
        return tau.astype(np.float64)

    def _gait(self, period, offset, duty):
        """`bmpc_gait` for a schedule that departs from this solver's default (None: the default)."""
        if period is None and offset is None and duty is None:
            return None
        gait = _lib.CGait()
        _lib.check(self._lib.bmpc_gait_default(C.byref(gait), int(self.cparams.half)))
        if period is not None:
            gait.period = int(period)
        if offset is not None:
            gait.offset[0], gait.offset[1] = int(offset[0]), int(offset[1])
        if duty is not None:
            gait.duty[0], gait.duty[1] = int(duty[0]), int(duty[1])
        return gait

    def contact_sequence(self, t, period=None, offset=None, duty=None, want_contact=True):
        """Batched gait scheduler on the device (REF:50-59 and the phase index of REF:99-100).
        t (B,) fp64 -> phase (B,) int32, contact (B,h,2) uint8.  Default schedule: the reference's, at this
        solver's half period; otherwise leg g stands at schedule step n iff ((n + offset[g]) % period) < duty[g]."""
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1))
        B = t.shape[0]
        gait = self._gait(period, offset, duty)
        phase = np.empty(B, np.int32)
        contact = np.empty((B, self.h, 2), np.uint8) if want_contact else None
        _lib.check(self._lib.bmpc_contact_sequence(self._h, B, _ptr(t), None if gait is None else C.byref(gait),
                                                   _ptr(phase), _ptr(contact)))
        return phase, contact

    def contact_sequence_device(self, t, phase=None, contact=None, period=None, offset=None, duty=None, stream=None):
        """`contact_sequence` on device tensors: t (B,) float64 CUDA tensor -> (phase int32 (B,), contact uint8
        (B,h,2)), asynchronous on `stream` (default: torch's current stream); nothing crosses PCIe."""
        space = _Device(self.device, t.device, stream)
        B = t.shape[0]
        tp = space.ptr("t", t, "float64", tuple(t.shape))
        if phase is None:
            phase = space.empty("int32", (B,))
        if contact is None:
            contact = space.empty("uint8", (B, self.h, 2))
        gait = self._gait(period, offset, duty)
        _lib.check(self._lib.bmpc_contact_sequence_device(self._h, B, tp, None if gait is None else C.byref(gait),
                                                          phase.data_ptr(), contact.data_ptr(), *space.tail))
        return phase, contact

    # ---- receding-horizon use --------------------------------------------------
    def set_warm_start(self, enable=True, shift=0, theta=0.5):
        """Later solves of the same batch size start from the state the previous solve left on the device
        (`bmpc_set_warm_start`): `shift` horizon steps later, penalties pulled back by rho0 (rho / rho0)^theta."""
        _lib.check(self._lib.bmpc_set_warm_start(self._h, 1 if enable else 0, int(shift), float(theta)))

    def reset_warm_start(self):
        _lib.check(self._lib.bmpc_reset_warm_start(self._h))

    def set_dispatch_order(self, order=None, longest_first_rollouts=True):
        """`bmpc_set_dispatch_order`: `order` is None or an int32 CUDA(HIP) tensor holding a permutation of 0 .. B-1
        (workgroup g solves instance order[g]; keep the tensor alive while it is set); `longest_first_rollouts`:
        roll-outs dispatch each period's instances by descending iteration count of the period before.  Results never
        depend on the order, only the time a batch takes."""
        import torch
        ptr = None
        if order is not None:
            if not (isinstance(order, torch.Tensor) and order.is_cuda and order.dtype == torch.int32 and order.is_contiguous()):
                raise ValueError("order must be a contiguous int32 tensor on the solver's device")
            ptr = order.data_ptr()
        self._order_keepalive = order
        _lib.check(self._lib.bmpc_set_dispatch_order(self._h, ptr, 1 if longest_first_rollouts else 0))

    def rollout_device(self, x_fb, foot, t, steps, x_cmd=None, mu=None, period=None, offset=None, duty=None,
                       want_iters=True, stream=None):
        """`steps` closed-loop control periods on device tensors (`bmpc_rollout_device`): x_fb (B,12) float32 and
        t (B,) float64 are advanced IN PLACE; returns dict(u0 (steps,B,12), x (steps,B,12), iters (steps,B) | None,
        status_any (B,)).  Asynchronous on `stream` (default: torch's current stream)."""
        space = _Device(self.device, x_fb.device, stream)
        B = x_fb.shape[0]
        gait = self._gait(period, offset, duty)
        u0 = space.empty("float32", (steps, B, 12))
        xt = space.empty("float32", (steps, B, 12))
        its = space.empty("int32", (steps, B)) if want_iters else None
        st_any = space.empty("int32", (B,))
        a = space.ptrs(_loop_rows, (x_fb, foot, t, x_cmd, mu), B, self.h)
        _lib.check(self._lib.bmpc_rollout_device(
            self._h, B, int(steps), *a[:3], None if gait is None else C.byref(gait), *a[3:],
            u0.data_ptr(), xt.data_ptr(), None if its is None else its.data_ptr(), st_any.data_ptr(), *space.tail))
        return dict(u0=u0, x=xt, iters=its, status_any=st_any)

    # ---- the plant and the closed loop on it (bmpc_plant_step*, bmpc_simulate_device) ---------------
    @staticmethod
    def _plant(integrator, substeps, move_feet=True, push_from=0, push_steps=0):
        """`bmpc_plant` from the keyword arguments; an unknown integrator name or a value the library would refuse is a ValueError."""
        if integrator not in _lib.PLANT_INTEGRATORS:
            raise ValueError(f"integrator must be one of {sorted(_lib.PLANT_INTEGRATORS)}, not {integrator!r}")
        if not 1 <= int(substeps) <= 64:
            raise ValueError(f"substeps must be in [1, 64], not {substeps}")
        if int(push_from) < 0 or int(push_steps) < 0:
            raise ValueError("push_from and push_steps must be >= 0")
        return _lib.CPlant(_lib.PLANT_INTEGRATORS[integrator], int(substeps), 1 if move_feet else 0, int(push_from), int(push_steps))

    @staticmethod
    def _body(space, body, B):
        """A `body` mapping of float64 arrays in `space` -- any of m (B,), I (B,3,3) or (B,9), g (B,) -- as the `bmpc_plant_body`
        argument of an entry (None for None); anything but a mapping with those keys is a ValueError."""
        if body is None:
            return None
        if not hasattr(body, "keys") or set(body.keys()) - {"m", "I", "g"}:
            raise ValueError("body must be a mapping with any of the keys 'm', 'I', 'g'")
        cb = _lib.CPlantBody()
        for k, shapes in (("m", ((B,),)), ("I", ((B, 3, 3), (B, 9))), ("g", ((B,),))):
            setattr(cb, k, space.ptr(f"body[{k!r}]", body.get(k), "float64", *shapes))
        return C.byref(cb)

    @staticmethod
    def _ground_mu(ground, want_applied=False):
        """The `mu` of a `ground` mapping, or None ({}: the handle's mu); anything but a mapping whose only key is 'mu', or
        `want_applied` without a ground, is a ValueError."""
        if ground is None:
            if want_applied:
                raise ValueError("want_applied needs a ground")
            return None
        if not hasattr(ground, "keys") or set(ground.keys()) - {"mu"}:
            raise ValueError("ground must be a mapping whose only key is 'mu'")
        return ground.get("mu")

    @classmethod
    def _ground(cls, space, ground, B):
        """A `ground` mapping -- mu, a float64 array (B,2) in `space`, or absent -- as the `bmpc_plant_ground` argument of an entry
        (None for None)."""
        if ground is None:
            return None
        return C.byref(_lib.CPlantGround(space.ptr("ground['mu']", cls._ground_mu(ground), "float64", (B, 2))))

    def _step(self, space, B, plant, body, ground, want_applied, inputs, x_next):
        """One plant step on exactly-typed arrays in `space` (`inputs`: x_fb, u0, foot, contact0, wrench | None): the plain entry
        without a body and a ground, the body's without a ground, else the ground's.  Returns x_next, or with `want_applied`
        (x_next, u_applied, flags)."""
        args = space.ptrs(_step_rows, inputs + (x_next,), B)
        ua = fl = None
        if ground is None and body is None:
            entry, structs = "bmpc_plant_step", ()
        elif ground is None:
            entry, structs = "bmpc_plant_step_body", (self._body(space, body, B),)
        else:
            entry, structs = "bmpc_plant_step_ground", (self._body(space, body, B), self._ground(space, ground, B))
            if want_applied:
                ua, fl = space.empty("float32", (B, 12)), space.empty("uint8", (B,))
            args += [space.address(ua), space.address(fl)] if want_applied else [None, None]
        _lib.check(getattr(self._lib, entry + space.suffix)(self._h, B, C.byref(plant), *structs, *args, *space.tail))
        return (x_next, ua, fl) if want_applied else x_next

    def plant_step(self, x_fb, u0, foot, contact0, wrench=None, integrator="rk4", substeps=4, body=None, ground=None,
                   want_applied=False):
        """One control period of the plant -- the nonlinear single rigid body of include/bmpc.h, NOT the controller's linear model --
        under held controls (`bmpc_plant_step`): x_fb (B,12), u0 (B,12) = [f1 f2 m1 m2], foot (B,6), contact0 (B,2) (a leg with bit 0
        transmits nothing), wrench (B,6) = [F, M] in the world frame or None -> x_next (B,12) fp64.  A bad instance (non-finite input,
        pitch at +-90 degrees) comes back all NaN.  `body`: a mapping with any of m (B,), I (B,3,3) or (B,9), g (B,) as float64
        arrays -- the PLANT's mass, body inertia and gravity per instance in place of this solver's (`bmpc_plant_step_body`); a bad
        body (non-finite, m <= 0, singular I) comes back all NaN too.
        `ground`: a mapping whose only allowed key is mu, float64 (B,2) -- the true friction under each leg; {} means this solver's
        mu.  A flat floor with Coulomb friction then stands between u0 and the body (`bmpc_plant_step_ground`): a stance leg with
        fz <= 0 transmits nothing (flag 4 << leg), a loaded one whose tangential force exceeds mu fz has it scaled onto the cone
        (flag 1 << leg); a mu that is NaN or negative comes back all NaN.  With `want_applied` the result is (x_next, u_applied
        (B,12) float32 -- what reached the body --, flags (B,) uint8)."""
        plant = self._plant(integrator, substeps)
        self._ground_mu(ground, want_applied)
        a = np.asarray(x_fb, np.float32)
        if a.ndim != 2 or a.shape[1] != 12:
            raise ValueError(f"x_fb must have shape (B, 12), not {a.shape}")
        B = a.shape[0]
        inputs = (np.ascontiguousarray(a), _host_array("u0", u0, (B, 12)), _host_array("foot", foot, (B, 6)),
                  _host_array("contact0", None if contact0 is None else np.asarray(contact0) != 0, (B, 2), np.uint8),
                  _host_array("wrench", wrench, (B, 6), required=False))
        res = self._step(_Host(), B, plant, body, ground, want_applied, inputs, np.empty((B, 12), np.float32))
        return (res[0].astype(np.float64),) + res[1:] if want_applied else res.astype(np.float64)

    def plant_step_device(self, x_fb, u0, foot, contact0, wrench=None, integrator="rk4", substeps=4, x_next=None, stream=None,
                          body=None, ground=None, want_applied=False):
        """`plant_step` on device tensors (`bmpc_plant_step_device`): float32 x_fb (B,12), u0 (B,12), foot (B,6), uint8 contact0 (B,2),
        float32 wrench (B,6) or None -> x_next (B,12) float32 (allocated unless given).  `body`: as for `plant_step`, of float64
        tensors on the device (`bmpc_plant_step_body_device`).  `ground`, `want_applied`: as for `plant_step`, mu a float64 tensor
        (B,2) on the device (`bmpc_plant_step_ground_device`); with `want_applied` the result is (x_next, u_applied (B,12) float32,
        flags (B,) uint8).  Asynchronous on `stream` (default: torch's current stream); nothing crosses PCIe."""
        plant = self._plant(integrator, substeps)
        self._ground_mu(ground, want_applied)
        space = _Device(self.device, x_fb.device, stream)
        if x_fb.dim() != 2:
            raise ValueError("x_fb must have shape (B, 12)")
        B = x_fb.shape[0]
        if x_next is None:
            x_next = space.empty("float32", (B, 12))
        return self._step(space, B, plant, body, ground, want_applied, (x_fb, u0, foot, contact0, wrench), x_next)

    def simulate_device(self, x_fb, foot, t, steps, x_cmd=None, mu=None, period=None, offset=None, duty=None, integrator="rk4",
                        substeps=4, move_feet=True, push=None, push_from=0, push_steps=0, want_iters=True, stream=None, body=None,
                        fall=None, ground=None, fz_floor=0.0):
        """`steps` closed-loop control periods against the plant of `plant_step` (`bmpc_simulate_device`): `rollout_device`'s loop
        with the rigid body in place of the controller's own prediction.  x_fb (B,12) float32, foot (B,6) float32 and t (B,) float64
        are advanced IN PLACE (so `foot` must be writable): with `move_feet` a leg that lands gets the swing controller's foothold
        target at the new state.  push (B,6) float32 = [F, M] (world frame) or None acts in periods push_from <= s < push_from +
        push_steps.  Returns dict(u0 (steps,B,12), x (steps,B,12), foot (steps,B,6) -- the footholds after each period's update --,
        iters (steps,B) | None, status_any (B,)).  Asynchronous on `stream` (default: torch's current stream).
        `body`: the PLANT's m (B,), I (B,3,3) or (B,9), g (B,) per instance as float64 device tensors (any subset; the rest is this
        solver's) -- the controller inside the loop keeps this solver's model: one model, many bodies (`bmpc_simulate_body_device`).
        `fall` = (tilt_max, z_min): the dict also carries first_fall (B,) int32 -- the first period after which
        !(|roll| <= tilt_max and |pitch| <= tilt_max and p_z >= z_min), a NaN state included, or -1 --, max_tilt (B,) and min_z (B,)
        float32, the extrema of max(|roll|, |pitch|) and p_z over the periods that are not NaN.  Fallen instances run on.
        `ground`: a mapping whose only allowed key is mu, a float64 device tensor (B,2) -- the TRUE friction under each leg; {} means
        this solver's mu (`bmpc_simulate_ground_device`).  The `mu` argument stays the controller's belief.  The plant integrates
        what the ground transmits of each command (see `plant_step`), u0 keeps recording the command, and the dict also carries
        u_applied (steps,B,12) float32, contact_flags (steps,B) uint8 (1, 2: leg 0 / 1 slipped; 4, 8: unloaded), first_slip (B,)
        int32 -- the first period with a slip, or -1 --, slip_periods and unloaded_periods (B,2) int32, and mu_demand (B,) float32:
        the largest tangential over normal force any loaded leg with fz >= `fz_floor` asked for, NaN if none did.  A slipping foot
        keeps its foothold."""
        import torch
        plant = self._plant(integrator, substeps, move_feet, push_from, push_steps)
        self._ground_mu(ground)
        floor = None if ground is None else _fz_floor(fz_floor)
        if fall is not None:
            tilt_max, z_min = _fall(fall)
        space = _Device(self.device, x_fb.device, stream)
        dev = space.dev
        if x_fb.dim() != 2 or int(steps) < 0:
            raise ValueError("x_fb must have shape (B, 12) and steps must be >= 0")
        B, steps = x_fb.shape[0], int(steps)
        cb = self._body(space, body, B)
        a = space.ptrs(_loop_rows, (x_fb, foot, t, x_cmd, mu, push), B, self.h)
        args, opt = a[:3], a[3:]
        gait = self._gait(period, offset, duty)
        u0 = torch.empty((steps, B, 12), dtype=torch.float32, device=dev)
        xt = torch.empty((steps, B, 12), dtype=torch.float32, device=dev)
        ft = torch.empty((steps, B, 6), dtype=torch.float32, device=dev)
        its = torch.empty((steps, B), dtype=torch.int32, device=dev) if want_iters else None
        st_any = torch.zeros(B, dtype=torch.int32, device=dev)
        out = dict(u0=u0, x=xt, foot=ft, iters=its, status_any=st_any)
        traj = [u0.data_ptr(), xt.data_ptr(), ft.data_ptr(), None if its is None else its.data_ptr(), st_any.data_ptr()]
        if cb is None and fall is None and ground is None:
            _lib.check(self._lib.bmpc_simulate_device(
                self._h, B, steps, C.byref(plant), *args, None if gait is None else C.byref(gait), *opt, *traj, *space.tail))
            return out
        co = None
        if fall is not None:
            # (filled here as the entry does it, so that steps == 0 or B == 0, where the entry touches nothing, reads the same)
            out.update(first_fall=torch.full((B,), -1, dtype=torch.int32, device=dev),
                       max_tilt=torch.full((B,), float("nan"), dtype=torch.float32, device=dev),
                       min_z=torch.full((B,), float("nan"), dtype=torch.float32, device=dev))
            co = _lib.CSimOutcome(tilt_max, z_min, out["first_fall"].data_ptr(), out["max_tilt"].data_ptr(), out["min_z"].data_ptr())
        if ground is not None:
            # (the reduced arrays filled here as the entry does it, like the outcome's)
            out.update(u_applied=torch.empty((steps, B, 12), dtype=torch.float32, device=dev),
                       contact_flags=torch.empty((steps, B), dtype=torch.uint8, device=dev),
                       first_slip=torch.full((B,), -1, dtype=torch.int32, device=dev),
                       slip_periods=torch.zeros((B, 2), dtype=torch.int32, device=dev),
                       unloaded_periods=torch.zeros((B, 2), dtype=torch.int32, device=dev),
                       mu_demand=torch.full((B,), float("nan"), dtype=torch.float32, device=dev))
            go = _lib.CGroundOut(floor, *[out[k].data_ptr() for k in ("u_applied", "contact_flags", "first_slip", "slip_periods",
                                                                                "unloaded_periods", "mu_demand")])
            _lib.check(self._lib.bmpc_simulate_ground_device(
                self._h, B, steps, C.byref(plant), cb, self._ground(space, ground, B), *args,
                None if gait is None else C.byref(gait), *opt, *traj, None if co is None else C.byref(co), C.byref(go), *space.tail))
            return out
        _lib.check(self._lib.bmpc_simulate_body_device(
            self._h, B, steps, C.byref(plant), cb, *args, None if gait is None else C.byref(gait), *opt,
            *traj, None if co is None else C.byref(co), *space.tail))
        return out

    # ---- S candidate plans per instance on the plant (bmpc_plant_rollout_samples*) ---------------------
    _ROLLOUT_OUTPUTS = (("cost", "float64", ("B", "S")), ("score", "float64", ("B", "S")), ("x_end", "float32", ("B", "S", 12)),
                        ("foot_end", "float32", ("B", "S", 6)), ("x_traj", "float32", ("B", "S", "h", 12)),
                        ("first_fall", "int32", ("B", "S")), ("max_tilt", "float32", ("B", "S")), ("min_z", "float32", ("B", "S")),
                        ("first_slip", "int32", ("B", "S")), ("slip_periods", "int32", ("B", "S", 2)),
                        ("unloaded_periods", "int32", ("B", "S", 2)), ("mu_demand", "float32", ("B", "S")), ("best", "int32", ("B",)),
                        ("n_valid", "int32", ("B",)), ("weights", "float64", ("B", "S")), ("u_mean", "float64", ("B", "h", 12)),
                        ("ess", "float64", ("B",)))
    _ROLLOUT_GROUND_ONLY = ("first_slip", "slip_periods", "unloaded_periods", "mu_demand")

    @classmethod
    def _rollout_opts(cls, S, push_from, push_steps, integrator, substeps, move_feet, ground, fall, fz_floor, w_fall, w_slip, w_unloaded,
                      temperature, want):
        """(`bmpc_plant`, `bmpc_rollout_price`, the names of the wanted outputs) from the keyword arguments of the roll-out methods,
        checked as the library checks them (ValueError).  `want` None: every output there is (the ground's four only with a ground)."""
        plant = cls._plant(integrator, substeps, move_feet, push_from, push_steps)
        cls._ground_mu(ground)
        w = [float(v) for v in (w_fall, w_slip, w_unloaded)]
        if not all(np.isfinite(v) and v >= 0.0 for v in w):
            raise ValueError("w_fall, w_slip and w_unloaded must be finite and >= 0")
        T, (tilt_max, z_min), floor = _temperature(temperature), _fall(fall), _fz_floor(fz_floor)
        names = [k for k, _, _ in cls._ROLLOUT_OUTPUTS]
        if want is None:
            want = [k for k in names if ground is not None or k not in cls._ROLLOUT_GROUND_ONLY]
        want = list(want)
        if not want or not set(want) <= set(names):
            raise ValueError(f"want names at least one output among {names}")
        if ground is None and set(want) & set(cls._ROLLOUT_GROUND_ONLY):
            raise ValueError(f"{', '.join(cls._ROLLOUT_GROUND_ONLY)} need a ground")
        if not 1 <= int(S) <= SAMPLES_MAX:
            raise ValueError(f"controls must hold 1 <= S <= {SAMPLES_MAX} plans per instance")
        return plant, _lib.CRolloutPrice(int(S), 0, *w, T, tilt_max, z_min, floor), want

    def _rollout(self, space, B, S, opts, inputs, body, ground):
        """The plan roll-out on exactly-typed arrays in `space`: `opts` as `_rollout_opts` returns them, `inputs` in the order of
        `_rollout_input_rows`.  The wanted outputs are allocated here; one call; returns their dict."""
        plant, price, want = opts
        args = space.ptrs(_rollout_input_rows, inputs, B, self.h, S)
        cb, cg = self._body(space, body, B), self._ground(space, ground, B)
        res = {k: space.empty(dtype, _shape(shape, B, self.h, S)) for k, dtype, shape in self._ROLLOUT_OUTPUTS if k in want}
        out = _lib.CRolloutOut(**{k: space.address(a) for k, a in res.items()})
        if B == 0 and space.empty_is_null:      # (nothing to do, and an empty tensor has no address to hand over)
            return res
        _lib.check(getattr(self._lib, "bmpc_plant_rollout_samples" + space.suffix)(
            self._h, B, *args, C.byref(plant), cb, cg, C.byref(price), C.byref(out), *space.tail))
        return res

    def plant_rollout_samples(self, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0,
                              integrator="rk4", substeps=4, move_feet=True, body=None, ground=None, fall=(float("inf"), float("-inf")),
                              fz_floor=0.0, w_fall=0.0, w_slip=0.0, w_unloaded=0.0, temperature=float("inf"), want=None):
        """What the rigid body makes of S whole plans per instance, in one launch (`bmpc_plant_rollout_samples`, include/bmpc.h):
        x_fb (B,12), foot (B,6), contact (B,h,2) -- row k holds over period k --, controls (B,S,h,12), plan s of instance b; nothing
        is replicated and `max_batch` bounds B, not B S.  Per period the plant of `plant_step` integrates the plan's control (through
        the `ground`, where given; under `push` (B,6) in periods push_from <= k < push_from + push_steps), the new state is stored in
        fp32 and the next period starts from it; with `move_feet` a leg whose contact bit goes 0 -> 1 from row k to row k + 1 lands
        on the swing controller's target at that state.  `body`, `ground`: as for `plant_step`; `fall` = (tilt_max, z_min) and
        `fz_floor`: as for `simulate_device`; x_cmd (B,12): per-instance commands; x_ref (B,h,12): the state reference in the kernel
        layout (None: generated as the solve generates it).  Returns a dict of NumPy arrays -- all of them, or those named in `want`:
        cost (B,S) = sum_k sum_i Q_i (x_k,i - x_ref_k,i)^2 + R_i u_k,i^2 on the stored states and the COMMANDED controls; score (B,S)
        = cost + w_fall [fell] + w_slip (periods a leg slipped) + w_unloaded (periods a stance leg was unloaded); x_end (B,S,12),
        foot_end (B,S,6), x_traj (B,S,h,12) float32; first_fall (B,S) int32, max_tilt, min_z (B,S) float32; with a ground first_slip
        (B,S), slip_periods, unloaded_periods (B,S,2) int32 and mu_demand (B,S) float32; and per instance best, n_valid (B,) int32,
        weights (B,S), u_mean (B,h,12), ess (B,) as `evaluate_samples` forms them from these scores at `temperature`.  A plan with a
        non-finite control, or one whose plant step goes bad, has a NaN state from that period on, NaN cost and score, first_fall at
        that period and weight 0; a bad instance (non-finite x_fb / foot / push / reference, bad body, mu NaN or negative) makes
        every plan of it so."""
        c32 = _samples_f32(controls, self.h)
        B, S, h = c32.shape[0], c32.shape[1], self.h
        opts = self._rollout_opts(S, push_from, push_steps, integrator, substeps, move_feet, ground, fall, fz_floor, w_fall, w_slip,
                                  w_unloaded, temperature, want)
        inputs = (_host_array("x_fb", x_fb, (B, 12)), _host_array("foot", foot, (B, 6)), _contact_u8(contact, B, h),
                  _host_array("x_cmd", x_cmd, (B, 12), required=False), _host_array("x_ref", x_ref, (B, h, 12), required=False),
                  _host_array("push", push, (B, 6), required=False), c32)
        return self._rollout(_Host(), B, S, opts, inputs, body, ground)

    def plant_rollout_samples_device(self, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0,
                                     integrator="rk4", substeps=4, move_feet=True, body=None, ground=None,
                                     fall=(float("inf"), float("-inf")), fz_floor=0.0, w_fall=0.0, w_slip=0.0, w_unloaded=0.0,
                                     temperature=float("inf"), want=None, stream=None):
        """`plant_rollout_samples` on CUDA(HIP) torch tensors of this solver's device (`bmpc_plant_rollout_samples_device`): float32
        x_fb (B,12), foot (B,6), controls (B,S,h,12), x_cmd (B,12), x_ref (B,h,12), push (B,6), uint8 contact (B,h,2); `body` and
        `ground` of float64 device tensors as for `plant_step_device`.  The outputs -- all of them, or those named in `want` -- are
        allocated here; one launch, and a second for the per-instance reductions where one of them is wanted.  Asynchronous on
        `stream` (default: torch's current stream) unless the handle's scratch has to grow (include/bmpc.h); nothing crosses PCIe.
        Returns the dict of output tensors."""
        if x_fb.dim() != 2 or controls.dim() != 4:
            raise ValueError(f"x_fb must have shape (B, 12) and controls (B, S, {self.h}, 12)")
        B, S = x_fb.shape[0], int(controls.shape[1])
        opts = self._rollout_opts(S, push_from, push_steps, integrator, substeps, move_feet, ground, fall, fz_floor, w_fall, w_slip,
                                  w_unloaded, temperature, want)
        return self._rollout(_Device(self.device, x_fb.device, stream), B, S, opts, (x_fb, foot, contact, x_cmd, x_ref, push, controls),
                             body, ground)

    # ---- the gradient of the plan roll-out (bmpc_plant_rollout_grad*) ------------------------------------
    _ROLLOUT_GRAD_OUTPUTS = (("cost", "float64", ("B", "S")), ("grad_u", "float64", ("B", "S", "h", 12)),
                             ("grad_x0", "float64", ("B", "S", 12)), ("grad_foot", "float64", ("B", "S", 6)),
                             ("x_traj", "float32", ("B", "S", "h", 12)), ("first_bad", "int32", ("B", "S")))

    @classmethod
    def _rollout_grad_opts(cls, S, push_from, push_steps, integrator, substeps, move_feet, ground, want):
        """(`bmpc_plant`, the names of the wanted outputs) from the keyword arguments of the gradient methods, checked as the library
        checks them (ValueError).  `want` None: every output."""
        plant = cls._plant(integrator, substeps, move_feet, push_from, push_steps)
        cls._ground_mu(ground)
        names = [k for k, _, _ in cls._ROLLOUT_GRAD_OUTPUTS]
        want = names if want is None else list(want)
        if not want or not set(want) <= set(names):
            raise ValueError(f"want names at least one output among {names}")
        if not 1 <= int(S) <= SAMPLES_MAX:
            raise ValueError(f"controls must hold 1 <= S <= {SAMPLES_MAX} plans per instance")
        return plant, want

    def _rollout_grad(self, space, B, S, opts, inputs, body, ground):
        """The roll-out gradient on exactly-typed arrays in `space`: `opts` as `_rollout_grad_opts` returns them, `inputs` in the
        order of `_rollout_input_rows`.  The wanted outputs are allocated here; one call; returns their dict."""
        plant, want = opts
        args = space.ptrs(_rollout_input_rows, inputs, B, self.h, S)
        cb, cg = self._body(space, body, B), self._ground(space, ground, B)
        res = {k: space.empty(dtype, _shape(shape, B, self.h, S)) for k, dtype, shape in self._ROLLOUT_GRAD_OUTPUTS if k in want}
        out = _lib.CRolloutGradOut(**{k: space.address(a) for k, a in res.items()})
        if B == 0 and space.empty_is_null:      # (nothing to do, and an empty tensor has no address to hand over)
            return res
        _lib.check(getattr(self._lib, "bmpc_plant_rollout_grad" + space.suffix)(
            self._h, B, S, *args, C.byref(plant), cb, cg, C.byref(out), *space.tail))
        return res

    def plant_rollout_grad(self, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0,
                           integrator="rk4", substeps=4, move_feet=True, body=None, ground=None, want=None):
        """Which way each of S whole plans per instance should move on the rigid body (`bmpc_plant_rollout_grad`, include/bmpc.h):
        the cost of `plant_rollout_samples` on the same arguments and its gradient, the discrete adjoint of that roll-out -- every
        substep and stage of the plant step, the ground on the branch the forward pass took, the footholds landing legs take.  The
        fp32 rounding of the stored states is the identity in the derivative; the references, the commands, the body, mu, the push
        and the contact table are held fixed.  Returns a dict of NumPy arrays -- all of them, or those named in `want`: cost (B,S),
        grad_u (B,S,h,12) = d cost / d controls, grad_x0 (B,S,12) = d cost / d x_fb, grad_foot (B,S,6) = d cost / d foot, float64;
        x_traj (B,S,h,12) float32, the stored states; first_bad (B,S) int32: -1, or the period from which the plan's state is NaN
        -- such a plan has NaN cost and gradients, and no other plan is touched."""
        c32 = _samples_f32(controls, self.h)
        B, S, h = c32.shape[0], c32.shape[1], self.h
        opts = self._rollout_grad_opts(S, push_from, push_steps, integrator, substeps, move_feet, ground, want)
        inputs = (_host_array("x_fb", x_fb, (B, 12)), _host_array("foot", foot, (B, 6)), _contact_u8(contact, B, h),
                  _host_array("x_cmd", x_cmd, (B, 12), required=False), _host_array("x_ref", x_ref, (B, h, 12), required=False),
                  _host_array("push", push, (B, 6), required=False), c32)
        return self._rollout_grad(_Host(), B, S, opts, inputs, body, ground)

    def plant_rollout_grad_device(self, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0,
                                  integrator="rk4", substeps=4, move_feet=True, body=None, ground=None, want=None, stream=None):
        """`plant_rollout_grad` on CUDA(HIP) torch tensors of this solver's device (`bmpc_plant_rollout_grad_device`): float32 x_fb
        (B,12), foot (B,6), controls (B,S,h,12), x_cmd (B,12), x_ref (B,h,12), push (B,6), uint8 contact (B,h,2); `body` and `ground`
        of float64 device tensors as for `plant_step_device`.  The outputs -- all of them, or those named in `want` -- are allocated
        here; one launch.  Asynchronous on `stream` (default: torch's current stream) unless the handle's scratch has to grow;
        nothing crosses PCIe.  Returns the dict of output tensors."""
        if x_fb.dim() != 2 or controls.dim() != 4:
            raise ValueError(f"x_fb must have shape (B, 12) and controls (B, S, {self.h}, 12)")
        B, S = x_fb.shape[0], int(controls.shape[1])
        opts = self._rollout_grad_opts(S, push_from, push_steps, integrator, substeps, move_feet, ground, want)
        return self._rollout_grad(_Device(self.device, x_fb.device, stream), B, S, opts,
                                  (x_fb, foot, contact, x_cmd, x_ref, push, controls), body, ground)

    def plant_cost_torch(self, x_fb, foot, contact, controls, x_cmd=None, x_ref=None, push=None, push_from=0, push_steps=0,
                         integrator="rk4", substeps=4, move_feet=True, body=None, ground=None):
        """`plant_rollout_samples`' cost as a differentiable torch value: float64 tensor (B,S) on the device, with gradients to
        `controls` (B,S,h,12) in its dtype and, where they require one, to `x_fb` (B,12) and `foot` (B,6) -- the sums over an
        instance's plans of grad_x0 and grad_foot, each scaled by the incoming gradient.  Every other argument is
        non-differentiable.  The forward is ONE `bmpc_plant_rollout_grad_device` launch on torch's current stream, which leaves the
        gradients behind; the backward scales them -- no second launch, no second derivative (`once_differentiable`).  What is
        held fixed is what `plant_rollout_grad` holds fixed."""
        return _plant_cost_function()(self, x_fb, foot, contact, controls, x_cmd, x_ref, push,
                                      dict(push_from=push_from, push_steps=push_steps, integrator=integrator, substeps=substeps,
                                           move_feet=move_feet, body=body, ground=ground))

    def last_kernel_ms(self):
        ms = C.c_float(-1.0)
        _lib.check(self._lib.bmpc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def synchronize(self):
        _lib.check(self._lib.bmpc_synchronize(self._h))


class SolverStatusWarning(RuntimeWarning):
    """Some instances stopped at the iteration cap (status 1): their controls are the last iterate."""


def _check_status(info, where):
    """The reference never looks at its solver's status (REF:297-300); a drop-in that silently hands a
    non-converged or non-finite iterate to `lowLevelControl` would be worse than that.  Status 2 (NaN/Inf
    iterate: non-finite inputs) is an error, status 1 (iteration cap) a warning.  Callers who want to
    handle it themselves pass `return_info=True`."""
    import warnings
    status = info["status"]
    nbad = int((status == 2).sum())
    if nbad:
        raise FloatingPointError(f"{where}: {nbad} of {status.size} instances produced a NaN/Inf iterate "
                                 f"(status 2; first at index {int(np.flatnonzero(status == 2)[0])})")
    ncap = int((status == 1).sum())
    if ncap:
        warnings.warn(f"{where}: {ncap} of {status.size} instances stopped at the iteration cap "
                      f"(status 1); their controls are the last iterate", SolverStatusWarning, stacklevel=3)


_SOLVERS = {}          # (h, device) -> BatchSolver: ONE handle per horizon and device, whatever the parameters


def _cached_solver(mpc, biped, half, device, solver_options):
    """The drop-in wrappers keep one handle per (horizon, device) and push a changed parameter block
    through `bmpc_set_params`; a control loop that varies `mpc.x_cmd`, `Q`, `mu` ... from step to step
    therefore never creates a second handle (stream + events + staging buffers)."""
    cp = pack_params(mpc, biped, half, solver_options)
    key = (int(cp.h), int(device))
    s = _SOLVERS.get(key)
    if s is None:
        s = BatchSolver(cparams=cp, device=device)
        _SOLVERS[key] = s
    elif params_key(cp) != params_key(s.cparams):
        s.set_params(cp)
    return s


def _mpc_or_default(mpc):
    return mpc if mpc is not None else MPC()


def _solver_and_phase(mpc, biped, half, device, solver_options, t, phase):
    """What every batch wrapper ends its preamble with, AFTER its checks (which need `_mpc_or_default(mpc).h` and must come before
    a solver handle can be created): the cached solver, and the phase from `t` unless it was given."""
    solver = _cached_solver(mpc, biped, half, device, solver_options)
    return solver, phase_indices(t, mpc.dt, mpc.h) if phase is None else phase


def close_cached_solvers():
    """Destroy the handles the drop-in wrappers keep (tests; orderly shutdown)."""
    for s in _SOLVERS.values():
        s.close()
    _SOLVERS.clear()


def _batch_call(controls, t, mpc, biped, half, device, phase, x_ref, foot_ref, act_tol=0.0):
    """What the `*_mpc_batch` wrappers of the evaluation family do before their call: the default `MPC`, `controls` as the
    evaluation takes them, the references from the reference's orientation to the kernel layout, a NaN `act_tol` refused (the
    certificate's; the others leave the default), the cached solver, the phase from `t`.  Every check comes before a solver handle
    can be created.  Returns (solver, phase, x_ref, foot_ref, controls)."""
    mpc = _mpc_or_default(mpc)
    c32 = _controls_f32(controls, int(mpc.h))
    xr, fr = references_to_kernel_layout(x_ref, foot_ref, int(mpc.h))
    _act_tol(act_tol)
    return _solver_and_phase(mpc, biped, half, device, None, t, phase) + (xr, fr, c32)


def _contact_rows(contact, h):
    """`contact` of a single-instance call as an array with at least h rows of 2 (ValueError otherwise)."""
    contact = np.asarray(contact)
    if contact.ndim != 2 or contact.shape[1] != 2 or contact.shape[0] < h:
        raise ValueError(f"contact must have at least {h} rows of 2 (REF:239-249 indexes contact[k] for k < h)")
    return contact


def _batch_of_one(x_fb, t, foot, mpc, contact, controls, x_ref, foot_ref):
    """One instance with `solve_mpc`'s arguments and `controls` (h,12) as a batch of one: the positional arguments of the
    `*_mpc_batch` wrappers of the evaluation family and their reference keywords.  Shapes are checked here (ValueError)."""
    h = int(mpc.h)
    c = np.asarray(controls)
    if c.shape != (h, 12):
        raise ValueError(f"controls must have shape ({h}, 12), got {c.shape}")
    contact = _contact_rows(contact, h)
    args = (np.asarray(x_fb, float).reshape(1, 12), [t], np.asarray(foot, float).reshape(1, 6), contact[None, :h, :], c[None])
    refs = dict(x_ref=None if x_ref is None else np.asarray(x_ref)[None], foot_ref=None if foot_ref is None else np.asarray(foot_ref)[None])
    return args, refs


def solve_mpc_batch(x_fb, t, foot, contact, mpc=None, biped=None, x_cmd=None, mu=None, phase=None, half=None,
                    device=0, solver_options=None, return_info=False, x_ref=None, foot_ref=None):
    """B instances of REF:187 `solve_mpc`.  x_fb (B,12), t (B,) seconds [or phase (B,) directly],
    foot (B,6), contact (B,h,2); optional per-instance x_cmd (B,12) and mu (B,h,2).
    Optional references to track instead of the generated ones, in the reference's orientation: x_ref (B,13,h) (or (B,12,h)) and
    foot_ref (B,6,h) -- what `reference_trajectories_batch` returns, so "generate, edit, pass back" works.
    Returns states (B,h,13), controls (B,h,12) [, info].  Without `return_info` a NaN/Inf instance raises
    FloatingPointError and instances stopped at the iteration cap raise a SolverStatusWarning."""
    mpc = _mpc_or_default(mpc)
    xr, fr = references_to_kernel_layout(x_ref, foot_ref, int(mpc.h))
    solver, phase = _solver_and_phase(mpc, biped, half, device, solver_options, t, phase)
    states, controls, info = solver.solve(x_fb, foot, contact, phase, x_cmd=x_cmd, mu=mu, x_ref=xr, foot_ref=fr)
    if return_info:
        return states, controls, info
    _check_status(info, "solve_mpc")
    return states, controls


def solve_mpc(x_fb, t, foot, mpc, biped, contact, half=None, device=0, solver_options=None, x_ref=None, foot_ref=None):
    """Drop-in for REF:187-304: same arguments, same return shapes and dtypes (fp64 `states (h,13)`,
    `controls (h,12)`), inputs not mutated, silent.  `x_ref` (13,h) / `foot_ref` (6,h): what the solve tracks in place of
    REF:61-70 / REF:72-109 -- e.g. `get_reference_trajectory(...)` edited (stairs, a crouch, a planner's footholds)."""
    h = int(mpc.h)
    contact = _contact_rows(contact, h)
    x_fb = np.asarray(x_fb, float).reshape(12)
    foot = np.asarray(foot, float).reshape(6)
    states, controls = solve_mpc_batch(x_fb[None], [t], foot[None], contact[None, :h, :], mpc=mpc, biped=biped,
                                       half=half, device=device, solver_options=solver_options,
                                       x_ref=None if x_ref is None else np.asarray(x_ref)[None],
                                       foot_ref=None if foot_ref is None else np.asarray(foot_ref)[None])
    return states[0], controls[0]


def evaluate_mpc_batch(x_fb, t, foot, contact, controls, mpc=None, biped=None, x_cmd=None, mu=None, phase=None, half=None,
                       device=0, x_ref=None, foot_ref=None):
    """What the model of REF:187-304 makes of given control sequences: `solve_mpc_batch`'s call surface (references in the
    reference's orientation, the cached handle per horizon and device) with `controls` (B,h,12) added.  Returns
    dict(cost (B,), objective (B,), violation (B,4), states (B,h,13)) as `BatchSolver.evaluate`."""
    solver, phase, xr, fr, c32 = _batch_call(controls, t, mpc, biped, half, device, phase, x_ref, foot_ref)
    return solver.evaluate(x_fb, foot, contact, phase, c32, x_cmd=x_cmd, mu=mu, x_ref=xr, foot_ref=fr, want_states=True)


def evaluate_mpc(x_fb, t, foot, mpc, biped, contact, controls, half=None, device=0, x_ref=None, foot_ref=None):
    """`evaluate_mpc_batch` for one instance with `solve_mpc`'s arguments and `controls` (h,12) -- e.g. what `solve_mpc` returned.
    Returns dict(cost float, objective float, violation (4,), states (h,13))."""
    args, refs = _batch_of_one(x_fb, t, foot, mpc, contact, controls, x_ref, foot_ref)
    r = evaluate_mpc_batch(*args, mpc=mpc, biped=biped, half=half, device=device, **refs)
    return dict(cost=float(r["cost"][0]), objective=float(r["objective"][0]), violation=r["violation"][0], states=r["states"][0])


def evaluate_samples_mpc_batch(x_fb, t, foot, contact, controls, mpc=None, biped=None, x_cmd=None, mu=None, phase=None, half=None,
                               device=0, x_ref=None, foot_ref=None, w_viol=(0, 0, 0, 0), temperature=float("inf")):
    """S candidate plans per instance scored, ranked and blended: `evaluate_mpc_batch`'s call surface (references in the reference's
    orientation, the cached handle per horizon and device) with `controls` (B,S,h,12), the prices `w_viol` of the four violation
    classes and the `temperature` of the softmin weights.  Returns the dict of `BatchSolver.evaluate_samples`.  Every check comes
    before a solver handle can be created."""
    mpc = _mpc_or_default(mpc)
    c32 = _samples_f32(controls, int(mpc.h))
    _samples_desc(c32.shape[1], w_viol, temperature)
    xr, fr = references_to_kernel_layout(x_ref, foot_ref, int(mpc.h))
    solver, phase = _solver_and_phase(mpc, biped, half, device, None, t, phase)
    return solver.evaluate_samples(x_fb, foot, contact, phase, c32, x_cmd=x_cmd, mu=mu, x_ref=xr, foot_ref=fr, w_viol=w_viol,
                                   temperature=temperature)


def evaluate_grad_mpc_batch(x_fb, t, foot, contact, controls, mpc=None, biped=None, x_cmd=None, mu=None, phase=None, half=None,
                            device=0, x_ref=None, foot_ref=None):
    """Gradient of the cost `evaluate_mpc_batch` returns: the same call surface (references in the reference's orientation, the
    cached handle per horizon and device).  Returns dict(cost (B,), grad_u (B,h,12), grad_x0 (B,12)) as `BatchSolver.evaluate_grad`."""
    solver, phase, xr, fr, c32 = _batch_call(controls, t, mpc, biped, half, device, phase, x_ref, foot_ref)
    return solver.evaluate_grad(x_fb, foot, contact, phase, c32, x_cmd=x_cmd, mu=mu, x_ref=xr, foot_ref=fr)


def evaluate_grad_mpc(x_fb, t, foot, mpc, biped, contact, controls, half=None, device=0, x_ref=None, foot_ref=None):
    """`evaluate_grad_mpc_batch` for one instance with `evaluate_mpc`'s arguments.  Returns dict(cost float, grad_u (h,12),
    grad_x0 (12,))."""
    args, refs = _batch_of_one(x_fb, t, foot, mpc, contact, controls, x_ref, foot_ref)
    r = evaluate_grad_mpc_batch(*args, mpc=mpc, biped=biped, half=half, device=device, **refs)
    return dict(cost=float(r["cost"][0]), grad_u=r["grad_u"][0], grad_x0=r["grad_x0"][0])


def certify_mpc_batch(x_fb, t, foot, contact, controls, mpc=None, biped=None, x_cmd=None, mu=None, phase=None, half=None,
                      device=0, x_ref=None, foot_ref=None, act_tol=ACT_TOL):
    """KKT certificate of given control sequences: `evaluate_grad_mpc_batch`'s call surface (references in the reference's
    orientation, the cached handle per horizon and device) plus `act_tol`.  Returns the dict of `BatchSolver.certify`."""
    solver, phase, xr, fr, c32 = _batch_call(controls, t, mpc, biped, half, device, phase, x_ref, foot_ref, act_tol)
    return solver.certify(x_fb, foot, contact, phase, c32, x_cmd=x_cmd, mu=mu, x_ref=xr, foot_ref=fr, act_tol=act_tol)


def certify_mpc(x_fb, t, foot, mpc, biped, contact, controls, half=None, device=0, x_ref=None, foot_ref=None, act_tol=ACT_TOL):
    """`certify_mpc_batch` for one instance with `evaluate_mpc`'s arguments -- e.g. on what `solve_mpc` returned.  Returns
    dict(lam (h,36), resid (h,12), summary (4,), stationarity, primal_ineq, complementarity, grad_scale floats, n_active, status ints)."""
    args, refs = _batch_of_one(x_fb, t, foot, mpc, contact, controls, x_ref, foot_ref)
    r = certify_mpc_batch(*args, mpc=mpc, biped=biped, half=half, device=device, **refs, act_tol=act_tol)
    out = dict(lam=r["lam"][0], resid=r["resid"][0], summary=r["summary"][0], n_active=int(r["n_active"][0]), status=int(r["status"][0]))
    for k in ("stationarity", "primal_ineq", "complementarity", "grad_scale"):
        out[k] = float(r[k][0])
    return out


def reference_trajectories_batch(x_fb, t, foot, contact, mpc=None, biped=None, x_cmd=None, phase=None, half=None, device=0):
    """Batched REF:61-109 on the device (the generators phase 1 of the solve kernel runs, exposed through
    `bmpc_debug_assemble`): x_ref (B,13,h) and foot_ref (B,6,h), fp64, in the reference's row/column order."""
    mpc = _mpc_or_default(mpc)
    solver, phase = _solver_and_phase(mpc, biped, half, device, None, t, phase)
    x_fb = np.asarray(x_fb, float).reshape(-1, 12)
    x_ref, foot_ref, _, _ = solver.assemble(x_fb, foot, contact, phase, x_cmd=x_cmd, want_matrices=False)
    B, h = x_ref.shape[0], x_ref.shape[1]
    xr = np.concatenate([x_ref.transpose(0, 2, 1), np.ones((B, 1, h))], axis=1)       # REF:62: 13th row of ones
    return xr, foot_ref.transpose(0, 2, 1)


def get_reference_trajectory(x_fb, mpc, device=0):
    """Drop-in for REF:61-70: returns x_ref (13,h) fp64."""
    h = int(mpc.h)
    xr, _ = reference_trajectories_batch(np.asarray(x_fb, float).reshape(1, 12), [0.0], np.zeros((1, 6)),
                                         np.ones((1, h, 2), np.uint8), mpc=mpc, device=device)
    return xr[0]


def get_reference_foot_trajectory(x_fb, t, foot, mpc, contact, half=None, device=0):
    """Drop-in for REF:72-109: returns foot_ref (6,h) fp64 (`contact` as REF:102 reads it: its first row decides)."""
    h = int(mpc.h)
    contact = np.asarray(contact)
    # REF:102 reads contact[0, :] only, and REF:58 hands over ten rows whatever mpc.h is: row 0 is repeated h times
    c = np.broadcast_to(contact.reshape(-1, 2)[0:1], (h, 2))
    _, fr = reference_trajectories_batch(np.asarray(x_fb, float).reshape(1, 12), [float(t)], np.asarray(foot, float).reshape(1, 6),
                                         c[None], mpc=mpc, half=half, device=device)
    return fr[0]


def getFootPositionWorld(x_fb, q, biped, mpc=None, device=0):
    """Drop-in for REF:406-424: returns pf_w (6,1) fp64 like the reference."""
    solver = _cached_solver(_mpc_or_default(mpc), biped, None, device, None)
    return solver.foot_position_world(np.asarray(x_fb, float).reshape(1, 12), np.asarray(q, float).reshape(1, 10)).reshape(6, 1)


def lowLevelControl(x_fb, t, pf_w, q, qd, mpc, biped, contact, u, device=0):
    """Drop-in for REF:444-470: same arguments (u is the (12,1) column REF:493 builds), returns tau (10,1) fp64."""
    solver = _cached_solver(mpc, biped, None, device, None)
    contact = np.asarray(contact)
    tau = solver.low_level_control(np.asarray(x_fb, float).reshape(1, 12), [float(t)], np.asarray(pf_w, float).reshape(1, 6),
                                   np.asarray(q, float).reshape(1, 10), np.asarray(qd, float).reshape(1, 10),
                                   contact[0, 0:2].reshape(1, 2), np.asarray(u, float).reshape(1, 12))
    return tau.reshape(10, 1)
