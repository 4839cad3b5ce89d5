"""A stand-in for libbmpc.so that holds the Python binding to what it hands the library (tests/test_api_calls_cpu.py,
tests/test_gpu_api_calls.py).  A solver made without a handle gets a `RecordingLib` as its `_lib`; every entry the binding calls is
compared, argument by argument, with the next row of a table the test wrote by hand, and returns 0.  A row is (entry name, [one
descriptor per argument]); a descriptor is

    HANDLE                 the solver's handle
    an int or a float      a scalar passed by value (B, steps, act_tol, the stream), or the value of a scalar struct member
    a list                 the value of an array struct member (CGait.offset, CSamples.w_viol)
    None                   a NULL pointer
    In(value, dtype)       a host pointer with np.ascontiguousarray(value, dtype).tobytes() behind it
    At(address)            exactly this address (a tensor's data_ptr())
    Out(key, dtype, shape) an output pointer: on the host it is filled with a byte of its own, and `check_outputs` then wants the
                           result under `key` to have that dtype and shape, to carry the bytes and to live at the address handed over
                           (`returned`: the dtype the method converts the result to; then only the values are compared); on the
                           device nothing is written and the result must be a tensor of that dtype and shape at that address
    St(cls, **members)     a `C.byref` of a `cls` whose members are as described; members not named are NULL / 0
"""
import ctypes as C

import numpy as np

HANDLE = object()
H, B, S, STEPS = 10, 3, 4, 2

# the outputs of the plan roll-out (`bmpc_rollout_out`): dtype, leading dimensions ("B" or "BS" for (B, S)), trailing dimensions
ROLLOUT = dict(cost=(np.float64, "BS"), score=(np.float64, "BS"), x_end=(np.float32, "BS", 12), foot_end=(np.float32, "BS", 6),
               x_traj=(np.float32, "BS", H, 12), first_fall=(np.int32, "BS"), max_tilt=(np.float32, "BS"), min_z=(np.float32, "BS"),
               first_slip=(np.int32, "BS"), slip_periods=(np.int32, "BS", 2), unloaded_periods=(np.int32, "BS", 2),
               mu_demand=(np.float32, "BS"), best=(np.int32, "B"), n_valid=(np.int32, "B"), weights=(np.float64, "BS"),
               u_mean=(np.float64, "B", H, 12), ess=(np.float64, "B"))
GROUND_ONLY = ("first_slip", "slip_periods", "unloaded_periods", "mu_demand")


class In:
    def __init__(self, value, dtype):
        self.bytes = np.ascontiguousarray(value, dtype).tobytes()


class At:
    def __init__(self, address):
        self.address = address


class Out:
    def __init__(self, key, dtype, shape, returned=None):
        self.key, self.dtype, self.shape, self.returned = key, dtype, tuple(shape), returned


class St:
    def __init__(self, cls, **members):
        self.cls, self.members = cls, members


class RecordingLib:
    """Checks each call against `rows` as it comes; `fill`: write into host outputs (a device test has no host memory to fill)."""

    def __init__(self, rows, fill=True):
        self.rows, self.fill, self.outs = list(rows), fill, []

    def __getattr__(self, name):
        if not name.startswith("bmpc_"):
            raise AttributeError(name)

        def entry(*args):
            assert self.rows, f"unexpected call of {name}"
            want_name, want = self.rows.pop(0)
            assert name == want_name
            assert len(args) == len(want), f"{name}: {len(args)} arguments, not {len(want)}"
            for i, (w, a) in enumerate(zip(want, args)):
                self._arg(f"{name}[{i}]", w, a)
            return 0
        return entry

    def _arg(self, where, w, a):
        if w is HANDLE:
            assert isinstance(a, C.c_void_p) and a.value == 1, where
        elif w is None:
            assert a is None, f"{where} must be NULL"
        elif isinstance(w, In):
            assert isinstance(a, int) and a != 0, f"{where} must be a pointer"
            assert C.string_at(a, len(w.bytes)) == w.bytes, f"{where}: other bytes than the caller's"
        elif isinstance(w, At):
            assert a == w.address, f"{where}: another address than the tensor's"
        elif isinstance(w, Out):
            assert isinstance(a, int) and a != 0, f"{where} must be a pointer"
            byte = 0x21 + len(self.outs)                 # (0x21 .. 0x3f repeated: a finite float in either width, a small integer)
            if self.fill:
                C.memset(a, byte, int(np.prod(w.shape)) * np.dtype(w.dtype).itemsize)
            self.outs.append((w, a, byte))
        elif isinstance(w, St):
            assert type(a) is type(C.byref(C.c_int())) and type(a._obj) is w.cls, f"{where} must be a byref of {w.cls.__name__}"
            for member, _ in w.cls._fields_:
                v = getattr(a._obj, member)
                if member in w.members:
                    self._arg(f"{where}.{member}", w.members[member], v)
                else:
                    assert v is None or v == 0 or (isinstance(v, C.Array) and not any(v)), f"{where}.{member} must be NULL / 0"
        elif isinstance(w, list):
            assert list(a) == w, f"{where}: {list(a)} != {w}"
        else:
            assert type(a) is type(w) and a == w, f"{where}: {a!r} != {w!r}"

    def check_outputs(self, result):
        """After the method returned `result` (a dict): every row was used, and every output handed over is in the result."""
        assert not self.rows, f"calls that did not come: {[r[0] for r in self.rows]}"
        handed = set()
        for w, a, byte in self.outs:
            r = result[w.key]
            handed.add(w.key)
            if not self.fill:
                assert r.dtype == w.dtype and tuple(r.shape) == w.shape and r.data_ptr() == a, w.key
                continue
            assert isinstance(r, np.ndarray) and r.dtype == (w.returned or w.dtype) and r.shape == w.shape, w.key
            pattern = np.frombuffer(bytes([byte]) * (r.size * np.dtype(w.dtype).itemsize), w.dtype).reshape(w.shape)
            assert np.array_equal(r, pattern.astype(r.dtype)), w.key
            if w.returned is None and r.size:
                assert r.__array_interface__["data"][0] == a, w.key
        assert {k for k, v in result.items() if v is not None} == handed
        return result


def solver(rows, fill=True):
    """A `BatchSolver` without a handle whose library is a `RecordingLib` expecting `rows`."""
    import biped_mpc_py_amd as bm
    from biped_mpc_py_amd import _lib
    s = object.__new__(bm.BatchSolver)
    s.h, s.device, s._h, s.cparams = H, 0, C.c_void_p(1), _lib.CParams(h=H, half=5)
    s._lib = RecordingLib(rows, fill)
    return s
