"""ctypes driver of tests/emu/bmpc_emu_staging.cpp (TEST INFRASTRUCTURE): the library's `stage_layout`
(csrc/bmpc_host_staging.hpp) compiled by host clang from the same header, in a small shared library of its own, built on first use
with the flags of `emu.build`."""
import ctypes as C
import os
import subprocess

from tests.emu import emu

SO = os.path.join(emu.HERE, "libbmpc_emu_staging.so")


def build(force=False):
    srcs = [os.path.join(emu.HERE, "bmpc_emu_staging.cpp"), os.path.join(emu.ROOT, "biped_mpc_py_amd", "csrc", "bmpc_host_staging.hpp")]
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call([emu.CLANG, "-std=c++20", "-O1", "-fPIC", "-shared", "-x", "c++", srcs[0], "-o", SO])
    return SO


def stage_layout(rows):
    """`stage_layout` on `rows` of (present, bytes): ([byte offset of each row, None where it reports the row absent], the bytes of
    the block)."""
    lib = C.CDLL(build())
    n = len(rows)
    present = (C.c_uint8 * n)(*[1 if p else 0 for p, _ in rows])
    size = (C.c_uint64 * n)(*[int(b) for _, b in rows])
    off = (C.c_uint64 * n)()
    lib.bmpc_emu_stage_layout.restype = C.c_uint64
    total = lib.bmpc_emu_stage_layout(present, size, n, off)
    return [None if o == 2 ** 64 - 1 else int(o) for o in off], int(total)
