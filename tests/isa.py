"""The gfx950 ISA and code object metadata of the kernel sources, for the resource tests (no GPU needed): compiled with the library's
flags, once per process and source; read with the parsers of tools/isa_diff.py."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_diff import functions, metadata  # noqa: E402

_TEXT = {}


def compile_isa(source):
    """The device-only assembly listing of csrc/<source> (self-contained kernel files compile on their own in seconds;
    bmpc_capi.hip is every kernel of the library)."""
    if source not in _TEXT:
        import __graft_entry__ as ge
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, os.path.splitext(source)[0] + ".s")
            subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                                   "-S", "-x", "hip", os.path.join(ge.CSRC, source), "-o", out] + ge.KERNEL_FLAGS,
                                  cwd=ge.CSRC, stderr=subprocess.DEVNULL)
            _TEXT[source] = open(out).read()
    return _TEXT[source]


def kernel(text, mangled_prefix):
    """(body, meta) of the one kernel whose mangled name starts with `mangled_prefix`: its instruction lines and block labels (.LBBn_m, no other label) as the
    listing has them, comments and directives dropped, and the integer fields of its code object metadata."""
    body = [v for k, v in functions(text, normalise=False).items() if k.startswith(mangled_prefix)]
    meta = [v for k, v in metadata(text).items() if k.startswith(mangled_prefix)]
    assert len(body) == 1 and len(meta) == 1, (mangled_prefix, len(body), len(meta))
    return [x for x in body[0] if not x.startswith(".") or re.match(r"\.LBB\d+_\d+:", x)], meta[0]
