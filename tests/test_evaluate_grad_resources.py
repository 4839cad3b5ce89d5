"""Compile-time resources of the cost-gradient kernel (csrc/bmpc_evaluate_grad.hip), read from the gfx950 ISA and code object metadata
as tests/test_evaluate_resources.py reads the evaluation kernel's (no GPU needed): no scratch, no vector spill, fp64 arithmetic,
wave-wide permutes, no LDS and no barrier.  The file is compiled on its own with the library's flags; docs/history_r10.md quotes the
register counts and occupancy printed here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = r"_ZN4bmpc20evaluate_grad_kernelE"


@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("isa") / "bmpc_evaluate_grad.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                           "-S", "-x", "hip", os.path.join(ge.CSRC, "bmpc_evaluate_grad.hip"), "-o", out] + ge.KERNEL_FLAGS,
                          cwd=ge.CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(text):
    lines = text.splitlines()
    i = next(k for k, ln in enumerate(lines) if re.match(NAME + r"\S*:", ln))
    end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    body = [x.split(";")[0].strip() for x in lines[i + 1:end]]
    body = [x for x in body if x and (not x.startswith(".") or re.match(r"\.LBB\d+_\d+:", x))]
    meta = None
    for entry in re.split(r"\n\s+- (?=\.agpr_count:)", text)[1:]:
        if re.search(r"\.name:\s+" + NAME, entry):
            meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", entry.split(".wavefront_size")[0]) if k not in ("offset", "size")}
    assert meta is not None
    return body, meta


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not available")
def test_gradient_kernel_has_no_scratch_no_lds_and_is_fp64(isa_text):
    body, meta = _kernel(isa_text)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print("evaluate_grad_kernel:", meta, "waves per SIMD by registers:", 512 // max(regs, 1))
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64
    assert any(x.startswith("ds_bpermute_b32") for x in body)                 # the cross-lane traffic: wave-wide permutes
    assert meta["group_segment_fixed_size"] == 0                              # no LDS ...
    assert not any(x.startswith("s_barrier") for x in body)                   # ... and no barrier
