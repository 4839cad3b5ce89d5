"""Compile-time resources of the evaluation kernel (csrc/bmpc_evaluate.hip), read from the gfx950 ISA and code object metadata as
tests/test_kernel_resources.py reads the solve kernels' (no GPU needed): no scratch, no vector spill, fp64 arithmetic, and -- should
it ever use LDS -- the s_waitcnt-before-s_barrier rule of the other kernels.  The file is self-contained, so it is compiled on its
own (seconds) with the library's flags; docs/history_r08.md quotes the register count and occupancy printed here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("isa") / "bmpc_evaluate.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                           "-S", "-x", "hip", os.path.join(ge.CSRC, "bmpc_evaluate.hip"), "-o", out] + ge.KERNEL_FLAGS,
                          cwd=ge.CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(text):
    lines = text.splitlines()
    i = next(k for k, ln in enumerate(lines) if re.match(r"_ZN4bmpc15evaluate_kernelE\S*:", ln))
    end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    body = [x.split(";")[0].strip() for x in lines[i + 1:end]]
    body = [x for x in body if x and (not x.startswith(".") or re.match(r"\.LBB\d+_\d+:", x))]
    meta = None
    for entry in re.split(r"\n\s+- (?=\.agpr_count:)", text)[1:]:
        if re.search(r"\.name:\s+_ZN4bmpc15evaluate_kernelE", entry):
            meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", entry.split(".wavefront_size")[0]) if k not in ("offset", "size")}
    assert meta is not None
    return body, meta


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not available")
def test_evaluation_kernel_has_no_scratch_and_is_fp64(isa_text):
    body, meta = _kernel(isa_text)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print("evaluate_kernel:", meta, "waves per SIMD by registers:", 512 // max(regs, 1))
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64
    assert any(x.startswith("ds_bpermute_b32") for x in body)                 # the cross-lane traffic: wave-wide permutes
    # LDS: none is allocated; if that ever changes, every s_barrier must come behind an s_waitcnt lgkmcnt(0)
    if meta["group_segment_fixed_size"] == 0:
        assert not any(x.startswith("s_barrier") for x in body)
    for k, x in enumerate(body):
        if not x.startswith("s_barrier"):
            continue
        j = k - 1
        while True:
            assert j >= 0, "barrier at the top of the kernel"
            y = body[j]
            if y.startswith("s_waitcnt") and "lgkmcnt(0)" in y:
                break
            assert not (y.startswith("ds_") or y.startswith(".LBB") or y.startswith("s_cbranch") or y.startswith("s_branch")), \
                ("s_barrier reachable without lgkmcnt(0)", body[max(0, j - 3):k + 1])
            j -= 1
