"""Compile-time resources of the certificate kernel (csrc/bmpc_certify.hip), read from the gfx950 ISA and code object metadata as
tests/test_evaluate_grad_resources.py reads the gradient kernel's (no GPU needed): no scratch, at most 256 registers, fp64
arithmetic, wave-wide permutes, `s_waitcnt lgkmcnt(0)` in front of every barrier (if there is one) and no scalar store.  The file is
compiled on its own with the library's flags; DESIGN.md section 8 quotes the register count and occupancy printed here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = r"_ZN4bmpc14certify_kernelE"
# scalar stores to memory and what goes with them: opcode prefixes, assembled here so that this file does not spell them out
FORBIDDEN = tuple("s_" + x for x in ("store_", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb", "dcache_discard"))


@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("isa") / "bmpc_certify.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                           "-S", "-x", "hip", os.path.join(ge.CSRC, "bmpc_certify.hip"), "-o", out] + ge.KERNEL_FLAGS,
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
def test_certify_kernel_has_no_scratch_and_fits_two_waves_per_simd(isa_text):
    body, meta = _kernel(isa_text)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    lds = meta["group_segment_fixed_size"]
    print("certify_kernel:", meta, "waves per SIMD by registers:", 512 // max(regs, 1), "workgroups per CU by LDS:", 163840 // max(lds, 1))
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert regs <= 256, meta                                                  # accumulation registers included: two waves per SIMD
    assert 2 * lds <= 163840, meta                                            # ... and two workgroups per CU (160 KB of LDS)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64
    assert any(x.startswith("ds_bpermute_b32") for x in body)                 # the cross-lane traffic: wave-wide permutes
    for k, x in enumerate(body):                                              # no barrier is expected; if one appears, it is guarded
        if x.startswith("s_barrier"):
            assert body[k - 1].startswith("s_waitcnt") and "lgkmcnt(0)" in body[k - 1], (k, body[k - 1])
    assert not any(x.startswith(FORBIDDEN) for x in body)
