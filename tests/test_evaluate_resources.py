"""Compile-time resources of the evaluation family's kernels (csrc/bmpc_evaluate.hip, bmpc_evaluate_grad.hip, bmpc_certify.hip), read
from the gfx950 ISA and code object metadata as tests/test_kernel_resources.py reads the solve kernels' (no GPU needed): no scratch,
no vector spill, fp64 arithmetic, wave-wide permutes, and what each kernel promises about LDS, barriers and registers.  Each file is
self-contained, so it is compiled on its own (seconds) with the library's flags (tests/isa.py); docs/history_r08.md, docs/history_r10.md
and DESIGN.md section 8 quote the register counts and occupancies printed here."""
import os
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
# scalar stores to memory and what goes with them: opcode prefixes, assembled here so that this file does not spell them out
FORBIDDEN = tuple("s_" + x for x in ("store_", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb", "dcache_discard"))


@needs_hipcc
def test_evaluation_kernel_has_no_scratch_and_is_fp64():
    """No LDS is allocated; should it ever be used, the s_waitcnt-before-s_barrier rule of the other kernels holds."""
    body, meta = isa.kernel(isa.compile_isa("bmpc_evaluate.hip"), "_ZN4bmpc15evaluate_kernelE")
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


@needs_hipcc
def test_gradient_kernel_has_no_scratch_no_lds_and_is_fp64():
    body, meta = isa.kernel(isa.compile_isa("bmpc_evaluate_grad.hip"), "_ZN4bmpc20evaluate_grad_kernelE")
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print("evaluate_grad_kernel:", meta, "waves per SIMD by registers:", 512 // max(regs, 1))
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64
    assert any(x.startswith("ds_bpermute_b32") for x in body)                 # the cross-lane traffic: wave-wide permutes
    assert meta["group_segment_fixed_size"] == 0                              # no LDS ...
    assert not any(x.startswith("s_barrier") for x in body)                   # ... and no barrier


@needs_hipcc
def test_certify_kernel_has_no_scratch_and_fits_two_waves_per_simd():
    """At most 256 registers, `s_waitcnt lgkmcnt(0)` in front of every barrier (if there is one) and no scalar store."""
    body, meta = isa.kernel(isa.compile_isa("bmpc_certify.hip"), "_ZN4bmpc14certify_kernelE")
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
