"""Compile-time resources of the sampling kernels (csrc/bmpc_evaluate_samples.hip), read from the gfx950 ISA and code object metadata
as tests/test_evaluate_resources.py reads the evaluation family's (no GPU needed).  evaluate_samples_kernel: no scratch, no vector
spill, two waves per SIMD by registers, fp64 arithmetic, wave-wide permutes, no LDS, no barrier, and every fp64 sincos ahead of the
sample loop -- the set-up really is paid once per group.  sample_reduce_kernel: no scratch, no spill, every barrier behind an
`s_waitcnt lgkmcnt(0)`.  docs/history_r20.md quotes the register counts and occupancies printed here."""
import os
import re
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
# the large-argument reduction of an fp64 sincos is inlined at every call site with this many v_trig_preop_f64 (the six call
# sites of evaluate_kernel hold 18, the three of evaluate_grad_kernel 9)
TRIG_PREOP_PER_SINCOS = 3


def _back_edges(body):
    """(index of the label, index of the branch) of every branch of `body` to a label above it."""
    at = {x[:-1]: k for k, x in enumerate(body) if x.endswith(":")}
    out = []
    for k, x in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", x)
        if m and at.get(m.group(1), k) < k:
            out.append((at[m.group(1)], k))
    return out


@needs_hipcc
def test_sampling_kernel_resources_and_set_up_outside_the_loop():
    body, meta = isa.kernel(isa.compile_isa("bmpc_evaluate_samples.hip"), "_ZN4bmpc23evaluate_samples_kernelE")
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print("evaluate_samples_kernel:", meta, "waves per SIMD by registers:", 512 // max(regs, 1))
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert regs <= 256, meta                                                  # two waves per SIMD
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64
    assert any(x.startswith("ds_bpermute_b32") for x in body)                 # the cross-lane traffic: wave-wide permutes
    assert meta["group_segment_fixed_size"] == 0                              # no LDS ...
    assert not any(x.startswith("s_barrier") for x in body)                   # ... and no barrier
    # the sample loop: the widest back-edge (the prefix and butterfly loops lie inside it); it holds the prefetch, the
    # cross-lane traffic and the stores
    top, end = max(_back_edges(body), key=lambda e: e[1] - e[0])
    inside = body[top:end]
    assert all(any(x.startswith(op) for x in inside) for op in ("global_load_dword", "ds_bpermute_b32", "v_fma_f64", "global_store_dwordx2"))
    trig = [k for k, x in enumerate(body) if x.startswith("v_trig_preop_f64")]
    print("fp64 sincos call sites:", len(trig) // TRIG_PREOP_PER_SINCOS, "sample loop from instruction", top, "of", len(body))
    assert len(trig) == 6 * TRIG_PREOP_PER_SINCOS                             # three of the reference attitude, three of x_fb
    assert max(trig) < top                                                    # all of them before the sample loop


@needs_hipcc
def test_reduction_kernel_has_no_scratch_and_guards_its_barriers():
    body, meta = isa.kernel(isa.compile_isa("bmpc_evaluate_samples.hip"), "_ZN4bmpc20sample_reduce_kernelE")
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print("sample_reduce_kernel:", meta, "waves per SIMD by registers:", min(8, 512 // max(regs, 1)))
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") for x in body)
    assert any(x.startswith("s_barrier") for x in body) and any(x.startswith("v_exp_f64") or x.startswith("v_ldexp_f64") for x in body)
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
