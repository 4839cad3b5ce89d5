"""Compile-time resources of the plant's kernels (csrc/bmpc_plant.hip), read from the gfx950 ISA and code object metadata like
tests/test_evaluate_resources.py (no GPU needed): no scratch, no vector or scalar spill, fp64 arithmetic, no LDS, and the register
bound of at most 128 VGPRs.

Figures as built: plant_step_kernel 126 VGPRs, simulate_feedback_kernel 128 VGPRs, 0 AGPRs, no spill of either kind, private
segment 0, no LDS (docs/history_r15.md has the road there)."""
import os
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
KERNELS = ("_ZN4bmpc17plant_step_kernelE", "_ZN4bmpc24simulate_feedback_kernelE")


@needs_hipcc
@pytest.mark.parametrize("name", KERNELS)
def test_plant_kernels_have_no_scratch_no_spill_no_lds(name):
    body, meta = isa.kernel(isa.compile_isa("bmpc_plant.hip"), name)
    print(name, meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") or x.startswith("ds_") or x.startswith("s_barrier") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64


@needs_hipcc
@pytest.mark.parametrize("name", KERNELS)
def test_plant_kernels_fit_128_registers(name):
    _, meta = isa.kernel(isa.compile_isa("bmpc_plant.hip"), name)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print(name, "registers", regs)
    assert regs <= 128, meta
