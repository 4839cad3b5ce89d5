"""Compile-time resources of the plant's ground kernels (csrc/bmpc_plant.hip), read from the gfx950 ISA and code object metadata like
tests/test_plant_body_resources.py (no GPU needed): no scratch, no vector or scalar spill, fp64 arithmetic, no LDS, and the register
bound of the occupancy step of the body kernels they derive from -- three waves per SIMD, at most 168 registers.  The ground is
done before the stages begin and leaves twelve fp32 values where the command was, so it is not expected to cost a wave.

Figures as built: plant_step_ground_kernel 166 VGPRs, simulate_ground_feedback_kernel 168 VGPRs, 0 AGPRs, no spill of either
kind, private segment 0, no LDS (docs/history_r18.md; the feedback kernel holds every scalar register there is, which is why the
reductions over the periods are ground_reduce_kernel's)."""
import os
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
KERNELS = ("_ZN4bmpc24plant_step_ground_kernelE", "_ZN4bmpc31simulate_ground_feedback_kernelE")
EXISTING = ("_ZN4bmpc17plant_step_kernelE", "_ZN4bmpc24simulate_feedback_kernelE", "_ZN4bmpc22plant_step_body_kernelE",
            "_ZN4bmpc29simulate_body_feedback_kernelE")
REGISTERS = 168                        # three waves per SIMD


@needs_hipcc
@pytest.mark.parametrize("name", KERNELS)
def test_ground_kernels_have_no_scratch_no_spill_no_lds(name):
    body, meta = isa.kernel(isa.compile_isa("bmpc_plant.hip"), name)
    print(name, meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") or x.startswith("ds_") or x.startswith("s_barrier") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64


@needs_hipcc
@pytest.mark.parametrize("name", KERNELS)
def test_ground_kernels_fit_three_waves_per_simd(name):
    _, meta = isa.kernel(isa.compile_isa("bmpc_plant.hip"), name)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    print(name, "registers", regs)
    assert regs <= REGISTERS, meta


@needs_hipcc
def test_the_reduction_kernel_is_small_and_clean():
    body, meta = isa.kernel(isa.compile_isa("bmpc_plant.hip"), "_ZN4bmpc20ground_reduce_kernelE")
    print(meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] == 0 and meta["vgpr_count"] + meta["agpr_count"] <= 64, meta
    assert not any(x.startswith("scratch_") or x.startswith("ds_") for x in body)


@needs_hipcc
@pytest.mark.parametrize("name", EXISTING)
def test_the_existing_kernels_are_still_there_under_their_names(name):
    """One match each (isa.kernel asserts it): the ground kernels' names do not start with theirs."""
    body, _ = isa.kernel(isa.compile_isa("bmpc_plant.hip"), name)
    assert len(body) > 100
