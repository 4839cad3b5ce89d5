"""Compile-time resources of plant_rollout_grad_kernel (csrc/bmpc_plant_rollout_grad.hip), read from the code object metadata of the
gfx950 build like tests/test_plant_rollout_resources.py (no GPU needed): no private segment, no vector register spilt, and at most the
512 registers a lane of a SIMD has (one wave per SIMD is accepted: the forward kernel alone holds 253).  Registers, waves per SIMD and
LDS are printed.

Figures as built: 428 registers of the unified file (256 VGPRs + 172 AGPRs: `vgpr_count` is their total), one wave per SIMD, private
segment 0, no vector spill, 36864 bytes of LDS (the per-lane slab of the saved stage rates: 18 doubles x 256 lanes)."""
import os
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
KERNEL = "_ZN4bmpc25plant_rollout_grad_kernelE"
VGPRS_PER_SIMD = 512                   # gfx950: the unified register file of a SIMD holds 512 registers per lane
LDS_PER_CU = 160 * 1024


@needs_hipcc
def test_gradient_kernel_has_no_private_segment_no_vector_spill_and_fits_the_register_file():
    _, meta = isa.kernel(isa.compile_isa("bmpc_plant_rollout_grad.hip"), KERNEL)
    regs = meta["vgpr_count"]                      # (gfx950: the unified total, AGPRs included)
    granule = -(-regs // 8) * 8
    print(KERNEL, meta, "registers", regs, "waves per SIMD", min(8, VGPRS_PER_SIMD // granule), "LDS bytes", meta["group_segment_fixed_size"])
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert regs <= VGPRS_PER_SIMD and meta["agpr_count"] <= regs, meta
    assert meta["group_segment_fixed_size"] == 18 * 8 * 256 <= LDS_PER_CU, meta


@needs_hipcc
def test_the_roll_out_kernel_is_still_there_under_its_name():
    """The new file includes bmpc_plant_rollout.hip: its kernel compiles from there as it did (one match, isa.kernel asserts it)."""
    body, meta = isa.kernel(isa.compile_isa("bmpc_plant_rollout_grad.hip"), "_ZN4bmpc28plant_rollout_samples_kernelE")
    assert len(body) > 50 and meta["private_segment_fixed_size"] == 0
