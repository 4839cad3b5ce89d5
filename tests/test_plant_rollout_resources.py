"""Compile-time resources of plant_rollout_samples_kernel (csrc/bmpc_plant_rollout.hip), read from the gfx950 ISA and code object
metadata like tests/test_plant_ground_resources.py (no GPU needed): no scratch instruction and no private segment, no vector
register spilt, no LDS and no barrier, and fp64 arithmetic.  Registers and waves per SIMD are printed, not asserted: the horizon
loop around the stage loop is new, and what it costs is a figure of docs/history_r21.md, not a contract.

Figures as built: 253 VGPRs, 0 AGPRs (two waves per SIMD, the launch bound), private segment 0, no LDS; the uniform side (the
handle's body, the scheme, Q, R, the commands, the thresholds: about 200 scalar values) does not fit the scalar file and part of it
lives in lanes of vector registers (sgpr_spill_count, printed) -- not in scratch."""
import os
import shutil

import pytest

from tests import isa

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
KERNEL = "_ZN4bmpc28plant_rollout_samples_kernelE"
VGPRS_PER_SIMD = 512                   # gfx950: the unified register file of a SIMD holds 512 registers per lane


@needs_hipcc
def test_rollout_kernel_has_no_scratch_no_vector_spill_no_lds_no_barrier():
    body, meta = isa.kernel(isa.compile_isa("bmpc_plant_rollout.hip"), KERNEL)
    regs = meta["vgpr_count"] + meta["agpr_count"]
    granule = -(-regs // 8) * 8
    print(KERNEL, meta, "registers", regs, "waves per SIMD", min(8, VGPRS_PER_SIMD // granule), "instructions", len(body))
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] == 0, meta
    assert not any(x.startswith("scratch_") or x.startswith("ds_") or x.startswith("s_barrier") for x in body)
    assert sum(1 for x in body if x.startswith("v_fma_f64")) >= 50            # it really is fp64


@needs_hipcc
def test_the_plant_kernels_are_still_there_under_their_names():
    """The new file includes bmpc_plant.hip: its kernels compile from there as they did (one match each, isa.kernel asserts it)."""
    text = isa.compile_isa("bmpc_plant_rollout.hip")
    for name in ("_ZN4bmpc17plant_step_kernelE", "_ZN4bmpc24plant_step_ground_kernelE", "_ZN4bmpc20ground_reduce_kernelE"):
        body, _ = isa.kernel(text, name)
        assert len(body) > 50
