"""What the mat-vec of an iteration (phase P4, gamma = V beta) asks of the LDS array and of the vector port at h = 10, read off
the gfx950 ISA of solve_kernel<10> (no GPU needed).

After a row-pair sweep V stays in the row-pair layout: a lane holds half the columns of its half for TWO
rows, so it fetches one quarter of beta -- 4 ds_read_b128 where the row-half layout needs 8 reads -- and every fetched entry
feeds both rows of one packed FMA, 15 of them.  Held here, for the code between the two workgroup barriers of the phase:
  * exactly 4 ds_read_b128, no other LDS read, and exactly 15 v_pk_fma_f32;
and for the kernel: no scratch, at most 256 vector registers, and an LDS image of at most 40 960 bytes (four instances per CU).
The listing is the one the other resource tests read: the library's flags and the sources' defaults, BMPC_ROWPAIR_MATVEC =
BMPC_RECLASSIFY_ONCE = 1."""
import os
import re
import shutil

import pytest

from tests import isa

HIPCC = isa.HIPCC
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not available")


def matvec_phase(body):
    """The instructions of phase P4 in the kernel's body (tests/isa.py: instructions and block labels): the one stretch between two
    consecutive s_barriers, outside the sweep loop, that is straight-line code (no label, no branch), multiplies on the packed-f32
    pipe and exchanges across the quad (DPP quad_perm:[2,3,0,1]) -- or, in the row-half layout, across the pair only."""
    bars = [k for k, x in enumerate(body) if x.startswith("s_barrier")]
    found = []
    for a, b in zip(bars, bars[1:]):
        seg = body[a + 1:b]
        if any(x.endswith(":") or x.startswith(("s_cbranch", "s_branch")) for x in seg):
            continue
        # a sweep step is such a stretch too: it publishes a pivot column (a two-address store) and holds 2 FMAs per register pair
        if any(x.startswith("ds_write2") for x in seg):
            continue
        if any(x.startswith("v_pk_fma_f32") for x in seg):
            found.append(seg)
    assert len(found) == 1, [len(s) for s in found]
    return found[0]


@pytest.fixture(scope="module")
def kernel10():
    """(instructions, metadata) of solve_kernel<10> in the listing the resource tests share (tests/isa.py: the library's flags and
    the sources' defaults, compiled once per process)."""
    return isa.kernel(isa.compile_isa("bmpc_capi.hip"), "_ZN4bmpc12solve_kernelILi10EE")


@needs_hipcc
def test_matvec_fetches_a_quarter_of_beta(kernel10):
    seg = matvec_phase(kernel10[0])
    ds = [x.split()[0] for x in seg if x.startswith("ds_")]
    reads = [x for x in ds if x.startswith("ds_read")]
    fmas = sum(1 for x in seg if x.startswith("v_pk_fma_f32"))
    valu = sum(1 for x in seg if x.startswith("v_"))
    print("P4: %d instructions, %d vector (%d v_pk_fma_f32), LDS: %s" % (len(seg), valu, fmas, " ".join(ds)))
    assert reads.count("ds_read_b128") == 4 and len(reads) == 4, reads
    assert fmas == 15, fmas
    # the two copies of gamma and nothing else are stored
    assert [x for x in ds if not x.startswith("ds_read")] == ["ds_write_b32"], ds
    assert sum(1 for x in seg if re.search(r"quad_perm:\[2,3,0,1\]", x)) == 4, seg


@needs_hipcc
def test_four_instances_still_share_a_cu(kernel10):
    meta = kernel10[1]
    print(meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert not [x for x in kernel10[0] if x.startswith(("scratch_", "buffer_"))]
    assert meta["vgpr_count"] + meta["agpr_count"] <= 256, meta
    assert meta["group_segment_fixed_size"] <= 40960, meta
