"""Instruction order of the symmetric sweep's two-pivot steps in the gfx950 ISA of solve_kernel<10> (no GPU needed).

A step is the code between two s_barriers of the sweep loop.  Its cost is set by what sits between the barrier and the
FMAs and between the publication of the next pivot columns and the next barrier, not by the FMAs themselves
(DESIGN.md section 9).  Two orders are held here:
  * the pivot-row reads (ds_read_b128) go out before the pivot algebra (v_rcp_f32), so that their latency runs under it;
  * the store of the next pivot columns is followed by at least 20 of the step's packed FMAs, so that its round trip
    runs under them and the lgkmcnt(0) in front of the barrier finds it landed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def sweep_steps(tmp_path_factory):
    """The sweep steps of solve_kernel<10>: lists of instructions, each from one s_barrier to the next (the last one to the
    loop's back edge)."""
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("isa") / "bmpc.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", os.path.join(ge.CSRC, "bmpc_capi.hip"), "-o", out] + ge.KERNEL_FLAGS,
                          cwd=ge.CSRC, stderr=subprocess.DEVNULL)
    lines = open(out).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"_ZN4bmpc\d+solve_kernelILi10EE\S*:", ln))
    end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
    body = [x.split(";")[0].strip() for x in lines[start + 1:end]]
    body = [x for x in body if x and (not x.startswith(".") or re.match(r"\.LBB\d+_\d+:", x))]
    # the sweep loop: the innermost backward branch that encloses a whole column half of steps (as in
    # test_kernel_resources.test_no_scratch_access_in_the_hot_loops)
    pk = [k for k, x in enumerate(body) if x.startswith("v_pk_fma_f32")]
    labels = {mm.group(1): k for k, x in enumerate(body) for mm in [re.match(r"(\.LBB\d+_\d+):", x)] if mm}
    loops = []
    for k, x in enumerate(body):
        mm = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", x)
        if mm and mm.group(1) in labels and labels[mm.group(1)] < k:
            a = labels[mm.group(1)]
            loops.append((k - a, sum(1 for q in pk if a <= q <= k), a, k))
    _, _, a, b = min(x for x in loops if x[1] >= 60)
    bars = [k for k in range(a, b + 1) if body[k].startswith("s_barrier")]
    return [body[s:e] for s, e in zip(bars, bars[1:] + [b + 1])]


needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not available")


@needs_hipcc
def test_one_step_per_pivot_pair(sweep_steps):
    # h = 10: 60 columns, 30 per half, 15 two-pivot steps per half (the loop over the halves is not unrolled); every
    # step updates the 15 register pairs of its lane with two packed FMAs each
    assert len(sweep_steps) == 15, len(sweep_steps)
    for s in sweep_steps:
        assert sum(1 for x in s if x.startswith("v_pk_fma_f32")) == 30, s


@needs_hipcc
def test_pivot_rows_are_fetched_before_the_pivot_algebra(sweep_steps):
    for n, s in enumerate(sweep_steps):
        reads = [k for k, x in enumerate(s) if x.startswith("ds_read_b128")]
        rcp = [k for k, x in enumerate(s) if x.startswith("v_rcp_f32")]
        assert reads, (n, "no pivot-row reads in the step")
        assert not rcp or max(reads) < min(rcp), (n, "pivot-row read behind the pivot algebra", s)


@needs_hipcc
def test_publication_runs_under_the_fmas(sweep_steps):
    for n, s in enumerate(sweep_steps):
        writes = [k for k, x in enumerate(s) if x.startswith("ds_write")]
        assert len(writes) == 1, (n, writes)            # the next pivot columns: two entries, one ds_write2_b32
        behind = sum(1 for x in s[writes[0]:] if x.startswith("v_pk_fma_f32"))
        assert behind >= 20, (n, "publication followed by only %d packed FMAs" % behind, s)
