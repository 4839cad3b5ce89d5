"""What a two-pivot step of the symmetric sweep asks of the LDS array and of the vector port, read off the gfx950 ISA of
solve_kernel<10> (no GPU needed).

Four instances share a CU's one LDS array, and the sweep's pivot-row reads are what loads it: in the
row-pair form a lane holds half the columns of TWO rows, so every fetched pivot-row entry feeds both halves of a packed FMA
and a step needs 8 ds_read_b128 instead of 14.  Held here, per step (the code between two s_barriers of the sweep loop):
  * at most 8 ds_read_b128 and no ds_read2_b64;
  * at most 56 LDS-array cycles, counted per wave-instruction with the figures measured for this chip (b32 / b64 reads 2,
    b128 and the two-address b32 reads 4, ds_read2_b64 8; stores by the transfer of their address and data registers:
    b32 4, b64 / write2_b32 6, b96 10, b128 / write2_b64 13) -- a broadcast costs what distinct addresses cost;
  * at most 38 vector instructions other than the 30 packed FMAs (the second row's multipliers are the price of the form)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# the form is selected by horizon (3 h <= BMPC_ROWPAIR_HN); stated here, so that the budget is held whatever the default is
ROWPAIR = "-DBMPC_ROWPAIR_HN=30"

# LDS-array cycles per wave-instruction
LDS_CYCLES = {
    "ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b96": 8, "ds_read_b128": 4,
    "ds_read2_b32": 4, "ds_read2st64_b32": 4, "ds_read2_b64": 8, "ds_read2st64_b64": 8,
    "ds_write_b32": 4, "ds_write_b64": 6, "ds_write2_b32": 6, "ds_write2st64_b32": 6,
    "ds_write_b96": 10, "ds_write_b128": 13, "ds_write2_b64": 13, "ds_write2st64_b64": 13,
}


def sweep_steps_of(asm_path):
    """The sweep steps of solve_kernel<10> in the assembly file: lists of instructions, each from one s_barrier to the next
    (the last one to the loop's back edge)."""
    lines = open(asm_path).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"_ZN4bmpc\d+solve_kernelILi10EE\S*:", ln))
    end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
    body = [x.split(";")[0].strip() for x in lines[start + 1:end]]
    body = [x for x in body if x and (not x.startswith(".") or re.match(r"\.LBB\d+_\d+:", x))]
    # the sweep loop: the innermost backward branch that encloses a whole column half of steps
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


def step_costs(step):
    """(ds_read_b128 count, ds_read2_b64 count, LDS-array cycles, vector instructions other than packed FMAs) of a step."""
    ds = [x.split()[0] for x in step if x.startswith("ds_")]
    unknown = [x for x in ds if x not in LDS_CYCLES]
    assert not unknown, ("LDS instruction without a cycle figure", unknown)
    valu = sum(1 for x in step if x.startswith("v_") and not x.startswith("v_pk_fma_f32"))
    return ds.count("ds_read_b128"), ds.count("ds_read2_b64"), sum(LDS_CYCLES[x] for x in ds), valu


@pytest.fixture(scope="module")
def sweep_steps(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("isa") / "bmpc.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", os.path.join(ge.CSRC, "bmpc_capi.hip"), "-o", out, ROWPAIR] + ge.KERNEL_FLAGS,
                          cwd=ge.CSRC, stderr=subprocess.DEVNULL)
    return sweep_steps_of(out)


needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not available")


@needs_hipcc
def test_pivot_row_reads_are_halved(sweep_steps):
    assert len(sweep_steps) == 15, len(sweep_steps)
    for n, s in enumerate(sweep_steps):
        b128, r2b64, _, _ = step_costs(s)
        print("step %2d: %d ds_read_b128, %d ds_read2_b64" % (n, b128, r2b64))
        assert b128 <= 8, (n, b128)
        assert r2b64 == 0, (n, r2b64)


@needs_hipcc
def test_lds_array_cycles_per_step(sweep_steps):
    for n, s in enumerate(sweep_steps):
        _, _, cyc, _ = step_costs(s)
        print("step %2d: %d LDS-array cycles: %s" % (n, cyc, " ".join(x.split()[0] for x in s if x.startswith("ds_"))))
        assert cyc <= 56, (n, cyc)


@needs_hipcc
def test_vector_instructions_beside_the_fmas(sweep_steps):
    for n, s in enumerate(sweep_steps):
        _, _, _, valu = step_costs(s)
        print("step %2d: %d vector instructions other than packed FMAs" % (n, valu))
        assert valu <= 38, (n, valu)
