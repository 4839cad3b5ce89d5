"""tools/isa_diff.py on two hand-written listings: comments, directives and label numbers do not count, an opcode does."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """\t.type\tkern,@function
kern:                                   ; @kern
; %%bb.0:
\t.loc\t1 %d 0
\ts_load_dword s2, s[0:1], 0x0
.LBB%d_1:                                ; =>This Inner Loop
\t%s v0, v0, v1
\ts_cbranch_scc1 .LBB%d_1
\ts_endpgm
.Lfunc_end0:
"""


def _run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), str(pa), str(pb)], capture_output=True, text=True)


def test_label_numbers_and_line_markers_do_not_count(tmp_path):
    r = _run(tmp_path, LISTING % (10, 0, "v_add_f32", 0), LISTING % (99, 7, "v_add_f32", 7))
    assert r.returncode == 0 and "identical (4 instructions)" in r.stdout, r.stdout


def test_a_changed_opcode_is_reported_with_its_place(tmp_path):
    r = _run(tmp_path, LISTING % (10, 0, "v_add_f32", 0), LISTING % (10, 0, "v_sub_f32", 0))
    assert r.returncode == 1 and "DIFFERS: 4 / 4 instructions" in r.stdout and "v_sub_f32" in r.stdout, r.stdout
