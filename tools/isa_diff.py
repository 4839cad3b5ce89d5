#!/usr/bin/env python3
"""Compare two gfx950 assembly listings kernel by kernel: python tools/isa_diff.py A.s B.s

A.s / B.s: what tests/test_kernel_resources.py compiles (`hipcc --offload-arch=gfx950 -std=c++17 --cuda-device-only -S
bmpc_capi.hip` + KERNEL_FLAGS) for two states of the sources.  Per function symbol the instruction text is compared after
dropping comments, directives and source-line markers (local labels keep their order, not their numbers).  Prints
`identical`, or the instruction counts, the first differing line and the code-object metadata of both sides.  Exit status 1 if any symbol differs."""
import re
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def functions(text, normalise=True):
    """{symbol: [instruction lines]} of every `.type sym,@function` of the listing.  `normalise`: local labels numbered by order of
    appearance and runs of blanks collapsed (what a comparison wants); without it the lines keep the listing's own labels."""
    out, cur, labels = {}, None, {}
    names = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, flags=re.M))
    for ln in text.split("\n"):
        m = re.match(r"^(\S+):", ln)
        if m and m.group(1) in names:
            cur, labels = out.setdefault(m.group(1), []), {}
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            cur = None
            continue
        ln = ln.split(";")[0].strip()
        if not ln or (ln.startswith(".") and not re.match(r"^\.L\w+:", ln)):
            continue                                    # comments, directives, .loc / .file markers
        if normalise:
            # local labels (.LBB3_7, .LJTI3_0 ...): numbered in order of first appearance within the function
            ln = re.sub(r"\.L[A-Za-z]\w*", lambda k: labels.setdefault(k.group(0), ".L%d" % len(labels)), ln)
            ln = re.sub(r"\s+", " ", ln)
        cur.append(ln)
    return out


def metadata(text):
    out = {}
    for entry in re.split(r"\n\s+- (?=\.agpr_count:)", text)[1:]:
        m = re.search(r"\.name:\s+(\S+)", entry)
        if m:
            f = dict(re.findall(r"\.(\w+):\s+(\d+)\n", entry.split(".wavefront_size")[0]))
            out[m.group(1)] = {k: int(f[k]) for k in META if k in f}
    return out


def count(lines):
    return sum(1 for x in lines if not x.endswith(":"))


def main(a, b):
    ta, tb = open(a).read(), open(b).read()
    fa, fb, ma, mb = functions(ta), functions(tb), metadata(ta), metadata(tb)
    differ = 0
    for sym in sorted(set(fa) | set(fb)):
        if sym not in fa or sym not in fb:
            print("%-90s only in %s" % (sym, a if sym in fa else b))
            differ += 1
        elif fa[sym] == fb[sym] and ma.get(sym) == mb.get(sym):
            print("%-90s identical (%d instructions)" % (sym, count(fa[sym])))
        else:
            differ += 1
            print("%-90s DIFFERS: %d / %d instructions" % (sym, count(fa[sym]), count(fb[sym])))
            k = next((i for i, (x, y) in enumerate(zip(fa[sym], fb[sym])) if x != y), min(len(fa[sym]), len(fb[sym])))
            print("    first difference at line %d of the symbol: A `%s` | B `%s`" % (
                k, fa[sym][k] if k < len(fa[sym]) else "<end>", fb[sym][k] if k < len(fb[sym]) else "<end>"))
            print("    A:", ma.get(sym))
            print("    B:", mb.get(sym))
    print("%d symbols, %d differ" % (len(set(fa) | set(fb)), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
