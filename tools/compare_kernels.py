#!/usr/bin/env python3
"""Are the kernels of two builds the same, instruction for instruction?

    for f in featurematching_amd/csrc/*.hip; do
      hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ifeaturematching_amd/csrc --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    done                                   # once per build, then:
    python tools/compare_kernels.py DIR_A DIR_B [--counts KERNEL ...]

A kernel template is emitted where the host code first names it, so a host-only change reorders the kernels of a file
and renumbers their local labels.  Each .s is therefore cut into one piece per kernel, from `; -- Begin function NAME`
to its `.end_amdhsa_kernel` (the instructions and the resource block: registers, LDS, scratch, kernarg size), the
function's number in local labels (`.LBB12_3` -> `.LBB_3`) and runs of blanks are dropped, and the pieces are compared
by name - across files: a kernel's (mangled) name is unique in the library, and one that moved to another translation
unit is compared where it went and listed as moved.  Prints the kernel count per file, every moved kernel and every
missing or differing kernel; exit status 1 if there is any of the latter two.

--counts NAME (a substring of the mangled name): for a kernel that differs, the two things that tell a reordering from
a change - its resource block (the .amdhsa_ directives) side by side, and its instructions counted per opcode."""
import collections
import pathlib
import re
import sys

PIECE = re.compile(r"; -- Begin function (\S+)\n.*?^\s*\.end_amdhsa_kernel$", re.M | re.S)
LABEL = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp|\.LJTI|\bBB)\d+")   # (BBn_m: how comments name .LBBn_m)
BLANKS = re.compile(r"[ \t]+")       # (a label's comment is aligned to the label's length)
OPCODE = re.compile(r"^\s+([a-z][a-z0-9_]+)(?:\s|$)", re.M)                      # (directives start with a dot, labels at column 0)
RESOURCE = re.compile(r"^\s*(\.amdhsa_\S+)\s+(\S+)", re.M)


def kernels(path):
    return {m.group(1): BLANKS.sub(" ", LABEL.sub(r"\1", m.group(0))) for m in PIECE.finditer(path.read_text())}


def build(d):
    """{kernel: (file, text)} of a directory of .s files, and the kernel count per file"""
    out, per_file = {}, {}
    for p in sorted(pathlib.Path(d).glob("*.s")):
        ks = kernels(p)
        per_file[p.name] = len(ks)
        for k, text in ks.items():
            assert k not in out, f"{k} in {out[k][0]} and {p.name}"
            out[k] = (p.name, text)
    return out, per_file


def counts(name, ta, tb):
    """resource block and per-opcode instruction counts of one kernel in both builds"""
    ra, rb = dict(RESOURCE.findall(ta)), dict(RESOURCE.findall(tb))
    res = [f"    {k} {ra.get(k)} -> {rb.get(k)}" for k in sorted(ra.keys() | rb.keys()) if ra.get(k) != rb.get(k)]
    ca, cb = collections.Counter(OPCODE.findall(ta)), collections.Counter(OPCODE.findall(tb))
    ops = [f"    {k} {ca[k]} -> {cb[k]}" for k in sorted(ca.keys() | cb.keys()) if ca[k] != cb[k]]
    print(f"{name}:\n  resource block: {len(ra)} / {len(rb)} directives, " + (f"{len(res)} differ" if res else "identical"))
    print("\n".join(res) if res else "", end="\n" if res else "")
    print(f"  instructions: {sum(ca.values())} / {sum(cb.values())}, {len(ca)} / {len(cb)} opcodes, "
          + (f"{len(ops)} opcode counts differ" if ops else "the same multiset per opcode"))
    print("\n".join(ops) if ops else "", end="\n" if ops else "")


def main(dir_a, dir_b, *rest):
    (a, fa), (b, fb) = build(dir_a), build(dir_b)
    for f in sorted(fa.keys() | fb.keys()):
        print(f"{f}: {fa.get(f, 0)} / {fb.get(f, 0)} kernels")
    for k in sorted(a.keys() & b.keys()):
        if a[k][0] != b[k][0]:
            print(f"moved: {k}: {a[k][0]} -> {b[k][0]}")
    bad = [f"{k}: missing on one side ({(a.get(k) or b.get(k))[0]})" for k in sorted(a.keys() ^ b.keys())]
    bad += [f"{b[k][0]}: {k}: differs" for k in sorted(a.keys() & b.keys()) if a[k][1] != b[k][1]]
    print("\n".join(bad) if bad else f"{len(a)} kernels in {len(fa)} files, no kernel missing or differing")
    if rest and rest[0] == "--counts":
        for want in rest[1:]:
            for k in sorted(a.keys() & b.keys()):
                if want in k:
                    counts(k, a[k][1], b[k][1])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
