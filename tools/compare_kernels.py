#!/usr/bin/env python3
"""Are the kernels of two builds the same, instruction for instruction?

    for f in featurematching_amd/csrc/*.hip; do
      hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ifeaturematching_amd/csrc --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    done                                   # once per build, then:
    python tools/compare_kernels.py DIR_A DIR_B

A kernel template is emitted where the host code first names it, so a host-only change reorders the kernels of a file
and renumbers their local labels.  Each .s is therefore cut into one piece per kernel, from `; -- Begin function NAME`
to its `.end_amdhsa_kernel` (the instructions and the resource block: registers, LDS, scratch, kernarg size), the
function's number in local labels (`.LBB12_3` -> `.LBB_3`) and runs of blanks are dropped, and the pieces are compared
by name.  Prints the kernel count per file and every missing or differing kernel; exit status 1 if there is any."""
import pathlib
import re
import sys

PIECE = re.compile(r"; -- Begin function (\S+)\n.*?^\s*\.end_amdhsa_kernel$", re.M | re.S)
LABEL = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp|\.LJTI|\bBB)\d+")   # (BBn_m: how comments name .LBBn_m)
BLANKS = re.compile(r"[ \t]+")       # (a label's comment is aligned to the label's length)


def kernels(path):
    return {m.group(1): BLANKS.sub(" ", LABEL.sub(r"\1", m.group(0))) for m in PIECE.finditer(path.read_text())}


def main(dir_a, dir_b):
    a, b = ({p.name: kernels(p) for p in sorted(pathlib.Path(d).glob("*.s"))} for d in (dir_a, dir_b))
    bad = [f"{f}: only in one directory" for f in sorted(a.keys() ^ b.keys())]
    for f in sorted(a.keys() & b.keys()):
        bad += [f"{f}: {k}: missing on one side" for k in sorted(a[f].keys() ^ b[f].keys())]
        bad += [f"{f}: {k}: differs" for k in sorted(a[f].keys() & b[f].keys()) if a[f][k] != b[f][k]]
        print(f"{f}: {len(a[f])} / {len(b[f])} kernels")
    print("\n".join(bad) if bad else f"{len(a)} files, no kernel missing or differing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
