#!/usr/bin/env python3
"""A/B of the descriptor quantisation pass (k_prep_split) of two or more builds of the library in ONE process,
interleaved rounds (devices and runs differ by ~10 %: never compare numbers of different jobs):

    python tools/ab_prep.py build/variants/libfmatch_A.so build/variants/libfmatch_B.so [--workloads cfg2 cfg3]
        [--flat]      time fm_debug_launch_flat(which = 0), the variant that writes the float16 planes too
        [--stamps]    the libraries are -DFM_DIAG_CLOCK builds: print the constant-clock stamps of every workgroup's phases
        [--identity]  no timing: every prep output region of every library against the first one's, byte for byte, on
                      seeded 'peaky' / 'mixed' / 'borderline' inputs (both launch forms)

Inputs are drawn on the device with the statistics of featurematching_amd.synth (gain, noise, the 'mixed' rows); the
workspace is a full-size one, cleared once.  The kernel reads nothing but the descriptors (and writes every byte it
owns), so no complete call has to come first.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import _lib, synth  # noqa: E402
import bench  # noqa: E402

FNS = ("fm_debug_launch_prep", "fm_debug_launch_flat", "fm_debug_coarse_layout", "fm_coarse_workspace_bytes",
       "fm_default_cand_slots")
STAMPS = ["start", "loads issued", "loads landed", "quantised", "end"]


def open_lib(path):
    v = C.CDLL(os.path.abspath(path))
    for fn in FNS:
        getattr(v, fn).restype, getattr(v, fn).argtypes = _lib.ALL_SIGNATURES[fn]
    return v


def descriptors(seed, n, l, c, dist, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    gain, sigma = synth.DISTRIBUTIONS[dist]
    f0 = gain * torch.randn(n, l, c, device=dev, generator=g)
    f1 = torch.empty_like(f0)
    for b in range(n):
        f1[b] = f0[b][torch.randperm(l, device=dev, generator=g)] + sigma * torch.randn(l, c, device=dev, generator=g)
    if dist == "mixed":
        f0[torch.rand(n, l, device=dev, generator=g) < synth.MIXED_FRACTION] *= synth.MIXED_SCALE
        f1[torch.rand(n, l, device=dev, generator=g) < synth.MIXED_FRACTION] *= synth.MIXED_SCALE
    return f0, f1


def regions(v, n, l, c, slots):
    """name -> (byte offset, bytes) of everything k_prep_split writes.  The layout call names q0, q1, sigimg, l1_0 and the
    float16 planes; l1_1 and the block statistics follow l1_0, every region on the next 256-byte boundary."""
    lay = (C.c_int64 * 41)()
    _lib.check(v.fm_debug_coarse_layout(n, l, l, c, slots, lay, 41), "layout")
    lp, sp, cp = int(lay[4]), int(lay[5]), int(lay[3])

    def up(x):
        return (x + 255) // 256 * 256
    l1_0 = int(lay[21])
    l1_1 = up(l1_0 + n * lp * 4)
    bstat0 = up(l1_1 + n * sp * 4)
    bstat1 = up(bstat0 + n * lp // 32 * 16)
    return {"prep_zero": (int(lay[10]), int(lay[18]) - int(lay[10])), "q0": (int(lay[18]), n * lp * cp),
            "q1": (int(lay[19]), n * sp * cp), "sigimg": (int(lay[20]), n * 8), "l1_0": (l1_0, n * lp * 4),
            "l1_1": (l1_1, n * sp * 4), "bstat0": (bstat0, n * lp // 32 * 16), "bstat1": (bstat1, n * sp // 32 * 16),
            "hi0": (int(lay[14]), n * lp * cp * 2), "lo0": (int(lay[15]), n * lp * cp * 2),
            "hi1": (int(lay[16]), n * sp * cp * 2), "lo1": (int(lay[17]), n * sp * cp * 2), "colB": (int(lay[25]), 0)}


def workspace(v, n, l, c, slots, dev):
    nbytes = C.c_size_t()
    _lib.check(v.fm_coarse_workspace_bytes(n, l, l, c, slots, C.byref(nbytes)), "workspace bytes")
    ws = torch.zeros(nbytes.value + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    return ws, off, C.c_void_p(ws.data_ptr() + off)


def launch(v, flat, ptr, f0, f1, n, l, c, slots, st):
    f0p, f1p = C.c_void_p(f0.data_ptr()), C.c_void_p(f1.data_ptr())
    if flat:
        return v.fm_debug_launch_flat(ptr, f0p, f1p, n, l, l, c, slots, 0.1, 0.2, 0, st)
    return v.fm_debug_launch_prep(ptr, f0p, f1p, n, l, l, c, slots, st)


def identity(a, vs, names, dev, st):
    bad = 0
    for wl in a.workloads:
        wld = bench.WORKLOADS[wl]
        sh = synth.config_shapes(wld)
        n, l, c = wld["n"], sh["l"], wld["c"]
        slots = vs[0].fm_default_cand_slots(0.2)
        ws, off, ptr = workspace(vs[0], n, l, c, slots, dev)
        reg = regions(vs[0], n, l, c, slots)
        for dist in ("peaky", "mixed", "borderline"):
            differ = 0
            for seed in range(a.seeds):
                f0, f1 = descriptors(1000 + seed, n, l, c, dist, dev)
                for flat in (False, True):
                    want = None
                    for v in vs:
                        ws.fill_(0xA5)                   # (whatever a build leaves unwritten shows as a difference too)
                        _lib.check(launch(v, flat, ptr, f0, f1, n, l, c, slots, st), "launch")
                        torch.cuda.synchronize()
                        got = {k: ws[off + o: off + o + nb].clone() for k, (o, nb) in reg.items()
                               if nb and (flat or k[:2] not in ("hi", "lo"))}
                        if want is None:
                            want = got
                        else:
                            for k in got:
                                if not torch.equal(got[k], want[k]):
                                    differ += 1
                                    print(f"   DIFFERENT {wl} {dist} seed {1000 + seed} flat={int(flat)} {k}")
            print(f"identity {wl} {dist:10s}: {a.seeds} seeded inputs x (prep, flat) x {len(vs) - 1} build(s) against "
                  f"{names[0]}: {differ} regions differ")
            bad += differ
    print("identity:", "every region byte-identical" if bad == 0 else f"{bad} regions DIFFER")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--workloads", nargs="+", default=["cfg2", "cfg3"])
    ap.add_argument("--dist", default="peaky")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--seeds", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vs = [open_lib(p) for p in a.libs]
    names = [os.path.basename(p) for p in a.libs]
    if a.identity:
        sys.exit(1 if identity(a, vs, names, dev, st) else 0)
    for wl in a.workloads:
        wld = bench.WORKLOADS[wl]
        sh = synth.config_shapes(wld)
        n, l, c = wld["n"], sh["l"], wld["c"]
        slots = vs[0].fm_default_cand_slots(0.2)
        f0, f1 = descriptors(1017, n, l, c, a.dist, dev)
        ws, off, ptr = workspace(vs[0], n, l, c, slots, dev)
        reps = 200 if n * l <= 4 * 4800 else 30
        t = [[] for _ in vs]
        for rnd in range(a.rounds + 1):
            for k, v in enumerate(vs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch(v, a.flat, ptr, f0, f1, n, l, c, slots, st)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    t[k].append(e0.elapsed_time(e1) * 1e3 / reps)
        for k, nm in enumerate(names):
            print(f"{wl} {'flat' if a.flat else 'prep'} {nm:36s} median {np.median(t[k]):9.2f} us  min {min(t[k]):9.2f}"
                  f"  max {max(t[k]):9.2f} us per launch")
        if a.stamps:
            reg = regions(vs[0], n, l, c, slots)
            nb = 2 * n * int(reg["l1_0"][1] // 4 // n) // 32
            for k, v in enumerate(vs):
                launch(v, a.flat, ptr, f0, f1, n, l, c, slots, st)
                torch.cuda.synchronize()
                o = off + reg["colB"][0]
                d = ws[o: o + nb * 8 * 4].view(torch.float32).cpu().numpy().reshape(nb, 8)[:, :5]
                d = d[d[:, 0] != 0]                      # (a slot nobody stamped would read as the epoch)
                # (24-bit ticks of 10 ns: differences are taken modulo 2^24, centred, so a counter that wrapped inside the
                # launch does not show as 168 ms)
                half = 1 << 23
                rel = ((d - np.median(d[:, 0]) + half) % (2 * half) - half) * 0.01     # us around the median start
                rel -= np.percentile(rel[:, 0], 1)                                      # ... since the first starts
                own = ((d - d[:, :1]) % (2 * half)) * 0.01                              # us since the workgroup's own start
                print(f"{wl} stamps {names[k]}: {len(d)} workgroups")
                for j, nme in enumerate(STAMPS):
                    print(f"   {nme:13s} since the first workgroups' start: median {np.median(rel[:, j]):6.2f}  max "
                          f"{rel[:, j].max():6.2f}   in the workgroup: median {np.median(own[:, j]):6.2f}  "
                          f"max {own[:, j].max():6.2f}")


if __name__ == "__main__":
    main()
