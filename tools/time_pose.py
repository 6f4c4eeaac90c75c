#!/usr/bin/env python3
"""Device time of post.estimate_poses and of each of its kernels: one 640x480 scene of 4000 matches (30 % outliers, 0.5 px
noise), samples = 2048, one pair and a batch of 64 copies.  The whole call is bracketed with device events (two rounds of
ten calls after three warm-up calls); the kernels' own durations come from the profiler's device activity records of one
more round.  Writes profiles/pose_time.txt.

    python tools/time_pose.py [--out profiles/pose_time.txt] [--samples 2048] [--matches 4000]"""
import argparse
import collections
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_ref as pr  # noqa: E402
from featurematching_amd import post  # noqa: E402


def event_ms(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_us(fn, iters=5):
    """{kernel name: mean microseconds per call} of the k_pose_* kernels, from the profiler's device records"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    tot = collections.defaultdict(float)
    for ev in prof.events():
        m = re.search(r"k_pose_[a-z]+", ev.name)
        if m:
            tot[m.group(0)] += getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
    return {k: v / iters for k, v in sorted(tot.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.txt"))
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--matches", type=int, default=4000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = pr.scene(seed=77, n=a.matches, noise=0.5, outliers=0.3)
    lines = [f"post.estimate_poses: {a.matches} matches per pair (30 % outliers, 0.5 px noise), samples = {a.samples}; "
             f"{torch.cuda.get_device_name(0)}"]
    for n in (1, 64):
        k0, k1, bids, K0, K1, _ = pr.batch([sc] * n)
        g = lambda x: torch.as_tensor(x, device=dev)
        args = (g(k0), g(k1), g(bids), g(K0), g(K1))
        fn = lambda: post.estimate_poses(*args, samples=a.samples, seed=0)
        out = fn()
        rounds = [event_ms(fn), event_ms(fn)]
        per = out.per_pair[0].tolist()
        r_err = pr.rotation_angle_deg(out.R[0].cpu().numpy(), sc["R"])
        lines.append(f"N = {n:2d}: {rounds[0]:.3f} / {rounds[1]:.3f} ms per call (two rounds of 10, events, allocation of the workspace "
                     f"and outputs included); pair 0: {per[1]} inliers of {per[0]}, R_err {r_err:.3f} deg")
        per_kernel = kernel_us(fn)
        if set(per_kernel) != {"k_pose_prep", "k_pose_solve", "k_pose_score", "k_pose_final"}:
            raise RuntimeError(f"the profiler recorded {sorted(per_kernel)}, not the four kernels of the call")
        for name, us in per_kernel.items():
            lines.append(f"    {name:14s} {us / 1e3:9.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
