#!/usr/bin/env python3
"""Same-process timing, for information, of the supervision and fine-loss calls next to what the reference does on the
device: ops.supervise_matches against a de-duplication by np.unique on the host with the copies around it, and
ops.fine_loss forward + backward against the same loss in torch ops (modules.fine_loss_torch) with autograd.  Alternating repetitions, host clock around a device synchronise,
median (min - max).  Needs an MI355X.

    python tools/time_supervision.py [--reps 30] > profiles/supervision_fine_loss_time.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from featurematching_amd import modules, ops          # noqa: E402
import supervision_ref as sref                        # noqa: E402

DEV = "cuda:0"


def host_unique_preprocess(kp0, kp1, h_c, w_c):
    """The de-duplication the way the reference does it: the image-1 cells go to the host, np.unique picks one row per
    cell there (a second pass over the kept rows, as the reference makes, finds nothing more), the choice comes back as an
    index tensor and two scatters fill the per-cell tables."""
    keep = torch.arange(kp0.shape[0], device=kp0.device)
    for _ in range(2):
        on_host = torch.floor(kp1[keep] / 8).cpu().numpy()
        first = np.unique(on_host, axis=0, return_index=True)[1]
        keep = keep[torch.from_numpy(first).to(kp0.device)]
    tables = []
    for kp in (kp0[keep], kp1[keep]):
        cx, cy = torch.floor(kp / 8).long().unbind(-1)
        table = torch.zeros(h_c * w_c, 2, device=kp.device)
        table[cx + w_c * cy] = kp
        tables.append(table)
    return keep, tables


def timed(fns, reps):
    """{name: times in us}: the functions alternate within every repetition"""
    out = {name: [] for name in fns}
    for rep in range(reps + 3):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:                                   # three warm-up rounds
                out[name].append((time.perf_counter() - t0) * 1e6)
    return out


def report(title, times):
    print(title)
    for name, t in times.items():
        print(f"    {name:34s} {statistics.median(t):9.1f} us  ({min(t):.1f} - {max(t):.1f}, {len(t)} reps)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    print("host clock around a device synchronise, alternating repetitions; whole calls (allocations, launches and the one")
    print("host read of the HIP path; host copies and np.unique of the host route), not kernel times")
    for hw, k in (((60, 80), 2000), ((60, 80), 20000)):
        kp0 = torch.as_tensor(sref.points(5, k, hw, 0), device=DEV)
        kp1 = torch.as_tensor(sref.points(5, k, hw, 1), device=DEV)
        report(f"supervision, grid {hw[0]} x {hw[1]}, K = {k}", timed({
            "ops.supervise_matches": lambda: ops.supervise_matches(kp0, kp1, hw, hw),
            "np.unique on the host (reference)": lambda: host_unique_preprocess(kp0, kp1, *hw)}, args.reps))
    for m in (500, 4000):
        g0, g1 = sref.points(7, m, (60, 80), 0) + np.float32(0.5), sref.points(7, m, (60, 80), 1) + np.float32(0.5)
        g0[4::5, 0] = 0
        e0, e1 = (torch.as_tensor(a, device=DEV).requires_grad_(True) for a in sref.fine_inputs(7, g0, g1))
        g0, g1 = torch.as_tensor(g0, device=DEV), torch.as_tensor(g1, device=DEV)

        def step(fn):
            e0.grad = e1.grad = None
            fn(e0, e1, g0, g1).backward()
        report(f"fine loss forward + backward, M = {m}", timed({
            "ops.fine_loss": lambda: step(ops.fine_loss),
            "torch ops (modules.fine_loss_torch)": lambda: step(modules.fine_loss_torch)}, args.reps))


if __name__ == "__main__":
    main()
