#!/usr/bin/env python3
"""A training step of the coarse level two ways, time and peak allocator bytes, in one process:

  (a) conf_matrix route: ops.coarse_match(conf_matrix=True) + ops.attach_conf_matrix_grad + the reference's loss
      expression in torch (losses/loss.py:27-67 on a dense conf_matrix_gt) + backward()
  (b) matrix-free route: ops.coarse_match(stats=True) + ops.coarse_loss + backward()

at one 640x480 pair and at 64 pairs (L = S = 4800, C = 256, 'borderline' descriptors; supervision: every third match the
matcher found + 500 random triples per pair + 5 repeats), focal and cross entropy.  The two routes alternate rep by rep;
every rep is timed with device events around the whole step; medians and the min .. max spread are printed.  The dense
conf_matrix_gt of route (a) is built once, outside the timed region (the supervision code writes it, not the loss).

    python tools/time_coarse_loss.py [--pairs 1 64] [--reps 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import ops, synth  # noqa: E402

HW, L, C = (60, 80), 4800, 256


def reference_loss(conf, conf_gt, kind, alpha=0.25, gamma=2.0):
    """losses/loss.py:27-67 with pos_weight = neg_weight = 1 (its two .any() host syncs included)"""
    pos_mask, neg_mask = conf_gt == 1, conf_gt == 0
    w_pos = w_neg = 1.0
    if not pos_mask.any():
        pos_mask[0, 0, 0] = True
        w_pos = 0.
    if not neg_mask.any():
        neg_mask[0, 0, 0] = True
        w_neg = 0.
    conf = torch.clamp(conf, 1e-6, 1 - 1e-6)
    if kind == 'cross_entropy':
        return w_pos * (-torch.log(conf[pos_mask])).mean() + w_neg * (-torch.log(1 - conf[neg_mask])).mean()
    loss_pos = -alpha * torch.pow(1 - conf[pos_mask], gamma) * (conf[pos_mask]).log()
    loss_neg = -alpha * torch.pow(conf[neg_mask], gamma) * (1 - conf[neg_mask]).log()
    return w_pos * loss_pos.mean() + w_neg * loss_neg.mean()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}; L = S = {L}, C = {C}, 'borderline'; ms per step: median (min .. max) of "
             f"{args.reps} alternating reps after 2 warm-up steps each; peak: allocator bytes above the inputs"]
    f0n, f1n = synth.coarse_descriptors(23, 1, L, C, "borderline")
    for n in args.pairs:
        f0 = torch.as_tensor(f0n, device=dev).repeat(n, 1, 1).contiguous()
        f1 = torch.as_tensor(f1n, device=dev).repeat(n, 1, 1).contiguous()
        m = ops.coarse_match(f0, f1, HW, HW, 8.0)
        g = torch.Generator().manual_seed(41)
        rnd = torch.stack([torch.randint(n, (500 * n,), generator=g), torch.randint(L, (500 * n,), generator=g),
                           torch.randint(L, (500 * n,), generator=g)], 1).to(dev)
        ids = torch.cat([torch.stack([m['b_ids'][::3], m['i_ids'][::3], m['j_ids'][::3]], 1), rnd], 0)
        ids = torch.cat([ids, ids[:5]], 0).contiguous()
        del m
        a0, a1 = f0.clone().requires_grad_(True), f1.clone().requires_grad_(True)
        for kind in ("focal", "cross_entropy"):
            last = {}

            def route_b():
                a0.grad = a1.grad = None
                out = ops.coarse_match(f0, f1, HW, HW, 8.0, stats=True)
                loss = ops.coarse_loss(a0, a1, ids[:, 0], ids[:, 1], ids[:, 2], out['_coarse_buffers'], kind)
                loss.backward()
                last['b'] = (loss.detach(), a0.grad, a1.grad)

            try:
                gt = torch.zeros(n, L, L, device=dev)
                gt[ids[:, 0], ids[:, 1], ids[:, 2]] = 1

                def route_a():
                    a0.grad = a1.grad = None
                    out = ops.coarse_match(f0, f1, HW, HW, 8.0, conf_matrix=True)
                    conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])
                    loss = reference_loss(conf, gt, kind)
                    loss.backward()
                    last['a'] = (loss.detach(), a0.grad, a1.grad)

                for _ in range(2):
                    route_a()
                    route_b()
                have_a = True
            except torch.cuda.OutOfMemoryError:
                have_a = False
                gt = None
                torch.cuda.empty_cache()
                route_b()
                route_b()
            ta, tb = [], []
            for _ in range(args.reps):
                if have_a:
                    ta.append(timed(route_a))
                tb.append(timed(route_b))
            fmt = lambda t: f"{statistics.median(t):9.3f} ({min(t):.3f} .. {max(t):.3f})"
            la, d0a, d1a = last['a'] if have_a else (None, None, None)
            lb, d0b, d1b = last['b']
            last.clear()
            pb = peak_of(route_b)
            last.clear()
            line = f"N={n:3d} {kind:13s} | (b) matrix-free {fmt(tb)} ms, peak {pb / 1e6:9.1f} MB"
            if have_a:
                pa = peak_of(route_a)
                last.clear()
                diff = max(((x - y).abs().max() / y.abs().max()).item() for x, y in ((d0b, d0a), (d1b, d1a)))
                line += (f" | (a) conf_matrix {fmt(ta)} ms, peak {pa / 1e6:9.1f} MB (+ conf_matrix_gt {gt.numel() * 4 / 1e6:.0f} MB)"
                         f" | [N,L,S] float32 = {n * L * L * 4 / 1e6:.0f} MB | loss (b) {lb.item():.7f} (a) {la.item():.7f}, "
                         f"gradients differ by {diff:.1e} of max|grad|")
            else:
                line += f" | (a) conf_matrix: out of memory at this batch | [N,L,S] float32 = {n * L * L * 4 / 1e6:.0f} MB"
            print(line, flush=True)
            lines.append(line)
            del gt
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
