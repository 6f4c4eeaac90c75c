"""Time the fine stage's two HIP backward calls at cfg#2 sizes (640 x 480: coarse 60 x 80, fine 240 x 320, Cf = 64,
stride 4) next to torch autograd of the same formulas in float32:
  fine   : fm_fine_match_backward (one kernel + the fixed-order d_mix reduction) against autograd through the torch
           restatement of fine_matching_new.py:50-79 (the backward part of the autograd step, timed alone)
  crop   : fm_gather_windows_backward (CSR count / scan / fill / sort + the per-pixel gather) against autograd through
           the reference's route F.unfold -> rearrange -> select (its backward: index_put into the unfold, then fold)
M = 1 000 and 4 800 matches, W = 5 and 7.  Median of the per-call times (CUDA events, 50 calls after 10 warm-up).
Usage: python tools/time_fine_backward.py"""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from featurematching_amd import ops  # noqa: E402

DEV = "cuda:0"
HC, WC, HF, WF, CF, STRIDE = 60, 80, 240, 320, 64, 4


def timed(fn, iters=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def fine_torch(win0, win1, mix0, mix1, w):
    ww = w * w
    t = torch.arange(w, device=win0.device, dtype=win0.dtype) / (w - 1) * 2 - 1
    gx, gy = t.repeat(w), t.repeat_interleave(w)
    outs = []
    for wa, wb, mix in ((win0, win1, mix0), (win1, win0, mix1)):
        q = torch.einsum('r,mrc->mc', mix[:ww], wa) + mix[ww]
        h = torch.softmax(torch.einsum('mc,mrc->mr', q, wb) / math.sqrt(wa.shape[2]), dim=1)
        co = torch.stack([(h * gx).sum(1), (h * gy).sum(1)], 1)
        var = torch.stack([(h * gx * gx).sum(1), (h * gy * gy).sum(1)], 1) - co ** 2
        outs.append(torch.cat([co * (w // 2) * 2.0 + w // 2, torch.sqrt(torch.clamp(var, min=1e-10)).sum(1, keepdim=True)], 1))
    return outs


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    print(f"cfg#2 sizes: coarse {HC}x{WC}, fine map {HF}x{WF}x{CF}, stride {STRIDE}; median us per call")
    print(f"{'M':>6} {'W':>2} | {'fine HIP':>9} {'fine torch':>10} | {'crop HIP':>9} {'crop torch':>10}")
    for m in (1000, 4800):
        for w in (5, 7):
            ww = w * w
            win0 = torch.randn(m, ww, CF, device=DEV, generator=g)
            win1 = torch.randn(m, ww, CF, device=DEV, generator=g)
            mix0 = torch.rand(ww + 1, device=DEV, generator=g) / w
            mix1 = torch.rand(ww + 1, device=DEV, generator=g) / w
            kc = torch.zeros(m, 2, device=DEV)
            d0, d1 = torch.randn(m, 3, device=DEV, generator=g), torch.randn(m, 3, device=DEV, generator=g)
            b = torch.zeros(m, dtype=torch.int64, device=DEV)
            ids = torch.randint(HC * WC, (m,), device=DEV, generator=g)
            feat = torch.randn(1, CF, HF, WF, device=DEV, generator=g)
            d_win = torch.randn(m, ww, CF, device=DEV, generator=g)

            leaves = [t.clone().requires_grad_(True) for t in (win0, win1, mix0, mix1)]
            k0, k1 = ops.fine_match_grad(*leaves, kc, kc, 2.0)
            t_fine_hip = timed(lambda: torch.autograd.grad((k0, k1), leaves, (d0, d1), retain_graph=True))
            o0, o1 = fine_torch(*leaves, w)
            t_fine_torch = timed(lambda: torch.autograd.grad((o0, o1), leaves, (d0, d1), retain_graph=True))

            fl = feat.clone().requires_grad_(True)
            win = ops.gather_windows_grad(fl, b, ids, w, STRIDE, WC, HC)
            t_crop_hip = timed(lambda: torch.autograd.grad(win, fl, d_win, retain_graph=True))
            u = F.unfold(fl, kernel_size=(w, w), stride=STRIDE, padding=2)
            u = u.view(1, CF, ww, -1).permute(0, 3, 2, 1)[b, ids]
            t_crop_torch = timed(lambda: torch.autograd.grad(u, fl, d_win, retain_graph=True))
            print(f"{m:>6} {w:>2} | {t_fine_hip:>9.1f} {t_fine_torch:>10.1f} | {t_crop_hip:>9.1f} {t_crop_torch:>10.1f}")


if __name__ == "__main__":
    main()
