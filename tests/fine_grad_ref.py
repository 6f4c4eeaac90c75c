"""float64 restatements of the fine stage (fine_matching_new.py:50-79) and of the backward formula the HIP kernels
implement (include/fmatch.h, fm_fine_match_backward): the yardsticks of tests/test_fine_grad_abi.py and
tests/test_gpu_fine_grad.py."""
import math

import torch


def grid(w: int, dtype=torch.float64):
    """(gx, gy) [W*W] of kornia's normalised meshgrid, position r = wy * W + wx"""
    t = torch.arange(w, dtype=dtype) / (w - 1) * 2 - 1
    return t.repeat(w), t.repeat_interleave(w)


def fine_forward(win0, win1, mix0, mix1, mkpts0_c, mkpts1_c, scale):
    """(out0, out1) [M, 3] = (x, y, std) in the dtype of the inputs; mix = [WW + 1] (weights, then bias)"""
    m, ww, c = win0.shape
    w = int(math.isqrt(ww))
    gx, gy = (g.to(win0.dtype).to(win0.device) for g in grid(w))
    outs = []
    for wa, wb, mix, kc in ((win0, win1, mix0, mkpts0_c), (win1, win0, mix1, mkpts1_c)):
        q = torch.einsum('r,mrc->mc', mix[:ww], wa) + mix[ww]
        h = torch.softmax(torch.einsum('mc,mrc->mr', q, wb) / math.sqrt(c), dim=1)
        co = torch.stack([(h * gx).sum(1), (h * gy).sum(1)], 1)
        var = torch.stack([(h * gx * gx).sum(1), (h * gy * gy).sum(1)], 1) - co ** 2
        std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(1)
        outs.append(torch.cat([kc + co * (w // 2) * scale + w // 2, std[:, None]], 1))
    return outs[0], outs[1]


def fine_backward(win0, win1, mix0, mix1, scale, d_out0, d_out1):
    """(d_win0, d_win1, d_mix0, d_mix1) by the formula of fm_fine_match_backward, in the dtype of the inputs"""
    m, ww, c = win0.shape
    w = int(math.isqrt(ww))
    t = 1 / math.sqrt(c)
    gx, gy = (g.to(win0.dtype).to(win0.device) for g in grid(w))
    d_win = [torch.zeros_like(win0), torch.zeros_like(win1)]
    d_mix = [torch.zeros_like(mix0), torch.zeros_like(mix1)]
    wins, mixes, gs = (win0, win1), (mix0, mix1), (d_out0, d_out1)
    for d in range(2):
        wa, wb, mix, g = wins[d], wins[1 - d], mixes[d], gs[d]
        q = torch.einsum('r,mrc->mc', mix[:ww], wa) + mix[ww]
        h = torch.softmax(t * torch.einsum('mc,mrc->mr', q, wb), dim=1)
        co = [(h * gx).sum(1), (h * gy).sum(1)]
        var = [(h * gx * gx).sum(1) - co[0] ** 2, (h * gy * gy).sum(1) - co[1] ** 2]
        dvar = [torch.where(v >= 1e-10, g[:, 2] * 0.5 / torch.sqrt(v.clamp(min=1e-10)), torch.zeros_like(v)) for v in var]
        dco = [g[:, k] * (w // 2) * scale - 2 * co[k] * dvar[k] for k in range(2)]
        dh = (dco[0][:, None] * gx + dco[1][:, None] * gy + dvar[0][:, None] * gx ** 2 + dvar[1][:, None] * gy ** 2)
        ds = h * (dh - (h * dh).sum(1, keepdim=True))
        dq = t * torch.einsum('mr,mrc->mc', ds, wb)
        d_win[1 - d] += t * ds[:, :, None] * q[:, None, :]
        d_win[d] += mix[:ww][None, :, None] * dq[:, None, :]
        d_mix[d][:ww] += torch.einsum('mc,mrc->r', dq, wa)
        d_mix[d][ww] += dq.sum()
    return d_win[0], d_win[1], d_mix[0], d_mix[1]


def crop_adjoint(d_win, b_ids, ids, shape, w: int, stride: int, w_c: int, pad: int = 2):
    """(d_feat, reads) float64 [N, Cf, Hf, Wf] by index_add: the sum of d_win over every (match, window position) that
    read each pixel, and how many reads each pixel had"""
    n, cf, hf, wf = shape
    m = d_win.shape[0]
    b_ids, ids = b_ids.long().cpu(), ids.long().cpu()
    wy = torch.arange(w).repeat_interleave(w)
    wx = torch.arange(w).repeat(w)
    y = (ids // w_c)[:, None] * stride - pad + wy[None, :]
    x = (ids % w_c)[:, None] * stride - pad + wx[None, :]
    ok = (y >= 0) & (y < hf) & (x >= 0) & (x < wf)
    pix = (b_ids[:, None] * hf + y) * wf + x                     # [M, WW] flat (b, y, x)
    src = d_win.double().cpu().reshape(m, w * w, cf)[ok]         # [K, Cf]
    out = torch.zeros(n * hf * wf, cf, dtype=torch.float64).index_add_(0, pix[ok], src)
    reads = torch.zeros(n * hf * wf, dtype=torch.int64).index_add_(0, pix[ok], torch.ones_like(pix[ok]))
    return out.view(n, hf, wf, cf).permute(0, 3, 1, 2), reads.view(n, 1, hf, wf)
