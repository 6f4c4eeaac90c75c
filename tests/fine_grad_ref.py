"""float64 restatements of the fine stage (fine_matching_new.py:50-79) and of the backward formula the HIP kernels
implement (include/fmatch.h, fm_fine_match_backward): the yardsticks of tests/test_fine_grad_abi.py,
tests/test_gpu_fine_grad.py and tests/test_gpu_fine_backward.py."""
import math

import torch


def grid(w: int, dtype=torch.float64):
    """(gx, gy) [W*W] of kornia's normalised meshgrid, position r = wy * W + wx"""
    t = torch.arange(w, dtype=dtype) / (w - 1) * 2 - 1
    return t.repeat(w), t.repeat_interleave(w)


def fine_forward(win0, win1, mix0, mix1, mkpts0_c, mkpts1_c, scale):
    """(out0, out1) [M, 3] = (x, y, std) in the dtype of the inputs; mix = [WW + 1] (weights, then bias).
    fine_forward_parts below repeats this body line for line (tests/test_fine_ref.py holds the two to torch.equal):
    an edit here belongs there too"""
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


def fine_forward_parts(win0, win1, mix0, mix1, mkpts0_c, mkpts1_c, scale):
    """fine_forward, plus what the keypoint add and the clamp hide: (out0, out1, off0, off1, var0, var1) with
    off_d [M, 2] = co * (W // 2) * scale + W // 2 (the offsets before mkpts_c is added) and var_d [M, 2] = the (x, y)
    variances of the heat map before clamp(min=1e-10); out_d is fine_forward's, operation for operation.  The dtype
    follows the inputs"""
    m, ww, c = win0.shape
    w = int(math.isqrt(ww))
    gx, gy = (g.to(win0.dtype).to(win0.device) for g in grid(w))
    outs, offs, vars_ = [], [], []
    for wa, wb, mix, kc in ((win0, win1, mix0, mkpts0_c), (win1, win0, mix1, mkpts1_c)):
        q = torch.einsum('r,mrc->mc', mix[:ww], wa) + mix[ww]
        h = torch.softmax(torch.einsum('mc,mrc->mr', q, wb) / math.sqrt(c), dim=1)
        co = torch.stack([(h * gx).sum(1), (h * gy).sum(1)], 1)
        var = torch.stack([(h * gx * gx).sum(1), (h * gy * gy).sum(1)], 1) - co ** 2
        std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(1)
        outs.append(torch.cat([kc + co * (w // 2) * scale + w // 2, std[:, None]], 1))
        offs.append(co * (w // 2) * scale + w // 2)
        vars_.append(var)
    return outs[0], outs[1], offs[0], offs[1], vars_[0], vars_[1]


# ---- inputs with known answers (tests/test_fine_ref.py pins them on the yardstick, tests/test_gpu_fine_forward.py
# runs them on the device).  All of them: mix weights 0, bias 1, so q = 1 in every channel and the logit of window
# position r is sum_c win_other[r, c] / 8.
def known_mix(ww: int, dtype=torch.float64):
    mix = torch.zeros(ww + 1, dtype=dtype)
    mix[ww] = 1
    return mix


def one_hot_windows(w: int, direction: int, dtype=torch.float64):
    """(win0, win1) [WW, WW, 64]: match r has a heat map of `direction` that is one-hot at window position r (the window
    that direction correlates against is 40 at position r in every channel: logit 320 there, 0 elsewhere; exp(-320)
    is 0 in float32 and 1e-139 in float64).  The other window is zero, so the other direction's heat map is flat;
    direction 2: both windows are the hot one, both heat maps one-hot at r"""
    ww = w * w
    hot = torch.zeros(ww, ww, 64, dtype=dtype)
    hot[torch.arange(ww), torch.arange(ww)] = 40
    zero = torch.zeros(ww, ww, 64, dtype=dtype)
    if direction == 2:
        return hot, hot.clone()
    return (zero, hot) if direction == 0 else (hot, zero)     # direction 0 reads its heat map off win1


def two_point_windows(w: int, dtype=torch.float64):
    """(win0, win1, pairs): match k has the same window on both sides, 40 at the two positions pairs[k] = (r, s) in
    every channel: both directions' heat maps are 1/2 at r and at s (everything else exp(-320))"""
    ww = w * w
    g = torch.Generator().manual_seed(w)
    r = torch.arange(ww)
    s = (r + 1 + torch.randint(ww - 1, (ww,), generator=g)) % ww          # any other position
    win = torch.zeros(ww, ww, 64, dtype=dtype)
    win[r, r] = 40
    win[r, s] = 40
    return win, win.clone(), torch.stack([r, s], 1)


def two_point_answer(w: int, pairs, scale: float):
    """(off [K, 2], var [K, 2]) float64: the closed form for a heat map that is 1/2 at each of the two positions
    pairs[k] - the mean of the two grid points, and per axis the square of half their distance"""
    g = torch.stack(grid(w), 1)                                        # [WW, 2]
    a, b = g[pairs[:, 0]], g[pairs[:, 1]]
    return (a + b) / 2 * (w // 2) * scale + w // 2, ((a - b) / 2) ** 2


def flat_answer(w: int, k: int):
    """(off [K, 2], var [K, 2]) float64 of a flat heat map: the window centre, and the mean of the squared grid"""
    gx, _ = grid(w)
    return torch.full((k, 2), float(w // 2), dtype=torch.float64), torch.full((k, 2), (gx ** 2).mean().item(),
                                                                             dtype=torch.float64)


# ---- the regimes of the fine forward's accuracy test: windows gain * N(0, 1)
FINE_GAINS = (0.0, 0.02, 0.3, 1.0, 3.0, 10.0)
FINE_M = 2002           # >= 2000, no multiple of 4 (k_fine runs four matches per workgroup)
FINE_TIED = 300         # the first rows have win1 = 3 * win0 (the recipe of test_fine_match_vs_oracle)
FINE_SCALE = 2.0


def regime_inputs(w: int, gain: float, m: int = FINE_M, tied: int = FINE_TIED):
    """(win0, win1, mix0, mix1) float32 on the CPU, seeded by (W, gain): windows gain * N(0, 1), the first `tied`
    rows with win1 = 3 * win0, mix = [WW + 1] uniform in +-1/sqrt(WW) (torch's init range of Linear(WW, 1)).
    tests/test_fine_ref.py holds the bits of the default call to a digest"""
    ww = w * w
    g = torch.Generator().manual_seed(1000 * w + int(round(gain * 100)))
    win0 = gain * torch.randn(m, ww, 64, generator=g)
    win1 = gain * torch.randn(m, ww, 64, generator=g)
    win1[:tied] = 3 * win0[:tied]
    mix0, mix1 = ((2 * torch.rand(ww + 1, generator=g) - 1) / math.sqrt(ww) for _ in range(2))
    return win0, win1, mix0, mix1


def fine_yardstick(win0, win1, mix0, mix1, scale=FINE_SCALE):
    """(off64 [M, 4], var64 [M, 4], e32, d0) of float32 inputs with mkpts_c = 0: the float64 offsets and variances
    (columns: direction 0 x, y, direction 1 x, y) and the errors of torch's float32 fine_forward_parts on the very same
    inputs against them - e32 = its largest offset error (px), d0 = its largest variance error.  Nothing here comes
    from a kernel"""
    z = torch.zeros(win0.shape[0], 2)
    p64 = fine_forward_parts(win0.double(), win1.double(), mix0.double(), mix1.double(), z.double(), z.double(), scale)
    p32 = fine_forward_parts(win0, win1, mix0, mix1, z, z, scale)
    off64, var64 = torch.cat(p64[2:4], 1), torch.cat(p64[4:6], 1)
    e32 = (torch.cat(p32[2:4], 1).double() - off64).abs().max().item()
    d0 = (torch.cat(p32[4:6], 1).double() - var64).abs().max().item()
    return off64, var64, e32, d0


# the float32 kernel sums in another order and uses the hardware exponential: FINE_MULT times the error of torch's own
# float32 forward, plus a floor of FINE_FLOOR_ULPS float32 ulps of the offset range W // 2 * scale (offsets) and of 1
# (variances: sums of heat * g^2 <= 1)
FINE_MULT = 4.0
FINE_FLOOR_ULPS = 4
F32_EPS = 2.0 ** -23


FINE_CAP_PX = 1e-4        # up to gain 3 the offset bar never exceeds a tenth of the older tests' 1e-3 px


def fine_bars(w: int, e32: float, d0: float, scale=FINE_SCALE, mult=FINE_MULT, cap_off=None):
    """(offset bar in px, variance bar); cap_off: an upper limit of the offset bar (e32 is a float32 sum on the CPU and
    moves with the number of threads torch sums with: the cap keeps the bar where the regime test promises it)"""
    bar_off = mult * e32 + FINE_FLOOR_ULPS * F32_EPS * (w // 2) * scale
    return (bar_off if cap_off is None else min(bar_off, cap_off)), mult * d0 + FINE_FLOOR_ULPS * F32_EPS


def std_interval(var64, d):
    """[M, 2] -> (lo, hi) [M]: the std a forward may give whose variances are within d of var64, sum over the axes of
    sqrt(max(v -+ d, 1e-10))"""
    lo = torch.sqrt(torch.clamp(var64 - d, min=1e-10)).sum(1)
    hi = torch.sqrt(torch.clamp(var64 + d, min=1e-10)).sum(1)
    return lo, hi


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


# ---- the cases of the fine backward's accuracy test (tests/test_gpu_fine_backward.py runs them on the device,
# tests/test_fine_ref.py asserts from the CPU what that file assumes about them).  A case is (W, gain, target, M):
# regime_inputs(W, gain, m=M, tied=M // 2), so a small M holds tied and free rows, and a d_out seeded by (W, M).
BWD_TARGETS = ("xy", "std", "all")      # d_out with std column 0 / with x, y columns 0 / all three columns non-zero
BWD_GAINS = (0.02, 0.3, 1.0)
BWD_M = 600
# scale_f per (W, gain): each of 1, 2, 4 meets every target, as the targets are crossed with (W, gain)
BWD_SCALE = {(5, 0.02): 1.0, (5, 0.3): 2.0, (5, 1.0): 4.0, (7, 0.02): 2.0, (7, 0.3): 4.0, (7, 1.0): 1.0}
BWD_REGULAR = [(w, gain, target, BWD_M) for w in (5, 7) for gain in BWD_GAINS for target in BWD_TARGETS]
# either side of the four matches of a workgroup of k_fine_bwd, of a wave and of the 256-match stride of
# k_fine_mix_reduce, two and four strides
BWD_EDGE_M = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 1025)
BWD_EDGES = [(w, 0.3, "all", m) for w in (5, 7) for m in BWD_EDGE_M]
BWD_NAMES = ("d_win0", "d_win1", "d_mix0", "d_mix1")
# twice the largest e32_m / top_m of torch's float32 autograd over BWD_REGULAR (4.90e-6: W = 5, gain 1.0, std, d_win1),
# measured on the CPU by tests/test_fine_ref.py: profiles/fine_backward_accuracy.txt
BWD_FLOOR = 2 * 4.90e-6


def backward_d_out(w: int, m: int, target: str):
    """(d_out0, d_out1) float32 [M, 3] = N(0, 1), seeded by (W, M); the columns the target leaves out are zero"""
    g = torch.Generator().manual_seed(77 * w + m)
    d = [torch.randn(m, 3, generator=g), torch.randn(m, 3, generator=g)]
    for t in d:
        if target == "xy":
            t[:, 2] = 0
        elif target == "std":
            t[:, :2] = 0
        else:
            assert target == "all" and (t != 0).all()
    return d[0], d[1]


def backward_inputs(w: int, gain: float, target: str, m: int):
    """(win0, win1, mix0, mix1, d_out0, d_out1, scale_f) of a case, float32 on the CPU"""
    return (*regime_inputs(w, gain, m=m, tied=m // 2), *backward_d_out(w, m, target), BWD_SCALE.get((w, gain), FINE_SCALE))


def backward_autograd(win0, win1, mix0, mix1, d_out0, d_out1, scale, dtype, fn=fine_forward, device="cpu"):
    """[d_win0, d_win1, d_mix0, d_mix1] of fn (fine_forward, or a drop-in for it) under autograd in `dtype` on
    `device`, mkpts_c = 0, in the leaves' dtype"""
    leaves = [t.detach().to(device, dtype).clone().requires_grad_(True) for t in (win0, win1, mix0, mix1)]
    z = torch.zeros(win0.shape[0], 2, device=device, dtype=dtype)
    outs = fn(*leaves, z, z, scale)
    return list(torch.autograd.grad(outs, leaves, [d_out0.to(device, dtype), d_out1.to(device, dtype)]))


def backward_yardstick(w: int, gain: float, target: str, m: int):
    """(g64, g32, var64 [M, 4], var_bar) of a case: the gradients of fine_forward under float64 and under float32
    autograd on the CPU (both as float64 tensors), the float64 variances and the variance bar of fine_bars (mult * d0
    + 4 ulp, d0 = the float32 forward's own largest variance error on this case) that tests/test_gpu_fine_forward.py
    holds the kernel's variances within - 0 for target xy, whose gradient does not pass through a variance.  Nothing
    here comes from a kernel"""
    inp = backward_inputs(w, gain, target, m)
    g64 = backward_autograd(*inp, torch.float64)
    g32 = [t.double() for t in backward_autograd(*inp, torch.float32)]
    _, var64, e32, d0 = fine_yardstick(*inp[:4], scale=inp[6])
    return g64, g32, var64, (0.0 if target == "xy" else fine_bars(w, e32, d0, scale=inp[6])[1])


def backward_bars(g64, g32, var64, var_bar, floor=BWD_FLOOR, mult=FINE_MULT):
    """(bar, top, e32) [M] per match of a window gradient [M, WW, C]:
        bar_m = mult * e32_m + (floor + COND_m) * top_m,  top_m = max |g64[m]|,  e32_m = max |g32[m] - g64[m]|
    COND_m = var_bar / (2 vmin_m), vmin_m = the smallest of match m's four float64 variances: the kernel's variances
    are within var_bar of float64 and d sqrt(var) = g / (2 sqrt(var)) inherits half their relative error.  var_bar = 0
    (target xy: no std gradient) leaves COND out"""
    top = g64.abs().flatten(1).amax(1)
    e32 = (g32 - g64).abs().flatten(1).amax(1)
    cond = var_bar / (2 * var64.amin(1))
    return mult * e32 + (floor + cond) * top, top, e32


def backward_mix_bars(g64, g32, var64, var_bar, floor=BWD_FLOOR, mult=FINE_MULT):
    """(bar, top, e32) per entry of a mix gradient [WW + 1]: the same form with top = max |g64| over the tensor (a
    scalar), e32 per entry and COND at the smallest variance of the case"""
    top = g64.abs().max()
    e32 = (g32 - g64).abs()
    cond = var_bar / (2 * var64.min())
    return mult * e32 + (floor + cond) * top, top, e32


def backward_excess(name, got, g64, g32, var64, var_bar):
    """(|got - g64| per match or per entry, its bar, e32) of tensor `name` of BWD_NAMES; got as float64 on the CPU"""
    bars = backward_bars if name.startswith("d_win") else backward_mix_bars
    bar, _, e32 = bars(g64, g32, var64, var_bar)
    err = (got - g64).abs()
    return (err.flatten(1).amax(1) if name.startswith("d_win") else err), bar, e32


# (Cf, W, stride, pad) of the general crop tests (tests/test_crop_ref.py pins the yardsticks at these,
# tests/test_gpu_crop_general.py runs the kernels at them), on a 2 x Cf x 37 x 45 map
CROP_CASES = [
    (64, 7, 4, 2),      # the fast paths, as the anchor
    (64, 7, 4, 3),      # fast kernels with a pad other than 2
    (64, 5, 2, 2),      # fast kernels, overlapping windows: three covering cells per axis in the backward
    (32, 3, 2, 1),      # Cf < 64: idle lanes of the backward's wave
    (20, 9, 8, 4),      # ... a large stride under a large window
    (20, 3, 8, 1),      # ... windows narrower than the stride: pixels between the windows
    (65, 7, 4, 2),      # k_crop_bwd<2>: the first channel past a wave
    (96, 7, 1, 3),      # ... stride 1: 49 covering cells
    (128, 7, 4, 3),
    (130, 5, 4, 0),     # k_crop_bwd<4>; pad 0: no negative origin
    (200, 7, 3, 2),     # ... a stride that does not divide W
    (256, 5, 2, 2),
    (260, 3, 1, 1),     # k_crop_bwd<8>
    (512, 3, 1, 1),     # ... the ABI's upper Cf
    (6, 15, 4, 7),      # the ABI's upper W; Cf not a multiple of 4: NCHW only in the forward
    (64, 15, 4, 7),     # the largest NCHW tile of the generic crop that fits the LDS (58 500 bytes)
    (1, 1, 1, 0),       # degenerate sizes
]
CROP_MAP = (2, 37, 45)  # N, Hf, Wf: odd on purpose, Wf no multiple of the backward's 64 / 32 / 16 / 8 pixel tiles


def unfold_grid(hf: int, wf: int, w: int, stride: int, pad: int):
    """(h_c, w_c) of F.unfold(kernel_size=w, stride=stride, padding=pad) on an hf x wf map"""
    return (hf + 2 * pad - w) // stride + 1, (wf + 2 * pad - w) // stride + 1


def crop_unfold(feat, b_ids, ids, w: int, stride: int, pad: int, h_c: int, w_c: int):
    """[M, W*W, Cf]: the crop through torch's own unfold (differentiable; the float32 autograd route the backward's
    tolerance is measured with).  The map is zero-padded by `pad` on the top / left and by whatever the h_c x w_c grid
    needs on the bottom / right, so a grid that overhangs the map is served too"""
    n, cf, hf, wf = feat.shape
    pb = max(0, (h_c - 1) * stride + w - hf - pad)
    pr = max(0, (w_c - 1) * stride + w - wf - pad)
    big = torch.nn.functional.pad(feat, (pad, pr, pad, pb))
    w_u = (big.shape[3] - w) // stride + 1                      # unfold's own grid width (>= w_c)
    u = torch.nn.functional.unfold(big, kernel_size=w, stride=stride)       # [N, Cf*WW, L], rows c * WW + r
    u = u.view(n, cf, w * w, -1).permute(0, 3, 2, 1)
    b_ids, ids = b_ids.long(), ids.long()
    return u[b_ids, (ids // w_c) * w_u + ids % w_c]


def crop_ref(feat, b_ids, ids, w: int, stride: int, pad: int, w_c: int):
    """[M, W*W, Cf] in feat's dtype: the window crop by plain index arithmetic, y = (id // w_c) * stride - pad + wy,
    x = (id % w_c) * stride - pad + wx, position wy * W + wx, zero outside the map.  Any pad, any grid: nothing assumes
    that the coarse grid times the stride equals the map"""
    feat = feat.cpu()
    n, cf, hf, wf = feat.shape
    b_ids, ids = b_ids.long().cpu(), ids.long().cpu()
    wy = torch.arange(w).repeat_interleave(w)
    wx = torch.arange(w).repeat(w)
    y = (ids // w_c)[:, None] * stride - pad + wy[None, :]
    x = (ids % w_c)[:, None] * stride - pad + wx[None, :]
    ok = (y >= 0) & (y < hf) & (x >= 0) & (x < wf)
    pix = (b_ids[:, None] * hf + y) * wf + x                     # [M, WW] flat (b, y, x)
    rows = feat.permute(0, 2, 3, 1).reshape(n * hf * wf, cf)
    out = torch.zeros(ids.shape[0], w * w, cf, dtype=feat.dtype)
    out[ok] = rows[pix[ok]]
    return out


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
