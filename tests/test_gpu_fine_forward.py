"""The fine stage's forward (fine_core / soft_argmax2 of csrc/fine.hip, the helpers of fm_fine_device.h / fm_wave_device.h) on
every route that computes it - k_fine<5|7> on window tensors and the eight k_fine_maps instantiations behind
fm_fine_match_maps*, the NCHW routes through k_nchw_to_nhwc64 and the copy a coarse call prepared - against the float64
yardstick of tests/fine_grad_ref.py (pinned by tests/test_fine_ref.py).

Bars.  Nothing is a fixed tolerance: for every data set the error of torch's own float32 forward against float64 on the
very same inputs is measured on the CPU (e32: offsets in px, d0: variances), and the kernel - another summation order,
the hardware exponential - gets FINE_MULT = 4 times that plus FINE_FLOOR_ULPS = 4 float32 ulps of the offset range
W // 2 * scale (of 1 for the variances).  std is checked through the variance: it must lie in the interval
sum over the axes of sqrt(max(v -+ d, 1e-10)) around the float64 variances v, widened by two float32 ulps for the
rounding of the two square roots, their sum and of the constant 1e-10f itself.  The offsets are compared with
mkpts_c = 0, so the float32 add of a keypoint of some hundred px (4e-5 px by itself) hides nothing; the add has a test
of its own.  Lines starting with ACC are the record profiles/fine_forward_accuracy.txt is made of."""
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, ops

from fine_grad_ref import (F32_EPS, FINE_CAP_PX, FINE_GAINS, FINE_MULT, FINE_SCALE, crop_ref, fine_bars, fine_yardstick, flat_answer,
                           grid, known_mix, one_hot_windows, regime_inputs, std_interval, two_point_answer,
                           two_point_windows, unfold_grid)
from helpers import case_inputs, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
by_w = pytest.mark.parametrize("w", [5, 7])
STD_SLACK = 4 * F32_EPS             # two float32 ulps, relative


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _untouched(t):
    """still the NaN it was pre-filled with, bit for bit"""
    return _same_bits(t, torch.full_like(t, float("nan")))


def _count(k):
    return torch.tensor([k, 0], dtype=torch.int32, device=DEV)


def _stream():
    return ops._stream(torch.device(DEV))


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _fine(win0, win1, mix0, mix1, k0=None, k1=None, count=None, m_max=None, outs=None, scale=FINE_SCALE):
    """fm_fine_match straight through ctypes on device tensors, into outputs pre-filled with NaN unless given;
    mkpts_c = 0 unless given"""
    rows, ww, cf = win0.shape
    m_max = rows if m_max is None else m_max
    k0 = torch.zeros(rows, 2, device=DEV) if k0 is None else k0
    k1 = torch.zeros(rows, 2, device=DEV) if k1 is None else k1
    o0, o1 = (_nan(rows, 3), _nan(rows, 3)) if outs is None else outs
    st = _lib.load().fm_fine_match(ops._ptr(win0), ops._ptr(win1), m_max, ops._ptr(count), ww, cf, ops._ptr(mix0),
                                   ops._ptr(mix1), ops._ptr(k0), ops._ptr(k1), float(scale), ops._ptr(o0), ops._ptr(o1),
                                   _stream())
    torch.cuda.synchronize()
    assert st == 0, f"fm_fine_match: status {st}"
    return o0, o1


def _needed_d(std, var2):
    """the smallest variance error d (bisected) with which std [M] lies in std_interval(var2 [M, 2], d)"""
    def ok(d):
        lo, hi = std_interval(var2, d)
        return bool(((std >= lo * (1 - STD_SLACK)) & (std <= hi * (1 + STD_SLACK))).all())
    if ok(0.0):
        return 0.0
    lo, hi = 0.0, 4.0
    for _ in range(60):
        mid = (lo + hi) / 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def _check(tag, w, got, yard, mult=FINE_MULT, cap_off=None):
    """got = (out0, out1) of a run with mkpts_c = 0, yard = (off64 [M, 4], var64 [M, 4], e32, d0): offsets within the
    offset bar, std within the interval the variance bar allows; prints the record line first"""
    off64, var64, e32, d0 = yard
    bar_off, bar_var = fine_bars(w, e32, d0, mult=mult, cap_off=cap_off)
    g = torch.cat([got[0], got[1]], 1).double().cpu()
    assert torch.isfinite(g).all(), f"{tag}: not finite"
    err = (g[:, [0, 1, 3, 4]] - off64).abs().max().item()
    need = max(_needed_d(g[:, 2], var64[:, :2]), _needed_d(g[:, 5], var64[:, 2:]))
    print(f"ACC {tag}: e32 {e32:.2e} px, d0 {d0:.2e}; kernel: offsets {err:.2e} px (bar {bar_off:.2e}), "
          f"variance error implied by std {need:.2e} (bar {bar_var:.2e}); multiple {mult:g}")
    assert err <= bar_off, f"{tag}: offsets {err:.3e} px > {bar_off:.3e}"
    assert need <= bar_var, f"{tag}: std needs a variance error of {need:.3e} > {bar_var:.3e}"
    return err, need


# ------------------------------------------------------------------ a. k_fine by regime
@by_w
@pytest.mark.parametrize("gain", FINE_GAINS)
def test_k_fine_against_float64_by_regime(w, gain):
    """windows gain * N(0, 1), 2002 matches (no multiple of 4), 300 of them with win1 = 3 * win0, mkpts_c = 0.
    tests/test_fine_ref.py checks what the regimes hold: up to gain 1 no variance near the clamp, at gain 3 a few per
    cent of the heat maps sharp, at gain 10 most of them.  Up to gain 3 the offset bar is capped at 1e-4 px, a tenth of
    the older tests' bar"""
    win0, win1, mix0, mix1 = regime_inputs(w, gain)
    yard = fine_yardstick(win0, win1, mix0, mix1)
    got = _fine(*_dev(win0, win1, mix0, mix1))
    _check(f"k_fine W={w} gain={gain:g}", w, got, yard, cap_off=FINE_CAP_PX if gain <= 3 else None)


# ------------------------------------------------------------------ b. large logits
@by_w
@pytest.mark.parametrize("gain", [100.0, 1e4])
def test_large_logits_stay_finite_and_in_range(w, gain):
    """logits of 1e5 .. 1e9: without the max subtraction in heat_exp2 every exponential overflows.  No accuracy bar -
    torch's float32 forward is itself off by 2.5e-3 px at gain 100 - but the outputs are finite, every offset lies in
    the window and std between the clamp's 2e-5 and 2.83"""
    win0, win1, mix0, mix1 = regime_inputs(w, gain, m=1001)
    got = torch.cat(_fine(*_dev(win0, win1, mix0, mix1)), 1).cpu()
    assert torch.isfinite(got).all()
    wh = w // 2
    off, std = got[:, [0, 1, 3, 4]], got[:, [2, 5]]
    print(f"W={w} gain={gain:g}: offsets in [{off.min().item():.7f}, {off.max().item():.7f}], "
          f"std in [{std.min().item():.4e}, {std.max().item():.4f}]")
    assert off.min().item() >= wh - wh * FINE_SCALE and off.max().item() <= wh + wh * FINE_SCALE
    # (2e-5 as float32 arithmetic gives it: sqrtf(1e-10f) + sqrtf(1e-10f), the smallest std the kernel can write)
    clamp = np.sqrt(np.float32(1e-10)) + np.sqrt(np.float32(1e-10))
    assert std.min().item() >= float(clamp) and std.max().item() <= 2.83


# ------------------------------------------------------------------ c. known answers
def _ulps(got, want):
    """|got - want| in float32 ulps of want (float32 tensors)"""
    w64 = want.double().numpy()
    return np.abs(got.double().numpy() - w64) / np.spacing(np.abs(want.numpy())).astype(np.float64)


@by_w
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_one_hot_heat_map_at_every_position(w, direction):
    """match r is one-hot at window position r: offsets = the grid point, which pins tr_index, grid_xy and the x / y
    order; std = the clamp on both axes, exactly sqrtf(1e-10f) + sqrtf(1e-10f).

    The offsets are compared twice.  (1) With the float64 closed form, to one float32 ulp of the offset range
    W // 2 * scale: the offset is cx * (W // 2) * scale + W // 2 with cx a float32 in [-1, 1], and the rounding of cx
    alone (3e-8 at 2/3) moves it by 1.8e-7 px - more than an ulp of an offset near 1 - so the ulp of the range is the
    unit float32 can deliver; a grid constant wrong in the sixth digit still misses it by a factor of ten.  (2) With
    the closed form evaluated on the reference's own float32 grid, to one ulp of each offset.  That grid is restated
    here from the reference, not from fm_fine_device.h: kornia's create_meshgrid(normalized_coordinates=True), which
    the reference's fine matching calls, computes (linspace(0, W - 1, W) / (W - 1) - 0.5) * 2 in float32, rounding at
    every step (oracle/matcher_ref.py restates the same lines); grid_xy has to reproduce it, not the other way round"""
    ww, wh = w * w, w // 2
    win0, win1 = one_hot_windows(w, direction, torch.float32)
    mix = known_mix(ww, torch.float32)
    yard = fine_yardstick(win0, win1, mix, mix)
    got = _fine(*_dev(win0, win1, mix, mix))
    _check(f"k_fine W={w} one-hot, direction {'01b'[direction]}", w, got, yard)
    gx, gy = grid(w)
    want64 = torch.stack([gx, gy], 1) * wh * FINE_SCALE + wh
    t32 = (torch.arange(w, dtype=torch.float32) / (w - 1) - 0.5) * 2
    g32 = torch.stack([t32.repeat(w), t32.repeat_interleave(w)], 1)
    want_f32_grid = (g32.double() * wh * FINE_SCALE + wh).float()
    clamp = np.sqrt(np.float32(1e-10)) + np.sqrt(np.float32(1e-10))
    assert clamp.dtype == np.float32
    range_ulp = float(np.spacing(np.float32(wh * FINE_SCALE)))
    for d in range(2):
        if direction not in (d, 2):
            continue
        o = got[d].cpu()
        err = (o[:, :2].double() - want64).abs().max().item()
        u = _ulps(o[:, :2], want_f32_grid).max()
        exact = torch.equal(o[:, :2], want64.float())
        print(f"W={w} one-hot direction {d}: |offset - float64| {err:.3e} px = {err / range_ulp:.2f} ulp of "
              f"{wh * FINE_SCALE:g}; {u:.2f} ulp from the float32-grid closed form; equal to float32(float64): {exact}; "
              f"std bits {set(o[:, 2].view(torch.int32).tolist())} (clamp {clamp.view(np.int32)})")
        assert err <= range_ulp
        assert u <= 1.0
        assert (o[:, 2].numpy() == clamp).all(), "std is not sqrtf(1e-10f) + sqrtf(1e-10f)"


@by_w
def test_flat_and_two_point_heat_maps(w):
    """all-zero windows (any mix: every logit 0) and two equal logits of 320 against their closed forms, within the
    bars of the regime test (e32 / d0 of torch's float32 forward on these inputs, which are ~0: the floor decides)"""
    ww = w * w
    _, _, mix0, mix1 = regime_inputs(w, 1.0, m=1)
    zero = torch.zeros(37, ww, 64)
    _, _, e32, d0 = fine_yardstick(zero, zero, mix0, mix1)
    off, var = flat_answer(w, 37)
    _check(f"k_fine W={w} all-zero windows", w, _fine(*_dev(zero, zero, mix0, mix1)),
           (torch.cat([off, off], 1), torch.cat([var, var], 1), e32, d0))
    win0, win1, pairs = two_point_windows(w, torch.float32)
    mix = known_mix(ww, torch.float32)
    _, _, e32, d0 = fine_yardstick(win0, win1, mix, mix)
    off, var = two_point_answer(w, pairs, FINE_SCALE)
    _check(f"k_fine W={w} two-point heat maps", w, _fine(*_dev(win0, win1, mix, mix)),
           (torch.cat([off, off], 1), torch.cat([var, var], 1), e32, d0))


# ------------------------------------------------------------------ d. the keypoint add
def _add_ok(tag, with_k, k0, k1, without):
    """out(mkpts_c) = float32(mkpts_c) + out(mkpts_c = 0) evaluated in float32, to one ulp of the result; std the same
    bits.  Returns whether everything is bit-equal"""
    equal = True
    for o, k, z in zip(with_k, (k0, k1), without):
        o, z = o.cpu(), z.cpu()
        want = k.cpu().float() + z[:, :2]
        assert _ulps(o[:, :2], want).max() <= 1.0, f"{tag}: the keypoint add is off by more than an ulp"
        assert _same_bits(o[:, 2], z[:, 2]), f"{tag}: std depends on mkpts_c"
        equal = equal and _same_bits(o[:, :2], want)
    return equal


@by_w
def test_keypoint_add(w):
    win0, win1, mix0, mix1 = _dev(*regime_inputs(w, 1.0, m=601))
    g = torch.Generator().manual_seed(w)
    k0, k1 = _dev(5000 * torch.rand(601, 2, generator=g), 5000 * torch.rand(601, 2, generator=g))
    assert (k0 != k0.round()).any() and k0.max().item() > 4900
    equal = _add_ok(f"W={w}", _fine(win0, win1, mix0, mix1, k0, k1), k0, k1, _fine(win0, win1, mix0, mix1))
    print(f"W={w}: out(mkpts_c) bit-equal to float32(mkpts_c) + out(0): {equal}")


# ------------------------------------------------------------------ the maps routes
# route -> (element type of the maps, layout of the call: 0 NCHW, 1 channels-last, 2 NCHW with image 1's copy prepared)
ROUTES = {
    "nhwc_f32": (torch.float32, 1),         # k_fine_maps<W, false, F32>
    "nchw_f32": (torch.float32, 0),         # k_nchw_to_nhwc64<float>, k_fine_maps<W, true, F32>
    "prepared_f32": (torch.float32, 2),     # the copy fm_coarse_match_maps made, k_fine_maps<W, true, F32>
    "nhwc_f16": (torch.float16, 1),         # k_fine_maps<W, false, F16>
    "nchw_f16": (torch.float16, 0),         # k_nchw_to_nhwc64<unsigned short> twice, k_fine_maps<W, false, F16>
    "nhwc_bf16": (torch.bfloat16, 1),       # k_fine_maps<W, false, BF16>
    "nchw_bf16": (torch.bfloat16, 0),
}
N = 3


@functools.lru_cache(maxsize=None)
def _coarse_inputs():
    inp = case_inputs(load_golden("cfg1_peaky")['meta'], "peaky", with_fine=False)
    return torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV), inp['hw_c']


def _prepared(side):
    """the channels-last copy of `side` (NCHW float32 on the device) as a coarse call leaves it: the side job of
    fm_coarse_match_maps' assignment launch (its shape is independent of the coarse problem)"""
    t0, t1, hw_c = _coarse_inputs()
    buf = ops.coarse_match_async(t0, t1, hw_c, hw_c, 8.0, side_map=side)
    assert buf.read_count() > 0
    return buf.side_scratch


class Stores:
    """the device buffers of a pair of logical [N, 64, Hf, Wf] maps (CPU tensors of the route's element type) for
    `route`, and fm_fine_match_maps_dtype on them straight through ctypes"""

    def __init__(self, f0, f1, route):
        dtype, self.layout = ROUTES[route]
        assert f0.dtype == dtype and f1.dtype == dtype
        self.dt = ops._DTYPES[dtype]
        self.shape = (f0.shape[0], 64, *f0.shape[2:], *f1.shape[2:])
        put = (lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)) if self.layout == 1 else (lambda t: t.contiguous().to(DEV))
        self.s0, self.s1 = put(f0), put(f1)
        self.scratch = None
        if self.layout == 2:
            self.scratch = _prepared(self.s1)
        elif self.layout == 0:
            need = int(_lib.load().fm_fine_maps_scratch_bytes_dtype(*self.shape, 0, self.dt))
            assert need > 0
            self.scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run(self, w, stride, pad, w0c, w1c, b, i, j, mix0, mix1, k0, k1, count=None, m_max=None, outs=None):
        rows = b.shape[0]
        m_max = rows if m_max is None else m_max
        o0, o1 = (_nan(rows, 3), _nan(rows, 3)) if outs is None else outs
        n, cf, hf0, wf0, hf1, wf1 = self.shape
        st = _lib.load().fm_fine_match_maps_dtype(
            ops._ptr(self.s0), ops._ptr(self.s1), self.dt, self.layout, n, cf, hf0, wf0, hf1, wf1, w, stride, pad, w0c, w1c,
            ops._ptr(b), ops._ptr(i), ops._ptr(j), ops._ptr(count), m_max, ops._ptr(mix0), ops._ptr(mix1), ops._ptr(k0),
            ops._ptr(k1), float(FINE_SCALE), ops._ptr(self.scratch), ops._ptr(o0), ops._ptr(o1), _stream())
        torch.cuda.synchronize()
        assert st == 0, f"fm_fine_match_maps_dtype: status {st}"
        return o0, o1


# (stride, pad, (Hf0, Wf0), (Hf1, Wf1), extra rows / columns of the coarse grid beyond unfold's own, sorted b_ids):
# every stride of {1, 2, 3, 4, 8} and pad of {0, 2, 3, 7}, pad > stride, the two images different in height, width and
# grid width, widths around the transpose's 64-pixel tile, grids that overhang the map (windows wholly in the padding;
# with pad 7 the corner windows of W = 5 are wholly outside as well)
GEOMETRY = [
    (4, 2, (36, 40), (44, 64), 0, True),            # the shipped geometry as the anchor
    (1, 0, (20, 65), (17, 40), 0, True),            # stride 1, no padding: no negative origin, windows overlap
    (2, 3, (30, 64), (25, 130), 0, True),           # pad > stride
    (3, 7, (22, 130), (31, 65), 0, False),          # a stride that does not divide anything; unsorted b_ids
    (8, 2, (40, 65), (33, 40), 2, True),            # stride > W: pixels between the windows; the grid overhangs
    (4, 3, (19, 40), (28, 130), 3, True),           # overhang with a pad other than 2
    (2, 0, (26, 130), (30, 64), 4, True),
    (8, 7, (35, 64), (41, 65), 2, False),
    (1, 7, (12, 40), (14, 65), 0, True),            # pad 7 at stride 1: whole rows of cells in the padding
]
GEO_IDS = [f"s{g[0]}-p{g[1]}-{g[2][0]}x{g[2][1]}-{g[3][0]}x{g[3][1]}{'-overhang' if g[4] else ''}{'' if g[5] else '-unsorted'}"
           for g in GEOMETRY]


def _cells(seed, h_c, w_c, m):
    """m random cells, then the four corners and a cell on each border"""
    g = torch.Generator().manual_seed(seed)
    cells = h_c * w_c
    border = torch.tensor([0, w_c - 1, (h_c - 1) * w_c, cells - 1, w_c // 2, (h_c // 2) * w_c, (h_c // 2) * w_c + w_c - 1,
                           (h_c - 1) * w_c + w_c // 2])
    return torch.cat([torch.randint(cells, (m,), generator=g), border, border.flip(0)])


def _match_list(seed, grid0, grid1, m, sorted_b):
    """(b, i, j) int64: i and j hit every corner and border of their grids (in different rows of the list, so corner
    meets interior too); b_ids sorted as the coarse stage leaves them, or shuffled"""
    i = _cells(seed, *grid0, m)
    j = _cells(seed + 1, *grid1, m).roll(5)
    g = torch.Generator().manual_seed(seed + 2)
    b = torch.randint(N, (i.shape[0],), generator=g)
    b = torch.sort(b).values if sorted_b else b
    assert sorted_b or not torch.equal(b, torch.sort(b).values)
    return b, i, j


def _geometry(w, geo, seed):
    stride, pad, hw0, hw1, extra, sorted_b = geo
    grid0 = tuple(v + extra for v in unfold_grid(*hw0, w, stride, pad))
    grid1 = tuple(v + extra + 1 for v in unfold_grid(*hw1, w, stride, pad)) if extra else unfold_grid(*hw1, w, stride, pad)
    b, i, j = _match_list(seed, grid0, grid1, 250, sorted_b)
    g = torch.Generator().manual_seed(seed + 7)
    mix0, mix1 = ((2 * torch.rand(w * w + 1, generator=g) - 1) / w for _ in range(2))
    # keypoints as the coarse stage would give them (cell * 8), plus a fraction
    k0 = torch.stack([i % grid0[1], i // grid0[1]], 1).float() * 8 + 0.375
    k1 = torch.stack([j % grid1[1], j // grid1[1]], 1).float() * 8 + 0.625
    return stride, pad, hw0, hw1, grid0, grid1, b, i, j, mix0, mix1, k0, k1


def _maps(seed, hw0, hw1, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 64, *hw0, generator=g).to(dtype), torch.randn(N, 64, *hw1, generator=g).to(dtype)


# ------------------------------------------------------------------ e. every maps route at general geometry
@pytest.mark.parametrize("geo", GEOMETRY, ids=GEO_IDS)
@by_w
def test_maps_routes_at_general_geometry(w, geo):
    """Per element type: the windows are crop_ref's (index arithmetic, pinned against F.unfold) of the map up-cast
    exactly; fm_gather_windows* + fm_fine_match on the device give them bit for bit and a result within the bars of
    the regime test of the float64 yardstick on them; every maps route of that type - and the float32 routes on the
    up-cast of a half-precision map - then gives that result bit for bit, with the keypoints added"""
    stride, pad, hw0, hw1, grid0, grid1, b, i, j, mix0, mix1, k0, k1 = _geometry(w, geo, 40 + w)
    bd, idev, jd, m0d, m1d, k0d, k1d = _dev(b, i, j, mix0, mix1, k0, k1)
    tag = GEO_IDS[GEOMETRY.index(geo)]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        f0, f1 = _maps(3, hw0, hw1, dtype)
        win0 = crop_ref(f0.float(), b, i, w, stride, pad, grid0[1])
        win1 = crop_ref(f1.float(), b, j, w, stride, pad, grid1[1])
        if geo[4]:
            assert (win0.abs().amax((1, 2)) == 0).any() and (win1.abs().amax((1, 2)) == 0).any(), "no window wholly outside"
        yard = fine_yardstick(win0, win1, mix0, mix1)
        # the crop path: list kernels (float32) / generic kernels (half precision), then k_fine
        d0 = ops.gather_windows(f0.to(DEV), bd, idev, w, stride, grid0[1], pad=pad)
        d1 = ops.gather_windows(f1.to(DEV), bd, jd, w, stride, grid1[1], pad=pad)
        assert _same_bits(d0, win0) and _same_bits(d1, win1)
        plain = _fine(d0, d1, m0d, m1d)
        name = str(dtype).split('.')[1]
        _check(f"crop + k_fine W={w} {tag} {name}", w, plain, yard)
        with_k = _fine(d0, d1, m0d, m1d, k0d, k1d)
        _add_ok(f"{tag} {name}", with_k, k0d, k1d, plain)
        runs = [(r, f0, f1) for r, (dt, _) in ROUTES.items() if dt == dtype]
        if dtype != torch.float32:          # a half type and its up-cast: the float32 routes on the exact up-cast
            runs += [(r, f0.float(), f1.float()) for r in ("nhwc_f32", "nchw_f32")]
        for route, a0, a1 in runs:
            got = Stores(a0, a1, route).run(w, stride, pad, grid0[1], grid1[1], bd, idev, jd, m0d, m1d, k0d, k1d)
            for g_, r_ in zip(got, with_k):
                assert _same_bits(g_, r_), f"{tag} {name} {route}: differs from fm_gather_windows + fm_fine_match"
        # ... and with mkpts_c = 0 one route per type against float64 directly (the record's line of the maps kernels)
        z = torch.zeros_like(k0d)
        route = runs[0][0]
        _check(f"{route} W={w} {tag}", w, Stores(f0, f1, route).run(w, stride, pad, grid0[1], grid1[1], bd, idev, jd, m0d,
                                                                      m1d, z, z), yard)


# ------------------------------------------------------------------ f. counts
# (Not covered here: fm_fine_match_maps_dtype caps its grid at 2^20 workgroups - above 4 M matches, or with the
# tuning build's FM_FINE_GRID - and k_fine_maps then walks the list in grid strides, where `m >= M` ends the loop.
# With at most 257 rows every launch takes one window per wave; the strided walk is exercised by no test of this file.)
COUNT_M = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 257)


def _check_counts(run, rows):
    """run(m_max, count or None, outs) on a list of `rows` matches.  Rows at or beyond min(*d_count, m_max) keep the NaN
    they were pre-filled with bit for bit, the rows before equal the full-list run's.  Per M of COUNT_M the count comes
    from m_max alone (d_count = NULL), from a device count above m_max, from a device count below an m_max of the whole
    list; and *d_count = 0 writes nothing"""
    full = (_nan(rows, 3), _nan(rows, 3))
    run(rows, None, full)
    assert all(torch.isfinite(t).all() for t in full)

    def expect(m_max, count, live, what):
        outs = (_nan(rows, 3), _nan(rows, 3))
        run(m_max, count, outs)
        for o, f in zip(outs, full):
            assert _same_bits(o[:live], f[:live]), f"{what}: counted rows differ from the full list's"
            assert _untouched(o[live:]), f"{what}: a row at or beyond the count was written"

    for m in COUNT_M:
        assert m <= rows
        expect(m, None, m, f"m_max {m}, d_count NULL")
        expect(m, _count(m + 1000), m, f"m_max {m}, *d_count {m + 1000}")
        expect(rows, _count(m), m, f"m_max {rows}, *d_count {m}")
        expect(m, _count(0), 0, f"m_max {m}, *d_count 0")
    expect(rows, _count(0), 0, f"m_max {rows}, *d_count 0")


@by_w
def test_counts_on_fine_match(w):
    win0, win1, mix0, mix1 = _dev(*regime_inputs(w, 1.0, m=257))
    k = torch.arange(514, dtype=torch.float32, device=DEV).view(257, 2)

    def run(m_max, count, outs):
        _fine(win0, win1, mix0, mix1, k, k + 0.5, count=count, m_max=m_max, outs=outs)
    _check_counts(run, 257)


@pytest.mark.parametrize("route", list(ROUTES))
@by_w
def test_counts_on_the_maps_routes(w, route):
    geo = GEOMETRY[0]
    stride, pad, hw0, hw1, grid0, grid1, b, i, j, mix0, mix1, k0, k1 = _geometry(w, geo, 90 + w)
    rows = 257
    args = _dev(b[:rows], i[:rows], j[:rows], mix0, mix1, k0[:rows], k1[:rows])
    stores = Stores(*_maps(5, hw0, hw1, ROUTES[route][0]), route)

    def run(m_max, count, outs):
        stores.run(w, stride, pad, grid0[1], grid1[1], *args, count=count, m_max=m_max, outs=outs)
    _check_counts(run, rows)
