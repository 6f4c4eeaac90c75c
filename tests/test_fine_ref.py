"""The yardstick of the fine forward tests (tests/fine_grad_ref.py: fine_forward, fine_forward_parts) on the CPU: in
float32 it is the oracle's fine_match (the restatement the golden fixtures pin) to float32 rounding, in float64 it gives
the closed-form answers of one-hot, flat and two-point heat maps, and the seeded regimes tests/test_gpu_fine_forward.py
runs populate both sides of the variance clamp as that file assumes."""
import math

import pytest
import torch

from oracle import matcher_ref as orc

from fine_grad_ref import (F32_EPS, FINE_CAP_PX, FINE_GAINS, FINE_M, FINE_SCALE, FINE_TIED, fine_bars, fine_forward,
                           fine_forward_parts, fine_yardstick, flat_answer, grid, known_mix, one_hot_windows, regime_inputs,
                           std_interval, two_point_answer, two_point_windows)

by_w = pytest.mark.parametrize("w", [5, 7])


@by_w
@pytest.mark.parametrize("kmax", [0.0, 600.0])
def test_float32_yardstick_equals_the_oracle(w, kmax):
    """fine_forward in float32 and oracle.matcher_ref.fine_match are two float32 evaluations of one function: each is
    measured against float64 on the same inputs, and they differ from each other by no more than twice the larger of
    those two errors (with a floor of two float32 ulps of the largest output)"""
    win0, win1, mix0, mix1 = regime_inputs(w, 1.0, m=600)
    ww = w * w
    g = torch.Generator().manual_seed(w)
    k0, k1 = kmax * torch.rand(600, 2, generator=g), kmax * torch.rand(600, 2, generator=g)
    a = torch.cat(fine_forward(win0, win1, mix0, mix1, k0, k1, FINE_SCALE), 1).double()
    b = torch.cat(orc.fine_match(win0, win1, mix0[:ww], mix0[ww], mix1[:ww], mix1[ww], k0, k1, FINE_SCALE), 1).double()
    r = torch.cat(fine_forward(*(t.double() for t in (win0, win1, mix0, mix1, k0, k1)), FINE_SCALE), 1)
    ea, eb, diff = (a - r).abs().max().item(), (b - r).abs().max().item(), (a - b).abs().max().item()
    floor = 2 * F32_EPS * r.abs().max().item()
    print(f"W={w} mkpts_c <= {kmax}: |fine_forward f32 - f64| {ea:.2e}, |oracle - f64| {eb:.2e}, "
          f"|fine_forward f32 - oracle| {diff:.2e}, floor {floor:.2e}")
    assert diff <= max(2 * max(ea, eb), floor)
    assert max(ea, eb) <= 64 * F32_EPS * r.abs().max().item()          # both are float32-accurate at all
    # the variant with the parts returns fine_forward's outputs, operation for operation
    p = fine_forward_parts(win0, win1, mix0, mix1, k0, k1, FINE_SCALE)
    f = fine_forward(win0, win1, mix0, mix1, k0, k1, FINE_SCALE)
    assert torch.equal(p[0], f[0]) and torch.equal(p[1], f[1])
    assert p[0].dtype == torch.float32 and p[2].dtype == torch.float32 and p[4].dtype == torch.float32
    # ... and its parts are what the outputs are made of (fine_forward adds mkpts_c before W // 2: with keypoints the
    # sum of the parts rounds differently)
    if kmax == 0:
        assert torch.equal(p[2], f[0][:, :2]) and torch.equal(p[3], f[1][:, :2])
    assert torch.equal(torch.sqrt(torch.clamp(p[4], min=1e-10)).sum(1), f[0][:, 2])
    assert torch.equal(torch.sqrt(torch.clamp(p[5], min=1e-10)).sum(1), f[1][:, 2])


def _flat_std(w):
    return 2 * math.sqrt(flat_answer(w, 1)[1][0, 0].item())


@by_w
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_one_hot_heat_map_at_every_position(w, direction):
    ww, wh = w * w, w // 2
    win0, win1 = one_hot_windows(w, direction)
    mix = known_mix(ww)
    z = torch.zeros(ww, 2, dtype=torch.float64)
    p = fine_forward_parts(win0, win1, mix, mix, z, z, FINE_SCALE)
    gx, gy = grid(w)
    want = torch.stack([gx, gy], 1) * wh * FINE_SCALE + wh           # match r is one-hot at position r
    for d in range(2):
        if direction in (d, 2):
            assert torch.equal(p[d][:, :2], want) and torch.equal(p[2 + d], want)
            assert (p[d][:, 2] - 2e-5).abs().max().item() <= 1e-18
            assert p[4 + d].abs().max().item() <= 1e-130             # variance: 24 terms of exp(-320) at the most
        else:       # this direction correlates against an all-zero window: a flat heat map
            assert (p[d][:, :2] - wh).abs().max().item() <= 1e-14
            assert (p[d][:, 2] - _flat_std(w)).abs().max().item() <= 1e-14


@by_w
def test_all_zero_windows(w):
    ww = w * w
    _, _, mix0, mix1 = regime_inputs(w, 1.0, m=1)                     # any mix: q = bias, every logit 0
    zero = torch.zeros(9, ww, 64, dtype=torch.float64)
    z = torch.zeros(9, 2, dtype=torch.float64)
    o0, o1 = fine_forward(zero, zero, mix0.double(), mix1.double(), z, z, FINE_SCALE)
    assert abs(_flat_std(w) - {5: 1.41421356, 7: 1.33333333}[w]) <= 5e-9
    for o in (o0, o1):
        assert (o[:, :2] - w // 2).abs().max().item() <= 1e-14
        assert (o[:, 2] - _flat_std(w)).abs().max().item() <= 1e-14


@by_w
def test_two_point_heat_map(w):
    ww = w * w
    win0, win1, pairs = two_point_windows(w)
    assert (pairs[:, 0] != pairs[:, 1]).all()
    same_x = (pairs[:, 0] % w == pairs[:, 1] % w).sum().item()
    same_y = (pairs[:, 0] // w == pairs[:, 1] // w).sum().item()
    assert same_x > 0 and same_y > 0                                  # one axis clamped, the other not
    mix = known_mix(ww)
    z = torch.zeros(ww, 2, dtype=torch.float64)
    off, var = two_point_answer(w, pairs, FINE_SCALE)
    std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(1)              # (the axis they share: clamped, sqrt(1e-10))
    for o in fine_forward(win0, win1, mix, mix, z, z, FINE_SCALE):
        assert (o[:, :2] - off).abs().max().item() <= 1e-14
        assert (o[:, 2] - std).abs().max().item() <= 1e-8             # (var = E[g^2] - E[g]^2 cancels to ~1e-16)


@by_w
@pytest.mark.parametrize("gain", FINE_GAINS)
def test_regimes_populate_both_sides_of_the_clamp(w, gain):
    """the conditions tests/test_gpu_fine_forward.py relies on, at the seeds it uses, from float64 alone: up to gain 1
    no variance comes near the clamp, at gain 3 a few per cent of the heat maps are sharp (std < 1e-3), at gain 10 more
    than half; and the bars derived from torch's float32 error sit at least 10x below the 1e-3 px of the older tests up
    to gain 3"""
    win0, win1, mix0, mix1 = regime_inputs(w, gain)
    assert win0.shape == (FINE_M, w * w, 64) and FINE_M >= 2000 and FINE_M % 4
    assert torch.equal(win1[:FINE_TIED], 3 * win0[:FINE_TIED])
    assert gain == 0 or not torch.equal(win1[FINE_TIED:], 3 * win0[FINE_TIED:])
    off64, var64, e32, d0 = fine_yardstick(win0, win1, mix0, mix1)
    std = torch.stack([std_interval(var64[:, :2], 0.0)[0], std_interval(var64[:, 2:], 0.0)[0]], 1)
    sharp = (std < 1e-3).double().mean().item()
    bar_off, bar_var = fine_bars(w, e32, d0, cap_off=FINE_CAP_PX if gain <= 3 else None)
    print(f"W={w} gain={gain}: e32 {e32:.2e} px, d0 {d0:.2e}, bars {bar_off:.2e} px / {bar_var:.2e}, "
          f"min var {var64.min().item():.2e}, min std {std.min().item():.3g}, std < 1e-3: {100 * sharp:.1f} %")
    if gain <= 1:
        assert var64.min().item() >= 1e-4
    elif gain == 3:
        assert 0.01 <= sharp <= 0.05
    else:
        assert sharp > 0.5
    if gain <= 3:           # (the cap rarely decides: e32 itself leaves room, whatever thread count summed it)
        assert bar_off <= 1e-4 and e32 <= 5e-5
    if gain == 0:
        assert (off64 == w // 2).all()
