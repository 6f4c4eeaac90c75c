"""The yardstick of the fine forward tests (tests/fine_grad_ref.py: fine_forward, fine_forward_parts) on the CPU: in
float32 it is the oracle's fine_match (the restatement the golden fixtures pin) to float32 rounding, in float64 it gives
the closed-form answers of one-hot, flat and two-point heat maps, and the seeded regimes tests/test_gpu_fine_forward.py
runs populate both sides of the variance clamp as that file assumes.  And what tests/test_gpu_fine_backward.py assumes
of its cases and of its bars: every variance away from the clamp, no match without a gradient, the floor of the bars
above the float32 reference's own error, and three wrong backward formulas well outside the bars."""
import functools
import hashlib
import math

import pytest
import torch

from oracle import matcher_ref as orc

from fine_grad_ref import (BWD_EDGES, BWD_FLOOR, BWD_NAMES, BWD_REGULAR, BWD_SCALE, BWD_TARGETS, F32_EPS, FINE_CAP_PX,
                           FINE_GAINS, FINE_M, FINE_SCALE, FINE_TIED, backward_bars, backward_excess, backward_inputs,
                           backward_yardstick, fine_backward, fine_bars, fine_forward, fine_forward_parts, fine_yardstick,
                           flat_answer, grid, known_mix, one_hot_windows, regime_inputs, std_interval, two_point_answer,
                           two_point_windows)

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


# sha256 over the bytes of (win0, win1, mix0, mix1) of regime_inputs(W, gain) with its defaults, taken before the helper
# got its keyword `tied`
REGIME_DIGESTS = {
    (5, 0.0): '13ea896b655f0cecd648153def29c0535766f94a80f4d5e9604e55e7df54c39b',
    (5, 0.02): '73118e6ce4ecf09e021a6d34547dff7275f7469a9f57deda47f521347d5fcc43',
    (5, 0.3): 'a432281fbbcae580520bee51e427c3faf9a0cf65beaf2732e9eaa0cb6b369baa',
    (5, 1.0): 'b7fe2d527e750b958ce901eccd8c177b431349eaf6016779b5177fd9b1927ac0',
    (5, 3.0): '1c5599167c12ab817604bdf884c9bf84534a4aae5ea858ea6b5b30282f3fd252',
    (5, 10.0): 'fc49476db5660d084cfe76f9b9c51960266eb3c73c176f857f096b1c1e67f394',
    (7, 0.0): '5f87b90b42deacd712aeecb6a8015c43746fab5d32e3b363e55ce85429ef80aa',
    (7, 0.02): '5f81ca5984e2116ebb7b778cc71299a57dfe4b2d7769e3516c984731d2252954',
    (7, 0.3): 'c013f26bea9b7082fbb585a3327f8d492b7a4baa5fd81471e2d741306b830531',
    (7, 1.0): 'b935269343114945431605037b076e5f1c23b27933d724050cd372a49a3a729e',
    (7, 3.0): 'd501e726a7457aa47b0411d9036bdb08a2d8b83fe303e94d68cc76ff33ce46fa',
    (7, 10.0): 'e8cfd2d963a901b9835ab950ef71387059d7edd2a48940422e275fc6571fdad2',
}


@by_w
@pytest.mark.parametrize("gain", FINE_GAINS)
def test_regime_inputs_default_bits(w, gain):
    """the keyword `tied` changed nothing for the callers that do not pass it"""
    h = hashlib.sha256()
    for t in regime_inputs(w, gain):
        h.update(t.contiguous().numpy().tobytes())
    assert h.hexdigest() == REGIME_DIGESTS[(w, gain)]
    # ... and the keyword does what it says
    a, b = regime_inputs(w, gain, m=9), regime_inputs(w, gain, m=9, tied=4)
    assert torch.equal(a[0], b[0]) and torch.equal(b[1][:4], 3 * b[0][:4]) and torch.equal(a[2], b[2])
    assert gain == 0 or not (b[1][4:] == 3 * b[0][4:]).any()


# ---- the cases of tests/test_gpu_fine_backward.py
_yard = functools.lru_cache(maxsize=None)(backward_yardstick)
_case_id = lambda c: f"W{c[0]}-g{c[1]:g}-{c[2]}-m{c[3]}"


def test_backward_cases_cover_what_was_asked():
    """every (W, gain, target) at M = 600, and each scale_f of 1, 2, 4 with every target"""
    assert len(set(BWD_REGULAR)) == 18 and all(c[3] == 600 for c in BWD_REGULAR)
    assert {(BWD_SCALE[(w, gain)], target) for w, gain, target, _ in BWD_REGULAR} == \
        {(s, t) for s in (1.0, 2.0, 4.0) for t in BWD_TARGETS}
    assert len(set(BWD_EDGES)) == 32 and all(c[1:3] == (0.3, "all") and (c[0], c[1]) in BWD_SCALE for c in BWD_EDGES)


@pytest.mark.parametrize("case", BWD_REGULAR + BWD_EDGES, ids=_case_id)
def test_backward_case_conditions(case):
    """What the GPU file relies on, from float64 alone: tied and free rows in every case that has room for both; every
    variance >= 1e-3 (COND_m <= var_bar / 2e-3, and the clamp's branch never decides); every match has a gradient
    (top_m > 0: a relative bar means something) and a finite, positive bar in every tensor; and the float32 reference
    is itself within the bars' floor of float64, match by match (BWD_FLOOR is twice the largest such figure this test
    prints over the regular cases: profiles/fine_backward_accuracy.txt - so a torch that sums in another order has a
    factor of two before this assertion speaks)"""
    w, gain, target, m = case
    win0, win1, _, _, d0, d1, scale = backward_inputs(*case)
    assert win0.shape == (m, w * w, 64) and d0.shape == (m, 3)
    tied = (win1 == 3 * win0).flatten(1).all(1)
    assert tied[:m // 2].all() and not tied[m // 2:].any()
    for d in (d0, d1):
        assert (d[:, :2] != 0).all() == (target != "std") and (d[:, 2] != 0).all() == (target != "xy")
        assert (d[:, :2] == 0).all() == (target == "std") and (d[:, 2] == 0).all() == (target == "xy")
    g64, g32, var64, var_bar = _yard(*case)
    assert var64.shape == (m, 4) and var64.min().item() >= 1e-3
    assert (var_bar == 0) == (target == "xy") and var_bar <= 4e-6
    for name, a, b in zip(BWD_NAMES, g64, g32):
        err, bar, e32 = backward_excess(name, b, a, b, var64, var_bar)
        assert bar.shape == err.shape == ((m,) if name.startswith("d_win") else (w * w + 1,))
        assert torch.isfinite(bar).all() and (bar > 0).all()
        if name.startswith("d_win"):
            top = backward_bars(a, b, var64, var_bar)[1]
            assert (top > 0).all(), f"{name}: a match without a gradient"
            ratio = (e32 / top).max().item()
            print(f"E32 {_case_id(case)} {name}: largest e32_m / top_m {ratio:.3e}, top_m {top.min().item():.2e} .. "
                  f"{top.max().item():.2e}, min var {var64.min().item():.3e}, var_bar {var_bar:.2e}")
            assert ratio <= BWD_FLOOR, "the float32 reference is off by more than the floor of the bars"


def _backward_formula(win0, win1, mix0, mix1, scale, d_out0, d_out1, cross=-2.0, swap_dvar=False):
    """fine_grad_ref.fine_backward restated with its two mutable points as parameters: `cross` is the factor of
    co_k dvar_k in dco_k (-2: the formula; 0: the term dropped; +2: its sign flipped) and swap_dvar exchanges dvar_x
    and dvar_y.  With the defaults it is fine_backward operation for operation (asserted below, bit for bit)"""
    m, ww, c = win0.shape
    w = int(math.isqrt(ww))
    t = 1 / math.sqrt(c)
    gx, gy = (g.to(win0.dtype) for g in grid(w))
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
        if swap_dvar:
            dvar = dvar[::-1]
        dco = [g[:, k] * (w // 2) * scale + cross * co[k] * dvar[k] for k in range(2)]       # (a + (-2 c) d == a - 2 c d)
        dh = (dco[0][:, None] * gx + dco[1][:, None] * gy + dvar[0][:, None] * gx ** 2 + dvar[1][:, None] * gy ** 2)
        ds = h * (dh - (h * dh).sum(1, keepdim=True))
        dq = t * torch.einsum('mr,mrc->mc', ds, wb)
        d_win[1 - d] += t * ds[:, :, None] * q[:, None, :]
        d_win[d] += mix[:ww][None, :, None] * dq[:, None, :]
        d_mix[d][:ww] += torch.einsum('mc,mrc->r', dq, wa)
        d_mix[d][ww] += dq.sum()
    return d_win[0], d_win[1], d_mix[0], d_mix[1]


MUTANTS = {"cross term dropped": dict(cross=0.0), "cross term's sign flipped": dict(cross=2.0),
           "dvar_x and dvar_y swapped": dict(swap_dvar=True)}


@by_w
@pytest.mark.parametrize("gain", [0.3, 1.0])
@pytest.mark.parametrize("target", ["std", "all"])
def test_wrong_backward_formulas_exceed_the_bars(w, gain, target):
    """The bars of tests/test_gpu_fine_backward.py against three wrong formulas, in float64 on the CPU.  The right
    formula (fine_backward, and its restatement here with the default parameters) is within a thousandth of every bar
    - float64 rounding only.  Each mutant misses the bar in all four tensors; in d_win0 and d_win1 in more than nine
    matches of ten (a mutant's error scales with the match's own std gradient, as the bar does), and its largest
    e_m / top_m is at least 1e-3 where the bars sit near 1e-5"""
    case = (w, gain, target, 600)
    win0, win1, mix0, mix1, d0, d1, scale = (t.double() if torch.is_tensor(t) else t for t in backward_inputs(*case))
    g64, g32, var64, var_bar = _yard(*case)
    right = fine_backward(win0, win1, mix0, mix1, scale, d0, d1)
    same = _backward_formula(win0, win1, mix0, mix1, scale, d0, d1)
    for name, a, b, r in zip(BWD_NAMES, right, same, g64):
        assert torch.equal(a, b), f"{name}: the restated formula is not fine_backward's"
        err, bar, _ = backward_excess(name, a, r, g32[BWD_NAMES.index(name)], var64, var_bar)
        assert (err <= 1e-3 * bar).all(), f"{name}: the right formula misses a bar"
    for what, kw in MUTANTS.items():
        mutant = _backward_formula(win0, win1, mix0, mix1, scale, d0, d1, **kw)
        for name, a, r, s in zip(BWD_NAMES, mutant, g64, g32):
            err, bar, _ = backward_excess(name, a, r, s, var64, var_bar)
            over = (err > bar).double().mean().item()
            if name.startswith("d_win"):
                rel = (err / backward_bars(r, s, var64, var_bar)[1])
                print(f"MUT {_case_id(case)} {what}, {name}: {100 * over:.1f} % of the matches over the bar, e_m / top_m "
                      f"{rel.min().item():.2e} .. {rel.max().item():.2e}, bar_m / top_m up to "
                      f"{(bar / backward_bars(r, s, var64, var_bar)[1]).max().item():.2e}")
                assert over > 0.9 and rel.max().item() >= 1e-3, f"{what}: {name} passes"
            else:
                print(f"MUT {_case_id(case)} {what}, {name}: {100 * over:.1f} % of the entries over the bar, largest e / bar "
                      f"{(err / bar).max().item():.2e}")
                assert over > 0, f"{what}: {name} passes"
