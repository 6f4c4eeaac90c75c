"""The fine matching backward (fm_fine_match_backward: k_fine_bwd + k_fine_mix_reduce of csrc/fine_grad.hip) against
float64 per match, per target and per count.

Yardstick: tests/fine_grad_ref.py's fine_forward under float64 autograd on the CPU (g64); e_ref is the same function
under float32 autograd on the CPU (g32).  Nothing comes from the kernel.

Bars (fine_grad_ref.backward_bars / backward_mix_bars).  Per match m of d_win0 and d_win1, with top_m = max |g64[m]|,
e_hip_m = max |hip[m] - g64[m]|, e32_m = max |g32[m] - g64[m]|:

    e_hip_m <= 4 e32_m + (FLOOR + COND_m) top_m

4 = FINE_MULT, the project's allowance for another summation order and the hardware exponential.  FLOOR = twice the
largest e32_m / top_m over the regular cases, measured on the CPU (profiles/fine_backward_accuracy.txt).  COND_m = 0
for target xy; for std and all it is var_bar / (2 vmin_m): vmin_m = the smallest of match m's four float64 variances,
var_bar = the variance bar of fine_grad_ref.fine_bars for the case (4 d0 + 4 ulp), within which
tests/test_gpu_fine_forward.py holds the kernel's variances - the gradient of sqrt(var) inherits half that relative
error.  d_mix0 / d_mix1: the same form per entry with top = max |d_mix64|, e32 per entry and COND at the case's smallest
variance.  No match and no entry is left out of a comparison.

Cases (fine_grad_ref.BWD_REGULAR, BWD_EDGES): regime_inputs(W, gain, m=M, tied=M // 2) and a d_out seeded by (W, M) with
the std column zero (xy), the x and y columns zero (std) or no column zero (all).  tests/test_fine_ref.py asserts on the
CPU what this file assumes about them: every variance >= 1e-3 (the smallest is 3.77e-3, at W = 5, gain 1.0, M = 600),
every top_m > 0, tied and free rows in every case, the float32 reference within FLOOR per match, and three wrong
backward formulas (cross term of dco dropped, its sign flipped, dvar_x and dvar_y swapped) far outside these bars.
Gains 3 and above stay with tests/test_gpu_fine_grad.py on its own bar (its docstrings say why no yardstick separates a
right kernel from a wrong one on sharp heat maps).

Lines starting with ACC are the record profiles/fine_backward_accuracy.txt is made of (pytest -s)."""
import functools

import pytest
import torch

from featurematching_amd import _lib, ops

from fine_grad_ref import (BWD_EDGES, BWD_FLOOR, BWD_NAMES, BWD_REGULAR, backward_autograd, backward_excess,
                           backward_inputs, backward_yardstick)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = BWD_FLOOR       # 2 x 4.90e-6: profiles/fine_backward_accuracy.txt, the largest e32_m / top_m over BWD_REGULAR
by_w = pytest.mark.parametrize("w", [5, 7])
_case_id = lambda c: f"W{c[0]}-g{c[1]:g}-{c[2]}-m{c[3]}"
_yard = functools.lru_cache(maxsize=None)(backward_yardstick)        # computed once per case, never written to


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32).cpu(),
                                                                     b.contiguous().view(torch.int32).cpu())


def _hip(win0, win1, mix0, mix1, d_out0, d_out1, scale):
    """[d_win0, d_win1, d_mix0, d_mix1] through ops.fine_match_grad, on the device, in the leaves' dtypes"""
    return backward_autograd(win0, win1, mix0, mix1, d_out0, d_out1, scale, torch.float32, ops.fine_match_grad, DEV)


def _hip_case(case, d_out=None):
    inp = backward_inputs(*case)
    if d_out is not None:
        inp = (*inp[:4], *d_out, inp[6])
    return _hip(*inp)


def _abi(win0, win1, mix0, mix1, d_out0, d_out1, scale, m_max=None, count=None):
    """fm_fine_match_backward straight through ctypes on device tensors: [d_win0, d_win1, d_mix0, d_mix1] pre-filled
    with NaN, d_win of m_max rows; count = *d_count (an int) or None for d_count = NULL"""
    lib = _lib.load()
    rows, ww, cf = win0.shape
    m_max = rows if m_max is None else m_max
    assert m_max <= rows
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    outs = [nan(m_max, ww, cf), nan(m_max, ww, cf), nan(ww + 1), nan(ww + 1)]
    cnt = None if count is None else torch.tensor([count, 0], dtype=torch.int32, device=DEV)
    need = int(lib.fm_fine_match_backward_workspace_bytes(m_max, ww))
    assert need >= m_max * 2 * (ww + 1) * 4
    ws, wsp = ops._aligned_workspace(need, DEV)
    st = lib.fm_fine_match_backward(ops._ptr(win0), ops._ptr(win1), m_max, ops._ptr(cnt), ww, cf, ops._ptr(mix0),
                                    ops._ptr(mix1), float(scale), ops._ptr(d_out0), ops._ptr(d_out1), wsp, need,
                                    *[ops._ptr(t) for t in outs], ops._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert st == 0, f"fm_fine_match_backward: status {st}"
    return outs


def _check(case, got, what=""):
    """every match of d_win0 / d_win1 and every entry of d_mix0 / d_mix1 of `got` (device tensors) within its bar;
    prints the record lines first"""
    g64, g32, var64, var_bar = _yard(*case)
    m = case[3]
    lines, bad = [], []
    for name, t, a, b in zip(BWD_NAMES, got, g64, g32):
        assert t.dtype == torch.float32 and t.shape == a.shape, name
        hip = t.double().cpu()
        assert torch.isfinite(hip).all(), f"{name}: not finite"
        err, bar, e32 = backward_excess(name, hip, a, b, var64, var_bar)
        assert err.shape == bar.shape == ((m,) if name.startswith("d_win") else a.shape)     # nothing left out
        top = a.abs().max().item()
        k = int((err / bar).argmax())
        lines.append(f"ACC {_case_id(case)}{what} {name}: max|g64| {top:.3e}  e_ref {e32.max().item():.3e}  e_hip "
                     f"{err.max().item():.3e}  largest e_hip / bar {(err / bar).max().item():.3f} (at {k}: e_hip "
                     f"{err[k].item():.3e}, e_ref {e32[k].item():.3e}, bar {bar[k].item():.3e})")
        if not (err <= bar).all():
            bad.append(f"{name}: {int((err > bar).sum())} of {err.numel()} over the bar, worst at {k}")
    print("\n".join(lines))
    assert not bad, f"{_case_id(case)}{what}: " + "; ".join(bad)


# ------------------------------------------------------------------ a. against float64
@pytest.mark.parametrize("case", BWD_REGULAR, ids=_case_id)
def test_regular_cases_against_float64_per_match(case):
    """W x gain x target at M = 600, scale_f of 1, 2 and 4 (BWD_SCALE: each with every target)"""
    _check(case, _hip_case(case))


@pytest.mark.parametrize("case", BWD_EDGES, ids=_case_id)
def test_m_edges_against_float64_per_match(case):
    """M below, at and above the four matches of a workgroup of k_fine_bwd (whole waves return at m >= m_max), a wave,
    and the 256-match stride of k_fine_mix_reduce; gain 0.3, target all"""
    _check(case, _hip_case(case))


# ------------------------------------------------------------------ b. properties
@by_w
@pytest.mark.parametrize("m", [65, 257])
def test_permuting_the_matches_permutes_the_window_gradients(w, m):
    """a match's gradient does not depend on which wave of which workgroup computed it: d_win0 / d_win1 of the permuted
    list are the permuted d_win0 / d_win1 bit for bit; d_mix (another summation order) stays within its bar"""
    case = (w, 0.3, "all", m)
    win0, win1, mix0, mix1, d0, d1, scale = backward_inputs(*case)
    p = torch.randperm(m, generator=torch.Generator().manual_seed(m))
    assert not torch.equal(p, torch.arange(m))
    plain = _hip(win0, win1, mix0, mix1, d0, d1, scale)
    perm = _hip(win0[p], win1[p], mix0, mix1, d0[p], d1[p], scale)
    pd = p.to(DEV)
    assert _same_bits(perm[0], plain[0][pd]) and _same_bits(perm[1], plain[1][pd])
    inv = torch.argsort(pd)
    _check(case, [perm[0][inv], perm[1][inv], perm[2], perm[3]], " permuted")


@by_w
def test_linear_in_d_out(w):
    """every operation of the backward is linear in d_out and 2 is exact: d_out * 2 doubles all four outputs bit for
    bit, d_out = 0 gives outputs that compare equal to 0 everywhere"""
    case = (w, 0.3, "all", 257)
    d0, d1 = backward_inputs(*case)[4:6]
    once, twice = _hip_case(case), _hip_case(case, (2 * d0, 2 * d1))
    for name, a, b in zip(BWD_NAMES, once, twice):
        assert a.abs().max().item() > 0 and _same_bits(b, 2 * a), name
    for name, t in zip(BWD_NAMES, _hip_case(case, (torch.zeros_like(d0), torch.zeros_like(d1)))):
        assert (t == 0).all(), name


@by_w
def test_a_match_depends_on_its_own_d_out_only(w):
    """d_out of one match changed (a first, a last and a middle wave of a workgroup, either direction): d_win0 / d_win1
    of that match change, every other match keeps its bits"""
    case = (w, 0.3, "all", 65)
    d0, d1 = backward_inputs(*case)[4:6]
    base = _hip_case(case)
    for k, side in ((0, 0), (6, 1), (63, 0), (64, 1)):
        e = [d0.clone(), d1.clone()]
        e[side][k] += torch.tensor([1.0, -2.0, 0.5])
        got = _hip_case(case, e)
        others = torch.arange(65, device=DEV) != k
        for name, a, b in zip(BWD_NAMES[:2], base, got):
            assert _same_bits(a[others], b[others]), f"{name}: match {k}'s d_out reached another match"
            assert not torch.equal(a[k], b[k]), f"{name}: match {k} ignores its d_out"


@by_w
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_windows_get_gradients_of_their_type(w, dtype):
    """float16 / bfloat16 windows through ops.fine_match_grad: the gradients come back in that type and are the float32
    call's gradients at the up-cast windows, rounded"""
    win0, win1, mix0, mix1, d0, d1, scale = backward_inputs(w, 0.3, "all", 65)
    h0, h1 = win0.to(dtype), win1.to(dtype)
    leaves = [t.to(DEV).requires_grad_(True) for t in (h0, h1, mix0, mix1)]
    z = torch.zeros(65, 2, device=DEV)
    got = torch.autograd.grad(ops.fine_match_grad(*leaves, z, z, scale), leaves, [d0.to(DEV), d1.to(DEV)])
    want = _hip(h0.float(), h1.float(), mix0, mix1, d0, d1, scale)
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[2].dtype == torch.float32
    for name, a, b in zip(BWD_NAMES, got, want):
        assert b.abs().max().item() > 0 and torch.equal(a, b.to(a.dtype)), name


@by_w
def test_two_calls_give_the_same_bits(w):
    case = (w, 0.3, "all", 1025)
    for name, a, b in zip(BWD_NAMES, _hip_case(case), _hip_case(case)):
        assert _same_bits(a, b), name


# ------------------------------------------------------------------ c. counts
@by_w
@pytest.mark.parametrize("m_max", [9, 261])
def test_device_count(w, m_max):
    """*d_count of 0, 1, 4, 5, m_max - 1, m_max, m_max + 7 and -3 through the C ABI.  live = min(*d_count, m_max), a
    negative count is 0 (include/fmatch.h).  Rows at or beyond live are NaN in win0, win1 and d_out: they are never
    read.  d_win below live, d_mix0 and d_mix1 equal bit for bit the call on the first live rows alone (m_max = live,
    d_count = NULL); d_win at or beyond live is exactly 0; live = 0 gives all-zero d_mix"""
    win0, win1, mix0, mix1, d0, d1, scale = (t.to(DEV) if torch.is_tensor(t) else t
                                             for t in backward_inputs(w, 0.3, "all", m_max))
    for count in (0, 1, 4, 5, m_max - 1, m_max, m_max + 7, -3):
        live = max(0, min(count, m_max))
        a = [t.clone() for t in (win0, win1, d0, d1)]
        for t in a:
            t[live:] = float("nan")
        got = _abi(a[0], a[1], mix0, mix1, a[2], a[3], scale, count=count)
        what = f"m_max {m_max}, *d_count {count}"
        for t in got[:2]:
            assert (t[live:] == 0).all(), f"{what}: a row at or beyond the count is not zero"
        if live == 0:
            assert (got[2] == 0).all() and (got[3] == 0).all(), f"{what}: d_mix is not zero"
            continue
        alone = _abi(win0[:live].contiguous(), win1[:live].contiguous(), mix0, mix1, d0[:live].contiguous(),
                     d1[:live].contiguous(), scale)
        assert all(torch.isfinite(t).all() for t in alone)
        for name, t, r in zip(BWD_NAMES, got, alone):
            assert _same_bits(t[:live] if name.startswith("d_win") else t, r), f"{what}: {name} differs from the counted rows alone"
    # the counted call is the autograd path's call: the full list with d_count = NULL gives ops.fine_match_grad's bits
    full = _abi(win0, win1, mix0, mix1, d0, d1, scale)
    for name, t, r in zip(BWD_NAMES, full, _hip(win0, win1, mix0, mix1, d0, d1, scale)):
        assert _same_bits(t, r), name
