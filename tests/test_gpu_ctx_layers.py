"""The context-layer kernels - k_fine_tf (csrc/fine_tf.hip) and k_ctx_kv / k_ctx_kv_sum / k_ctx_layer (csrc/coarse_tf.hip) -
against the float64 yardstick of tests/ctx_layers_ref.py (pinned by tests/test_ctx_ref.py), called straight through
ctypes (fm_fine_transformer_start, fm_coarse_transformer_masked) into outputs pre-filled with NaN.

Bars.  Per row - a match of the fine layers, a token of the coarse ones -
    |got - out64| <= CTX_MULT * e32_row + CTX_FLOOR_ULPS * 2^-23 * max|out64_row|,
e32_row = the error of the float32 evaluation of the same inputs on the CPU against float64 (the oracle without masks,
the module's torch layers with them).  CTX_MULT = 4: the kernels' split products carry 22 significant bits against
float32's 24.  Nothing is calibrated on a kernel.  The older tests' absolute bars (2e-5 fine, 5e-5 coarse, times
max(1, max|out|) of the call) are kept as a cap of every row's bar.  What must be equal is compared bit for bit.
Lines starting with ACC are the record profiles/ctx_layers_accuracy.txt is made of."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, ops

import ctx_layers_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
by_w = pytest.mark.parametrize("w", [5, 7])
FM_E_UNSUPPORTED = -3


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _untouched(t):
    """still the NaN it was pre-filled with, bit for bit"""
    return _same_bits(t, torch.full_like(t, float("nan")))


def _dev(a):
    return torch.as_tensor(a, device=DEV).contiguous()


def _stream():
    return ops._stream(torch.device(DEV))


# ------------------------------------------------------------------ the two entry points
@functools.lru_cache(maxsize=None)
def _fine_packed():
    return ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in cr.fine_weights().items()}, DEV)


def _fine_raw(win0, win1, out0, out1, m_max, count=None, start=8):
    """fm_fine_transformer_start on device tensors -> (return code, FM_DEV_* status word, d_lowered)"""
    ww = win0.shape[1]
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    cnt = None if count is None else torch.tensor([count, 0], dtype=torch.int32, device=DEV)
    rc = _lib.load().fm_fine_transformer_start(ops._ptr(win0), ops._ptr(win1), m_max, ops._ptr(cnt), ww, 64,
                                               ops._ptr(_fine_packed()), ops._ptr(out0), ops._ptr(out1), ops._ptr(st), start,
                                               C.c_void_p(st.data_ptr() + 4), _stream())
    torch.cuda.synchronize()
    status, lowered = st.tolist()
    return rc, status, lowered


def _fine(x0, x1, m_max=None, count=None, rows=None):
    """(out0, out1, lowered) of a call on host arrays [M, WW, 64]; the outputs have `rows` rows (M unless given), all NaN
    before the call; status 0 is asserted"""
    win0, win1 = _dev(x0), _dev(x1)
    rows = win0.shape[0] if rows is None else rows
    out0, out1 = _nan(rows, *win0.shape[1:]), _nan(rows, *win0.shape[1:])
    rc, status, lowered = _fine_raw(win0, win1, out0, out1, win0.shape[0] if m_max is None else m_max, count)
    assert rc == 0 and status == 0, (rc, status)
    return out0, out1, lowered


@functools.lru_cache(maxsize=None)
def _coarse_packed(key):
    """key: ('plain', n_layers, seed) or ('layernorm', name)"""
    w = cr.coarse_weights(key[1], key[2]) if key[0] == 'plain' else cr.layernorm_cases(2)[key[1]]
    n_layers = len({k.split('.')[1] for k in w})
    return w, ops.pack_coarse_transformer({k: torch.as_tensor(v) for k, v in w.items()}, n_layers, DEV)


def _workspace_bytes(n, l, s):
    nb = C.c_size_t()
    assert _lib.load().fm_coarse_tf_workspace_bytes(n, l, s, C.byref(nb)) == 0
    return nb.value


def _coarse(x0, x1, packed, layers, mask0=None, mask1=None, workspace=None):
    """fm_coarse_transformer_masked on host arrays into NaN outputs; masks as uint8 bytes"""
    f0, f1 = _dev(x0), _dev(x1)
    n, l, _ = f0.shape
    s = f1.shape[1]
    if workspace is None:
        workspace = torch.zeros(_workspace_bytes(n, l, s), dtype=torch.uint8, device=DEV)
    m0 = None if mask0 is None else _dev(np.asarray(mask0, np.uint8))
    m1 = None if mask1 is None else _dev(np.asarray(mask1, np.uint8))
    kinds = (C.c_int * len(layers))(*[{'self': 0, 'cross': 1}[k] for k in layers])
    out0, out1 = _nan(*f0.shape), _nan(*f1.shape)
    rc = _lib.load().fm_coarse_transformer_masked(ops._ptr(f0), ops._ptr(f1), ops._ptr(m0), ops._ptr(m1), n, l, s, 256, 8, kinds,
                                                  len(layers), ops._ptr(packed), ops._ptr(workspace), workspace.numel(),
                                                  ops._ptr(out0), ops._ptr(out1), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert _same_bits(f0, _dev(x0)) and _same_bits(f1, _dev(x1))              # inputs untouched
    return out0, out1


# ------------------------------------------------------------------ the comparison
def _check(tag, got, yard, cap, rows, classes=None):
    """got = (out0, out1) of the kernel, yard = cr.yardstick(...): every row of both images within its bar.  classes:
    name -> (sel0, sel1) boolean row masks reported on ACC lines of their own.  Prints the record lines first"""
    red = (lambda t: t.flatten(1).max(1).values) if rows == "match" else (lambda t: t.max(2).values)
    worst = []
    for img, (g, (o64, e32, omax)) in enumerate(zip(got, yard)):
        g = g.double().cpu()
        assert g.shape == o64.shape and torch.isfinite(g).all(), f"{tag} image {img}: not finite"
        assert (e32 > 0).all(), f"{tag} image {img}: a row's bar is its floor alone"
        bar = cr.ctx_bar(e32, omax, cap=cap)
        worst.append((e32, red((g - o64).abs()), bar))
    ratio = lambda sel: max(((err / bar)[s_].max().item() if s_.any() else 0.0) for (_, err, bar), s_ in zip(worst, sel))
    top = lambda k, sel: max((w[k][s_].max().item() if s_.any() else 0.0) for w, s_ in zip(worst, sel))
    every = [torch.ones_like(w[0], dtype=torch.bool) for w in worst]
    lines = [("", every)] + [(f" [{name}]", [torch.as_tensor(s_) for s_ in sel]) for name, sel in (classes or {}).items()]
    for name, sel in lines:
        print(f"ACC {tag}{name}: rows {sum(int(s_.sum()) for s_ in sel)}, e32 {top(0, sel):.2e}, kernel {top(1, sel):.2e}, "
              f"bar {top(2, sel):.2e}, worst kernel/bar {ratio(sel):.3f}")
    assert ratio(every) <= 1.0, f"{tag}: a row is {ratio(every):.3f} x its bar"


# ------------------------------------------------------------------ fine layers
@functools.lru_cache(maxsize=None)
def _fine_case(w, calm=False):
    """(x0, x1, yardstick) of the mixed-gain case (calm: gains >= 40 replaced by 1)"""
    x0, x1 = cr.fine_inputs(w, cr.fine_gains(calm=calm))
    return x0, x1, cr.yardstick(x0, x1, cr.fine_weights(), cr.FINE_LAYERS, rows="match")


@functools.lru_cache(maxsize=None)
def _run_a(w, calm=False):
    x0, x1, _ = _fine_case(w, calm)
    return _fine(x0, x1)


def _gain_classes(gains):
    return {f"gain {g:g}": (gains == np.float32(g),) * 2 for g in sorted(set(gains.tolist()))}


@by_w
def test_a_mixed_regimes_inside_a_workgroup(w):
    """M = 37, per-match gain cycling [1e-3, 1, 8, 40, 120, 300, 1, 1e-3]: every workgroup of 8 waves holds matches that
    lower their activation scale and matches that do not.  Per-match bar; d_lowered is what the gain-300 matches give
    when they are called alone.
    On record (profiles/ctx_layers_accuracy.txt): while kv_phase split v / S, the matches of gain 1e-3 were at 1.28e-5
    against a bar of 9.9e-6 (W = 5) - v / S sat where the lo half of the split is a float16 subnormal; it splits v now"""
    x0, x1, yard = _fine_case(w)
    out0, out1, lowered = _run_a(w)
    gains = cr.fine_gains()
    ex = cr.exp_form_error(x0, x1, cr.fine_weights(), cr.FINE_LAYERS)
    for g in (40.0, 120.0, 300.0):           # (what e32 of these rows is made of: see exp_form_error)
        sel = torch.as_tensor(gains == np.float32(g))
        err = max((o.double().cpu() - y[0]).abs().flatten(1).max(1).values[sel].max().item() for o, y in zip((out0, out1), yard))
        print(f"ACC a fine W={w} gain {g:g}: float32 with exp(x) in place of expm1(x) + 1: {max(e[sel].max().item() for e in ex):.2e}, "
              f"kernel {err:.2e}")
    _check(f"a fine W={w} mixed gains", (out0, out1), yard, cr.CTX_CAP_FINE, "match", _gain_classes(gains))
    top = gains == np.float32(300.0)
    _, _, alone = _fine(x0[top], x1[top])
    print(f"ACC a fine W={w}: d_lowered {lowered}, of the gain-300 matches alone {alone}")
    assert lowered in (4, 8, 12) and lowered == alone


@by_w
def test_a_unit_gain(w):
    """the calm data of test b (no match lowers its scale) against float64 as well"""
    x0, x1, yard = _fine_case(w, True)
    out0, out1, lowered = _run_a(w, True)
    _check(f"a fine W={w} calm", (out0, out1), yard, cr.CTX_CAP_FINE, "match", _gain_classes(cr.fine_gains(calm=True)))
    assert lowered == 0


@by_w
def test_b_neighbours_and_determinism_bitwise(w):
    x0, x1, _ = _fine_case(w)
    a0, a1, _ = _run_a(w)
    b0, b1, _ = _fine(x0, x1)
    assert _same_bits(a0, b0) and _same_bits(a1, b1)                          # run twice
    # a neighbour's lowering does not reach a match that stays in range: the same rows beside unit-gain neighbours
    c0, c1, _ = _run_a(w, True)
    keep = torch.as_tensor(cr.fine_gains() <= cr.FINE_IN_RANGE)
    assert keep.sum() == 23 and _same_bits(a0[keep], c0[keep]) and _same_bits(a1[keep], c1[keep])
    for k in (3, 8, 13):                                                     # a prefix alone: part of, one, two workgroups
        p0, p1, _ = _fine(x0[:k], x1[:k])
        assert _same_bits(p0, a0[:k]) and _same_bits(p1, a1[:k]), k


@by_w
@pytest.mark.parametrize("m_max,count", [(1, None), (7, None), (8, None), (9, None), (37, 0), (37, 1), (37, 34), (37, 37),
                                         (37, 1000), (0, None), (0, 5)])
def test_c_counts(w, m_max, count):
    """rows at or beyond min(*d_count, m_max) keep their NaN bits in both outputs, the rows before have the bits of run
    a at that row; m_max = 0 is FM_OK and writes nothing"""
    x0, x1, _ = _fine_case(w)
    a0, a1, _ = _run_a(w)
    o0, o1, _ = _fine(x0, x1, m_max=m_max, count=count, rows=cr.FINE_M)
    k = m_max if count is None else min(count, m_max)
    assert _untouched(o0[k:]) and _untouched(o1[k:])
    assert _same_bits(o0[:k], a0[:k]) and _same_bits(o1[:k], a1[:k])


@by_w
def test_d_overlapping_buffers_are_refused(w):
    """the passes of a match that lowers its scale start again from the input windows, and every wave of its workgroup
    repeats them: an output that overlaps an input would feed them updated windows.  fm_fine_transformer_start refuses
    every byte-range overlap of an output with an input or the other output and touches nothing"""
    x0, x1, _ = _fine_case(w)
    a0, a1, _ = _run_a(w)
    m, ww = cr.FINE_M, w * w
    n = m * ww * 64

    def call(win0, win1, out0, out1):
        before = [t.clone() for t in (win0, win1, out0, out1)]
        rc, status, _ = _fine_raw(win0, win1, out0, out1, m)
        assert all(_same_bits(a, b) for a, b in zip(before, (win0, win1, out0, out1))) or rc == 0
        return rc

    for gains in (cr.fine_gains(calm=True), cr.fine_gains()):               # unit-gain data, then the mixed gains
        y0, y1 = (_dev(t) for t in cr.fine_inputs(w, gains))
        assert call(y0, y1, y0, y1) == FM_E_UNSUPPORTED                      # exactly in place
    y0, y1 = _dev(x0), _dev(x1)
    assert call(y0, y1, y1, y0) == FM_E_UNSUPPORTED                          # swapped
    assert call(y0, y1, y0, _nan(m, ww, 64)) == FM_E_UNSUPPORTED             # one output in place
    assert call(y0, y1, _nan(m, ww, 64), y0) == FM_E_UNSUPPORTED             # out1 == win0
    o = _nan(m, ww, 64)
    assert call(y0, y1, o, o) == FM_E_UNSUPPORTED                            # out0 == out1
    assert call(y0, y0, o, _nan(m, ww, 64)) == 0                             # the INPUTS may be one buffer (a self pair)
    # partial overlap: ranges of one allocation that share their last / first element; touching ranges are accepted
    buf = torch.cat([y0.flatten(), _nan(n)])
    view = lambda off: buf[off:off + n].view(m, ww, 64)
    assert call(view(0), y1, view(n - 1), _nan(m, ww, 64)) == FM_E_UNSUPPORTED
    assert call(view(0), y1, _nan(m, ww, 64), view(1)) == FM_E_UNSUPPORTED
    two = _nan(2 * n)
    assert call(y0, y1, two[:n].view(m, ww, 64), two[n - 64:2 * n - 64].view(m, ww, 64)) == FM_E_UNSUPPORTED
    o1 = _nan(m, ww, 64)
    assert call(view(0), y1, view(n), o1) == 0                               # out0 right behind win0
    assert _same_bits(view(n), a0) and _same_bits(o1, a1) and _same_bits(view(0), y0)


# ------------------------------------------------------------------ coarse layers
@functools.lru_cache(maxsize=None)
def _shape_case(n, l, s, layers):
    x0, x1 = cr.coarse_inputs(n, l, s)
    w, packed = _coarse_packed(('plain', len(layers), 91))
    return x0, x1, packed, cr.yardstick(x0, x1, w, list(layers))


@pytest.mark.parametrize("n,l,s,layers", cr.COARSE_SHAPES)
def test_e_shapes(n, l, s, layers):
    """single tokens, L = 1, ragged tiles with a batch, and 37 tiles (k_ctx_kv_sum's unrolled loop and then its tail);
    input gain 2, per-token bar; the same bits on a second run (no float atomics)"""
    x0, x1, packed, yard = _shape_case(n, l, s, tuple(layers))
    got = _coarse(x0, x1, packed, layers)
    _check(f"e coarse ({n},{l},{s}) {'/'.join(layers)}", got, yard, cr.CTX_CAP_COARSE, "token")
    again = _coarse(x0, x1, packed, layers)
    assert _same_bits(got[0], again[0]) and _same_bits(got[1], again[1])


def test_f_token_magnitudes_inside_a_tile():
    """per-token gains from {1e-3, 1, 30} inside every tile of 32, an all-zero token and a token with one channel at 1e4
    over 1e-3: a scale taken per tile instead of per token would cost the small tokens their accuracy"""
    x0, x1, c0, c1 = cr.token_gain_inputs()
    w, packed = _coarse_packed(('plain', 4, 91))
    yard = cr.yardstick(x0, x1, w, cr.FOUR_LAYERS)
    got = _coarse(x0, x1, packed, cr.FOUR_LAYERS)
    classes = {f"gain {g:g}": (c0 == k, c1 == k) for k, g in enumerate(cr.TOKEN_GAINS)}
    classes["zero / spike tokens"] = (c0 == -1, c1 == -1)
    _check("f coarse (2,77,45) token gains", got, yard, cr.CTX_CAP_COARSE, "token", classes)


@functools.lru_cache(maxsize=None)
def _mask_data():
    x0, x1 = cr.coarse_inputs(2, 77, 45)
    w, packed = _coarse_packed(('plain', 4, 91))
    return x0, x1, w, packed


@pytest.mark.parametrize("name", ["both", "mask0", "mask1", "sample0_padded"])
def test_g_masks_at_every_position(name):
    """mask0: sample 0 cut mid-tile, sample 1 with an interior hole; mask1: sample 0 fully padded, sample 1 cut; either
    mask alone; sample 0 fully padded in both images.  Every position is compared, the padded ones too"""
    x0, x1, w, packed = _mask_data()
    m0, m1 = cr.mask_cases()[name]
    yard = cr.yardstick(x0, x1, w, cr.FOUR_LAYERS, m0, m1)
    got = _coarse(x0, x1, packed, cr.FOUR_LAYERS, m0, m1)
    pad = lambda m, t: np.zeros(t.shape[:2], bool) if m is None else ~m
    _check(f"g coarse (2,77,45) masks {name}", got, yard, cr.CTX_CAP_COARSE, "token",
           {"padded": (pad(m0, x0), pad(m1, x1))})


def test_g_all_ones_masks_are_no_masks():
    x0, x1, w, packed = _mask_data()
    plain = _coarse(x0, x1, packed, cr.FOUR_LAYERS)
    ones = _coarse(x0, x1, packed, cr.FOUR_LAYERS, np.ones((2, 77), bool), np.ones((2, 45), bool))
    assert _same_bits(plain[0], ones[0]) and _same_bits(plain[1], ones[1])
    _check("g coarse (2,77,45) no masks", plain, cr.yardstick(x0, x1, w, cr.FOUR_LAYERS), cr.CTX_CAP_COARSE, "token")


@pytest.mark.parametrize("name", ["wide", "zero"])
def test_h_layernorm_affine_extremes(name):
    """norm1.weight with zeros and one entry of 25, norm1.bias up to 5 (the packed bound of LN1's output, 16 max|gamma| +
    max|beta| = 405, then fixes the operand scale of x as well); norm1.weight = norm1.bias = 0 (bound 0)"""
    x0, x1 = cr.coarse_inputs(1, 70, 45)
    w, packed = _coarse_packed(('layernorm', name))
    yard = cr.yardstick(x0, x1, w, ['self', 'cross'])
    got = _coarse(x0, x1, packed, ['self', 'cross'])
    _check(f"h coarse (1,70,45) norm1 {name}", got, yard, cr.CTX_CAP_COARSE, "token")


def test_i_workspace_reuse():
    """the partials and sums of an earlier call, or NaN bytes, in the workspace change no bit"""
    big, small = cr.COARSE_SHAPES[3], cr.COARSE_SHAPES[2]
    xb0, xb1, packed, _ = _shape_case(*big[:3], tuple(big[3]))
    xs0, xs1, _, _ = _shape_case(*small[:3], tuple(small[3]))
    nbytes = max(_workspace_bytes(*big[:3]), _workspace_bytes(*small[:3]))
    fresh_small, fresh_big = _coarse(xs0, xs1, packed, small[3]), _coarse(xb0, xb1, packed, big[3])
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)          # every float a NaN
    for x0, x1, layers, fresh in ((xs0, xs1, small[3], fresh_small), (xb0, xb1, big[3], fresh_big)):
        got = _coarse(x0, x1, packed, layers, workspace=ws.clone())
        assert _same_bits(got[0], fresh[0]) and _same_bits(got[1], fresh[1])
    _coarse(xb0, xb1, packed, big[3], workspace=ws)                           # 37 + 2 tiles of partials stay behind
    got = _coarse(xs0, xs1, packed, small[3], workspace=ws)
    assert _same_bits(got[0], fresh_small[0]) and _same_bits(got[1], fresh_small[1])
