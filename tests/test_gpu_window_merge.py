"""ops.window_merge (fm_window_merge_forward / _backward, csrc/window_merge.hip) and the `hip_merge` switch of
FinePreprocess, on the GPU.

The yardstick is float64 autograd through window_merge_ref.lines - the zero-padded crop and the merge layer of
FinePreprocess.forward for one image - on the up-cast inputs, on the device.  For each of out, d_feat, d_Ww, d_ctx:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through the same lines
    assert e_hip <= 4 e_ref + FLOOR
- the form and the factor of tests/test_gpu_qkv_projection.py.  FLOOR is twice the largest e_ref over this file's REGULAR
lines, measured on the MI355X from the float32 torch path, never from the kernels (profiles/window_merge_accuracy.txt holds
every ACC and MEM line these tests print and the figure).  Left out of that maximum, but held to the same bar: the
module-level lines.

Sizes of the implementation (csrc/window_merge.hip): a token is one (match, window position) pair; a wave's tile kWmTile =
32 tokens; a workgroup's chunk kWmFwdChunk = 256 tokens forward, kWmBwdChunk = 128 backward; at most kWmMaxGroups = 256
workgroups, so the forward's grid takes a second round above 65 536 tokens and the backward's above 32 768; k_wm_fold adds
the slabs in 8 slices (more than one slab per slice from 9 workgroups = 1025 tokens)."""
import numpy as np
import pytest
import torch

from featurematching_amd import _lib, modules, ops, synth

import train_layers_yardstick as yard
import window_merge_ref as wref
from helpers import case_inputs, load_golden

pytestmark = pytest.mark.gpu

FLOOR = 2 * 4.920e-6         # profiles/window_merge_accuracy.txt: the largest e_ref over the regular lines of this file
DEV = "cuda:0"
LAYOUTS = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}


def _case(seed, m, w, n=wref.N, hf=wref.HF, wf=wref.WF, hc=wref.HC, wc=wref.WC, ids=None, b_ids=None):
    """(feat, w_win, ctx, g, b_ids, ids) on the device"""
    dev = lambda a: torch.as_tensor(a, device=DEV)
    w_win, ctx, g, b, i = wref.inputs(seed, m, w, n=n, hc=hc, wc=wc, ids=ids, b_ids=b_ids)
    return dev(wref.fine_map(seed, n, hf, wf)), dev(w_win), dev(ctx), dev(g), dev(b), dev(i)


def _three(case, w, stride, hc, wc, pad, layout, **kw):
    feat, w_win, ctx, g, b, i = case
    args = (b, i, w, stride, hc, wc, pad)
    hip = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=LAYOUTS[layout], **kw)
    ref32 = wref.autograd(wref.lines, feat, w_win, ctx, g, *args, **kw)
    ref64 = wref.autograd(wref.lines, feat, w_win, ctx, g, *args, dtype=torch.float64, **kw)
    return hip, ref32, ref64


def _hold(tag, hip, ref32, ref64, names=wref.NAMES):
    """print every figure, then hold every tensor to the bar, at this file's floor; here every name has its tensor"""
    assert len(hip) == len(names), tag
    yard.hold(tag, names, hip, ref32, ref64, FLOOR)


def _check(tag, seed, m, w, layout, stride=wref.STRIDE, pad=wref.PAD, **kw):
    case = _case(seed, m, w, **kw)
    hc, wc = kw.get('hc', wref.HC), kw.get('wc', wref.WC)
    hip, ref32, ref64 = _three(case, w, stride, hc, wc, pad, layout)
    assert hip[1].is_contiguous(memory_format=LAYOUTS[layout])      # the map's gradient in the map's layout
    _hold(f"regular {tag} {layout}", hip, ref32, ref64)
    return hip


# ---- token counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("m", [1, 2, 3, 5, 6, 21, 300])
def test_match_counts_w7(m, layout):
    """49, 98, 147 (crosses the 128-token chunk), 245 and 294 (either side of 256), 1029 (9 slabs), 14 700 tokens; the
    samples and cells drawn at random: b_ids unsorted over both samples"""
    if m == 300:
        b = wref.inputs(100 + m, m, 7)[3]
        assert set(b.tolist()) == {0, 1} and (np.diff(b) < 0).any()  # the draw this case runs: both samples, unsorted
    _check(f"W7 M{m}", 100 + m, m, 7, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("m", [1, 5, 6, 11, 300])
def test_match_counts_w5(m, layout):
    """25, 125 and 150 (either side of 128), 275 (past 256), 7500 tokens"""
    _check(f"W5 M{m}", 200 + m, m, 5, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_more_than_one_round_of_the_grid(layout):
    """1400 matches at W = 7: 68 600 tokens - 268 chunks forward, 536 backward over 256 workgroups, the last tile ragged"""
    _check("W7 M1400", 90, 1400, 7, layout)


# ---- padding, grids, strides ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("w", [5, 7])
def test_every_cell_of_the_grid(w, layout):
    """every cell of both samples once: all four borders and corners read padding"""
    cells = wref.HC * wref.WC
    ids = np.tile(np.arange(cells), wref.N)
    b = np.repeat(np.arange(wref.N), cells)
    _check(f"W{w} every cell", 300 + w, wref.N * cells, w, layout, ids=ids, b_ids=b)


def test_padded_positions_are_the_context_row():
    """at a padded position out = ctx[m], exactly: cell 0's first row and column lie outside the map"""
    feat, w_win, ctx, g, b, i = _case(310, 4, 7, ids=np.zeros(4, np.int64))
    out = ops.window_merge(feat, w_win, ctx, b, i, 7, wref.STRIDE, wref.HC, wref.WC)
    for r in list(range(14)) + [14, 15, 21, 22, 42, 43]:             # rows 0, 1 and columns 0, 1 of the window
        assert torch.equal(out[:, r], ctx), r
    assert not torch.equal(out[:, 16], ctx)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_grid_that_overhangs_the_map(layout):
    """a 7 x 9 grid at stride 4 over the 24 x 32 map: the last row and column of cells start at the map's edge"""
    cells = 7 * 9
    ids = np.concatenate([np.arange(cells), np.arange(cells)[::-1]])
    _check("W7 grid 7x9", 320, 2 * cells, 7, layout, hc=7, wc=9, ids=ids)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("w,stride,pad,hc,wc", [(7, 4, 2, 6, 8), (7, 2, 3, 12, 16), (5, 8, 0, 3, 4), (5, 1, 1, 24, 32)])
def test_strides_and_paddings(w, stride, pad, hc, wc, layout):
    _check(f"W{w} s{stride} p{pad}", 330 + stride, 130, w, layout, stride=stride, pad=pad, hc=hc, wc=wc)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_one_cell_300_times(layout):
    """every window the same pixels: the crop adjoint's longest list, one owner per pixel"""
    _check("W7 one cell x300", 340, 300, 7, layout, ids=np.full(300, 19, np.int64), b_ids=np.ones(300, np.int64))


# ---- what is asked for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_weight_without_grad(monkeypatch, layout):
    """w_win does not require grad: the other gradients hold the bar, no weight gradient comes back (wref.autograd asserts
    it) and the backward is handed a NULL d_w_win"""
    lib = _lib.load()
    real, seen = lib.fm_window_merge_backward, []
    monkeypatch.setattr(lib, "fm_window_merge_backward", lambda *a: (seen.append(a), real(*a))[1])
    case = _case(350, 300, 7)
    hip, ref32, ref64 = _three(case, 7, wref.STRIDE, wref.HC, wref.WC, wref.PAD, layout, weight_grad=False)
    assert len(hip) == 3 and len(seen) == 1 and seen[0][20] is None and seen[0][19] is not None and seen[0][21] is not None
    _hold(f"regular data only {layout}", hip, ref32, ref64, ("out", "d_feat", "d_ctx"))
    with_w = _three(case, 7, wref.STRIDE, wref.HC, wref.WC, wref.PAD, layout)[0]
    assert len(seen) == 2 and seen[1][20] is not None
    for u, v in zip(hip, (with_w[0], with_w[1], with_w[3])):         # the same chains with and without the exchange
        assert torch.equal(u, v)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("weight_grad", [True, False])
def test_map_without_grad(monkeypatch, layout, weight_grad):
    """the map does not require grad (a frozen backbone): the backward is handed a NULL d_feat, no map gradient comes back,
    and the weight's and the context rows' gradients are the bits of the call that computes all three"""
    lib = _lib.load()
    real, seen = lib.fm_window_merge_backward, []
    monkeypatch.setattr(lib, "fm_window_merge_backward", lambda *a: (seen.append(a), real(*a))[1])
    feat, w_win, ctx, g, b, i = _case(355, 300, 7)
    args = (b, i, 7, wref.STRIDE, wref.HC, wref.WC, wref.PAD)
    full = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=LAYOUTS[layout])
    fz = feat.contiguous(memory_format=LAYOUTS[layout])
    wl, cl = w_win.clone().requires_grad_(weight_grad), ctx.clone().requires_grad_(True)
    out = ops.window_merge(fz, wl, cl, *args)
    out.backward(g)
    assert len(seen) == 2 and seen[1][19] is None and (seen[1][20] is not None) == weight_grad and seen[1][21] is not None
    assert fz.grad is None and torch.equal(out.detach(), full[0]) and torch.equal(cl.grad, full[3])
    assert torch.equal(wl.grad, full[2]) if weight_grad else wl.grad is None


def test_forward_only():
    feat, w_win, ctx, g, b, i = _case(360, 300, 7)
    with torch.no_grad():
        out = ops.window_merge(feat, w_win, ctx, b, i, 7, wref.STRIDE, wref.HC, wref.WC)
        r32 = wref.lines(feat, w_win, ctx, b, i, 7, wref.STRIDE, wref.HC, wref.WC)
        r64 = wref.lines(feat.double(), w_win.double(), ctx.double(), b, i, 7, wref.STRIDE, wref.HC, wref.WC)
    assert not out.requires_grad
    _hold("regular forward only", (out,), (r32,), (r64,), ("out",))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("w", [5, 7])
def test_same_bits_on_every_call(w, layout):
    feat, w_win, ctx, g, b, i = _case(370, 1400, w)
    args = (b, i, w, wref.STRIDE, wref.HC, wref.WC, wref.PAD)
    first = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=LAYOUTS[layout])
    second = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=LAYOUTS[layout])
    assert len(first) == 4
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def test_layouts_agree():
    """the two loaders feed the same chains: every output the same bits for an NCHW and a channels-last map"""
    feat, w_win, ctx, g, b, i = _case(380, 300, 7)
    args = (b, i, 7, wref.STRIDE, wref.HC, wref.WC, wref.PAD)
    a = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=torch.contiguous_format)
    c = wref.autograd(ops.window_merge, feat, w_win, ctx, g, *args, memory_format=torch.channels_last)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    """65 channels, W = 9 and a float16 map: window_merge_supported says no, the op raises, and the ABI's own check
    answers FM_E_UNSUPPORTED"""
    feat, w_win, ctx, g, b, i = _case(390, 5, 7)
    assert ops.window_merge_supported(feat, 7) and ops.window_merge_supported(feat, 5)
    assert ops.window_merge_supported(feat.contiguous(memory_format=torch.channels_last), 7)
    wide = torch.zeros(2, 65, wref.HF, wref.WF, device=DEV)
    for bad, w in ((wide, 7), (feat, 9), (feat.half(), 7), (feat.double(), 7), (feat[:, :, ::2], 7)):
        assert not ops.window_merge_supported(bad, w)
        with pytest.raises(ValueError):
            ops.window_merge(bad, w_win, ctx, b, i, w, wref.STRIDE, wref.HC, wref.WC)
    with pytest.raises(ValueError):
        ops.window_merge(feat, w_win, ctx[:3], b, i, 7, wref.STRIDE, wref.HC, wref.WC)
    with pytest.raises(RuntimeError):
        ops.window_merge(feat.cpu(), w_win, ctx, b, i, 7, wref.STRIDE, wref.HC, wref.WC)
    lib = _lib.load()
    p = feat.data_ptr()
    for cf, w in ((65, 7), (64, 9)):
        with pytest.raises(_lib.FMatchError) as err:                 # the ABI's own check, through the library
            _lib.check(lib.fm_window_merge_forward(p, 2, cf, wref.HF, wref.WF, 0, w, 4, 2, wref.HC, wref.WC, p, p, p, p, 5,
                                                   None, 0, p, None), "x")
        assert err.value.status == _lib.FM_E_UNSUPPORTED
    assert lib.fm_window_merge_workspace_bytes(2, wref.HC, wref.WC, 5, 9) == 0


# ---- the reference's own output ------------------------------------------------------------------------------------
def test_module_forward_against_the_reference_fixture(monkeypatch):
    """merge_cfg1_w7 - the reference FinePreprocess's own output - through a training-mode FinePreprocess(hip_merge=True),
    at the bars tests/test_gpu_parity.py::test_fused_crop_and_context_merge holds the fused eval-mode kernel to"""
    g = load_golden("merge_cfg1_w7")
    w = int(g['meta'][6])
    c = case_inputs(g['meta'][:6], "peaky")
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': w, 'coarse': {'d_model': c['cfg']['c']}, 'fine': {'d_model': 64}}
    fp = modules.FinePreprocess(cfg, hip_merge=True).to(DEV).train()
    dw, db, mw, mb = (torch.as_tensor(a, device=DEV) for a in synth.merge_weights(c['cfg']['seed'], c['cfg']['c'], 64))
    fp.load_state_dict({'down_proj.weight': dw, 'down_proj.bias': db, 'merge_feat.weight': mw, 'merge_feat.bias': mb})
    dev = lambda a: torch.as_tensor(a, device=DEV)
    data = {'hw0_f': c['hw_f'], 'hw0_c': c['hw_c'], 'hw1_c': c['hw_c'], 'b_ids': dev(g['b_ids'].astype(np.int64)),
            'i_ids': dev(g['i_ids'].astype(np.int64)), 'j_ids': dev(g['j_ids'].astype(np.int64))}
    calls = yard.count_calls(monkeypatch, "window_merge")
    got = fp(dev(c['ff0']), dev(c['ff1']), dev(c['f0']), dev(c['f1']), data)
    assert calls == {"window_merge": 2} and all(t.grad_fn is not None for t in got)
    pos = torch.arange(1, w * w + 1, dtype=torch.float64).view(1, w * w, 1)
    ch = torch.arange(1, 65, dtype=torch.float64).view(1, 1, -1)
    for t, key in zip(got, ('merged0', 'merged1')):
        t = t.detach().cpu()
        np.testing.assert_allclose(t[:3].numpy(), g[key + '_head'], rtol=0, atol=2e-5)
        np.testing.assert_allclose((t.double() * pos * ch).sum((1, 2)).numpy(), g[key + '_sum'], rtol=0,
                                   atol=1e-6 * float((pos * ch).sum()))


# ---- the module ----------------------------------------------------------------------------------------------------
def _module_run(fp, maps, descs, data, grads, dtype, memory_format=torch.contiguous_format):
    leaves = [t.detach().to(dtype, copy=True) for t in maps + descs]
    leaves = [t.contiguous(memory_format=memory_format) if t.dim() == 4 else t for t in leaves]
    for t in leaves:
        t.requires_grad_(True)
    w0, w1 = fp(*leaves, dict(data))
    assert w0.grad_fn is not None and w1.grad_fn is not None
    torch.autograd.backward([w0, w1], [g.to(dtype) for g in grads])
    params = sorted(fp.named_parameters())
    assert all(p.grad is not None for _, p in params)
    names = ["win0", "win1", "d_feat_f0", "d_feat_f1", "d_feat_c0", "d_feat_c1"] + [k for k, _ in params]
    return names, [w0.detach(), w1.detach()] + [t.grad for t in leaves] + [p.grad for _, p in params]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_module_training_step(monkeypatch, layout):
    """a training-mode FinePreprocess(hip_merge=True) against a float64 copy (its crop the torch gather: the HIP crop is
    float32), e_ref from hip_merge=False in float32: both outputs, the gradients of both maps, both coarse descriptors
    and the four parameters"""
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 32}, 'fine': {'d_model': 64}}
    m = 300
    _, _, _, b_ids, i_ids = wref.inputs(500, m, 7)
    j_ids = wref.inputs(501, m, 7)[4]
    dev = lambda a: torch.as_tensor(a, device=DEV)
    data = {'hw0_f': (wref.HF, wref.WF), 'hw0_c': (wref.HC, wref.WC), 'hw1_c': (wref.HC, wref.WC),
            'b_ids': dev(b_ids), 'i_ids': dev(i_ids), 'j_ids': dev(j_ids)}
    maps = [dev(wref.fine_map(s)) for s in (502, 503)]
    descs = [dev(synth.normal(504, k, (wref.N, wref.HC * wref.WC, 32))) for k in (1, 2)]
    grads = [dev(synth.normal(505, k, (m, 49, 64))) for k in (1, 2)]

    def module(dtype=torch.float32, **kw):
        torch.manual_seed(9)
        return modules.FinePreprocess(cfg, **kw).to(device=DEV, dtype=dtype).train()

    calls = yard.count_calls(monkeypatch, "window_merge")
    names, hip = _module_run(module(hip_merge=True), maps, descs, data, grads, torch.float32, LAYOUTS[layout])
    assert calls == {"window_merge": 2}                              # once per image
    assert hip[2].is_contiguous(memory_format=LAYOUTS[layout]) and hip[3].is_contiguous(memory_format=LAYOUTS[layout])
    _, ref32 = _module_run(module(), maps, descs, data, grads, torch.float32)
    assert calls == {"window_merge": 2}
    monkeypatch.setattr(ops, "gather_windows_grad", lambda feat, b, ids, w, stride, w_c, h_c, pad=2, cells=None:
                        wref.crop(feat, b, ids, w, stride, h_c, w_c, pad))
    _, ref64 = _module_run(module(torch.float64, hip_merge=True), maps, descs, data, grads, torch.float64)
    assert calls == {"window_merge": 2}                              # float64 tensors: the torch lines
    _hold(f"module {layout}", hip, ref32, ref64, names)
    with torch.no_grad():                                            # a call that wants no gradient: the lines as they are
        fp = module(hip_merge=True)
        fp(maps[0], maps[1], descs[0], descs[1], dict(data))
    assert calls == {"window_merge": 2}


# ---- memory --------------------------------------------------------------------------------------------------------
def test_peak_memory():
    """forward + backward above the inputs at M = 2000, W = 7 on one 640x480 map: out, the gradients and one workspace per
    call (g w_win is its bulk) - below what the torch lines hold, measured in the same test"""
    m, hc, wc = 2000, 60, 80
    feat, w_win, ctx, g, b, i = _case(600, m, 7, n=1, hf=240, wf=320, hc=hc, wc=wc)
    args = (b, i, 7, 4, hc, wc)
    small = _case(601, 5, 7)
    wref.autograd(ops.window_merge, *small[:4], *small[4:], 7, 4, wref.HC, wref.WC)      # (library loaded, attributes set)
    spare = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)   # (one cached segment: tests/test_gpu_qkv_projection.py)
    del spare
    peak_hip = yard.peak_above_inputs(ops.window_merge, (feat, w_win, ctx), g, *args)
    peak_torch = yard.peak_above_inputs(wref.lines, (feat, w_win, ctx), g, *args)
    print(f"MEM  window_merge M{m} W7  hip {peak_hip} B  torch {peak_torch} B  ({peak_torch / max(peak_hip, 1):.2f} x)")
    assert peak_hip < peak_torch, (peak_hip, peak_torch)
