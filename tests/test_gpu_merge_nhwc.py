"""The crop fused with the context merge on CHANNELS-LAST fine maps (fm_gather_merge_windows_nhwc), from the kernel up
to Matcher.forward_features.  The kernel feeds the values of the NCHW kernel to the same arithmetic, so the main check
is bit-identity with ops.gather_merge_windows on the NCHW map; the tolerances of every other check are those of the
NCHW tests in test_gpu_parity.py they are named after."""
import numpy as np
import pytest
import torch

from featurematching_amd import modules, ops, synth
from oracle import matcher_ref as orc
from helpers import load_golden, case_inputs, compare_match_sets, net_tail_inputs, NET_TAIL, NET_TAIL_CFG2, FLIPS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last


def _nhwc(a, dtype=None):
    """the logical [N,C,H,W] array as a channels-last device tensor (optionally rounded to a half-precision type)"""
    t = torch.as_tensor(a, device=DEV)
    if dtype is not None:
        t = t.to(dtype)
    t = t.contiguous(memory_format=CL)
    assert not t.is_contiguous() and t.is_contiguous(memory_format=CL)
    return t


def _ids(a):
    return torch.as_tensor(np.asarray(a).astype(np.int64), device=DEV)


def _merge_case(name, dist):
    """inputs of test_gpu_parity.py::test_fused_crop_and_context_merge: seeded maps and weights of the fixture, its match
    list, the per-cell context tables and the oracle's windows"""
    g = load_golden(name)
    w = int(g['meta'][6])
    c = case_inputs(g['meta'][:6], dist)
    hc, wc = c['hw_c']
    dw, db, mw, mb = (torch.as_tensor(a, device=DEV) for a in synth.merge_weights(c['cfg']['seed'], c['cfg']['c'], 64))
    w_c = mw[:, 64:]
    e_w, e_b = (w_c @ dw).contiguous(), (w_c @ db + mb).contiguous()
    ctx = [torch.nn.functional.linear(torch.as_tensor(c[k], device=DEV), e_w, e_b) for k in ('f0', 'f1')]
    ref = orc.fine_preprocess(c['ff0'], c['ff1'], c['f0'], c['f1'], g['b_ids'], g['i_ids'], g['j_ids'], w, 4, wc, wc,
                              down_proj=(dw.cpu(), db.cpu()), merge_feat=(mw.cpu(), mb.cpu()))
    return dict(g=g, w=w, hc=hc, wc=wc, packed=ops.pack_merge_weights(mw), ctx=ctx, ref=ref, ff=[c['ff0'], c['ff1']],
                b=_ids(g['b_ids']), ids=[_ids(g['i_ids']), _ids(g['j_ids'])])


MERGE_CASES = [("merge_cfg1_w7", "peaky"), ("merge_cfg2_w5", "borderline")]


@pytest.mark.parametrize("name,dist", MERGE_CASES)
def test_bit_identical_to_the_nchw_kernel_and_within_the_fixture_bars(name, dist):
    """One-image and pair form on the channels-last maps: torch.equal with ops.gather_merge_windows on the NCHW maps,
    and the three bars of test_fused_crop_and_context_merge against the reference's fixture and the oracle."""
    k = _merge_case(name, dist)
    w, hc, wc, g = k['w'], k['hc'], k['wc'], k['g']
    cl = [_nhwc(f) for f in k['ff']]
    pair = ops.gather_windows_pair(cl[0], cl[1], k['b'], k['ids'][0], k['ids'][1], w, 4, (hc, wc), (hc, wc), None,
                                   packed_w=k['packed'], ctx0=k['ctx'][0], ctx1=k['ctx'][1])
    pos = torch.arange(1, w * w + 1, dtype=torch.float64).view(1, w * w, 1)
    ch = torch.arange(1, 65, dtype=torch.float64).view(1, 1, -1)
    for im, key in ((0, 'merged0'), (1, 'merged1')):
        nchw = ops.gather_merge_windows(torch.as_tensor(k['ff'][im], device=DEV), k['packed'], k['ctx'][im], k['b'],
                                        k['ids'][im], w, 4, hc, wc)
        one = ops.gather_merge_windows(cl[im], k['packed'], k['ctx'][im], k['b'], k['ids'][im], w, 4, hc, wc)
        assert torch.equal(one, nchw)
        assert torch.equal(pair[im], nchw)
        got, ref = one.cpu(), k['ref'][im]
        err = (got - ref).abs().max().item()
        print(f"{name} image {im}: max |got - oracle| = {err:.3e}")
        assert err <= 4e-6
        np.testing.assert_allclose(got[:3].numpy(), g[key + '_head'], rtol=0, atol=2e-5)
        np.testing.assert_allclose((got.double() * pos * ch).sum((1, 2)).numpy(), g[key + '_sum'], rtol=0,
                                   atol=1e-6 * float((pos * ch).sum()))


def _ragged_case():
    """the case of test_pair_gather_equals_two_single_gathers: N = 2, 9x12 against 11x10 cells, border_rm = 0 (windows
    overhang every edge of the maps), one exact tie"""
    h0, w0, h1, w1 = 9, 12, 11, 10
    f0 = 4.0 * synth.normal(81, 1, (2, h0 * w0, 64))
    perm = synth.permutation(81, 3, h1 * w1)
    f1 = 4.0 * synth.normal(81, 2, (2, h1 * w1, 64))
    k = min(h0 * w0, h1 * w1) - 10
    f1[:, perm[:k]] = f0[:, :k] + 0.4 * synth.normal(81, 4, (2, k, 64))
    f1[0, perm[k]] = f1[0, perm[0]]                                  # tie: cell 0 of image 0 -> two cells of image 1
    buf = ops.coarse_match_async(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), (h0, w0), (h1, w1), 8.0,
                                 border_rm=0, dense=True)
    m = buf.read_count()
    o = buf.sliced(m)
    assert m > 100
    i_ids, j_ids = o['i_ids'].cpu().numpy(), o['j_ids'].cpu().numpy()
    assert len(set(zip(o['b_ids'].tolist(), i_ids.tolist()))) < m                  # the tie is there
    # windows overhang all four edges of both maps
    for ids, hh, ww in ((i_ids, h0, w0), (j_ids, h1, w1)):
        y, x = ids // ww, ids % ww
        assert y.min() == 0 and y.max() == hh - 1 and x.min() == 0 and x.max() == ww - 1
    ff0 = synth.fine_maps(81, 2, 64, h0 * 4, w0 * 4)[0]
    ff1 = synth.fine_maps(82, 2, 64, h1 * 4, w1 * 4)[1]
    packed = ops.pack_merge_weights(torch.as_tensor(synth.merge_weights(81, 64, 64)[2], device=DEV))
    ctx0 = torch.as_tensor(synth.normal(81, 7, (2, h0 * w0, 64)), device=DEV)
    ctx1 = torch.as_tensor(synth.normal(81, 8, (2, h1 * w1, 64)), device=DEV)
    return dict(hw0=(h0, w0), hw1=(h1, w1), o=o, m=m, ff=[ff0, ff1], packed=packed, ctx=[ctx0, ctx1])


@pytest.mark.parametrize("w", [5, 7])
def test_edges_ties_and_ragged_sizes(w):
    """pair form == the two one-image calls == the NCHW results, bit for bit"""
    k = _ragged_case()
    o, (h0, w0), (h1, w1) = k['o'], k['hw0'], k['hw1']
    cl0, cl1 = _nhwc(k['ff'][0]), _nhwc(k['ff'][1])
    p0, p1 = ops.gather_windows_pair(cl0, cl1, o['b_ids'], o['i_ids'], o['j_ids'], w, 4, (h0, w0), (h1, w1), None,
                                     packed_w=k['packed'], ctx0=k['ctx'][0], ctx1=k['ctx'][1])
    s0 = ops.gather_merge_windows(cl0, k['packed'], k['ctx'][0], o['b_ids'], o['i_ids'], w, 4, h0, w0)
    s1 = ops.gather_merge_windows(cl1, k['packed'], k['ctx'][1], o['b_ids'], o['j_ids'], w, 4, h1, w1)
    n0 = ops.gather_merge_windows(torch.as_tensor(k['ff'][0], device=DEV), k['packed'], k['ctx'][0], o['b_ids'], o['i_ids'],
                                  w, 4, h0, w0)
    n1 = ops.gather_merge_windows(torch.as_tensor(k['ff'][1], device=DEV), k['packed'], k['ctx'][1], o['b_ids'], o['j_ids'],
                                  w, 4, h1, w1)
    assert torch.isfinite(n0).all() and torch.isfinite(n1).all()
    assert torch.equal(p0, s0) and torch.equal(p1, s1)
    assert torch.equal(s0, n0) and torch.equal(s1, n1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("w", [5, 7])
def test_half_precision_maps_are_read_as_they_are(w, dtype):
    """float16 / bfloat16 channels-last maps (values rounded from the float32 ones; every one is exact in float32):
    torch.equal with the float32 call on .float() of the same map - one-image and pair form, edges included."""
    k = _ragged_case()
    o, (h0, w0), (h1, w1) = k['o'], k['hw0'], k['hw1']
    h = [_nhwc(k['ff'][0], dtype), _nhwc(k['ff'][1], dtype)]
    f = [t.float() for t in h]
    assert all(t.is_contiguous(memory_format=CL) and not t.is_contiguous() for t in f)
    args = (o['b_ids'], o['i_ids'], o['j_ids'], w, 4, (h0, w0), (h1, w1), None)
    kw = dict(packed_w=k['packed'], ctx0=k['ctx'][0], ctx1=k['ctx'][1])
    ph, pf = ops.gather_windows_pair(h[0], h[1], *args, **kw), ops.gather_windows_pair(f[0], f[1], *args, **kw)
    assert torch.equal(ph[0], pf[0]) and torch.equal(ph[1], pf[1])
    one = ops.gather_merge_windows(h[1], k['packed'], k['ctx'][1], o['b_ids'], o['j_ids'], w, 4, h1, w1)
    assert torch.equal(one, pf[1]) and torch.isfinite(one).all()
    # ... and the float32 call on the up-cast map is the NCHW kernel's answer on those values
    nchw = ops.gather_merge_windows(f[1].contiguous(), k['packed'], k['ctx'][1], o['b_ids'], o['j_ids'], w, 4, h1, w1)
    assert torch.equal(one, nchw)


@pytest.mark.parametrize("gain", [1e-6, 1.0, 300.0, 3e5])
def test_merge_follows_the_magnitude_of_channels_last_maps(gain):
    """test_fused_context_merge_follows_the_magnitude_of_the_maps on the channels-last path: per window 2^-20 of the
    window's own largest output"""
    g = load_golden("merge_cfg1_w7")
    c = case_inputs(g['meta'][:6], "peaky")
    hc, wc = c['hw_c']
    dw, db, mw, mb = (torch.as_tensor(a, device=DEV) for a in synth.merge_weights(c['cfg']['seed'], c['cfg']['c'], 64))
    w_c = mw[:, 64:]
    e_w, e_b = (w_c @ dw).contiguous(), (w_c @ db + mb).contiguous()
    packed = ops.pack_merge_weights(mw)
    ff0 = (c['ff0'] * np.float32(gain)).astype(np.float32)
    ff0[0, :, 40:44, 40:44] *= np.float32(1e-3)               # one cell's window three orders of magnitude smaller
    ref0, _ = orc.fine_preprocess(ff0, ff0, c['f0'], c['f1'], g['b_ids'], g['i_ids'], g['i_ids'], 7, 4, wc, wc,
                                  down_proj=(dw.cpu(), db.cpu()), merge_feat=(mw.cpu(), mb.cpu()))
    ctx = torch.nn.functional.linear(torch.as_tensor(c['f0'], device=DEV), e_w, e_b)
    got = ops.gather_merge_windows(_nhwc(ff0), packed, ctx, _ids(g['b_ids']), _ids(g['i_ids']), 7, 4, hc, wc).cpu()
    assert torch.isfinite(got).all()
    scale = ref0.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)
    rel = ((got - ref0).abs() / scale).max().item()
    print(f"gain {gain:g}: max error / window maximum = 2^{np.log2(max(rel, 1e-300)):.2f}")
    assert rel <= 2.0 ** -20


@pytest.mark.parametrize("w", [5, 7])
def test_rows_at_or_beyond_the_count_are_left_untouched(w):
    k = _ragged_case()
    o, m, (h0, w0), (h1, w1) = k['o'], k['m'], k['hw0'], k['hw1']
    cl0, cl1 = _nhwc(k['ff'][0]), _nhwc(k['ff'][1])
    args = (o['b_ids'], o['i_ids'], o['j_ids'], w, 4, (h0, w0), (h1, w1), None)
    kw = dict(packed_w=k['packed'], ctx0=k['ctx'][0], ctx1=k['ctx'][1])
    full0, full1 = ops.gather_windows_pair(cl0, cl1, *args, **kw)
    nan = lambda: torch.full((m, w * w, 64), float('nan'), device=DEV)
    for cnt in (m - 37, 5, 0):
        count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
        a0, a1 = ops.gather_windows_pair(cl0, cl1, *args, count=count, out0=nan(), out1=nan(), **kw)
        s1 = ops.gather_merge_windows(cl1, k['packed'], k['ctx'][1], o['b_ids'], o['j_ids'], w, 4, h1, w1, count=count,
                                      out=nan())
        for got, full in ((a0, full0), (a1, full1), (s1, full1)):
            assert torch.equal(got[:cnt], full[:cnt])
            assert torch.isnan(got[cnt:]).all()
    # a count beyond the capacity is clamped to it
    count = torch.tensor([m + 1000], dtype=torch.int32, device=DEV)
    a0, a1 = ops.gather_windows_pair(cl0, cl1, *args, count=count, out0=nan(), out1=nan(), **kw)
    assert torch.equal(a0, full0) and torch.equal(a1, full1)


def _module_case():
    """set-up of test_fine_preprocess_module_fused_equals_two_step"""
    g = load_golden("cfg1_peaky")
    inp = case_inputs(g['meta'], "peaky")
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 64}, 'fine': {'d_model': 64}}
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}).eval()
    torch.manual_seed(3)
    fp = modules.FinePreprocess(cfg).to(DEV).eval()
    data = {'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i'], 'hw0_c': inp['hw_c'], 'hw1_c': inp['hw_c'],
            'hw0_f': inp['hw_f'], 'hw1_f': inp['hw_f'], 'bs': 1}
    fc0, fc1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    ff0, ff1 = torch.as_tensor(inp['ff0'], device=DEV), torch.as_tensor(inp['ff1'], device=DEV)
    cm(fc0, fc1, data)
    return fp, data, fc0, fc1, ff0, ff1


def test_fine_preprocess_module_on_channels_last_maps():
    """FinePreprocess(cfg).eval() returns the same windows, bit for bit, for channels-last maps as for the NCHW maps
    (the torch layers of the un-fused route differ from the kernel in the last bits); an in-place weight update still
    invalidates the cached constants; half-precision maps equal their up-cast; train mode keeps the torch layers."""
    fp, data, fc0, fc1, ff0, ff1 = _module_case()
    cl0, cl1 = _nhwc(ff0), _nhwc(ff1)
    with torch.no_grad():
        a0, a1 = fp(ff0, ff1, fc0, fc1, data)
        b0, b1 = fp(cl0, cl1, fc0, fc1, data)
        assert a0.shape[0] > 50 and torch.equal(a0, b0) and torch.equal(a1, b1)
        # without this coarse call's cell maps (ids from elsewhere) the channels-last route is the same single launch
        d2 = {k: v for k, v in data.items() if k != '_fm_coarse'}
        e0, e1 = fp(cl0, cl1, fc0, fc1, d2)
        assert torch.equal(e0, a0) and torch.equal(e1, a1)
        h0, h1 = fp(cl0.half(), cl1.half(), fc0, fc1, data)
        g0, g1 = fp(cl0.half().float(), cl1.half().float(), fc0, fc1, data)
        assert h0.dtype == torch.float32 and torch.equal(h0, g0) and torch.equal(h1, g1)
        fp.merge_feat.bias.add_(1.0)                # an in-place weight update must invalidate the cached constants
        c0, c1 = fp(cl0, cl1, fc0, fc1, data)
        n0, n1 = fp(ff0, ff1, fc0, fc1, data)
    assert torch.equal(c0, n0) and torch.equal(c1, n1)
    scale = max(1.0, a0.abs().max().item())
    assert (c0 - (a0 + 1.0)).abs().max().item() <= 2e-5 * scale
    assert not a0.requires_grad and not b0.requires_grad
    # training mode: the crop with its HIP backward, then the torch layers - the outputs carry the autograd graph
    fp.train()
    t0, t1 = fp(cl0, cl1, fc0, fc1, data)
    assert t0.requires_grad and t1.requires_grad
    assert (t0.detach() - c0).abs().max().item() <= 2e-5 * scale and (t1.detach() - c1).abs().max().item() <= 2e-5 * scale


def _tail_matcher(inp):
    from featurematching_amd.matcher import Matcher
    m = Matcher().to(DEV).eval()
    t = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
    m.coarse.load_state_dict(t(inp['w_coarse']))
    m.fine.load_state_dict(t(inp['w_fine']))
    m.fine_preprocess.load_state_dict(t(inp['w_prep']))
    w0, b0, w1, b1 = inp['mix']
    with torch.no_grad():
        m.fine_matching.mix_feat_0.weight.copy_(torch.as_tensor(w0).view(1, -1)); m.fine_matching.mix_feat_0.bias.fill_(float(b0))
        m.fine_matching.mix_feat_1.weight.copy_(torch.as_tensor(w1).view(1, -1)); m.fine_matching.mix_feat_1.bias.fill_(float(b1))
    return m


@pytest.mark.parametrize("name,meta", [("net_tail_small", NET_TAIL), ("net_tail_cfg2", NET_TAIL_CFG2)])
def test_matcher_tail_on_channels_last_maps_against_reference_fixture(name, meta):
    """Matcher.forward_features on channels-last feat_c* and feat_f*: every assertion and tolerance of
    test_matcher_tail_against_reference_fixture (conf and guard band 4e-5, fine keypoints 5e-4 px, at most two
    reference matches absent).  The coarse maps need no copy either: flatten + transpose + contiguous is a view."""
    g = load_golden(name)
    inp = net_tail_inputs(meta)
    m = _tail_matcher(inp)
    fc0, fc1, ff0, ff1 = (_nhwc(inp[k]) for k in ('feat_c0', 'feat_c1', 'feat_f0', 'feat_f1'))
    assert fc0.flatten(2).transpose(1, 2).contiguous().data_ptr() == fc0.data_ptr()
    data = {'bs': meta['n'], 'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i']}
    m.forward_features(fc0, fc1, ff0, ff1, data)
    np.testing.assert_allclose(data['feat_c0'].double().sum((1, 2)).cpu().numpy(), g['c0_sum'], rtol=1e-5)
    got = {k: data[k].detach().cpu().numpy() for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c')}
    only_g, only_r, err = compare_match_sets(got, g)
    FLIPS.append((f"test_matcher_tail_on_channels_last_maps_against_reference_fixture[{name}]", len(only_g) + len(only_r),
                  len(g['i_ids']), err))
    assert all(abs(v - 0.2) < 4e-5 for _, v in only_g + only_r), (only_g, only_r)
    assert err <= 4e-5, err
    gk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(got['b_ids'], got['i_ids'], got['j_ids']))}
    rk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(g['b_ids'], g['i_ids'], g['j_ids']))}
    common = [k for k in gk if k in rk]
    gi, ri = np.array([gk[k] for k in common]), np.array([rk[k] for k in common])
    assert len(common) >= len(rk) - 2 and len(rk) > 80
    assert np.array_equal(got['mkpts0_c'][gi], g['mkpts0_c'][ri])
    e0 = np.abs(data['mkpts0_f'].cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max()
    e1 = np.abs(data['mkpts1_f'].cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max()
    print(f"{name}: conf err {err:.2e}, fine keypoints {e0:.2e} / {e1:.2e} px, {len(only_g) + len(only_r)} flips")
    assert e0 <= 5e-4 and e1 <= 5e-4


def _peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


def test_fine_preprocess_makes_no_layout_copy_at_640x480():
    """Around FinePreprocess.forward of the net_tail_cfg2 case (one 640x480 pair, maps of 19.7 MB): the peak of
    allocated memory grows by less than (both outputs + both context tables + half a map).  A layout copy or an
    un-fused crop adds at least one whole map, so the cap cannot hide one."""
    meta = NET_TAIL_CFG2
    inp = net_tail_inputs(meta)
    m = _tail_matcher(inp)
    fc0, fc1, ff0, ff1 = (_nhwc(inp[k]) for k in ('feat_c0', 'feat_c1', 'feat_f0', 'feat_f1'))
    data = {'bs': meta['n'], 'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i'], 'hw0_c': fc0.shape[2:], 'hw1_c': fc1.shape[2:],
            'hw0_f': ff0.shape[2:], 'hw1_f': ff1.shape[2:]}
    with torch.no_grad():
        c0, c1 = m.coarse(fc0.flatten(2).transpose(1, 2).contiguous(), fc1.flatten(2).transpose(1, 2).contiguous())
        m.coarse_matching(c0, c1, data)
        m.fine_preprocess._merge_constants()          # (cached per weight update, not per call)
        growth, (w0, w1) = _peak_growth(lambda: m.fine_preprocess(ff0, ff1, c0, c1, data))
    assert w0.shape[0] > 1000 and w0.shape[1:] == (49, 64)
    map_bytes = ff0.numel() * 4
    tables = (c0.shape[0] * c0.shape[1] + c1.shape[0] * c1.shape[1]) * 64 * 4
    outs = (w0.numel() + w1.numel()) * 4
    print(f"peak growth {growth} B; outputs {outs} B, tables {tables} B, one map {map_bytes} B")
    assert growth < outs + tables + map_bytes // 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_ops_make_no_layout_copy_and_no_upcast(dtype):
    """ops level, outputs pre-allocated, a 640x480 pair's maps: the peak grows by less than half a map - no
    .contiguous() of the channels-last map and no .float() of the float16 one."""
    k = _merge_case("merge_cfg2_w5", "borderline")
    w, hc, wc = k['w'], k['hc'], k['wc']
    cl = [_nhwc(f, None if dtype == torch.float32 else dtype) for f in k['ff']]
    map_bytes = cl[0].numel() * 4
    assert map_bytes > 15e6
    mm = k['b'].shape[0]
    o0, o1, o2 = (torch.empty(mm, w * w, 64, device=DEV) for _ in range(3))
    growth, _ = _peak_growth(lambda: ops.gather_windows_pair(cl[0], cl[1], k['b'], k['ids'][0], k['ids'][1], w, 4, (hc, wc),
                                                             (hc, wc), None, out0=o0, out1=o1, packed_w=k['packed'],
                                                             ctx0=k['ctx'][0], ctx1=k['ctx'][1]))
    print(f"pair form: peak growth {growth} B (one map {map_bytes} B)")
    assert growth < map_bytes // 2
    growth, _ = _peak_growth(lambda: ops.gather_merge_windows(cl[1], k['packed'], k['ctx'][1], k['b'], k['ids'][1], w, 4, hc,
                                                              wc, out=o2))
    print(f"one image: peak growth {growth} B")
    assert growth < map_bytes // 2
    assert torch.equal(o1, o2) and torch.isfinite(o0).all()
