"""The fine stage's training path on the GPU: the HIP backward of the fine matching (fm_fine_match_backward) and of the
window crop (fm_gather_windows_backward) against float64, the unchanged forward of the drop-in modules, and one training
step through CoarseMatching -> FinePreprocess -> fine LocalFeatureTransformer -> FineMatching against the same graph
built from torch ops."""
import math

import numpy as np
import pytest
import torch

from featurematching_amd import modules, ops, synth
from featurematching_amd.transformer import LocalFeatureTransformer
from oracle import matcher_ref as orc

from fine_grad_ref import crop_adjoint, fine_forward, grid, known_mix, one_hot_windows, regime_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# cfg#1 (240 x 320) and cfg#2 (480 x 640) sizes: (n, hc, wc, hf, wf)
SIZES = {"cfg1": (1, 30, 40, 120, 160), "cfg2": (1, 60, 80, 240, 320), "cfg1_n2": (2, 30, 40, 120, 160)}


def _ids(seed, n, hc, wc, m):
    """(b_ids, ids) int64: random cells, the four corners and border cells (windows reaching into the padding), one
    cell repeated 1, 2 and 300 times, in shuffled list order"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(n, (m,), generator=g)
    i = torch.randint(hc * wc, (m,), generator=g)
    border = torch.tensor([0, wc - 1, (hc - 1) * wc, hc * wc - 1, wc // 2, (hc // 2) * wc, (hc // 2) * wc + wc - 1])
    rep = [torch.full((k,), c) for k, c in ((1, wc + 3), (2, 2 * wc + 5), (300, 3 * wc + 7))]
    ii = torch.cat([i, border, *rep])
    bb = torch.cat([b, torch.randint(n, (len(border),), generator=g), *[torch.full_like(r, n - 1) for r in rep]])
    p = torch.randperm(len(ii), generator=g)
    return bb[p].contiguous(), ii[p].contiguous()


def _windows(seed, size, w, m, spread=1.0):
    n, hc, wc, hf, wf = size
    f0, f1 = synth.fine_maps(seed, n, 64, hf, wf)
    b, i = _ids(seed, n, hc, wc, m)
    j = torch.flip(_ids(seed + 1, n, hc, wc, m)[1], [0])[:len(i)]
    win0 = orc.crop_windows(torch.as_tensor(f0) * spread, b, i, w, hf // hc, wc)
    win1 = orc.crop_windows(torch.as_tensor(f1) * spread, b, j, w, hf // hc, wc)
    return win0, win1


def _mix(seed, ww):
    w0, b0, w1, b1 = synth.mix_weights(seed, ww)
    return (torch.as_tensor(np.concatenate([w0, [b0]]), dtype=torch.float32),
            torch.as_tensor(np.concatenate([w1, [b1]]), dtype=torch.float32))


def _min_var(win0, win1, mix0, mix1):
    """the smallest variance of any heat map (either direction, either axis), float64"""
    ww = win0.shape[1]
    gx, gy = grid(int(math.isqrt(ww)))
    out = []
    for wa, wb, mix in ((win0, win1, mix0), (win1, win0, mix1)):
        q = torch.einsum('r,mrc->mc', mix[:ww], wa) + mix[ww]
        h = torch.softmax(torch.einsum('mc,mrc->mr', q, wb) / 8, dim=1)
        for g in (gx, gy):
            out.append(((h * g * g).sum(1) - (h * g).sum(1) ** 2).min().item())
    return min(out)


@pytest.mark.parametrize("size", ["cfg1", "cfg2"])
@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("target", ["xy", "std"])
def test_fine_backward_against_float64(size, w, target):
    ww = w * w
    spread = 1.0 if target == "xy" else 0.02        # std: spread-out heat maps, every variance well above 1e-10
    win0, win1 = _windows(11, SIZES[size], w, 400 if size == "cfg1" else 1200, spread)
    mix0, mix1 = _mix(11, ww)
    m = win0.shape[0]
    g = torch.Generator().manual_seed(2)
    k0, k1 = torch.rand(m, 2, generator=g) * 300, torch.rand(m, 2, generator=g) * 300
    wt0, wt1 = torch.randn(m, 3, generator=g), torch.randn(m, 3, generator=g)
    if target == "xy":
        wt0[:, 2] = 0
        wt1[:, 2] = 0
    else:
        wt0[:, :2] = 0
        wt1[:, :2] = 0
    scale = 2.0

    def grads(dtype, fn, dev):
        leaves = [t.detach().to(dev, dtype).clone().requires_grad_(True) for t in (win0, win1, mix0, mix1)]
        o0, o1 = fn(*leaves, k0.to(dev, dtype), k1.to(dev, dtype), scale)
        ((o0 * wt0.to(dev, dtype)).sum() + (o1 * wt1.to(dev, dtype)).sum()).backward()
        return [t.grad.double().cpu() for t in leaves], (o0.detach().double().cpu(), o1.detach().double().cpu())

    g64, o64 = grads(torch.float64, fine_forward, "cpu")
    g32, _ = grads(torch.float32, fine_forward, "cpu")
    ghip, ohip = grads(torch.float32, ops.fine_match_grad, DEV)
    if target == "std":
        assert _min_var(win0.double(), win1.double(), mix0.double(), mix1.double()) >= 1e-4, "windows not spread out"
    for name, a, b, c in zip(("d_win0", "d_win1", "d_mix0", "d_mix1"), ghip, g64, g32):
        scale_ = b.abs().max().item()
        err, err32 = (a - b).abs().max().item(), (c - b).abs().max().item()
        assert scale_ > 0 and err <= 1e-4 * scale_, \
            f"{size} W={w} {target} {name}: |hip - f64| {err:.3e}, |torch f32 - f64| {err32:.3e}, max|g| {scale_:.3e}"
        print(f"{size} W={w} {target} {name}: rel err hip {err / scale_:.2e}, torch f32 {err32 / scale_:.2e}")
    # the forward of the autograd path is fine_match itself
    ref0, ref1 = ops.fine_match(win0.to(DEV), win1.to(DEV), mix0.to(DEV), mix1.to(DEV), k0.to(DEV), k1.to(DEV), scale)
    assert torch.equal(ohip[0], ref0.double().cpu()) and torch.equal(ohip[1], ref1.double().cpu())


@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_fine_backward_on_one_hot_heat_maps(w, direction):
    """The one-hot inputs of tests/test_gpu_fine_forward.py (match r one-hot at window position r; direction 2: both
    heat maps at once) with a random d_out whose std component is not zero.  The variance of a one-hot map is below the
    clamp (0, or the -3e-9 the FMA leaves at W = 7), so the branch vx >= 1e-10f of fine_grad.hip decides here while
    g[2] != 0: every gradient is finite, and where both heat maps are one-hot d_win0, d_win1 and d_mix are exactly
    zero - a one-hot h gives ds = h (dh - sum h dh) = 0, and the clamp passes nothing back.  (With one direction
    one-hot the other one's heat map is flat and has gradients of its own: finite is all that is asked there.)

    This test found a defect, fixed with it.  fine_grad.hip formed sum h dh = dcx cx + dcy cy + ... and
    dh = dcx gx + dcy gy + ... as two plain expressions, which the compiler contracted into FMAs in different orders.
    At W = 5 every grid value is a power of two or 0 and the products are exact; at W = 7 (thirds) the two sums rounded
    differently although cx == gx bit for bit, and with both heat maps one-hot d_win0 came out as 1.192e-07 (one
    float32 ulp of dh, times t q = 0.125) instead of 0.  Both sums are now the same explicit fmaf chain, identical
    operation for operation when cx == gx, cy == gy and dvx = dvy = 0; all six cases pass.

    There is no std-gradient test against float64 on sharp heat maps: with a variance near 1e-7 the float32 variance -
    a difference of two numbers near 1 - is 40 % rounding noise, its gradient 1 / (2 sqrt(var)) with it, and no
    yardstick separates a right kernel from a wrong one there."""
    ww = w * w
    win0, win1 = one_hot_windows(w, direction, torch.float32)
    mix = known_mix(ww, torch.float32)
    g = torch.Generator().manual_seed(w)
    d0, d1 = torch.randn(ww, 3, generator=g), torch.randn(ww, 3, generator=g)
    assert (d0[:, 2] != 0).all() and (d1[:, 2] != 0).all()
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (win0, win1, mix, mix)]
    z = torch.zeros(ww, 2, device=DEV)
    o0, o1 = ops.fine_match_grad(*leaves, z, z, 2.0)
    ((o0 * d0.to(DEV)).sum() + (o1 * d1.to(DEV)).sum()).backward()
    for name, t in zip(("d_win0", "d_win1", "d_mix0", "d_mix1"), leaves):
        assert torch.isfinite(t.grad).all(), name
        if direction == 2:
            assert (t.grad == 0).all(), f"{name}: max |g| {t.grad.abs().max().item():.3e}"


# (W, gain): the regimes of the forward test (tests/fine_grad_ref.py: regime_inputs).  Gain 0, 3 and 10 were asked for;
# at W = 5, gain 10 torch's own float32 autograd is off by up to 5.6e-5 of max |g64| (CPU, 600 matches) - more than a
# quarter of the bar, which then could not tell a right kernel from a wrong one - so that case runs at gain 5 (1.5e-5)
XY_REGIMES = [(5, 0.0), (5, 3.0), (5, 5.0), (7, 0.0), (7, 3.0), (7, 10.0)]


@pytest.mark.parametrize("w,gain", XY_REGIMES)
def test_fine_backward_xy_target_by_regime(w, gain):
    """the xy gradient on flat (gain 0), partly sharp (3) and mostly sharp (5 / 10) heat maps at the project's bar
    1e-4 * max |g64|, kept only where torch float32's own error on the same data is at most a quarter of it (asserted
    here from the CPU alone)"""
    m = 600
    win0, win1, mix0, mix1 = regime_inputs(w, gain, m=m)
    g = torch.Generator().manual_seed(2)
    wt0, wt1 = torch.randn(m, 3, generator=g), torch.randn(m, 3, generator=g)
    wt0[:, 2] = 0
    wt1[:, 2] = 0

    def grads(dtype, fn, dev):
        leaves = [t.detach().to(dev, dtype).clone().requires_grad_(True) for t in (win0, win1, mix0, mix1)]
        z = torch.zeros(m, 2, device=dev, dtype=dtype)
        o0, o1 = fn(*leaves, z, z, 2.0)
        ((o0 * wt0.to(dev, dtype)).sum() + (o1 * wt1.to(dev, dtype)).sum()).backward()
        return [t.grad.double().cpu() for t in leaves]

    g64 = grads(torch.float64, fine_forward, "cpu")
    g32 = grads(torch.float32, fine_forward, "cpu")
    ghip = grads(torch.float32, ops.fine_match_grad, DEV)
    for name, a, b, c in zip(("d_win0", "d_win1", "d_mix0", "d_mix1"), ghip, g64, g32):
        scale_ = b.abs().max().item()
        err, err32 = (a - b).abs().max().item(), (c - b).abs().max().item()
        print(f"W={w} gain={gain:g} xy {name}: |hip - f64| {err:.3e}, |torch f32 - f64| {err32:.3e}, max|g| {scale_:.3e}")
        assert scale_ > 0 or (gain == 0 and name.startswith("d_mix"))      # zero windows: d_mix is exactly zero
        assert err32 <= 0.25e-4 * scale_, f"{name}: torch float32 is itself off by {err32 / scale_:.2e}"
        assert torch.isfinite(a).all() and err <= 1e-4 * scale_, \
            f"W={w} gain={gain} {name}: |hip - f64| {err:.3e}, |torch f32 - f64| {err32:.3e}, max|g| {scale_:.3e}"


def test_fine_backward_rows_beyond_the_count_and_determinism():
    from featurematching_amd import _lib
    lib = _lib.load()
    win0, win1 = (t.to(DEV) for t in _windows(3, SIZES["cfg1"], 7, 60))
    mix0, mix1 = (t.to(DEV) for t in _mix(3, 49))
    m = win0.shape[0]
    d0, d1 = torch.randn(m, 3, device=DEV), torch.randn(m, 3, device=DEV)
    count = torch.tensor([m - 10, 0], dtype=torch.int32, device=DEV)
    need = int(lib.fm_fine_match_backward_workspace_bytes(m, 49))
    outs = []
    for _ in range(2):
        ws, wsp = ops._aligned_workspace(need, DEV)
        r = [torch.full_like(win0, 7.0), torch.full_like(win1, 7.0), torch.full_like(mix0, 7.0), torch.full_like(mix1, 7.0)]
        st = lib.fm_fine_match_backward(ops._ptr(win0), ops._ptr(win1), m, ops._ptr(count), 49, 64, ops._ptr(mix0),
                                        ops._ptr(mix1), 2.0, ops._ptr(d0), ops._ptr(d1), wsp, need, *[ops._ptr(t) for t in r],
                                        ops._stream(torch.device(DEV)))
        assert st == 0
        torch.cuda.synchronize()
        outs.append(r)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][0][m - 10:] == 0).all() and (outs[0][1][m - 10:] == 0).all()
    # the counted rows alone give the same answer
    k = m - 10
    ref = ops.fine_match_grad  # (autograd path on the first k rows)
    leaves = [win0[:k].clone().requires_grad_(True), win1[:k].clone().requires_grad_(True),
              mix0.clone().requires_grad_(True), mix1.clone().requires_grad_(True)]
    o0, o1 = ref(*leaves, torch.zeros(k, 2, device=DEV), torch.zeros(k, 2, device=DEV), 2.0)
    ((o0 * d0[:k]).sum() + (o1 * d1[:k]).sum()).backward()
    for a, leaf in zip(outs[0], leaves):
        got = a[:k] if a.dim() == 3 else a
        assert torch.equal(got, leaf.grad)


@pytest.mark.parametrize("size", ["cfg1", "cfg2", "cfg1_n2"])
@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("layout", [0, 1])
def test_crop_backward_against_float64(size, w, layout):
    n, hc, wc, hf, wf = SIZES[size]
    stride = hf // hc
    b, i = _ids(7, n, hc, wc, 500 if size != "cfg2" else 2000)
    m = b.shape[0]
    d_win = torch.randn(m, w * w, 64, generator=torch.Generator().manual_seed(1))
    ref, reads = crop_adjoint(d_win, b, i, (n, 64, hf, wf), w, stride, wc)
    got = [ops.gather_windows_backward(d_win.to(DEV), b.to(DEV), i.to(DEV), (n, 64, hf, wf), w, stride, wc, hc,
                                       layout=layout) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1]), "two calls differ"
    assert got[0].is_contiguous(memory_format=torch.channels_last if layout else torch.contiguous_format)
    hip = got[0].double().cpu()
    bar = 1e-6 * ref.abs().max().item()
    assert (hip - ref).abs().max().item() <= bar
    unread = (reads == 0).expand_as(hip)
    assert unread.any() and (hip[unread] == 0).all() and not torch.signbit(hip[unread]).any()
    # torch autograd through the reference's own route (F.unfold, rearrange, select), float32
    feat = torch.zeros(n, 64, hf, wf, requires_grad=True)
    orc.crop_windows_unfold(feat, b, i, w, stride).backward(d_win)
    assert (hip - feat.grad.double()).abs().max().item() <= bar


def test_crop_backward_through_autograd_and_half_maps():
    n, hc, wc, hf, wf = SIZES["cfg1_n2"]
    f0, _ = synth.fine_maps(5, n, 64, hf, wf)
    b, i = _ids(5, n, hc, wc, 300)
    d_win = torch.randn(b.shape[0], 49, 64, generator=torch.Generator().manual_seed(4))
    ref, _ = crop_adjoint(d_win, b, i, (n, 64, hf, wf), 7, 4, wc)
    for dtype, cl in ((torch.float32, False), (torch.float32, True), (torch.float16, False), (torch.bfloat16, True)):
        feat = torch.as_tensor(f0, device=DEV).to(dtype)
        if cl:
            feat = feat.contiguous(memory_format=torch.channels_last)
        feat.requires_grad_(True)
        win = ops.gather_windows_grad(feat, b.to(DEV), i.to(DEV), 7, 4, wc, hc)
        with torch.no_grad():
            assert torch.equal(win, ops.gather_windows(feat, b.to(DEV), i.to(DEV), 7, 4, wc))
        win.backward(d_win.to(DEV))
        assert feat.grad.dtype == dtype
        tol = 1e-6 if dtype == torch.float32 else 1e-2
        assert (feat.grad.double().cpu() - ref).abs().max().item() <= tol * ref.abs().max().item()


def _fine_setup(w, seed=9):
    n, hc, wc, hf, wf = SIZES["cfg1_n2"]
    c0, c1 = synth.coarse_descriptors(seed, n, hc * wc, 64, "peaky")
    f0, f1 = synth.fine_maps(seed, n, 64, hf, wf)
    b, i = _ids(seed, n, hc, wc, 200)
    j = torch.flip(_ids(seed + 1, n, hc, wc, 200)[1], [0])[:len(i)]
    data = dict(hw0_i=(4 * hf, 4 * wf), hw1_i=(4 * hf, 4 * wf), hw0_c=(hc, wc), hw1_c=(hc, wc), hw0_f=(hf, wf),
                hw1_f=(hf, wf), b_ids=b.to(DEV), i_ids=i.to(DEV), j_ids=j.to(DEV),
                mkpts0_c=torch.stack([i % wc, i // wc], 1).float().to(DEV) * 8,
                mkpts1_c=torch.stack([j % wc, j // wc], 1).float().to(DEV) * 8)
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': w, 'coarse': {'d_model': 64}, 'fine': {'d_model': 64}}
    torch.manual_seed(seed)
    fp = modules.FinePreprocess(cfg, fused_merge=False).to(DEV)
    fm = modules.FineMatching(window=w).to(DEV)
    t = lambda a: torch.as_tensor(a, device=DEV)
    return data, fp, fm, t(c0), t(c1), t(f0), t(f1)


@pytest.mark.parametrize("w", [5, 7])
def test_forward_unchanged(w):
    data, fp, fm, c0, c1, f0, f1 = _fine_setup(w)
    # eval / no-grad path
    fp.eval(), fm.eval()
    d_ref = dict(data)
    with torch.no_grad():
        w0, w1 = fp(f0, f1, c0, c1, d_ref)
        fm(w0, w1, d_ref)
    for t in (w0, w1, d_ref['mkpts0_f'], d_ref['mkpts1_f']):
        assert t.grad_fn is None
    # eval mode under grad mode, inputs without grad: the plain path, no graph
    d_eval = dict(data)
    e0, e1 = fp(f0, f1, c0.clone(), c1.clone(), d_eval)
    fm(e0.detach(), e1.detach(), d_eval)
    assert d_eval['mkpts0_f'].grad_fn is None and d_eval['mkpts1_f'].grad_fn is None
    # training mode: the autograd paths, same values
    fp.train(), fm.train()
    d_tr = dict(data)
    a0, a1 = fp(f0.clone().requires_grad_(True), f1.clone().requires_grad_(True), c0, c1, d_tr)
    fm(a0, a1, d_tr)
    assert d_tr['mkpts0_f'].grad_fn is not None and a0.grad_fn is not None
    assert torch.equal(a0, w0) and torch.equal(a1, w1)
    assert torch.equal(d_tr['mkpts0_f'], d_ref['mkpts0_f']) and torch.equal(d_tr['mkpts1_f'], d_ref['mkpts1_f'])
    # eval mode with inputs that require grad: the autograd paths too
    fp.eval(), fm.eval()
    d_rg = dict(data)
    r0, r1 = fp(f0.clone().requires_grad_(True), f1, c0, c1, d_rg)
    fm(r0, r1, d_rg)
    assert d_rg['mkpts0_f'].grad_fn is not None
    assert torch.equal(d_rg['mkpts0_f'], d_ref['mkpts0_f']) and torch.equal(d_rg['mkpts1_f'], d_ref['mkpts1_f'])


def _fine_loss(k0, k1, gt0, gt1):
    """the fine loss by its formula (std-weighted L2, weights detached and normalised to mean 1)"""
    std = k0[:, 2] + k1[:, 2]
    inv = 1.0 / torch.clamp(std, min=1e-10)
    wgt = (inv / inv.mean()).detach()
    return (((k0[:, :2] - gt0) ** 2).sum(-1) * wgt).mean() + (((k1[:, :2] - gt1) ** 2).sum(-1) * wgt).mean()


@pytest.mark.parametrize("w", [5, 7])
def test_one_training_step(w):
    data, fp, fm, c0, c1, f0, f1 = _fine_setup(w, seed=21)
    n, hc, wc, hf, wf = SIZES["cfg1_n2"]
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV)
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}, conf_matrix=True)
    for mod in (cm, fp, tf, fm):
        mod.train()
    g = torch.Generator().manual_seed(6)
    spv_b, spv_i = _ids(6, n, hc, wc, 150)
    spv_j = torch.randint(hc * wc, (spv_b.shape[0],), generator=g)
    gt0 = torch.rand(spv_b.shape[0], 2, generator=g).to(DEV) * 200
    gt1 = torch.rand(spv_b.shape[0], 2, generator=g).to(DEV) * 200
    hw = dict(hw0_i=data['hw0_i'], hw1_i=data['hw1_i'], hw0_c=data['hw0_c'], hw1_c=data['hw1_c'], hw0_f=data['hw0_f'],
              hw1_f=data['hw1_f'])
    spv = dict(spv_b_ids=spv_b.to(DEV), spv_i_ids=spv_i.to(DEV), spv_j_ids=spv_j.to(DEV))

    def focal(conf):
        p = torch.clamp(conf, 1e-6, 1 - 1e-6)[spv['spv_b_ids'], spv['spv_i_ids'], spv['spv_j_ids']]
        return (-0.25 * torch.pow(1 - p, 2.0) * p.log()).mean()

    # the HIP graph through the drop-in modules
    leaves = [t.clone().requires_grad_(True) for t in (c0, c1, f0, f1)]
    d = dict(hw, **spv)
    cm(leaves[0], leaves[1], d)
    w0, w1 = fp(leaves[2], leaves[3], leaves[0], leaves[1], d)
    w0, w1 = tf(w0, w1)
    fm(w0, w1, d)
    loss = focal(d['conf_matrix']) + _fine_loss(d['mkpts0_f'], d['mkpts1_f'], gt0, gt1)
    params = [p for mod in (fp, tf, fm) for p in mod.parameters()]
    loss.backward()
    got = [t.grad for t in leaves] + [p.grad for p in params]
    for t in got:
        assert t is not None
    for t in leaves:
        t.grad = None
    for p in params:
        p.grad = None
    # the same graph from torch ops: the oracle's crop and fine matching (float32 autograd)
    ref_leaves = [t.clone().requires_grad_(True) for t in (c0, c1, f0, f1)]
    sim = torch.einsum("nlc,nsc->nls", ref_leaves[0] / 8, ref_leaves[1] / 8) / 0.1
    conf = torch.softmax(sim, 1) * torch.softmax(sim, 2)
    b, i, j = d['b_ids'], d['i_ids'], d['j_ids']
    stride = hf // hc
    win0 = orc.crop_windows_unfold(ref_leaves[2], b, i, w, stride).to(DEV)
    win1 = orc.crop_windows_unfold(ref_leaves[3], b, j, w, stride).to(DEV)
    ctx = fp.down_proj(torch.cat([ref_leaves[0][b, i], ref_leaves[1][b, j]], 0))
    cat = fp.merge_feat(torch.cat([torch.cat([win0, win1], 0), ctx[:, None, :].expand(-1, w * w, -1)], -1))
    r0, r1 = tf(*torch.chunk(cat, 2, dim=0))
    mix = [torch.cat([lin.weight.view(-1), lin.bias]) for lin in (fm.mix_feat_0, fm.mix_feat_1)]
    scale = d['hw0_i'][0] / d['hw0_f'][0]
    # (the oracle builds its grid on the CPU: the fine matching's graph runs there, autograd carries it back)
    k0, k1 = orc.fine_match(r0.cpu(), r1.cpu(), mix[0][:-1].cpu(), mix[0][-1].cpu(), mix[1][:-1].cpu(), mix[1][-1].cpu(),
                            d['mkpts0_c'].cpu(), d['mkpts1_c'].cpu(), scale)
    ref_loss = focal(conf) + _fine_loss(k0, k1, gt0.cpu(), gt1.cpu()).to(DEV)
    ref_loss.backward()
    want = [t.grad for t in ref_leaves] + [p.grad for p in params]
    names = ["feat_c0", "feat_c1", "feat_f0", "feat_f1"] + [f"param{k}" for k in range(len(params))]
    for name, a, b_ in zip(names, got, want):
        scale_ = b_.abs().max().item()
        assert scale_ > 0, name
        err = (a - b_).abs().max().item()
        assert err <= 1e-4 * scale_, f"{name}: {err:.3e} vs max {scale_:.3e}"
