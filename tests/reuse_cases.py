"""The entry points that take a workspace, each as a case for tests/test_gpu_workspace_reuse.py and
tests/test_gpu_side_stream.py: `build(size)` gives the host inputs of the small problem - through the input builder of the
test that pins that problem to float64 - or of a bigger, different problem of the same entry point, `run(inputs)` makes
the call (forward, and backward where the entry point has one) on the current stream from device tensors and returns
every output and gradient by name.  Values of `build` that are no tensors (sizes, flags) pass through unchanged.

Nothing here runs on a GPU by itself, and `run` never names a stream: every launch must follow the caller's."""
import numpy as np
import torch

import encoder_tail_ref as tref
import fine_grad_ref as fref
import linear_attention_ref as lref
import pose_ref as pr
import qkv_projection_ref as qref
import step_cases as sc
import supervision_ref as sref
import window_merge_ref as wref
from featurematching_amd import ops, post, synth


def _t(a):
    return torch.as_tensor(a)


def _leaf(t):
    return t.detach().requires_grad_(True)


# ---------------------------------------------------------------------------------------------- the coarse family
def coarse_build_of(small, big):
    def build(size):
        if size == "small":         # the step's sets: 12 x 16 grids, n 2, C 64
            s = sc.input_set(small, 7001, 2, 64, 5)
            return dict(f0=_t(s['f0']), f1=_t(s['f1']), ff0=_t(s['ff0']), ff1=_t(s['ff1']), hw=(12, 16))
        f0, f1 = synth.coarse_descriptors(7001, 2, 320, 128, big)           # 16 x 20, C 128
        ff0, ff1 = synth.fine_maps(7003, 2, 64, 64, 80)
        return dict(f0=_t(f0), f1=_t(f1), ff0=_t(ff0), ff1=_t(ff1), hw=(16, 20))
    return build


coarse_build = coarse_build_of("borderline", "peaky")
# samples with flat similarity: the auto entry point's common-path attempt reports them and the call is resumed with the
# dense kernels on that attempt's results (the spans the assignment left are cleared with hipMemsetAsync)
coarse_build_mixed = coarse_build_of("mixed", "mixed")
coarse_build_empty = coarse_build_of("empty", "mixed")


def coarse_build_flat_then_peaked(size):
    """sample 0 with flat similarity and matches of its own (borderline), sample 1 peaked: the common-path attempt of the
    auto entry point and the dense pass that resumes it give sample 0 different lists, so sample 1's match indices move
    between the two assignments and what the first one left in the cell maps, tie lists and block totals is wrong"""
    d, p = coarse_build_of("borderline", "borderline")(size), coarse_build_of("peaky", "peaky")(size)
    for k in ("f0", "f1"):
        d[k] = d[k].clone()
        d[k][1] = p[k][1]
    return d


def coarse_build_half_empty(size):
    """a batch whose sample 0 is peaked and whose sample 1 has image 1's descriptors all zero: matches from sample 0, the
    resume from sample 1"""
    d = coarse_build_of("peaky", "peaky")(size)
    d['f1'] = d['f1'].clone()
    d['f1'][1] = 0
    return d


def _stat_arrays(buf):
    nr, sr, qr, nc, sc_, qc = buf.softmax_stats()
    n, l, s = buf._shape[:3]

    def read(p, pitch, k):
        o = p.value - buf.workspace.data_ptr()
        return buf.workspace[o:o + n * pitch * 4].view(torch.float32).view(n, pitch)[:, :k].clone()
    return dict(nm_r=read(nr, qr, l), sum_r=read(sr, qr, l), nm_c=read(nc, qc, s), sum_c=read(sc_, qc, s))


def coarse_run(variant):
    def run(d):
        out = ops.coarse_match(d['f0'], d['f1'], d['hw'], d['hw'], 8.0, stats=variant == "stats",
                               conf_matrix=variant == "conf_matrix")
        if variant == "cells":      # flat similarity in sample 1: the dense kernels served the call
            assert ops.HintMemory.decode(out['_coarse_buffers'].hint)['dense'] and out['i_ids'].shape[0] > 40
        res = {k: v for k, v in out.items() if k != "_coarse_buffers"}
        if variant in ("stats", "conf_matrix"):
            res.update(_stat_arrays(out['_coarse_buffers']))
        if variant == "cells":      # the cell -> match maps and tie lists the call left, through the cell-ordered crops
            res['win0'], res['win1'] = ops.gather_windows_pair(d['ff0'], d['ff1'], out['b_ids'], out['i_ids'], out['j_ids'], 5,
                                                               4, d['hw'], d['hw'], out['_coarse_buffers'].cell_maps())
        return res
    return run


def _after_coarse(d):
    """the side-stream test's hook behind a case's coarse call, whose host read of the count has drained the stream: it puts
    the descriptors behind pending work again, so that the launches that follow are tested too"""
    hook = d.get('after_coarse')
    if hook:
        hook(d)


def _upstream(k, dev):
    """a fixed upstream gradient per entry: 0.5, 1.0, 1.5, 2.0 in turn"""
    return (torch.arange(k, device=dev) % 4 + 1).float() * 0.5


def dsm_at_run(d):
    """dual_softmax_at at every third match of the call's own list, and its backward"""
    a0, a1 = _leaf(d['f0']), _leaf(d['f1'])
    out = ops.coarse_match(d['f0'], d['f1'], d['hw'], d['hw'], 8.0, stats=True)
    b, i, j = out['b_ids'][::3], out['i_ids'][::3], out['j_ids'][::3]
    if d.get('shared'):         # (b, i of the first, j of the second): two entries in one row and two in one column
        same = b[1:] == b[:-1]
        b, i, j = torch.cat([b, b[:-1][same]]), torch.cat([i, i[:-1][same]]), torch.cat([j, j[1:][same]])
    _after_coarse(d)
    conf = ops.dual_softmax_at(a0, a1, b, i, j, out['_coarse_buffers'])
    (conf * _upstream(conf.shape[0], conf.device)).sum().backward()
    return dict(conf_at=conf.detach(), d_feat0=a0.grad, d_feat1=a1.grad, i_ids=i, j_ids=j)


def coarse_build_shared(size):
    return dict(coarse_build(size), shared=True)


def conf_grad_run(dense):
    def run(d):
        """attach_conf_matrix_grad and its backward from a sparse upstream gradient (every third match: the sparse kernel)
        or a dense one (the streaming kernel)"""
        a0, a1 = _leaf(d['f0']), _leaf(d['f1'])
        out = ops.coarse_match(d['f0'], d['f1'], d['hw'], d['hw'], 8.0, conf_matrix=True)
        _after_coarse(d)
        conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])
        if dense:
            g = (_upstream(conf.numel(), conf.device) * 1e-2).view_as(conf)
        else:
            g = torch.zeros_like(conf)
            b, i, j = out['b_ids'][::3], out['i_ids'][::3], out['j_ids'][::3]
            g[b, i, j] = _upstream(b.shape[0], conf.device)
        conf.backward(g)
        return dict(conf=conf.detach(), d_feat0=a0.grad, d_feat1=a1.grad)
    return run


def coarse_loss_build(size):
    import test_gpu_coarse_loss as tcl
    f0, f1, ids, hw0, hw1 = tcl._inputs("a" if size == "small" else "pair640")      # 60 x 80 grids, C 256
    return dict(f0=_t(f0), f1=_t(f1), ids=ids.cpu(), hw0=hw0, hw1=hw1)


def coarse_loss_run(kind):
    def run(d):
        a0, a1 = _leaf(d['f0']), _leaf(d['f1'])
        out = ops.coarse_match(d['f0'], d['f1'], d['hw0'], d['hw1'], 8.0, stats=True)
        ids = d['ids']
        _after_coarse(d)
        loss = ops.coarse_loss(a0, a1, ids[:, 0], ids[:, 1], ids[:, 2], out['_coarse_buffers'], kind)
        loss.backward()
        return dict(loss=loss.detach(), d_feat0=a0.grad, d_feat1=a1.grad)
    return run


def supervise_build(size):
    hw, k = ((8, 12), 65) if size == "small" else ((60, 80), 20000)
    return dict(kp0=_t(sref.points(900 + k, k, hw, 0)), kp1=_t(sref.points(900 + k, k, hw, 1)), hw=hw)


def supervise_run(d):
    out = ops.supervise_matches(d['kp0'], d['kp1'], d['hw'], d['hw'])
    return {k: v for k, v in out.items() if torch.is_tensor(v)}


# ---------------------------------------------------------------------------------------------- the fine family
def fine_loss_build(size):
    import test_gpu_fine_loss as tfl
    e0, e1, g0, g1 = tfl._inputs("m257" if size == "small" else "m4097")
    return dict(e0=_t(e0), e1=_t(e1), g0=_t(g0), g1=_t(g1))


def fine_loss_run(d):
    e0, e1 = _leaf(d['e0']), _leaf(d['e1'])
    loss = ops.fine_loss(e0, e1, d['g0'], d['g1'])
    loss.backward()
    return dict(loss=loss.detach(), d_expec0=e0.grad, d_expec1=e1.grad)


def fine_grad_build(w):
    def build(size):
        win0, win1, mix0, mix1, g0, g1, scale = fref.backward_inputs(w, 0.3, "all", 65 if size == "small" else 300)
        return dict(win0=win0, win1=win1, mix0=mix0, mix1=mix1, g0=g0, g1=g1, scale=scale)
    return build


def fine_grad_run(d):
    leaves = [_leaf(d[k]) for k in ("win0", "win1", "mix0", "mix1")]
    z = torch.zeros(d['win0'].shape[0], 2, device=d['win0'].device)
    k0, k1 = ops.fine_match_grad(*leaves, z, z, d['scale'])
    torch.autograd.backward([k0, k1], [d['g0'], d['g1']])
    return dict(mkpts0_f=k0.detach(), mkpts1_f=k1.detach(), **{n: t.grad for n, t in zip(fref.BWD_NAMES, leaves)})


def crop_grad_build(channels_last):
    def build(size):
        """a 64-channel map, W 7, stride 4, pad 2; M list rows + the builder's corners, edges and one cell repeated 300 times"""
        import test_gpu_crop_general as tcg
        if size == "small":
            cf, w, stride, pad, h_c, w_c = tcg._case(64, 7, 4, 2)
            b, i = tcg._ids(7, h_c, w_c, m=65)
            feat = tcg._map(5, cf)
        else:
            import test_gpu_fine_grad as tfg
            n, h_c, w_c, hf, wf = tfg.SIZES["cfg1_n2"]
            b, i = tfg._ids(11, n, h_c, w_c, 300)
            feat = _t(synth.fine_maps(11, n, 64, hf, wf)[0])
            w, stride, pad = 7, 4, 2
        g = torch.randn(b.shape[0], w * w, 64, generator=torch.Generator().manual_seed(1))
        if channels_last:
            feat = feat.contiguous(memory_format=torch.channels_last)
        return dict(feat=feat, b=b, i=i, g=g, w=w, stride=stride, pad=pad, h_c=h_c, w_c=w_c)
    return build


def crop_grad_run(d):
    feat = _leaf(d['feat'])
    win = ops.gather_windows_grad(feat, d['b'], d['i'], d['w'], d['stride'], d['w_c'], d['h_c'], pad=d['pad'])
    win.backward(d['g'])
    return dict(win=win.detach(), d_feat=feat.grad)


def window_merge_build(layout):
    def build(size):
        m, seed = (21, 121) if size == "small" else (300, 400)
        w_win, ctx, g, b, i = wref.inputs(seed, m, 7)
        feat = _t(wref.fine_map(seed))
        if layout == "nhwc":
            feat = feat.contiguous(memory_format=torch.channels_last)
        return dict(feat=feat, w_win=_t(w_win), ctx=_t(ctx), g=_t(g), b=_t(b), i=_t(i))
    return build


def window_merge_run(d):
    feat, w_win, ctx = _leaf(d['feat']), _leaf(d['w_win']), _leaf(d['ctx'])
    out = ops.window_merge(feat, w_win, ctx, d['b'], d['i'], 7, wref.STRIDE, wref.HC, wref.WC, wref.PAD)
    out.backward(d['g'])
    return dict(zip(wref.NAMES, (out.detach(), feat.grad, w_win.grad, ctx.grad)))


def fine_maps_build(size):
    """fine_match_maps on NCHW float32 maps with the caller's scratch: the step's set 7001 and its oracle's match list;
    big: set 7003 at twice the batch (a scratch twice as large, left full of another map's channels-last copy)"""
    seed, n = (7001, 1) if size == "small" else (7003, 2)
    s = sc.input_set("peaky", seed, n, 64, 5)
    ref = sc.oracle_of(s)
    d = {k: _t(s[k]) for k in ("ff0", "ff1", "mix0", "mix1")}
    d.update({k: _t(ref[k]) for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c")})
    d['scratch'] = torch.zeros(s['ff1'].size * 4, dtype=torch.uint8)
    return d


def fine_maps_run(d):
    k0, k1 = ops.fine_match_maps(d['ff0'], d['ff1'], d['b_ids'], d['i_ids'], d['j_ids'], 5, sc.STRIDE, sc.HW_C[1], sc.HW_C[1],
                                 d['mix0'], d['mix1'], d['mkpts0_c'], d['mkpts1_c'], sc.HW_I[0] / sc.HW_F[0],
                                 scratch=d['scratch'])
    return dict(mkpts0_f=k0, mkpts1_f=k1)


# ---------------------------------------------------------------------------------------------- the training layers
def linear_attention_build(size):
    dims = (2, 33, 70, 8, 32) if size == "small" else (2, 300, 300, 8, 32)
    q, k, v, g = lref.inputs(70 + dims[1], dims)
    qm, km = lref.ragged_masks(dims)
    return dict(q=_t(q), k=_t(k), v=_t(v), g=_t(g), qm=_t(qm), km=_t(km))


def linear_attention_run(d):
    q, k, v = _leaf(d['q']), _leaf(d['k']), _leaf(d['v'])
    out = ops.linear_attention(q, k, v, q_mask=d['qm'], kv_mask=d['km'])
    out.backward(d['g'])
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def encoder_tail_build(size):
    T = 129 if size == "small" else 1025
    x, a, gy, p, _ = tref.inputs(200 + T, T)
    return dict(x=_t(x), a=_t(a), gy=_t(gy), **{k: _t(p[k]) for k in tref.PARAMS})


def encoder_tail_run(d):
    x, a = _leaf(d['x']), _leaf(d['a'])
    params = [_leaf(d[k]) for k in tref.PARAMS]
    y = ops.encoder_tail(x, a, *params, tref.EPS, tref.EPS)
    y.backward(d['gy'])
    return dict(zip(tref.NAMES, (y.detach(), x.grad, a.grad, *(p.grad for p in params))))


def qkv_build(cross):
    def build(size):
        tx, ts = ((75, 130) if cross else (129, None)) if size == "small" else ((1025, 1025) if cross else (1025, None))
        x, src, g, w = qref.inputs(1000 + 7 * tx + ts if cross else 100 + tx, tx, ts)
        d = dict(x=_t(x), gq=_t(g[0]), gk=_t(g[1]), gv=_t(g[2]), **{k: _t(w[k]) for k in qref.WEIGHTS})
        if cross:
            d['src'] = _t(src)
        return d
    return build


def qkv_run(d):
    x = _leaf(d['x'])
    src = _leaf(d['src']) if 'src' in d else None
    ws = [_leaf(d[k]) for k in qref.WEIGHTS]
    out = ops.qkv_projection(x, x if src is None else src, *ws)
    torch.autograd.backward(list(out), [d['gq'], d['gk'], d['gv']])
    res = dict(q=out[0].detach(), k=out[1].detach(), v=out[2].detach(), dx=x.grad, dWq=ws[0].grad, dWk=ws[1].grad,
               dWv=ws[2].grad)
    if src is not None:
        res['dsrc'] = src.grad
    return res


# ---------------------------------------------------------------------------------------------- pose
def pose_build(size):
    counts, samples = ((64, 65), 256) if size == "small" else ((300, 300, 300), 512)
    scenes = [pr.scene(seed=40 + b, n=m, noise=0.5, outliers=0.2) for b, m in enumerate(counts)]
    k0, k1, bids, K0, K1, _ = pr.batch(scenes)
    return dict(k0=_t(k0), k1=_t(k1), bids=_t(bids), K0=_t(K0), K1=_t(K1), samples=samples)


def pose_run(d):
    p = post.estimate_poses(d['k0'], d['k1'], d['bids'], d['K0'], d['K1'], samples=d['samples'])
    return dict(R=p.R, t=p.t, E=p.E, inliers=p.inliers, per_pair=p.per_pair)


# name -> (build, run, the call is documented as not synchronising the host)
CASES = {
    "coarse_match plain": (coarse_build, coarse_run("plain"), False),
    "coarse_match stats": (coarse_build, coarse_run("stats"), False),
    "coarse_match conf_matrix": (coarse_build, coarse_run("conf_matrix"), False),
    "coarse_match mixed": (coarse_build_mixed, coarse_run("plain"), False),
    "coarse_match half empty, cell maps": (coarse_build_half_empty, coarse_run("cells"), False),
    "coarse_match flat then peaked, cell maps": (coarse_build_flat_then_peaked, coarse_run("cells"), False),
    "coarse_match empty": (coarse_build_empty, coarse_run("plain"), False),
    "dual_softmax_at": (coarse_build, dsm_at_run, False),
    "dual_softmax_at, shared row and column": (coarse_build_shared, dsm_at_run, False),
    "attach_conf_matrix_grad sparse": (coarse_build, conf_grad_run(False), False),
    "attach_conf_matrix_grad dense": (coarse_build, conf_grad_run(True), False),
    "coarse_loss focal": (coarse_loss_build, coarse_loss_run("focal"), False),
    "coarse_loss cross_entropy": (coarse_loss_build, coarse_loss_run("cross_entropy"), False),
    "supervise_matches": (supervise_build, supervise_run, False),
    "fine_loss": (fine_loss_build, fine_loss_run, False),
    "fine_match_grad W5": (fine_grad_build(5), fine_grad_run, False),
    "fine_match_grad W7": (fine_grad_build(7), fine_grad_run, False),
    "gather_windows_grad nchw": (crop_grad_build(False), crop_grad_run, False),
    "gather_windows_grad nhwc": (crop_grad_build(True), crop_grad_run, False),
    "linear_attention long masked": (linear_attention_build, linear_attention_run, False),
    "encoder_tail": (encoder_tail_build, encoder_tail_run, False),
    "qkv_projection self": (qkv_build(False), qkv_run, False),
    "qkv_projection cross": (qkv_build(True), qkv_run, False),
    "window_merge nchw": (window_merge_build("nchw"), window_merge_run, False),
    "window_merge nhwc": (window_merge_build("nhwc"), window_merge_run, False),
    "fine_match_maps": (fine_maps_build, fine_maps_run, True),
    "estimate_poses": (pose_build, pose_run, True),
}


def to_device(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def same_bits(a, b):
    """two results of one case's `run`: the names whose bits differ (shape and dtype included)"""
    bad = [k for k in a if k not in b] + [k for k in b if k not in a]
    for k in a:
        if k in b:
            x, y = a[k].detach().cpu().contiguous().reshape(-1), b[k].detach().cpu().contiguous().reshape(-1)
            if a[k].shape != b[k].shape or x.dtype != y.dtype or not np.array_equal(x.view(torch.uint8).numpy(), y.view(torch.uint8).numpy()):
                bad.append(k)
    return bad


def difference(a, b, names):
    """for the names of same_bits: 'name max|a - b| / max|b|' of the floating-point ones, for the failure message"""
    out = []
    for k in names:
        if k in a and k in b and a[k].shape == b[k].shape and a[k].is_floating_point():
            x, y = a[k].detach().double().cpu(), b[k].detach().double().cpu()
            out.append(f"{k} differs by {(x - y).abs().max().item() / max(y.abs().max().item(), 1e-300):.2e} of its largest element")
        else:
            out.append(k)
    return out
