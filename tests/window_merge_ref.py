"""Inputs and the yardstick shared by the window crop + context merge tests (no tests here, nothing runs on a GPU by
itself): seeded maps, weights, context rows, ids and upstream gradients; the torch lines of FinePreprocess.forward for one
image - the zero-padded crop, then merge_feat over [window | context] with the position-independent half supplied as one
row per match - as a function of tensors, in the element type of its arguments; autograd through any such function; the
error measure of the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

from featurematching_amd import synth

from train_layers_yardstick import rel_err  # noqa: F401  (the error measure of the GPU tests)

N, HF, WF, HC, WC, STRIDE, PAD = 2, 24, 32, 6, 8, 4, 2        # the shared small map: 2 x 64 x 24 x 32, coarse grid 6 x 8
NAMES = ("out", "d_feat", "d_Ww", "d_ctx")


def fine_map(seed, n=N, hf=HF, wf=WF, cf=64):
    """[n, cf, hf, wf] float32 numpy, standard normal"""
    return synth.normal(seed, 1, (n, cf, hf, wf))


def inputs(seed, m, w, n=N, hc=HC, wc=WC, ids=None, b_ids=None):
    """(w_win [64, 64], ctx [m, 64], g [m, w w, 64], b_ids [m], ids [m]) numpy: the weight uniform in torch's default range
    for Linear(128, 64), context rows and gradients standard normal, the samples and cells drawn uniformly (unsorted)
    unless given."""
    bound = 1.0 / np.sqrt(128.0)
    w_win = ((synth.uniform(seed, 2, 64 * 64) * 2 - 1) * bound).astype(np.float32).reshape(64, 64)
    ctx = synth.normal(seed, 3, (m, 64))
    g = synth.normal(seed, 4, (m, w * w, 64))
    if b_ids is None:
        b_ids = (synth.hash_u64(seed, 5, m) % np.uint64(n)).astype(np.int64)
    if ids is None:
        ids = (synth.hash_u64(seed, 6, m) % np.uint64(hc * wc)).astype(np.int64)
    return w_win, ctx, g, np.asarray(b_ids, np.int64), np.asarray(ids, np.int64)


def crop(feat, b_ids, ids, w, stride, h_c, w_c, pad=PAD):
    """[M, w w, Cf]: F.unfold(feat, (w, w), stride, pad) at the listed cells (fine_preprocess.py:43-50), as a gather from
    the zero-padded map - differentiable, any element type, and any grid (one that overhangs the map reads zeros)"""
    n, cf, hf, wf = feat.shape
    hp = max(hf + 2 * pad, stride * (h_c - 1) + w)
    wp = max(wf + 2 * pad, stride * (w_c - 1) + w)
    fp = F.pad(feat, (pad, wp - wf - pad, pad, hp - hf - pad))
    r = torch.arange(w * w, device=feat.device)
    y, x = torch.div(ids, w_c, rounding_mode='floor'), ids % w_c
    py = (stride * y)[:, None] + torch.div(r, w, rounding_mode='floor')[None]
    px = (stride * x)[:, None] + (r % w)[None]
    return fp[b_ids[:, None], :, py, px]


def lines(feat, w_win, ctx, b_ids, ids, w, stride, h_c, w_c, pad=PAD):
    """merge_feat(cat[window, expand(context)]) of one image with the context half already applied: ctx [M, 64] =
    merge_feat.weight[:, 64:] down_proj(feat_c[b, ids]) + merge_feat.bias, w_win = merge_feat.weight[:, :64]"""
    return F.linear(crop(feat, b_ids, ids, w, stride, h_c, w_c, pad), w_win) + ctx[:, None, :]


def autograd(fn, feat, w_win, ctx, g, *args, dtype=None, weight_grad=True, memory_format=None):
    """(out, d_feat, d_Ww, d_ctx) of fn(feat, w_win, ctx, *args) under torch autograd with the upstream gradient g, in
    `dtype` (default: as given).  weight_grad=False: w_win does not require grad and there is no d_Ww (asserted)."""
    def leaf(t, grad=True):
        t = t.detach().to(dtype or t.dtype, copy=True)
        if memory_format is not None and t.dim() == 4:
            t = t.contiguous(memory_format=memory_format)
        return t.requires_grad_(grad)
    feat, w_win, ctx = leaf(feat), leaf(w_win, weight_grad), leaf(ctx)
    out = fn(feat, w_win, ctx, *args)
    out.backward(g.to(out.dtype))
    if not weight_grad:
        assert w_win.grad is None
        return out.detach(), feat.grad, ctx.grad
    return out.detach(), feat.grad, w_win.grad, ctx.grad
