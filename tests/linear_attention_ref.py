"""Inputs shared by the linear-attention tests and tests/golden/make_golden_linear_attention.py: seeded q, k, v and the
upstream gradient (regenerated, never stored), ragged masks, and the error measure of the GPU tests.  Nothing here runs on
a GPU by itself; the yardstick is featurematching_amd.transformer.linear_attention."""
import numpy as np
import torch

from featurematching_amd import synth

from train_layers_yardstick import rel_err  # noqa: F401  (the error measure of the GPU tests)

# the fixture's cases: name -> ((N, L, S, H, D), masked)
GOLDEN_CASES = {
    "window": ((3, 25, 49, 8, 8), False),
    "long": ((1, 17, 23, 8, 32), False),
    "long_masked": ((1, 17, 23, 8, 32), True),
}
GOLDEN_SEED = 61


def inputs(seed, dims, scale=1.0, sink=False):
    """(q, k, v, g) float32 numpy: standard normals, q and k times `scale`; sink = a tenth of the tokens (every tenth,
    from token 3 of q and token 7 of k) have q = k = -30, where phi underflows towards 0"""
    n, l, s, h, d = dims
    q = synth.normal(seed, 1, (n, l, h, d)) * np.float32(scale)
    k = synth.normal(seed, 2, (n, s, h, d)) * np.float32(scale)
    v = synth.normal(seed, 3, (n, s, h, d))
    g = synth.normal(seed, 4, (n, l, h, d))
    if sink:
        q[:, 3::10] = -30.0
        k[:, 7::10] = -30.0
    return q, k, v, g


def ragged_masks(dims, empty_kv_sample=None):
    """(q_mask [N, L], kv_mask [N, S]) bool numpy: sample b keeps its first L - (3 b + 4) % L query tokens and its first
    S - (5 b + 4) % S source tokens (at least one each); `empty_kv_sample` = a sample whose kv mask is all zero"""
    n, l, s, _, _ = dims
    qm = np.zeros((n, l), bool)
    km = np.zeros((n, s), bool)
    for b in range(n):
        qm[b, :max(1, l - (3 * b + 4) % l)] = True
        km[b, :max(1, s - (5 * b + 4) % s)] = True
    if empty_kv_sample is not None:
        km[empty_kv_sample] = False
    return qm, km


def autograd(fn, q, k, v, g, q_mask=None, kv_mask=None):
    """(out, dq, dk, dv) of fn(q, k, v, q_mask=, kv_mask=) under torch autograd with the upstream gradient g"""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = fn(q, k, v, q_mask=q_mask, kv_mask=kv_mask)
    out.backward(g)
    return out.detach(), q.grad, k.grad, v.grad
