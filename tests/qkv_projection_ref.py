"""Inputs and the yardstick shared by the q / k / v projection tests (no tests here, nothing runs on a GPU by itself):
seeded x, src, the three upstream gradients and one weight set; the three projection lines of
transformer.EncoderLayer.forward as a function of tensors; autograd through any such function; the error measure of the GPU
tests."""
import numpy as np
import torch
import torch.nn.functional as F

from encoder_tail_ref import _xavier
from train_layers_yardstick import rel_err  # noqa: F401  (the error measure of the GPU tests)

WEIGHTS = ("wq", "wk", "wv")
NAMES_SELF = ("q", "k", "v", "dx", "dWq", "dWk", "dWv")
NAMES_CROSS = ("q", "k", "v", "dx", "dsrc", "dWq", "dWk", "dWv")


def inputs(seed, tx, ts=None, scale=1.0):
    """(x [tx, 64], src [ts, 64] or None, (gq [tx, 64], gk, gv [ts, 64]), weights: name -> [64, 64]), float32 numpy.
    x, src = standard normals times `scale`, the gradients standard normal, the weights xavier-uniform.  ts=None: self mode,
    no src is drawn and gk, gv are [tx, 64]."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((tx, 64)) * scale).astype(np.float32)
    src = None if ts is None else (rng.standard_normal((ts, 64)) * scale).astype(np.float32)
    t = tx if ts is None else ts
    g = (rng.standard_normal((tx, 64)).astype(np.float32), rng.standard_normal((t, 64)).astype(np.float32),
         rng.standard_normal((t, 64)).astype(np.float32))
    w = {name: _xavier(rng, 64, 64) for name in WEIGHTS}
    return x, src, g, w


def proj(x, src, wq, wk, wv):
    """q_proj(x), k_proj(src), v_proj(src) - in the element type of its arguments"""
    return F.linear(x, wq), F.linear(src, wk), F.linear(src, wv)


def proj64(x, src, wq, wk, wv):
    """`proj` in float64 on the up-cast arguments (self mode stays self mode)"""
    xd = x.double()
    return proj(xd, xd if src is x else src.double(), wq.double(), wk.double(), wv.double())


def autograd(fn, x, src, g, weights, weight_grads=True):
    """(q, k, v, dx[, dsrc], dWq, dWk, dWv) of fn(x, src, *weights) under torch autograd with the upstream gradients g =
    (gq, gk, gv), all in fn's element type.  src=None is self mode: fn is called with x twice and there is no dsrc.
    weight_grads=False: no weight requires grad and the tuple ends after the data gradients."""
    x = x.detach().clone().requires_grad_(True)
    s = None if src is None else src.detach().clone().requires_grad_(True)
    weights = [w.detach().clone().requires_grad_(weight_grads) for w in weights]
    out = fn(x, x if s is None else s, *weights)
    torch.autograd.backward(list(out), [t.to(o.dtype) for t, o in zip(g, out)])
    data = (x.grad,) if s is None else (x.grad, s.grad)
    res = tuple(o.detach() for o in out) + data
    if not weight_grads:
        assert all(w.grad is None for w in weights)
        return res
    return res + tuple(w.grad for w in weights)
