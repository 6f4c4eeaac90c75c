#!/usr/bin/env python3
"""What does the operand split of k_fine_tf (csrc/fine_tf.hip) cost the windows of SMALL magnitude?  No GPU: the fine
context layers in float64 on the CPU, with one or all of the tensors the kernel packs into float16 operands replaced
by what the split keeps of them: x -> (hi + lo) / 2^e with hi = rtz_f16(2^e x), lo = rtz_f16(2^e x - hi), e = the
activation scale's exponent.  Below 2^-3 in the operand scale the lo half is a float16 SUBNORMAL: an absolute
resolution of 2^-24 instead of 22 significant bits (--flush drops such halves altogether; the kernel's figures on an
MI355X match the run without it).  Products and sums stay float64, so the figures are the split's share of the error.

    python tools/emulate_fine_tf_split.py [--gain 1e-3] [--scale 8] [--v-over-s] [--flush]

--v-over-s splits v / S, as kv_phase did before it applied 1 / S to the KV sums instead.  The inputs are those of
tests/test_gpu_ctx_layers.py::test_a (tests/ctx_layers_ref.py: fine_inputs), the matches of the given gain.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctx_layers_ref as cr  # noqa: E402  (the float64 layers and the seeded inputs)

OPERANDS = ("x", "Q", "K", "V", "kv", "att", "m1", "hid")


def rtz16(t):
    """float64 tensor -> its float16 value rounded toward zero, as float64"""
    a = t.numpy()
    h = a.astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) > np.abs(a), np.nextafter(h, np.float16(0)), h)
    return torch.as_tensor(h.astype(np.float64))


def split(t, e, flush):
    ts = t * 2.0 ** e
    hi = rtz16(ts)
    lo = rtz16(ts - hi)
    if flush:
        hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    return (hi + lo) / 2.0 ** e


def layer(x, src, w, p, e, on, v_over_s, flush):
    n, l, d = x.shape
    s, nh = src.shape[1], 8
    g = lambda name: torch.as_tensor(w[p + name]).double()
    op = lambda t, name: split(t, e, flush) if name in on else t
    xs, xq = op(src, "x"), op(x, "x")
    q, k, v = xq @ g("q_proj.weight").T, xs @ g("k_proj.weight").T, xs @ g("v_proj.weight").T
    Q = op(cr._elu1(q), "Q").view(n, l, nh, d // nh)
    K = op(cr._elu1(k), "K").view(n, s, nh, d // nh)
    if v_over_s:
        kv = torch.einsum("nshd,nshv->nhdv", K, op(v / s, "V").view(n, s, nh, d // nh))
    else:
        kv = torch.einsum("nshd,nshv->nhdv", K, op(v, "V").view(n, s, nh, d // nh)) / s
    kv = op(kv, "kv")
    z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(1)) + 1e-6)
    att = op((torch.einsum("nlhd,nhdv->nlhv", Q, kv) * z[..., None] * s).reshape(n, l, d), "att")
    ln = torch.nn.functional.layer_norm
    m1 = op(ln(att @ g("merge.weight").T, (d,), g("norm1.weight"), g("norm1.bias"), 1e-5), "m1")
    hid = op(torch.relu(torch.cat([xq, m1], 2) @ g("mlp.0.weight").T), "hid")
    return x + ln(hid @ g("mlp.2.weight").T, (d,), g("norm2.weight"), g("norm2.bias"), 1e-5)


def run(x0, x1, w, e, on, v_over_s, flush):
    x0, x1 = torch.as_tensor(x0).double(), torch.as_tensor(x1).double()
    x0, x1 = (layer(t, t, w, "layers.0.", e, on, v_over_s, flush) for t in (x0, x1))
    x0 = layer(x0, x1, w, "layers.1.", e, on, v_over_s, flush)
    return x0, layer(x1, x0, w, "layers.1.", e, on, v_over_s, flush)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gain", type=float, default=1e-3)
    ap.add_argument("--scale", type=int, default=8, choices=[8, 4, 0, -4])
    ap.add_argument("--v-over-s", action="store_true")
    ap.add_argument("--flush", action="store_true")
    a = ap.parse_args()
    w = cr.fine_weights()
    for win in (5, 7):
        sel = cr.fine_gains() == np.float32(a.gain)
        x0, x1 = (t[sel] for t in cr.fine_inputs(win))
        o64 = cr.ctx_layers64(x0, x1, w, cr.FINE_LAYERS)
        for on in [(name,) for name in OPERANDS] + [OPERANDS]:
            o = run(x0, x1, w, a.scale, on, a.v_over_s, a.flush)
            err = max((p - q).abs().max().item() for p, q in zip(o, o64))
            print(f"W={win} gain {a.gain:g} scale 2^{a.scale} split of {'+'.join(on):<28} max|out - out64| {err:.2e}")


if __name__ == "__main__":
    main()
