#!/usr/bin/env python3
"""The bits the fine training layers produce: a SHA-256 per output tensor of forward and backward of ops.encoder_tail,
ops.qkv_projection (self and cross mode), ops.window_merge (NCHW and channels-last, W = 5 and 7) and ops.linear_attention
(long route) on seeded inputs, for comparing two builds of the library line for line (csrc/fm_tile_device.h: the tile
products and the fold of the slabs decide these bits).  Token counts: 33 - one ragged chunk - and 32768 + 129 - more
than 256 workgroups of a backward, so the grid stride and a full fold both occur; window_merge takes the match counts
whose M W W is nearest.

    python tools/tile_bits.py [LIBRARY]             on the GPU; LIBRARY = a build of the same ABI (default: the tree's)
    python tools/tile_bits.py [LIBRARY] --sizes     no GPU: the four workspace queries over token counts at every edge
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOKENS = (33, 32768 + 129)
EDGES = (1, 31, 32, 33, 127, 128, 129, 32767, 32768, 32769, 1 << 24, (1 << 24) + 1)


def sizes(path):
    lib = ctypes.CDLL(path)
    queries = {"fm_encoder_tail_workspace_bytes": lambda t: (t, 64),
               "fm_qkv_projection_workspace_bytes": lambda t: (t, t, 64),
               "fm_window_merge_workspace_bytes W=5": lambda t: (2, 60, 80, -(-t // 25), 5),
               "fm_window_merge_workspace_bytes W=7": lambda t: (2, 60, 80, -(-t // 49), 7),
               "fm_linear_attention_workspace_bytes": lambda t: (1, t, t, 8, 32)}
    for name, args in queries.items():
        fn = getattr(lib, name.split()[0])
        fn.restype, fn.argtypes = ctypes.c_size_t, None
        for t in EDGES:
            print(f"{name} T={t} {args(t)}: {fn(*[ctypes.c_int(a) for a in args(t)])}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = os.path.abspath(args[0]) if args else os.path.join(ROOT, "featurematching_amd", "lib", "libfmatch_hip.so")
    if "--sizes" in sys.argv:
        return sizes(path)
    import torch
    from featurematching_amd import _lib, ops, synth
    _lib.load(path)
    dev = torch.device("cuda:0")
    stream = iter(range(1, 1 << 20))

    def rnd(*shape, scale=1.0, shift=0.0):
        return (torch.as_tensor(synth.normal(11, next(stream), shape), device=dev) * scale + shift).requires_grad_(True)

    def show(name, fn, leaves, names):
        """fn(*leaves) -> one output or several; their hashes, then those of the gradients under seeded cotangents"""
        outs = fn(*leaves)
        outs = outs if isinstance(outs, tuple) else (outs,)
        cot = [torch.as_tensor(synth.normal(12, next(stream), tuple(o.shape)), device=dev) for o in outs]
        grads = torch.autograd.grad(outs, leaves, cot)
        for label, t in [(f"out{i}", o) for i, o in enumerate(outs)] + [(f"d_{n}", g) for n, g in zip(names, grads)]:
            data = t.detach().contiguous().cpu().numpy().tobytes()
            print(f"{name} {label} {tuple(t.shape)} {hashlib.sha256(data).hexdigest()}", flush=True)

    for T in TOKENS:
        params = [rnd(64, 64, scale=1 / 8), rnd(64, scale=0.1, shift=1.0), rnd(64, scale=0.1), rnd(128, 128, scale=1 / 11),
                  rnd(64, 128, scale=1 / 11), rnd(64, scale=0.1, shift=1.0), rnd(64, scale=0.1)]
        show(f"encoder_tail T={T}", ops.encoder_tail, [rnd(T, 64), rnd(T, 64)] + params,
             ["x", "a", "merge_w", "ln1_w", "ln1_b", "mlp0_w", "mlp2_w", "ln2_w", "ln2_b"])
        w = [rnd(64, 64, scale=1 / 8) for _ in range(3)]
        show(f"qkv_projection self T={T}", lambda x, *ws: ops.qkv_projection(x, x, *ws), [rnd(T, 64)] + w,
             ["x", "wq", "wk", "wv"])
        show(f"qkv_projection cross T={T}", ops.qkv_projection, [rnd(T, 64), rnd(T, 64)] + w, ["x", "src", "wq", "wk", "wv"])
        for W in (5, 7):
            M = max(1, round(T / (W * W)))
            b_ids = torch.as_tensor((synth.hash_u64(13, W, M) % 2).astype("int64"), device=dev)
            cells = torch.as_tensor((synth.hash_u64(14, W, M) % (12 * 16)).astype("int64"), device=dev)
            for layout, fmt in (("NCHW", torch.contiguous_format), ("channels-last", torch.channels_last)):
                feat = rnd(2, 64, 48, 64).detach().contiguous(memory_format=fmt).requires_grad_(True)
                show(f"window_merge W={W} {layout} M={M}",
                     lambda f, ww, c: ops.window_merge(f, ww, c, b_ids, cells, W, 4, 12, 16),
                     [feat, rnd(64, 64, scale=1 / 8), rnd(M, 64)], ["feat", "w_win", "ctx"])
        show(f"linear_attention long L=S={T}", ops.linear_attention,
             [rnd(1, T, 8, 32, scale=0.5), rnd(1, T, 8, 32, scale=0.5), rnd(1, T, 8, 32)], ["q", "k", "v"])


if __name__ == "__main__":
    main()
