#!/usr/bin/env python3
"""ops.qkv_projection (fm_qkv_projection_forward / _backward, csrc/qkv_proj.hip) next to the torch path it replaces in a
training step - the three nn.Linear(64, 64, bias=False) lines at the top of transformer.EncoderLayer.forward, under
autograd, with the same weights - at the sizes a fine-level training step calls it with: [196000, 64] and [100000, 64] (4000
windows of 49 and of 25 tokens), in self mode (source is x) and in cross mode (source another tensor of the same size).
Device events, every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone and forward +
backward (the data gradients and all three weight gradients).

For the HIP calls: the bytes and FLOPs the algorithm needs per token of x (with as many tokens of source) -
    self   forward  256 B read,  768 B written, 24 576 FLOP;   backward 1024 B read, 256 B written, 49 152 FLOP
    cross  forward  512 B read,  768 B written, 24 576 FLOP;   backward 1280 B read, 512 B written, 49 152 FLOP
- the rate achieved against them, and the least time the hardware could take: bytes over the HBM's 8.0 TB/s against FLOPs
over the 157.3 TFLOP/s of the float32 matrix path; the larger of the two is the bound that applies.

Then one training-mode fine LocalFeatureTransformer call at [4000, 49, 64], forward + backward, with hip_attention=True,
hip_tail=True and hip_proj off, then on.

    python tools/time_qkv_projection.py [--out FILE]
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import ops, synth, transformer  # noqa: E402
from timing import say, timeit, write_log  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FP32_FLOPS = 157.3e12
SIZES = [196000, 100000]
# per token: (forward bytes, backward bytes), self and cross; the FLOPs are the mode's own
BYTES = {"self": (256 + 768, 1024 + 256), "cross": (512 + 768, 1280 + 512)}
FWD_FLOP, BWD_FLOP = 3 * 2 * 64 * 64, 6 * 2 * 64 * 64


def torch_proj(x, src, wq, wk, wv):
    return F.linear(x, wq), F.linear(src, wk), F.linear(src, wv)


def op_size(T, mode, dev):
    torch.manual_seed(3)
    layer = transformer.EncoderLayer(64, 8).to(dev).train()
    weights = [layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight]
    x, s, gq, gk, gv = (torch.as_tensor(synth.normal(5, i, (T, 64)), device=dev) for i in (1, 2, 3, 4, 5))
    xg = x.clone().requires_grad_(True)
    sg = s.clone().requires_grad_(True)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(x, x if mode == "self" else s, *weights)
        return run

    def both(fn):
        if mode == "self":
            return lambda: torch.autograd.grad(fn(xg, xg, *weights), [xg] + weights, [gq, gk, gv])
        return lambda: torch.autograd.grad(fn(xg, sg, *weights), [xg, sg] + weights, [gq, gk, gv])

    calls = {("hip", "fwd"): fwd(ops.qkv_projection), ("torch", "fwd"): fwd(torch_proj),
             ("hip", "fwd+bwd"): both(ops.qkv_projection), ("torch", "fwd+bwd"): both(torch_proj)}
    for fn in calls.values():                          # every shape and path warmed up
        fn(); fn()
    # the two compute the same thing at the size that is timed
    gh, gt = calls[("hip", "fwd+bwd")](), calls[("torch", "fwd+bwd")]()
    diff = max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(gh, gt))
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    say(f"qkv {mode:5s} [{T}, 64]   largest relative difference of the gradients, HIP vs torch: {diff:.2e}")
    fb, bb = BYTES[mode]
    for what, nbytes, flops in (("fwd", fb * T, FWD_FLOP * T), ("fwd+bwd", (fb + bb) * T, (FWD_FLOP + BWD_FLOP) * T)):
        hip, ref = ms[("hip", what)], ms[("torch", what)]
        slow = max(hip)
        t_mem, t_alu = nbytes / HBM_BYTES_PER_S * 1e3, flops / FP32_FLOPS * 1e3
        bound = "memory" if t_mem >= t_alu else "float32 MFMA"
        say(f"  {what:8s} HIP {hip[0]:8.4f} / {hip[1]:8.4f} ms   torch {ref[0]:8.4f} / {ref[1]:8.4f} ms   "
            f"torch / HIP (HIP's slower run, torch's faster) {min(ref) / slow:6.2f} x")
        say(f"           needs {nbytes / 1e6:8.2f} MB, {flops / 1e9:7.3f} GFLOP: {nbytes / (slow * 1e-3) / 1e9:7.1f} GB/s, "
            f"{flops / (slow * 1e-3) / 1e12:6.2f} TFLOP/s achieved; bound: {bound} ({max(t_mem, t_alu):.4f} ms at peak, "
            f"{100 * max(t_mem, t_alu) / slow:.1f} % of it reached)")
    ok = max(ms[("hip", "fwd+bwd")]) <= min(ms[("torch", "fwd+bwd")])
    say(f"  condition (HIP forward + backward no slower than torch): {'met' if ok else 'NOT met'}")
    return ok


def module_size(shape, dev):
    cfg = {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}
    x0 = torch.as_tensor(synth.normal(6, 1, (*shape, 64)), device=dev)
    x1 = torch.as_tensor(synth.normal(6, 2, (*shape, 64)), device=dev)
    mods = {}
    for flag in (False, True):
        m = transformer.LocalFeatureTransformer(cfg, hip_attention=True, hip_tail=True, hip_proj=flag)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, 64, 2).items()})
        mods[flag] = m.to(dev).train()

    def step(m):
        def run():
            a, b = x0.detach().requires_grad_(True), x1.detach().requires_grad_(True)
            o0, o1 = m(a, b)
            (o0.sum() + o1.sum()).backward()
            m.zero_grad(set_to_none=True)
        return run
    calls = {flag: step(m) for flag, m in mods.items()}
    for fn in calls.values():
        fn(); fn()
    ms = {flag: [] for flag in calls}
    for _ in range(2):
        for flag, fn in calls.items():
            ms[flag].append(timeit(fn))
    say(f"LocalFeatureTransformer fine: 2 layers, tokens {list(shape)} x 64, training mode, hip_attention=True, hip_tail=True, "
        f"forward + backward:  hip_proj off {ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms   on {ms[True][0]:8.3f} / "
        f"{ms[True][1]:8.3f} ms")
    ok = max(ms[True]) <= min(ms[False])
    say(f"  condition (on, slower round, no slower than off, faster round): {'met' if ok else 'NOT met'}")
    return ok


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_qkv_projection.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    results = [(T, mode, op_size(T, mode, dev)) for T in SIZES for mode in ("self", "cross")]
    say()
    module_ok = module_size((4000, 49), dev)
    say()
    for T, mode, ok in results:
        say(f"qkv {mode} [{T}, 64]: the condition is {'met' if ok else 'NOT met'}")
    say(f"module [4000, 49, 64]: the condition is {'met' if module_ok else 'NOT met'}")
    write_log(out)


if __name__ == "__main__":
    main()
