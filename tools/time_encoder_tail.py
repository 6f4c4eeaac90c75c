#!/usr/bin/env python3
"""ops.encoder_tail (fm_encoder_tail_forward / _backward, csrc/encoder_tail.hip) next to the torch path it replaces in a
training step - the three lines of transformer.EncoderLayer.forward behind the attention, under autograd, with the same
parameters - at the sizes a fine-level training step calls it with: [196000, 64] and [100000, 64] (4000 windows of 49 and
of 25 tokens).  Device events, every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone
and forward + backward (all seven parameter gradients included).

For the HIP calls: the bytes and FLOPs the algorithm needs per token (forward 512 B read, 256 B written, 57 344 FLOP;
backward with the forward recomputed 768 B read, 512 B written, 172 032 FLOP), the rate achieved against them, and the
least time the hardware could take - bytes over the HBM's 8.0 TB/s against FLOPs over the 157.3 TFLOP/s of the float32
matrix path; the larger of the two is the bound that applies.

Then one training-mode fine LocalFeatureTransformer call at [4000, 49, 64], forward + backward, with hip_attention=True
and hip_tail off, then on.

    python tools/time_encoder_tail.py [--out FILE]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import ops, synth, transformer  # noqa: E402
from timing import say, timeit, write_log  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FP32_FLOPS = 157.3e12
SIZES = [196000, 100000]
FWD_BYTES, BWD_BYTES, FWD_FLOP, BWD_FLOP = 768, 1280, 57344, 172032      # per token


def torch_tail(layer):
    """the three lines of EncoderLayer.forward behind the attention, with the layer's own modules"""
    def run(x, a):
        msg = layer.norm1(layer.merge(a))
        msg = layer.norm2(layer.mlp(torch.cat([x, msg], dim=-1)))
        return x + msg
    return run


def hip_tail(layer):
    def run(x, a):
        return ops.encoder_tail(x, a, layer.merge.weight, layer.norm1.weight, layer.norm1.bias, layer.mlp[0].weight,
                                layer.mlp[2].weight, layer.norm2.weight, layer.norm2.bias, layer.norm1.eps, layer.norm2.eps)
    return run


def tail_size(T, dev):
    torch.manual_seed(3)
    layer = transformer.EncoderLayer(64, 8).to(dev).train()
    with torch.no_grad():                                # LayerNorm parameters off their initial 1 and 0
        for norm in (layer.norm1, layer.norm2):
            norm.weight.uniform_(0.5, 1.5)
            norm.bias.uniform_(-0.5, 0.5)
    params = [layer.merge.weight, layer.norm1.weight, layer.norm1.bias, layer.mlp[0].weight, layer.mlp[2].weight,
              layer.norm2.weight, layer.norm2.bias]
    x, a, g = (torch.as_tensor(synth.normal(5, i, (T, 64)), device=dev) for i in (1, 2, 3))
    xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(x, a)
        return run

    def both(fn):
        return lambda: torch.autograd.grad(fn(xg, ag), [xg, ag] + params, g)

    calls = {("hip", "fwd"): fwd(hip_tail(layer)), ("torch", "fwd"): fwd(torch_tail(layer)),
             ("hip", "fwd+bwd"): both(hip_tail(layer)), ("torch", "fwd+bwd"): both(torch_tail(layer))}
    for fn in calls.values():                          # every shape and path warmed up
        fn(); fn()
    # the two compute the same thing at the size that is timed
    gh, gt = calls[("hip", "fwd+bwd")](), calls[("torch", "fwd+bwd")]()
    diff = max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(gh, gt))
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    say(f"tail [{T}, 64]   largest relative difference of the nine gradients, HIP vs torch: {diff:.2e}")
    for what, nbytes, flops in (("fwd", FWD_BYTES * T, FWD_FLOP * T), ("fwd+bwd", (FWD_BYTES + BWD_BYTES) * T,
                                                                      (FWD_FLOP + BWD_FLOP) * T)):
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
        m = transformer.LocalFeatureTransformer(cfg, hip_attention=True, hip_tail=flag)
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
    say(f"LocalFeatureTransformer fine: 2 layers, tokens {list(shape)} x 64, training mode, hip_attention=True, forward + "
        f"backward:  hip_tail off {ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms   on {ms[True][0]:8.3f} / {ms[True][1]:8.3f} ms")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_encoder_tail.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    results = [(T, tail_size(T, dev)) for T in SIZES]
    say()
    module_size((4000, 49), dev)
    say()
    for T, ok in results:
        say(f"tail [{T}, 64]: the condition is {'met' if ok else 'NOT met'}")
    write_log(out)


if __name__ == "__main__":
    main()
