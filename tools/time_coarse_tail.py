#!/usr/bin/env python3
"""ops.coarse_tail (fm_coarse_tail_forward / _backward, csrc/coarse_tail.hip) next to the torch path it replaces in a
training step - the three lines of transformer.EncoderLayer.forward behind the attention at d_model 256, under autograd,
with the same parameters - at [4800, 256] (one 640x480 image's coarse tokens) and [64 * 4800, 256] (a batch of 64).
Device events, every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone and forward +
backward (all seven parameter gradients included), and the peak memory of forward + backward above the inputs.

For the HIP calls: the FLOPs the algorithm needs per token (forward 917 504; backward with the forward recomputed
2 752 512), the rate achieved against the 157.3 TFLOP/s of the float32 matrix path.

Then one training-mode coarse LocalFeatureTransformer call (8 layers) at [1, 4800, 256], forward + backward, with
hip_attention=True and hip_coarse_tail off, then on.

    python tools/time_coarse_tail.py [--out FILE]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import ops, synth, transformer  # noqa: E402
from timing import say, timeit, write_log  # noqa: E402

FP32_FLOPS = 157.3e12
SIZES = [4800, 64 * 4800]
FWD_FLOP = 2 * (256 * 256 + 512 * 512 + 512 * 256)      # per token
BWD_FLOP = 3 * FWD_FLOP                                  # the forward again, the data gradients, the weight gradients


def torch_tail(layer):
    """the three lines of EncoderLayer.forward behind the attention, with the layer's own modules"""
    def run(x, a):
        msg = layer.norm1(layer.merge(a))
        msg = layer.norm2(layer.mlp(torch.cat([x, msg], dim=-1)))
        return x + msg
    return run


def hip_tail(layer):
    def run(x, a):
        return ops.coarse_tail(x, a, layer.merge.weight, layer.norm1.weight, layer.norm1.bias, layer.mlp[0].weight,
                               layer.mlp[2].weight, layer.norm2.weight, layer.norm2.bias, layer.norm1.eps, layer.norm2.eps)
    return run


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def tail_size(T, dev):
    torch.manual_seed(3)
    layer = transformer.EncoderLayer(256, 8).to(dev).train()
    with torch.no_grad():                                # LayerNorm parameters off their initial 1 and 0
        for norm in (layer.norm1, layer.norm2):
            norm.weight.uniform_(0.5, 1.5)
            norm.bias.uniform_(-0.5, 0.5)
    params = [layer.merge.weight, layer.norm1.weight, layer.norm1.bias, layer.mlp[0].weight, layer.mlp[2].weight,
              layer.norm2.weight, layer.norm2.bias]
    gen = torch.Generator(device=dev).manual_seed(5)
    x, a, g = (torch.randn(T, 256, device=dev, generator=gen) for _ in range(3))
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
    del gh, gt
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    say(f"tail [{T}, 256]   largest relative difference of the nine gradients, HIP vs torch: {diff:.2e}")
    for what, flops in (("fwd", FWD_FLOP * T), ("fwd+bwd", (FWD_FLOP + BWD_FLOP) * T)):
        hip, ref = ms[("hip", what)], ms[("torch", what)]
        slow = max(hip)
        spread = max(abs(v[0] - v[1]) / min(v) for v in (hip, ref))
        say(f"  {what:8s} HIP {hip[0]:9.4f} / {hip[1]:9.4f} ms   torch {ref[0]:9.4f} / {ref[1]:9.4f} ms   "
            f"torch / HIP (HIP's slower run, torch's faster) {min(ref) / slow:6.2f} x   two-round spread {100 * spread:.1f} %")
        say(f"           needs {flops / 1e9:8.3f} GFLOP: {flops / (slow * 1e-3) / 1e12:6.2f} TFLOP/s achieved, "
            f"{100 * flops / FP32_FLOPS * 1e3 / slow:.1f} % of the float32 matrix path's peak")
    mem = {k: peak(calls[(k, "fwd+bwd")]) for k in ("hip", "torch")}
    say(f"  peak memory of forward + backward above the inputs: HIP {mem['hip'] / 2**20:9.1f} MiB   torch "
        f"{mem['torch'] / 2**20:9.1f} MiB   ({mem['torch'] / max(mem['hip'], 1):.2f} x)")
    ok = max(ms[("hip", "fwd+bwd")]) <= min(ms[("torch", "fwd+bwd")])
    say(f"  HIP forward + backward no slower than torch: {'yes' if ok else 'NO'}")
    return ok


def module_size(shape, dev):
    cfg = {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross'] * 4}
    x0 = torch.as_tensor(synth.normal(6, 1, (*shape, 256)), device=dev)
    x1 = torch.as_tensor(synth.normal(6, 2, (*shape, 256)), device=dev)
    mods = {}
    for flag in (False, True):
        m = transformer.LocalFeatureTransformer(cfg, hip_attention=True, hip_coarse_tail=flag)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, 256, 8).items()})
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
    say(f"LocalFeatureTransformer coarse: 8 layers, tokens {list(shape)} x 256, training mode, hip_attention=True, forward + "
        f"backward:  hip_coarse_tail off {ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms   on {ms[True][0]:8.3f} / "
        f"{ms[True][1]:8.3f} ms")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_coarse_tail.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    results = [(T, tail_size(T, dev)) for T in SIZES]
    say()
    module_size((1, 4800), dev)
    say()
    for T, ok in results:
        say(f"tail [{T}, 256]: HIP forward + backward no slower than torch: {'yes' if ok else 'NO'}")
    write_log(out)


if __name__ == "__main__":
    main()
