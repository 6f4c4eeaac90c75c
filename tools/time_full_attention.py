#!/usr/bin/env python3
"""ops.full_attention (fm_full_attention_forward / _backward, csrc/full_attn.hip) next to the torch path it replaces -
transformer.full_attention under autograd, which stores the [N, L, S, H] scores - at the sizes a training step calls it
with: the fine level's windows [4000, 49, 8, 8], the coarse level's [N, 4800, 8, 32] for N = 1 and, if torch fits, 8.  Device
events, every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone and forward + backward,
and the peak memory of each above its inputs.

For the HIP calls: the FLOPs of the algorithm's tile products (forward 2, backward 7 products of 2 L S D each per head) and
the rate reached against the 157.3 TFLOP/s of the float32 matrix instructions.

Then one training-mode LocalFeatureTransformer(attention='full') call (forward + backward) with hip_attention off and on:
the fine layers at [4000, 49, 64] and the 8 coarse layers at N = 1, L = S = 4800.

    python tools/time_full_attention.py [--out FILE]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import ops, synth, transformer  # noqa: E402
from timing import say, timeit, write_log  # noqa: E402

FP32_FLOPS = 157.3e12
SIZES = [(4000, 49, 49, 8, 8), (1, 4800, 4800, 8, 32), (8, 4800, 4800, 8, 32)]


def peak(fn):
    """peak bytes allocated by one call above what is there already"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    del res
    return torch.cuda.max_memory_allocated() - base


def attention_size(dims, dev):
    n, l, s, h, d = dims
    q = torch.as_tensor(synth.normal(5, 1, (n, l, h, d)), device=dev)
    k = torch.as_tensor(synth.normal(5, 2, (n, s, h, d)), device=dev)
    v = torch.as_tensor(synth.normal(5, 3, (n, s, h, d)), device=dev)
    g = torch.as_tensor(synth.normal(5, 4, (n, l, h, d)), device=dev)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(q, k, v)
        return run

    def both(fn):
        return lambda: torch.autograd.grad(fn(qg, kg, vg), (qg, kg, vg), g)

    calls = {("hip", "fwd"): fwd(ops.full_attention), ("torch", "fwd"): fwd(transformer.full_attention),
             ("hip", "fwd+bwd"): both(ops.full_attention), ("torch", "fwd+bwd"): both(transformer.full_attention)}
    say(f"(N, L, S, H, D) = {dims}   scores [N, L, S, H] float32: {n * l * s * h * 4 / 1e6:.1f} MB")
    try:
        for fn in calls.values():                      # every shape and path warmed up
            fn(); fn()
        fits = True
    except torch.OutOfMemoryError:
        fits = False
        torch.cuda.empty_cache()
        say("  torch does not fit in memory at this size: HIP alone")
        calls = {key: fn for key, fn in calls.items() if key[0] == "hip"}
    if fits:                                           # the two compute the same thing at the size that is timed
        gh, gt = calls[("hip", "fwd+bwd")](), calls[("torch", "fwd+bwd")]()
        diff = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, gt))
        del gh, gt
        say(f"  largest relative difference of the gradients, HIP vs torch: {diff:.2e}")
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    mem = {key: peak(fn) for key, fn in calls.items()}
    pair = 2 * n * h * l * s * d                       # FLOPs of one tile product over the whole problem
    ok = None
    for what, flops in (("fwd", 2 * pair), ("fwd+bwd", 9 * pair)):
        hip = ms[("hip", what)]
        slow = max(hip)
        line = f"  {what:8s} HIP {hip[0]:9.4f} / {hip[1]:9.4f} ms  peak {mem[('hip', what)] / 1e6:9.2f} MB"
        if fits:
            ref = ms[("torch", what)]
            line += (f"   torch {ref[0]:9.4f} / {ref[1]:9.4f} ms  peak {mem[('torch', what)] / 1e6:9.2f} MB   "
                     f"torch / HIP (HIP's slower run, torch's faster) {min(ref) / slow:6.2f} x")
            ok = slow <= min(ref)
        say(line)
        say(f"           {flops / 1e9:8.2f} GFLOP of tile products: {flops / (slow * 1e-3) / 1e12:6.2f} TFLOP/s, "
            f"{100 * flops / FP32_FLOPS / (slow * 1e-3):.1f} % of the float32 matrix peak")
    if ok is not None:
        say(f"  HIP forward + backward no slower than torch: {'yes' if ok else 'NO'}")


def module_size(name, cfg, shape, dev):
    d = cfg['d_model']
    x0 = torch.as_tensor(synth.normal(6, 1, (*shape, d)), device=dev)
    x1 = torch.as_tensor(synth.normal(6, 2, (*shape, d)), device=dev)
    mods = {}
    for flag in (False, True):
        m = transformer.LocalFeatureTransformer(cfg, hip_attention=flag)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, d, len(cfg['layer_names'])).items()})
        mods[flag] = m.to(dev).train()

    def step(m):
        def run():
            a, b = x0.detach().requires_grad_(True), x1.detach().requires_grad_(True)
            o0, o1 = m(a, b)
            (o0.sum() + o1.sum()).backward()
            m.zero_grad(set_to_none=True)
        return run
    calls = {flag: step(m) for flag, m in mods.items()}
    try:
        for fn in calls.values():
            fn(); fn()
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        say(f"LocalFeatureTransformer {name} 'full': the torch layers do not fit in memory; not timed")
        return
    ms = {flag: [] for flag in calls}
    for _ in range(2):
        for flag, fn in calls.items():
            ms[flag].append(timeit(fn))
    mem = {flag: peak(fn) for flag, fn in calls.items()}
    say(f"LocalFeatureTransformer {name} 'full': {len(cfg['layer_names'])} layers, tokens {list(shape)} x {d}, training mode, "
        f"forward + backward:  hip_attention off {ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms, peak {mem[False] / 1e6:.1f} MB   "
        f"on {ms[True][0]:8.3f} / {ms[True][1]:8.3f} ms, peak {mem[True] / 1e6:.1f} MB")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_full_attention.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    for dims in SIZES:
        attention_size(dims, dev)
        torch.cuda.empty_cache()
    say()
    module_size("fine", {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross'], 'attention': 'full'}, (4000, 49), dev)
    torch.cuda.empty_cache()
    module_size("coarse", {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross'] * 4, 'attention': 'full'}, (1, 4800), dev)
    write_log(out)


if __name__ == "__main__":
    main()
