#!/usr/bin/env python3
"""ops.linear_attention (fm_linear_attention_forward / _backward, csrc/linear_attn.hip) next to the torch path it replaces in
a training step - transformer.linear_attention under autograd - at the sizes a training step calls it with: the fine
level's windows [4000, 49, 64] and [4000, 25, 64], the coarse level's [N, 4800, 256] for N = 1 and 4.  Device events,
every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone and forward + backward.

For the HIP calls: the bytes the algorithm needs (forward reads q, k, v and writes out; backward reads q, k, v, g and writes
dq, dk, dv), the rate achieved against them, and the least time the hardware could take - bytes over the HBM's 8.0 TB/s
against FLOPs over the 157.3 TFLOP/s of the float32 vector units; the larger of the two is the bound that applies.

Then, for information, one training-mode LocalFeatureTransformer call (forward + backward) with hip_attention off and on:
the fine layers at [4000, 49, 64] and the 8 coarse layers at N = 1, L = S = 4800.

    python tools/time_linear_attention.py [--out FILE]
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
SIZES = [("window", (4000, 49, 49, 8, 8)), ("window", (4000, 25, 25, 8, 8)), ("long", (1, 4800, 4800, 8, 32)),
         ("long", (4, 4800, 4800, 8, 32))]


def needs(dims):
    """(forward bytes, backward bytes, forward FLOPs, backward FLOPs) of the algorithm"""
    n, l, s, h, d = dims
    q, kv = n * l * h * d * 4, n * s * h * d * 4
    fwd_b, bwd_b = 2 * q + 2 * kv, 4 * q + 4 * kv
    # forward: A (2 D per k/v element) and Q A (2 D per output); backward: A again or t, dA, dQ, dK, dV: about three times that
    fwd_f = 2 * d * (n * s * h * d) + 2 * d * (n * l * h * d)
    return fwd_b, bwd_b, fwd_f, 3 * fwd_f


def attention_size(route, dims, dev):
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

    calls = {("hip", "fwd"): fwd(ops.linear_attention), ("torch", "fwd"): fwd(transformer.linear_attention),
             ("hip", "fwd+bwd"): both(ops.linear_attention), ("torch", "fwd+bwd"): both(transformer.linear_attention)}
    for fn in calls.values():                          # every shape and path warmed up
        fn(); fn()
    # the two compute the same thing at the size that is timed
    gh, gt = calls[("hip", "fwd+bwd")](), calls[("torch", "fwd+bwd")]()
    diff = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, gt))
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    fwd_b, bwd_b, fwd_f, bwd_f = needs(dims)
    say(f"{route} route  (N, L, S, H, D) = {dims}   largest relative difference of the gradients, HIP vs torch: {diff:.2e}")
    for what, nbytes, flops in (("fwd", fwd_b, fwd_f), ("fwd+bwd", fwd_b + bwd_b, fwd_f + bwd_f)):
        hip, ref = ms[("hip", what)], ms[("torch", what)]
        slow = max(hip)
        t_mem, t_alu = nbytes / HBM_BYTES_PER_S * 1e3, flops / FP32_FLOPS * 1e3
        bound = "memory" if t_mem >= t_alu else "float32 ALU"
        say(f"  {what:8s} HIP {hip[0]:8.4f} / {hip[1]:8.4f} ms   torch {ref[0]:8.4f} / {ref[1]:8.4f} ms   "
            f"torch / HIP (HIP's slower run, torch's faster) {min(ref) / slow:6.2f} x")
        say(f"           needs {nbytes / 1e6:8.2f} MB, {flops / 1e9:7.3f} GFLOP: {nbytes / (slow * 1e-3) / 1e9:7.1f} GB/s achieved; "
            f"bound: {bound} ({max(t_mem, t_alu):.4f} ms at peak, {100 * max(t_mem, t_alu) / slow:.1f} % of it reached)")
    ok = max(ms[("hip", "fwd+bwd")]) <= min(ms[("torch", "fwd+bwd")])
    say(f"  condition (HIP forward + backward no slower than torch): {'met' if ok else 'NOT met'}")
    return ok


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
    for fn in calls.values():
        fn(); fn()
    ms = {flag: [] for flag in calls}
    for _ in range(2):
        for flag, fn in calls.items():
            ms[flag].append(timeit(fn))
    say(f"LocalFeatureTransformer {name}: {len(cfg['layer_names'])} layers, tokens {list(shape)} x {d}, training mode, forward + "
        f"backward:  hip_attention off {ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms   on {ms[True][0]:8.3f} / {ms[True][1]:8.3f} ms")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_linear_attention.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    results = [(route, dims, attention_size(route, dims, dev)) for route, dims in SIZES]
    say()
    module_size("fine", {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}, (4000, 49), dev)
    module_size("coarse", {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross'] * 4}, (1, 4800), dev)
    say()
    for route in ("window", "long"):
        met = all(ok for r, _, ok in results if r == route)
        say(f"{route} route: the condition is {'met at every size' if met else 'NOT met at every size'}")
    write_log(out)


if __name__ == "__main__":
    main()
