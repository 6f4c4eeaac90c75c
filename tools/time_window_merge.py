#!/usr/bin/env python3
"""ops.window_merge (fm_window_merge_forward / _backward, csrc/window_merge.hip) next to the torch lines it replaces in a
training step - FinePreprocess.forward's crop with its HIP backward (ops.gather_windows_grad), then merge_feat over
cat[window, expand(context)], under autograd, with the same tensors - for one image of a 640x480 pair: a fine map
[1, 64, 240, 320], 4000 supervised matches on the 60 x 80 grid, W = 7 and W = 5, NCHW and channels-last.  Device events,
every shape warmed up, HIP and torch alternating in one process, two rounds; forward alone and forward + backward (the
map's, the weight's and the context's gradients).

For the HIP calls, the bytes the algorithm needs per call with T = M W W tokens (the map's windows overlap and stay in
the caches: the map is counted once per pass) -
    forward   the map + 256 B T written
    backward  g read twice (the products, the context sum) + the map + g w_win written and read once + the map's gradient
- and the rate achieved against the HBM's 8.0 TB/s.

Then the training-mode FinePreprocess call for both images, forward + backward, with hip_merge off and on.

    python tools/time_window_merge.py [--out FILE]
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import modules, ops, synth  # noqa: E402
from timing import say, timeit, write_log  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
N, HF, WF, HC, WC, STRIDE, M = 1, 240, 320, 60, 80, 4, 4000
LAYOUTS = {"NCHW": torch.contiguous_format, "channels-last": torch.channels_last}


def ids(seed, dev):
    cells = (synth.hash_u64(seed, 1, M) % (HC * WC)).astype('int64')
    return torch.zeros(M, dtype=torch.int64, device=dev), torch.as_tensor(cells, device=dev)


def torch_lines(feat, w_win, ctx, b_ids, cell_ids, w):
    """the parent's lines for one image; ctx stands in for the projected coarse descriptors (64 channels, as down_proj's
    output) and the merge weight is [w_win | identity]: the same crop, concatenation and [.., 128] x [128, 64] product"""
    win = ops.gather_windows_grad(feat, b_ids, cell_ids, w, STRIDE, WC, HC)
    cat = torch.cat([win, ctx[:, None, :].expand(-1, w * w, -1)], -1)
    return F.linear(cat, torch.cat([w_win, torch.eye(64, device=w_win.device)], 1))


def op_size(w, layout, dev):
    feat = torch.as_tensor(synth.normal(3, 1, (N, 64, HF, WF)), device=dev).contiguous(memory_format=LAYOUTS[layout])
    w_win = torch.as_tensor(synth.normal(3, 2, (64, 64)), device=dev) / 8
    ctx, g = (torch.as_tensor(synth.normal(3, k, shape), device=dev) for k, shape in ((3, (M, 64)), (4, (M, w * w, 64))))
    b_ids, cell_ids = ids(3, dev)
    leaves = [t.detach().requires_grad_(True) for t in (feat, w_win, ctx)]
    hip = lambda f, ww, c: ops.window_merge(f, ww, c, b_ids, cell_ids, w, STRIDE, HC, WC)
    ref = lambda f, ww, c: torch_lines(f, ww, c, b_ids, cell_ids, w)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(feat, w_win, ctx)
        return run
    both = lambda fn: (lambda: torch.autograd.grad(fn(*leaves), leaves, g))
    calls = {("hip", "fwd"): fwd(hip), ("torch", "fwd"): fwd(ref), ("hip", "fwd+bwd"): both(hip), ("torch", "fwd+bwd"): both(ref)}
    for fn in calls.values():
        fn(); fn()
    gh, gt = calls[("hip", "fwd+bwd")](), calls[("torch", "fwd+bwd")]()
    diff = max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(gh, gt))
    ms = {key: [] for key in calls}
    for _ in range(2):                                 # two alternating rounds
        for key, fn in calls.items():
            ms[key].append(timeit(fn))
    T, map_bytes = M * w * w, N * 64 * HF * WF * 4
    say(f"window_merge W = {w} {layout:13s} M = {M}   largest relative difference of the gradients, HIP vs torch: {diff:.2e}")
    fwd_bytes = map_bytes + 256 * T
    bwd_bytes = 2 * 256 * T + map_bytes + 2 * 256 * T + map_bytes
    for what, nbytes in (("fwd", fwd_bytes), ("fwd+bwd", fwd_bytes + bwd_bytes)):
        h, r = ms[("hip", what)], ms[("torch", what)]
        slow = max(h)
        say(f"  {what:8s} HIP {h[0]:8.4f} / {h[1]:8.4f} ms   torch {r[0]:8.4f} / {r[1]:8.4f} ms   "
            f"torch / HIP (HIP's slower run, torch's faster) {min(r) / slow:6.2f} x")
        say(f"           needs {nbytes / 1e6:8.2f} MB: {nbytes / (slow * 1e-3) / 1e9:7.1f} GB/s achieved, "
            f"{100 * nbytes / HBM_BYTES_PER_S * 1e3 / slow:.1f} % of 8 TB/s")
    ok = max(ms[("hip", "fwd+bwd")]) <= min(ms[("torch", "fwd+bwd")])
    say(f"  condition (HIP forward + backward no slower than torch): {'met' if ok else 'NOT met'}")
    return ok


def module_size(dev):
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 256}, 'fine': {'d_model': 64}}
    maps = [torch.as_tensor(synth.normal(4, k, (N, 64, HF, WF)), device=dev) for k in (1, 2)]
    descs = [torch.as_tensor(synth.normal(4, k, (N, HC * WC, 256)), device=dev) for k in (3, 4)]
    b_ids, i_ids = ids(4, dev)
    _, j_ids = ids(5, dev)
    data = {'hw0_f': (HF, WF), 'hw0_c': (HC, WC), 'hw1_c': (HC, WC), 'b_ids': b_ids, 'i_ids': i_ids, 'j_ids': j_ids}
    mods = {}
    for flag in (False, True):
        torch.manual_seed(7)
        mods[flag] = modules.FinePreprocess(cfg, hip_merge=flag).to(dev).train()

    def step(m):
        def run():
            leaves = [t.detach().requires_grad_(True) for t in maps + descs]
            w0, w1 = m(*leaves, dict(data))
            (w0.sum() + w1.sum()).backward()
            m.zero_grad(set_to_none=True)
        return run
    calls = {flag: step(m) for flag, m in mods.items()}
    for fn in calls.values():
        fn(); fn()
    ms = {flag: [] for flag in calls}
    for _ in range(2):
        for flag, fn in calls.items():
            ms[flag].append(timeit(fn))
    say(f"FinePreprocess, both images of one 640x480 pair, M = {M}, W = 7, training mode, forward + backward:  hip_merge off "
        f"{ms[False][0]:8.3f} / {ms[False][1]:8.3f} ms   on {ms[True][0]:8.3f} / {ms[True][1]:8.3f} ms")
    ok = max(ms[True]) <= min(ms[False])
    say(f"  condition (on, slower round, no slower than off, faster round): {'met' if ok else 'NOT met'}")
    return ok


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_window_merge.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   times in ms per call, round 1 / round 2 (HIP and torch alternating)")
    results = [(w, layout, op_size(w, layout, dev)) for w in (7, 5) for layout in LAYOUTS]
    say()
    module_ok = module_size(dev)
    say()
    for w, layout, ok in results:
        say(f"window_merge W = {w} {layout}: the condition is {'met' if ok else 'NOT met'}")
    say(f"FinePreprocess: the condition is {'met' if module_ok else 'NOT met'}")
    write_log(out)


if __name__ == "__main__":
    main()
