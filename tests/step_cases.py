"""The small step of the replay, workspace and side-stream tests: bench.py's step (bench.Pair.step, fine_maps, crop, fine)
restated with the ops calls it makes, on a 96 x 128 image - coarse grid 12 x 16 (L = S = 192), fine maps 64 x 48 x 64,
stride 4 - plus its seeded input sets and its yardstick.  Importing this module needs no GPU; `step` and what follows it do.

Input sets.  Coarse descriptors synth.coarse_descriptors(seed, n, 192, C, dist) for seeds 7001 ... 7004 (sample b of a batch
uses seed + b, so a batch of two takes seeds 7001 and 7003), fine maps synth.fine_maps(seed, n, 64, 48, 64), mix weights
synth.mix_weights(seed, W * W).  The EMPTY set has image 1's descriptors all zero: every similarity is 0, conf = 1 / (L S)
everywhere, no match.  COUNTS holds the match counts of the CPU oracle (thr 0.2, border_rm 2); tests/test_step_cases.py
pins them, and pins that no conf of any set lies within 4e-5 of the threshold: the match sets of the HIP path must EQUAL
the oracle's, no guard band.

The yardstick of a step's result is oracle.matcher_ref.match_features on the same arrays under the bars of
tests/test_bench.py: ids equal (in order), mkpts*_c equal, |mconf - ref| <= 1e-5, fine keypoints
within 1e-3 px.  Only the first M rows of a step's capacity-sized outputs count; rows at or beyond M are stale by design.
"""
import functools

import numpy as np

from featurematching_amd import synth

HW_I, HW_C, HW_F = (96, 128), (12, 16), (48, 64)
L, CF, STRIDE = 192, 64, 4
SEEDS = (7001, 7002, 7003, 7004)
THR, BORDER_RM = 0.2, 2
GUARD = 4e-5
ROUTES = ("maps_fused", "maps_nhwc", "windows")

# (C, dist) -> (M of n = 1 for seeds 7001 ... 7004, M of n = 2 for seeds 7001 and 7003)
COUNTS = {
    (64, "peaky"): ((49, 44, 50, 45), (93, 95)),
    (64, "borderline"): ((47, 40, 49, 45), (87, 94)),
    (64, "mixed"): ((35, 38, 34, 32), (73, 66)),
    (256, "peaky"): ((49, 44, 50, 45), (93, 95)),
    (256, "borderline"): ((49, 44, 50, 45), (93, 95)),
    (256, "mixed"): ((35, 38, 36, 31), (73, 67)),
}

# the combination include/fmatch.h names as serving any data (flat similarity, candidate overflow, a clipped int8 step)
GENERAL = dict(dense=True, exact_screening=True, exact_step=True, cand_slots=16, flat=False)


@functools.lru_cache(maxsize=None)
def input_set(dist, seed, n, c, w):
    """numpy arrays of one input set: f0, f1 [n, 192, c], ff0, ff1 [n, 64, 48, 64], mix (w0, b0, w1, b1) and mix0 / mix1
    (weights then bias, float32 [w*w + 1]).  dist "empty": the peaky set of that seed with image 1's descriptors zeroed.
    Cached and shared: callers must not write into the arrays."""
    f0, f1 = synth.coarse_descriptors(seed, n, L, c, "peaky" if dist == "empty" else dist)
    if dist == "empty":
        f1 = np.zeros_like(f1)
    ff0, ff1 = synth.fine_maps(seed, n, CF, *HW_F)
    mix = synth.mix_weights(seed, w * w)
    out = dict(dist=dist, seed=seed, n=n, c=c, w=w, f0=f0, f1=f1, ff0=ff0, ff1=ff1, mix=mix,
               mix0=np.concatenate([mix[0], [mix[1]]]).astype(np.float32),
               mix1=np.concatenate([mix[2], [mix[3]]]).astype(np.float32))
    return out


def name_of(s):
    return f"{s['dist']}{s['seed']} n{s['n']} C{s['c']} W{s['w']}"


@functools.lru_cache(maxsize=None)
def oracle(dist, seed, n, c, w, with_conf=False):
    """oracle.matcher_ref.match_features of input_set(...) as numpy arrays (computed once per set, shared, read-only)"""
    import torch
    from oracle import matcher_ref as orc
    s = input_set(dist, seed, n, c, w)
    ref = orc.match_features(s['f0'], s['f1'], s['ff0'], s['ff1'], HW_I, s['mix'], w=w, thr=THR, border_rm=BORDER_RM)
    ref = {k: np.asarray(v) for k, v in ref.items()}
    if with_conf:
        ref['conf_matrix'] = orc.conf_matrix(*(torch.as_tensor(s[k]) for k in ("f0", "f1")), 0.1).numpy()
    return ref


def oracle_of(s, with_conf=False):
    return oracle(s['dist'], s['seed'], s['n'], s['c'], s['w'], with_conf)


def oracle_errors(got, m, ref):
    """what of the first m rows of a step's outputs (numpy: b_ids, i_ids, j_ids, mkpts0_c, mkpts1_c, mconf, mkpts0_f,
    mkpts1_f; the last two optional) misses the yardstick: a list of strings, empty when every bar holds"""
    bad = []
    if m != ref['i_ids'].shape[0]:
        return [f"M {m}, the oracle has {ref['i_ids'].shape[0]}"]
    for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
        if not np.array_equal(got[k][:m], ref[k]):
            bad.append(f"{k} differs from the oracle")
    if m and not bad:
        err = float(np.abs(got['mconf'][:m].astype(np.float64) - ref['mconf']).max())
        if not err <= 1e-5:
            bad.append(f"mconf off by {err:.3e} > 1e-5")
        for k in ("mkpts0_f", "mkpts1_f"):
            if k in got:
                err = float(np.abs(got[k][:m].astype(np.float64) - ref[k]).max())
                if not err <= 1e-3:
                    bad.append(f"{k} off by {err:.3e} px > 1e-3")
    return bad


def bit_errors(got, want, m, keys=None):
    """keys whose first m rows differ in bits between two steps' outputs (numpy arrays)"""
    return [k for k in (keys or want) if k in got and not np.array_equal(got[k][:m].view(np.uint8), want[k][:m].view(np.uint8))]


# ------------------------------------------------------------------------------------------------ GPU side
class Bufs:
    """the caller-owned window and scratch buffers of a stream: two input sets of one stream may share them
    (bench.Pair(share=...)); sized for n samples and the widest window asked for"""

    def __init__(self, n, w, dev):
        import torch
        self.win0 = torch.empty(n * L, w * w, CF, device=dev)
        self.win1 = torch.empty_like(self.win0)
        self.scratch = torch.empty(n * CF * HW_F[0] * HW_F[1] * 4, dtype=torch.uint8, device=dev)


def to_device(s, route, dev):
    """device tensors of an input set as `route` reads them (maps_nhwc: channels-last storage of the same logical maps)"""
    import torch
    d = {k: torch.as_tensor(s[k], device=dev) for k in ("f0", "f1", "ff0", "ff1", "mix0", "mix1")}
    if route == "maps_nhwc":
        d['ff0'] = d['ff0'].contiguous(memory_format=torch.channels_last)
        d['ff1'] = d['ff1'].contiguous(memory_format=torch.channels_last)
    d.update(n=s['n'], w=s['w'])
    return d


INPUT_KEYS = ("f0", "f1", "ff0", "ff1", "mix0", "mix1")


def load(static, d):
    """copy_ a device-resident input set (to_device) into the static input tensors of a graph, on the current stream"""
    for k in INPUT_KEYS:
        static[k].copy_(d[k])


def coarse(d, mode, **more):
    from featurematching_amd import ops
    return ops.coarse_match_async(d['f0'], d['f1'], HW_C, HW_C, HW_I[0] / HW_C[0], thr=THR, border_rm=BORDER_RM,
                                  cap=d['n'] * L, cand_slots=mode['cand_slots'], dense=mode['dense'],
                                  exact_screening=mode['exact_screening'], exact_step=mode['exact_step'],
                                  flat=bool(mode['flat'] and mode['dense']), **more)


def step(d, route, mode, bufs):
    """Enqueue coarse_match_async(cap = n * L) and the fine half on the current stream; no host synchronisation (the match
    count stays on the device).  Returns (CoarseBuffers, mkpts0_f, mkpts1_f), capacity-sized."""
    from featurematching_amd import ops
    w, scale_f = d['w'], HW_I[0] / HW_F[0]
    if route == "maps_fused":       # image 1's channels-last copy rides in the coarse call's assignment launch
        buf = coarse(d, mode, side_map=d['ff1'], side_scratch=bufs.scratch, cell_maps=False)
        k0, k1 = ops.fine_match_maps(d['ff0'], d['ff1'], buf.b_ids, buf.i_ids, buf.j_ids, w, STRIDE, HW_C[1], HW_C[1],
                                     d['mix0'], d['mix1'], buf.mkpts0_c, buf.mkpts1_c, scale_f, count=buf.count,
                                     scratch=bufs.scratch, prepared=bufs.scratch)
    elif route == "maps_nhwc":
        buf = coarse(d, mode, cell_maps=False)
        k0, k1 = ops.fine_match_maps(d['ff0'], d['ff1'], buf.b_ids, buf.i_ids, buf.j_ids, w, STRIDE, HW_C[1], HW_C[1],
                                     d['mix0'], d['mix1'], buf.mkpts0_c, buf.mkpts1_c, scale_f, count=buf.count,
                                     scratch=bufs.scratch)
    elif route == "windows":
        buf = coarse(d, mode, cell_maps=True)
        m_max, ww = d['n'] * L, w * w
        win0 = bufs.win0.view(-1)[:m_max * ww * CF].view(m_max, ww, CF)     # (the buffers may be sized for a wider window)
        win1 = bufs.win1.view(-1)[:m_max * ww * CF].view(m_max, ww, CF)
        ops.gather_windows_pair(d['ff0'], d['ff1'], buf.b_ids, buf.i_ids, buf.j_ids, w, STRIDE, HW_C, HW_C, buf.cell_maps(),
                                count=buf.count, out0=win0, out1=win1)
        k0, k1 = ops.fine_match(win0, win1, d['mix0'], d['mix1'], buf.mkpts0_c, buf.mkpts1_c, scale_f, count=buf.count)
    else:
        raise ValueError(route)
    return buf, k0, k1


OUT_KEYS = ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c", "mconf", "count", "mkpts0_f", "mkpts1_f")


def outputs(res):
    """the device tensors of a step's result (step(...)'s or a bare coarse call's) by name"""
    buf = res[0] if isinstance(res, tuple) else res
    out = dict(b_ids=buf.b_ids, i_ids=buf.i_ids, j_ids=buf.j_ids, mkpts0_c=buf.mkpts0_c, mkpts1_c=buf.mkpts1_c,
               mconf=buf.mconf, count=buf.count)
    if isinstance(res, tuple):
        out.update(mkpts0_f=res[1], mkpts1_f=res[2])
    return out


def clones(res):
    """clones of a step's outputs and of `count`, enqueued on the current stream"""
    return {k: v.clone() for k, v in outputs(res).items()}


def host(cl):
    return {k: v.cpu().numpy() for k, v in cl.items()}


def learnt_mode(d, stats=False):
    """The mode the library's auto entry point settles on for this input set, found as bench.learnt_hint finds it:
    ops.coarse_match twice (learn, then confirm from the hint), HintMemory.decode of the second call's hint."""
    import torch
    from featurematching_amd import ops
    mem = ops.MODE_MEMORY.snapshot()
    ops.MODE_MEMORY.clear()
    h = 0
    for _ in range(2):
        out = ops.coarse_match(d['f0'], d['f1'], HW_C, HW_C, HW_I[0] / HW_C[0], thr=THR, border_rm=BORDER_RM, stats=stats)
        h = out['_coarse_buffers'].hint
        del out
    ops.MODE_MEMORY.clear()
    for k, v in mem.items():
        ops.MODE_MEMORY.finish(k, v['hint'])
    torch.cuda.synchronize()
    dec = ops.HintMemory.decode(h)
    return dict(dense=dec['dense'], exact_screening=dec['exact'], exact_step=dec['step'], flat=dec['flat'],
                cand_slots=dec['slots'] or None)


def eager(s, route, mode, dev, fine=True, **more):
    """One eager step on fresh buffers on the current stream, synchronised: (M, outputs as numpy, the result).  read_count
    raises when `mode` does not serve the set."""
    import torch
    d = to_device(s, route, dev)
    res = step(d, route, mode, Bufs(s['n'], s['w'], dev)) if fine else coarse(d, mode, **more)
    buf = res[0] if isinstance(res, tuple) else res
    m = buf.read_count()
    torch.cuda.current_stream(dev).synchronize()
    return m, host(outputs(res)), res
