"""Float64 yardstick of the coarse stage (coarse_matching_new.py:43-143, eval mode) and the seeded cases of
tests/test_gpu_coarse_edges.py, CPU only.  tests/test_coarse_ref.py pins it against oracle.coarse_match_bruteforce and the
reference-written fixtures (kats.npz, kats_r2.npz, kats_r3.npz) and asserts, for every case the GPU tests run, what lets
them demand EQUAL id lists: the undecided set is empty.

`yardstick(case)` returns
  conf64        the float64 dual softmax (:64-68) [N, L, S], lse_r [N, L] / lse_c [N, S] = logsumexp of sim over dim 2 /
                dim 1 (the natural-log softmax denominators), amax_r / amax_c = the largest |sim| of each row / column;
  the match list of :99-110: conf > thr, the reference's border slicing on both grids (oracle.mask_border: a border of
                at least half a grid side removes everything, 0 removes nothing), conf == row max == column max,
                torch.where order; keypoints in float32 the reference's way (:126-134);
  undecided     the entries a float32 implementation may decide either way: |conf64 - thr| <= BAND, or conf64 > thr -
                BAND and within BAND of the row's or the column's float64 maximum without being that maximum.  A
                CONDITION on the inputs (BAND = 1e-4, five times the suite's guard band), not a measurement;
  e32_conf / e32_lse   the float32 reference's own error against float64 on the same inputs: oracle.conf_matrix, and
                torch.logsumexp of the float32 similarity - what the value bars are multiples of.

Half-precision cases are rounded to their type first and up-cast: every case holds float32 arrays whose values are
exact in the type the GPU call hands over."""
import functools

import numpy as np
import torch

from featurematching_amd import synth
from oracle import matcher_ref as orc

BAND = 1e-4
CHANNELS = (4, 12, 36, 60, 68, 100, 124, 132, 192, 252)
KINDS = ("peaky", "borderline", "mixed")
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
GRIDS = (((1, 1), (1, 1)), ((1, 1), (5, 7)), ((5, 7), (1, 1)), ((1, 40), (40, 1)), ((2, 2), (3, 3)), ((5, 7), (16, 20)),
         ((16, 20), (3, 3)))
TRAIN_CHANNELS = (36, 100, 192)


def round_to(f, dtype):
    """float32 array -> the same values rounded to `dtype` (a key of DTYPES), as float32"""
    return torch.as_tensor(f).to(DTYPES[dtype]).float().numpy()


def sim64(f0, f1, temperature):
    """f0 . f1^T / (C T) in float64 with every entry summed in the same order (a product of two float32 values is exact
    in float64; BLAS may block columns differently, which would break the bit-equality of constructed ties)"""
    a, b = np.asarray(f0, np.float64), np.asarray(f1, np.float64)
    n, l, c = a.shape
    out = np.empty((n, l, b.shape[1]), np.float64)
    step = max(1, (1 << 22) // (b.shape[1] * c))
    for s in range(n):
        for r in range(0, l, step):
            out[s, r:r + step] = (a[s, r:r + step, None, :] * b[s][None]).sum(-1)
    return torch.from_numpy(out / (c * np.float64(temperature)))


def conf64_of(f0, f1, temperature):
    sim = sim64(f0, f1, temperature)
    return torch.softmax(sim, 1) * torch.softmax(sim, 2), sim


def yardstick(case):
    f0, f1 = case['f0'], case['f1']
    hw0, hw1 = case['hw0'], case['hw1']
    thr, border, temp = case.get('thr', 0.2), case.get('border', 2), case.get('temp', 0.1)
    n, l, _ = f0.shape
    s = f1.shape[1]
    conf, sim = conf64_of(f0, f1, temp)
    keep = torch.ones(n, hw0[0], hw0[1], hw1[0], hw1[1], dtype=torch.bool)
    orc.mask_border(keep, border, False)                                    # :101, the reference's slicing
    keep = keep.view(n, l, s)
    rmax, cmax = conf.max(dim=2, keepdim=True)[0], conf.max(dim=1, keepdim=True)[0]
    mask = (conf > thr) & keep & (conf == rmax) & (conf == cmax)            # :99-106
    b, i, j = torch.where(mask)                                             # :109
    near = conf > thr - BAND
    und = ((conf - thr).abs() <= BAND) | (near & (conf >= rmax - BAND) & (conf != rmax)) | \
          (near & (conf >= cmax - BAND) & (conf != cmax))
    scale = case['scale_px']                                                # :126
    s0 = scale * torch.as_tensor(case['scale0'])[b] if case.get('scale0') is not None else scale
    s1 = scale * torch.as_tensor(case['scale1'])[b] if case.get('scale1') is not None else scale
    k0 = torch.stack([i % hw0[1], torch.div(i, hw0[1], rounding_mode='floor')], dim=1) * s0
    k1 = torch.stack([j % hw1[1], torch.div(j, hw1[1], rounding_mode='floor')], dim=1) * s1
    t0, t1 = torch.as_tensor(f0), torch.as_tensor(f1)
    conf32 = orc.conf_matrix(t0, t1, temp)
    c = f0.shape[-1]
    sim32 = torch.einsum("nlc,nsc->nls", t0 / c ** .5, t1 / c ** .5) / temp
    lse_r, lse_c = torch.logsumexp(sim, 2), torch.logsumexp(sim, 1)
    e_lse = max((torch.logsumexp(sim32, 2).double() - lse_r).abs().max().item(),
                (torch.logsumexp(sim32, 1).double() - lse_c).abs().max().item())
    return dict(conf64=conf, sim64=sim, lse_r=lse_r, lse_c=lse_c, amax_r=sim.abs().amax(2), amax_c=sim.abs().amax(1),
                b_ids=b.numpy(), i_ids=i.numpy(), j_ids=j.numpy(), mconf64=conf[b, i, j].numpy(),
                mkpts0_c=k0.to(torch.float32).numpy(), mkpts1_c=k1.to(torch.float32).numpy(),
                undecided=torch.nonzero(und).numpy(), e32_conf=(conf32.double() - conf).abs().max().item(), e32_lse=e_lse,
                matches32=orc.coarse_match(f0, f1, (hw0[0] * scale, hw0[1] * scale), hw0, hw1, thr, border, temp,
                                           case.get('scale0'), case.get('scale1')))


# ---------------------------------------------------------------------------------------------------------- the cases
def _case(f0, f1, hw0, hw1, **kw):
    return dict(f0=np.ascontiguousarray(f0, np.float32), f1=np.ascontiguousarray(f1, np.float32), hw0=tuple(hw0),
                hw1=tuple(hw1), scale_px=8.0, **kw)


def partners(seed, n, l, s, c, kind):
    """image 1 as noisy permuted copies of image 0's descriptors, for any L and S: column j holds the copy of row
    idx[j] when idx[j] < L and a descriptor of its own otherwise (idx = a seeded permutation of max(L, S) per sample)"""
    g, sigma = synth.DISTRIBUTIONS[kind][:2]
    f0 = np.empty((n, l, c), np.float32)
    f1 = np.empty((n, s, c), np.float32)
    for b in range(n):
        z0 = g * synth.normal(seed + b, 1, (max(l, s), c))
        idx = synth.permutation(seed + b, 3, max(l, s))[:s]
        f0[b] = z0[:l]
        f1[b] = z0[idx] + np.float32(sigma) * synth.normal(seed + b, 2, (s, c))
    return f0, f1


def _channel(c, kind, dtype):
    """a. 9x11 against 9x11 cells, N = 2, seed 900 + C, the suite's defaults (thr 0.2, border 2, T 0.1)"""
    f0, f1 = synth.coarse_descriptors(900 + c, 2, 99, c, kind)
    return _case(round_to(f0, dtype), round_to(f1, dtype), (9, 11), (9, 11), dtype=dtype, kind=kind)


def _batch():
    """60 pairs of 5x7 cells at C = 100, kinds alternating (>= 448 row blocks: the batched screening form)"""
    f0 = np.empty((60, 35, 100), np.float32)
    f1 = np.empty_like(f0)
    for b in range(60):
        f0[b:b + 1], f1[b:b + 1] = synth.coarse_descriptors(1700 + b, 1, 35, 100, KINDS[b % 3])
    return _case(f0, f1, (5, 7), (5, 7), border=1, kind="mixed")


def grid_kind(c):
    return "peaky" if c == 256 else "borderline"


def _grid(c, g):
    hw0, hw1 = GRIDS[g]
    f0, f1 = partners(1300 + 10 * g + (c == 100), 2, hw0[0] * hw0[1], hw1[0] * hw1[1], c, grid_kind(c))
    return _case(f0, f1, hw0, hw1, border=0, kind=grid_kind(c))


ARG_C, ARG_HW0, ARG_HW1 = 100, (6, 7), (9, 5)
ARG_CASES = {**{f"border{b}_{k}": dict(border=b, kind=k) for b in (0, 1, 2, 3) for k in ("peaky", "borderline")},
             "thr0p02": dict(thr=0.02, border=1, kind="borderline"), "thr0p5": dict(thr=0.5, border=1, kind="borderline"),
             "thr0p9": dict(thr=0.9, border=1, kind="peaky"), "temp0p05": dict(temp=0.05, border=1, kind="borderline"),
             "temp1": dict(temp=1.0, border=1, kind="peaky"), "scales": dict(border=1, kind="peaky", n=3, scales=True),
             "cap": dict(border=0, kind="peaky")}


def _arg(name):
    kw = dict(ARG_CASES[name])
    n, scales = kw.pop('n', 2), kw.pop('scales', False)
    f0, f1 = partners(1500, n, 42, 45, ARG_C, kw['kind'])
    if scales:
        kw['scale0'] = (0.5 + 2.0 * synth.uniform(1500, 8, 2 * n)).astype(np.float32).reshape(n, 2)
        kw['scale1'] = (0.5 + 2.0 * synth.uniform(1500, 9, 2 * n)).astype(np.float32).reshape(n, 2)
    return _case(f0, f1, ARG_HW0, ARG_HW1, **kw)


def _train(c):
    """e. ragged L != S (15x17 against 11x13), N = 2, the data of the dense-gradient test of test_gpu_parity.py"""
    l, s = 15 * 17, 11 * 13
    f0, f1 = synth.coarse_descriptors(1900 + c, 2, l, c, "borderline")
    return _case(f0[:, :l], f1[:, :s], (15, 17), (11, 13), kind="borderline")


def _kat(fixture, name):
    from helpers import load_kats
    k = load_kats(fixture)[name]
    hw = [int(v) for v in k['hw']]
    return _case(k['f0'], k['f1'], hw[4:6], hw[6:8], thr=float(k['cfg'][0]), border=int(k['cfg'][1]), temp=float(k['cfg'][2]),
                 scale0=k.get('scale0'), scale1=k.get('scale1'), fixture=k, kind="kat") | dict(scale_px=hw[0] / hw[4])


KATS_R3 = ("c36_scale", "c100_tie", "c192")
_BUILDERS = {"channel": _channel, "batch": _batch, "grid": _grid, "arg": _arg, "train": _train, "kat": _kat}


def gpu_case_keys():
    """every case tests/test_gpu_coarse_edges.py runs"""
    keys = [("channel", c, k, d) for c in CHANNELS for k in KINDS for d in DTYPES]
    keys += [("batch",)] + [("grid", c, g) for c in (256, 100) for g in range(len(GRIDS))]
    keys += [("arg", name) for name in ARG_CASES] + [("train", c) for c in TRAIN_CHANNELS]
    return keys + [("kat", "kats_r3", name) for name in KATS_R3]


def built_empty(key):
    """the cases whose border removes every cell"""
    return key[0] == "arg" and ARG_CASES[key[1]].get('border') == 3


@functools.lru_cache(maxsize=None)
def case(key):
    return _BUILDERS[key[0]](*key[1:])


@functools.lru_cache(maxsize=None)
def yard(key):
    return yardstick(case(key))


# ------------------------------------------------------------------------------------------- training references (e)
def supervision(key, k_random=60):
    """distinct (b, i, j) triples [K, 3]: every third match of the yardstick + seeded random entries"""
    y, cs = yard(key), case(key)
    n, l, _ = cs['f0'].shape
    s = cs['f1'].shape[1]
    u = synth.uniform(77, 1, 3 * k_random).reshape(3, k_random)
    rnd = np.stack([(u[0] * n).astype(np.int64), (u[1] * l).astype(np.int64), (u[2] * s).astype(np.int64)], 1)
    ids = np.concatenate([np.stack([y['b_ids'][::3], y['i_ids'][::3], y['j_ids'][::3]], 1), rnd], 0)
    return np.unique(ids, axis=0)


def _leaves64(cs):
    return (torch.as_tensor(cs['f0'], dtype=torch.float64).requires_grad_(True),
            torch.as_tensor(cs['f1'], dtype=torch.float64).requires_grad_(True))


@functools.lru_cache(maxsize=None)
def train_reference(key):
    """float64 autograd through the reference's expression (coarse_loss_ref.conf_matrix = :64-68) for the four training
    entry points: the sparse weighted sum (fm_dual_softmax_backward), the dense weighted sum (_dense), the two losses."""
    import coarse_loss_ref as lr
    cs = case(key)
    ids = torch.as_tensor(supervision(key))
    n, l, _ = cs['f0'].shape
    s = cs['f1'].shape[1]
    g_sparse = torch.as_tensor(synth.normal(78, 1, (ids.shape[0],)))
    g_dense = torch.as_tensor(synth.normal(78, 2, (n, l, s)))
    out = dict(ids=ids.numpy(), g_sparse=g_sparse.numpy(), g_dense=g_dense.numpy())
    a0, a1 = _leaves64(cs)
    conf = lr.conf_matrix(a0, a1)
    out['conf_at'] = conf[ids[:, 0], ids[:, 1], ids[:, 2]].detach().numpy()
    (conf[ids[:, 0], ids[:, 1], ids[:, 2]] * g_sparse.double()).sum().backward()
    out['sparse'] = (a0.grad.numpy(), a1.grad.numpy())
    a0, a1 = _leaves64(cs)
    (lr.conf_matrix(a0, a1) * g_dense.double()).sum().backward()
    out['dense'] = (a0.grad.numpy(), a1.grad.numpy())
    mask = lr.gt_mask((n, l, s), ids[:, 0], ids[:, 1], ids[:, 2])
    for kind in ("focal", "cross_entropy"):
        a0, a1 = _leaves64(cs)
        l64 = lr.masked_loss(lr.conf_matrix(a0, a1), mask, kind, lo=lr.LO32, hi=lr.HI32)
        l64[0].backward()
        with torch.no_grad():
            l32 = lr.masked_loss(lr.conf_matrix(torch.as_tensor(cs['f0']), torch.as_tensor(cs['f1'])), mask, kind)
        out[kind] = dict(loss64=[v.item() for v in l64], loss32=[v.item() for v in l32], grads=(a0.grad.numpy(), a1.grad.numpy()))
    return out
