"""float64 restatement of the coarse level's training arithmetic with the softmax statistics HANDED IN, for
tests/test_dsm_grad_ref.py (CPU: pins this file against autograd) and tests/test_gpu_dsm_grad.py (the HIP kernels).

The five entry points (include/fmatch.h: fm_dual_softmax_conf_at, fm_dual_softmax_backward, _backward_dense,
fm_coarse_loss_forward / _backward) take the statistics of the two softmaxes as plain pointers:
    A_kl = softmax(sim, dim 1) = exp2(k2 x_kl + ofs_c[l]) / sum_c[l],    B_kl = softmax(sim, dim 2) = exp2(k2 x_kl + ofs_r[k]) / sum_r[k]
with x the raw dot product and k2 = log2(e) / (C temperature) in the float32 roundings fmatch.h spells out.  `stats`
builds them from float64 similarities; `grads` is the closed form at the top of dsm_grad.hip,
    dL/dsim_kl = 2 (g c)_kl - A_kl u_l - B_kl v_k,    u_l = sum_k (g c)_kl,    v_k = sum_l (g c)_kl,
    dL/df0 = dL/dsim . f1 / (C T),    dL/df1 = dL/dsim^T . f0 / (C T),
a function of the array g c alone (a listed (b, i, j, gc) is scattered into it, repeats adding up; a dense G is
multiplied by conf64); `term_bound` is the same sum with every term replaced by its magnitude,
    T0[k, c] = 1 / (C T) sum_l (2 |g c|_kl + A_kl ubar_l + B_kl vbar_k) |f1[l, c]|,      ubar / vbar = sums of |g c|
(T1 likewise with the roles swapped): what a float32 evaluation in any order can be expected to hold a few 2^-24 of,
however much the terms cancel.  `flush_bound` is the absolute allowance for flushed subnormals (1e-36 or so: it matters
on 'peaky' data alone, whose unmatched columns have gradients of 1e-38 and below).

The temperature the kernels are told is a float32; the float64 reference uses that float32's value, so what is measured
is the kernels' arithmetic and not the rounding of 0.1.

CASES is the one table both test files read."""
import collections
import functools

import numpy as np
import torch

import coarse_loss_ref as clr

LOG2E = 1.4426950408889634
LN2 = float(np.log(2.0))


def t32(temperature):
    return float(np.float32(temperature))


def inv_ct(c, temperature):
    return 1.0 / (c * t32(temperature))


def k2_f32(c, temperature):
    """fmatch.h: (1.0f / ((float)C * temperature)) * 1.4426950408889634f, every step in float32"""
    return float((np.float32(1.0) / (np.float32(c) * np.float32(temperature))) * np.float32(LOG2E))


def zsplit(n, r):
    # dsm_zsplit of dsm_grad.hip, compared by reading: wgs = N * ((R + 31) / 32); z = (512 + wgs - 1) / wgs (integer
    # division); clamped to 1 .. 4.  R is the OWNER image's row count: L for side 0, S for side 1.
    wgs = n * ((r + 31) // 32)
    return min(4, max(1, (512 + wgs - 1) // wgs))


def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))


def softmaxes(f0, f1, temperature):
    """dict: x (raw dot products), sim, A = softmax over i, B = softmax over j, conf = A B, lse_r [N, L], lse_c [N, S]"""
    x = np.einsum("nlc,nsc->nls", f0.astype(np.float64), f1.astype(np.float64))
    sim = x * inv_ct(f0.shape[-1], temperature)
    lse_c, lse_r = _lse(sim, 1), _lse(sim, 2)
    a, b = np.exp(sim - lse_c), np.exp(sim - lse_r)
    return dict(x=x, sim=sim, A=a, B=b, conf=a * b, lse_r=lse_r[:, :, 0], lse_c=lse_c[:, 0, :])


def stats(f0, f1, temperature, pitch_r=None, pitch_c=None):
    """(ofs_r, sum_r [N, pitch_r], ofs_c, sum_c [N, pitch_c] float32 with NaN beyond L / S, delta).
    ofs = -max(k2 x) rounded to float32; sum = sum exp2(k2 x + that rounded ofs) in float64, rounded to float32;
    delta = the largest relative error of exp2(-ofs) sum against the float64 log-sum-exp of sim (computed in logs)."""
    n, l, c = f0.shape
    s = f1.shape[1]
    pitch_r, pitch_c = pitch_r or l, pitch_c or s
    sm = softmaxes(f0, f1, temperature)
    y = sm['x'] * k2_f32(c, temperature)
    out, delta = [], 0.0
    for axis, count, pitch, lse in ((2, l, pitch_r, sm['lse_r']), (1, s, pitch_c, sm['lse_c'])):
        ofs = (-y.max(axis=axis)).astype(np.float32)
        tot = np.exp2(y + np.expand_dims(ofs.astype(np.float64), axis)).sum(axis=axis).astype(np.float32)
        delta = max(delta, stats_delta(ofs, tot, lse))
        for v in (ofs, tot):
            full = np.full((n, pitch), np.nan, np.float32)
            full[:, :count] = v
            out.append(full)
    return out[0], out[1], out[2], out[3], delta


def stats_delta(ofs, tot, lse):
    """largest |exp2(-ofs) sum / exp(lse) - 1| of handed statistics [N, R] against a float64 log-sum-exp [N, R]"""
    return float(np.abs(np.expm1(np.log(tot.astype(np.float64)) - ofs.astype(np.float64) * LN2 - lse)).max())


def scatter(shape, ids, values):
    """the [N, L, S] array with values added at ids [K, 3] (a triple listed twice counts twice)"""
    out = np.zeros(shape, np.float64)
    if len(ids):
        np.add.at(out, (ids[:, 0], ids[:, 1], ids[:, 2]), np.asarray(values, np.float64))
    return out


def grads(f0, f1, temperature, gc, sm=None):
    """(d_feat0, d_feat1) float64 of the closed form, gc = g conf [N, L, S] float64"""
    sm = sm or softmaxes(f0, f1, temperature)
    d = 2.0 * gc - sm['A'] * gc.sum(1, keepdims=True) - sm['B'] * gc.sum(2, keepdims=True)
    k = inv_ct(f0.shape[-1], temperature)
    return k * np.einsum("nls,nsc->nlc", d, f1.astype(np.float64)), k * np.einsum("nls,nlc->nsc", d, f0.astype(np.float64))


def term_bound(f0, f1, temperature, gc, sm=None):
    """(T0 [N, L, C], T1 [N, S, C]): the closed form's sums with every term replaced by its magnitude"""
    sm = sm or softmaxes(f0, f1, temperature)
    g = np.abs(gc)
    d = 2.0 * g + sm['A'] * g.sum(1, keepdims=True) + sm['B'] * g.sum(2, keepdims=True)
    k = inv_ct(f0.shape[-1], temperature)
    return (k * np.einsum("nls,nsc->nlc", d, np.abs(f1).astype(np.float64)),
            k * np.einsum("nls,nlc->nsc", d, np.abs(f0).astype(np.float64)))


def flush_bound(f0, f1, temperature, gc):
    """(U0 [N, 1, C], U1 [N, 1, C]): what flushed float32 subnormals can cost an element, absolutely.  Every term is a product
    of an exponential (or a conf) with a weight of at most 2 + max ubar + max vbar and a descriptor element; float32
    arithmetic that flushes subnormals (v_exp_f32 does; torch's float32 kernels may) loses at most 2^-126 of the first factor."""
    g = np.abs(gc)
    w = 2.0 + g.sum(1).max() + g.sum(2).max()
    k = 2.0 ** -126 * inv_ct(f0.shape[-1], temperature) * w
    return (k * np.abs(f1).astype(np.float64).sum(1, keepdims=True), k * np.abs(f0).astype(np.float64).sum(1, keepdims=True))


def autograd(f0, f1, temperature, g_dense, dtype=torch.float64, device="cpu"):
    """(d_feat0, d_feat1, conf) of sum G conf through the reference's expression (coarse_matching_new.py:64-68) by torch"""
    a0 = torch.as_tensor(f0, dtype=dtype, device=device).requires_grad_(True)
    a1 = torch.as_tensor(f1, dtype=dtype, device=device).requires_grad_(True)
    conf = clr.conf_matrix(a0, a1, t32(temperature))
    conf.backward(torch.as_tensor(g_dense, dtype=dtype, device=device))
    return a0.grad.double().cpu().numpy(), a1.grad.double().cpu().numpy(), conf.detach()


# ------------------------------------------------------------------------------------------------------------- data
# 'soft' is what the loss runs on.  dloss/dconf is a function of conf with relative sensitivity 1 / (1 - c) (l_neg' = 1 / (1 - c)
# for the cross entropy, alpha (c^2 / (1 - c) - 2 c log(1 - c)) for the focal loss), and a float32 conf carries 1 - c to
# 2^-24 at best: at the partners of 'borderline' data at 33 x 97 (conf up to 0.99997) any float32 implementation of the
# ABI is 1e-6 / 3e-5 = 3e-2 off in G there, which is the conditioning of the loss and not the sweep.  'soft' keeps every
# conf below 0.95 (checked on the CPU), a factor below 20, with entries either side of the clamp's lower bound.
GAINS = {"borderline": (1.0, 1.0), "scaled": (1.0, 1.0), "peaky": (20.0 ** 0.5, 0.4), "saturated": (1.5, 0.4), "soft": (0.6, 0.6)}
SCALED_ROW, SCALED_BY = 17, 30.0          # 'scaled': row min(L - 1, 17) of image 0, inside the first 32-row tile


def descriptors(kind, n, l, s, c, seed):
    """(f0 [n, l, c], f1 [n, s, c] float32, partner [n, s]: partner[b, j] = the row of image 0 that column j copies).
    Image 1 = a permuted, noisy copy of image 0 (of max(l, s) rows, cut to s); 'flat': every descriptor the same."""
    rs = np.random.RandomState(seed)
    m = max(l, s)
    f0, f1 = np.empty((n, l, c), np.float32), np.empty((n, s, c), np.float32)
    partner = np.empty((n, s), np.int64)
    for b in range(n):
        z0, z1, perm = rs.standard_normal((m, c)), rs.standard_normal((m, c)), rs.permutation(m)
        if kind == "flat":
            f0[b], f1[b] = z0[0], z0[0]
        else:
            g, sigma = GAINS[kind]
            f0[b], f1[b] = (g * z0)[:l], (g * z0[perm] + sigma * z1)[:s]
        partner[b] = perm[:s]
    if kind == "scaled":
        f0[:, min(l - 1, SCALED_ROW)] *= np.float32(SCALED_BY)
    return f0, f1, partner


def entries(spec, conf, partner, seed, skip_sample=None):
    """ids [K, 3] int64 for an entry spec of the case table.
    none | one | several (<= 7 per sample, distinct rows and columns, each row's best free column) | matches (the true
    partners: distinct rows and columns) | row | col (every entry in one row / column of sample 0) | triple3 (several,
    the first triple three times) | k1025 (1025 distinct random triples)"""
    n, l, s = conf.shape
    rs = np.random.RandomState(seed + 1000)
    ids = []
    if spec in ("several", "triple3", "one"):
        for b in range(n):
            free = np.ones(s, bool)
            for i in np.unique(np.linspace(0, l - 1, min(l, s, 7)).astype(np.int64)):
                j = int(np.argmax(np.where(free, conf[b, i], -1.0)))
                free[j] = False
                ids.append((b, int(i), j))
        if spec == "one":
            ids = ids[len(ids) // 2:len(ids) // 2 + 1]
        if spec == "triple3":
            ids = [ids[0]] + ids + [ids[0]]
    elif spec == "matches":
        ids = [(b, int(partner[b, j]), j) for b in range(n) for j in range(s) if partner[b, j] < l]
    elif spec == "row":
        ids = [(0, l // 2, j) for j in range(s)]
    elif spec == "col":
        ids = [(0, i, s // 2) for i in range(l)]
    elif spec == "k1025":
        flat = rs.permutation(n * l * s)[:1025]
        ids = [(int(f // (l * s)), int(f // s % l), int(f % s)) for f in flat]
    elif spec != "none":
        raise ValueError(spec)
    ids = [t for t in ids if t[0] != skip_sample]
    return np.asarray(ids, np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------ cases
# name, L, S, C, N, temperature, data kind, entry spec, pitch_r - L, pitch_c - S, modes, sample without an entry,
# z: the (side 0, side 1) split the case is there for (None: not a split case), bits: listed entries meant to give the same
# bits on two calls (distinct rows and columns)
Case = collections.namedtuple("Case", "name L S C N temp kind entries dr dc modes skip z bits")
LOSSES = ("focal", "cross_entropy")
ALL_MODES = ("sparse", "dense") + LOSSES


def _case(name, l, s, c=64, n=1, temp=0.1, kind="borderline", ent="several", dr=0, dc=0, modes=("sparse", "dense"),
          skip=None, z=None, bits=None):
    bits = ent in ("one", "several", "matches") if bits is None else bits
    return Case(name, l, s, c, n, temp, kind, ent, dr, dc, tuple(modes), skip, z, bits)


def _table():
    t = []
    # tile edges, N = 1: the diagonal of {1, 2, 31, 32, 33, 64, 65} and the lopsided pairs; K = 0, 1, several
    for l, s in [(v, v) for v in (1, 2, 31, 32, 33, 64, 65)] + [(1, 65), (65, 1), (33, 97), (97, 33)]:
        t.append(_case(f"tile{l}x{s}", l, s))
        t.append(_case(f"tile{l}x{s}_k1", l, s, ent="one", modes=("sparse",)))
        t.append(_case(f"tile{l}x{s}_k0", l, s, ent="none", modes=("sparse", "dense0")))
    # split edges: L = 33 (2 row blocks), S = 97 (4): N * 2 either side of 170 / 171, 255 / 256, 511 / 512
    for n in (85, 86, 127, 128, 255, 256):
        t.append(_case(f"split_n{n}", 33, 97, n=n, kind="soft", modes=ALL_MODES, skip=1, z=(zsplit(n, 33), zsplit(n, 97))))
    t.append(_case("split33x33", 33, 33, kind="soft", modes=ALL_MODES, z=(4, 4)))
    # channels: a partial and a full count of each instantiation (64 / 128 / 256) and the smallest valid C
    for c in (4, 60, 64, 68, 128, 252, 256):
        t.append(_case(f"chan{c}", 33, 97, c=c, n=2))
    # pitches of the statistics
    for dr, dc in ((0, 0), (7, 0), (0, 1), (7, 1)):
        t.append(_case(f"pitch_r{dr}_c{dc}", 33, 97, n=2, kind="soft", dr=dr, dc=dc, modes=("sparse", "dense", "focal")))
    # entries
    for ent in ("row", "col", "triple3", "k1025"):
        t.append(_case(f"ent_{ent}", 33, 97, n=2, ent=ent, modes=("sparse",)))
    # data and temperatures
    t.append(_case("data_peaky", 33, 97, n=2, kind="peaky", ent="matches"))
    t.append(_case("data_flat", 33, 97, n=2, kind="flat"))
    t.append(_case("data_scaled", 33, 97, n=2, kind="scaled"))
    for temp in (0.05, 1.0):
        t.append(_case(f"temp{temp}", 33, 97, n=2, temp=temp))
    # 'saturated': conf ~ 1 at the partners, which hold all of G: 2 g c - A u - B v cancels.  Grid shapes (the forward call
    # wants images): 5x7 | 5x7, 3x11 | 1x97, 8x8 | 5x13
    for l, s in ((35, 35), (33, 97), (64, 65)):
        t.append(_case(f"saturated{l}x{s}", l, s, kind="saturated", ent="matches"))
    return collections.OrderedDict((c.name, c) for c in t)


CASES = _table()
GRIDS = {35: (5, 7), 33: (3, 11), 97: (1, 97), 64: (8, 8), 65: (5, 13)}        # the forward call's grids of 'saturated'
REGULAR = [c.name for c in CASES.values() if c.kind in ("borderline", "soft")]  # the set that defines FLOOR


@functools.lru_cache(maxsize=4)
def build(name):
    """the case's inputs: f0, f1, partner, sm (softmaxes), ids, gc (float32 [K], = g conf64 rounded), G (dense float32)"""
    c = CASES[name]
    seed = 7 + 13 * list(CASES).index(name)
    f0, f1, partner = descriptors(c.kind, c.N, c.L, c.S, c.C, seed)
    sm = softmaxes(f0, f1, c.temp)
    ids = entries(c.entries, sm['conf'], partner, seed, c.skip)
    rs = np.random.RandomState(seed + 2000)
    k = len(ids)
    g = -np.ones(k) if c.kind == "saturated" else rs.choice([-1.0, 1.0], k) * (0.5 + rs.random_sample(k))
    gc = (g * sm['conf'][ids[:, 0], ids[:, 1], ids[:, 2]]).astype(np.float32)
    G = rs.standard_normal((c.N, c.L, c.S)).astype(np.float32)
    if c.kind == "saturated":
        G = (1e-3 * G + scatter(G.shape, ids, -np.ones(k))).astype(np.float32)
    return dict(f0=f0, f1=f1, partner=partner, sm=sm, ids=ids, gc=gc, G=G)


def loss_dconf(name, kind, dtype=torch.float64):
    """(the reference's three loss numbers, dloss/dconf [N, L, S]) with the float32-rounded clamp bounds (dtype float32: conf by torch in float32 through the reference's expression, no gradient)"""
    c, d = CASES[name], build(name)
    ids = torch.as_tensor(d['ids'])
    if dtype == torch.float32:
        with torch.no_grad():
            conf = clr.conf_matrix(torch.as_tensor(d['f0']), torch.as_tensor(d['f1']), t32(c.temp))
            return tuple(v.item() for v in clr.masked_loss(conf, clr.gt_mask(conf.shape, *ids.T), kind)), None
    # conf by the reference's own expression, bit for bit: l_neg = -c^gamma log(1 - c) is conditioned like eps / c in ANY
    # precision, so dloss/dconf of a conf one float64 rounding away differs by 1e-10 relative at c = 1e-6
    conf = clr.conf_matrix(torch.as_tensor(d['f0']).double(), torch.as_tensor(d['f1']).double(), t32(c.temp)).requires_grad_(True)
    out = clr.masked_loss(conf, clr.gt_mask(conf.shape, *ids.T), kind, lo=clr.LO32, hi=clr.HI32)
    out[0].backward()
    return tuple(v.item() for v in out), conf.grad.numpy()


@functools.lru_cache(maxsize=8)
def reference(name, mode):
    """dict: gc64 [N, L, S], g_dense (float64 dL/dconf for autograd), ref = (d0, d1), T = (T0, T1), U = flush_bound; loss
    modes: loss64 too"""
    c, d = CASES[name], build(name)
    sm, shape = d['sm'], d['sm']['conf'].shape
    out = {}
    if mode == "sparse":
        gc = scatter(shape, d['ids'], d['gc'])
        k = d['ids']
        g_dense = scatter(shape, k, d['gc'].astype(np.float64) / sm['conf'][k[:, 0], k[:, 1], k[:, 2]]) if len(k) else gc
    elif mode in ("dense", "dense0"):
        g_dense = d['G'].astype(np.float64) * (0.0 if mode == "dense0" else 1.0)
        gc = g_dense * sm['conf']
    else:
        out['loss64'], g_dense = loss_dconf(name, mode)
        gc = g_dense * sm['conf']
    out.update(gc=gc, g_dense=g_dense, ref=grads(d['f0'], d['f1'], c.temp, gc, sm), T=term_bound(d['f0'], d['f1'], c.temp, gc, sm),
               U=flush_bound(d['f0'], d['f1'], c.temp, gc))
    return out
