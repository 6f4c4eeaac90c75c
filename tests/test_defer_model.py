"""The screening's "sure" rule (deferred exact dot products) as a float32 numpy model, against the exact filters (no GPU).

k_screen_rows parks entry (i, j) when its integer screening product q exceeds min(thr_r[i], thr_c[j]); the exact phase
then forms the float32 dot product x of the two descriptor rows and lists the entry for its row iff
fma(x, k, nmr_i) > -32 and for its column iff fma(x, k, nmc_j) > -32.  With the deferral on, an entry with
    q > max(thr_r[i], thr_c[j]) + D            (D: one slack per sample, sure_slack in csrc/coarse_screen.hip)
is listed for both WITHOUT forming x.  This file replays, in float32 and in the kernels' order of operations,
  * the quantisation of k_prep_split (one step per image from 32 sampled rows, headroom 1.5, clamp at +-127, L1 norms,
    clipped mass),
  * the margins of fm_device.h (q8_margin_raw, margin_log2, neg_stabiliser_log2), sig_threshold and k_thresh,
  * D,
  * the exact phase's dot product (16 lanes, four 4-vectors each, one fma chain, row_sum16's order) and its two filters,
and demands on every tile: each entry the model calls sure passes BOTH exact filters, and its stand-in's exponential is
a normal float32.  Tiles: seeded 'peaked' pairs (where the share of parked entries the rule calls sure is asserted, so it
cannot pass by being vacuous), a row of an image that was not sampled for the step and clips heavily, and adversarial
entries bisected to within a few integer steps of BOTH thresholds plus D (weak partner of a row and of a column that each
own a strong one).  C = 64 and C = 256."""
import numpy as np
import pytest

from featurematching_amd import synth

F = np.float32
LOG2E = F(1.4426950408889634)
SKIP = F(32.0)
HEADROOM = F(1.5)


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def prep(f):
    """k_prep_split for one image [rows, C]: step, int8 plane, L1 norms, clipped mass, largest |x|"""
    rows = f.shape[0]
    ns = min(32, rows)
    sample = f[[t * rows // ns for t in range(ns)]]
    sigma = F(np.abs(sample).max()) * F(HEADROOM / F(127.0))
    inv = F(1.0) / sigma
    q = np.clip(np.rint(f * inv), -127, 127).astype(np.int64)
    ax = np.abs(f)
    clip = np.maximum(ax - F(127.0) * sigma, F(0)).astype(F).sum(1, dtype=F)
    return dict(sigma=sigma, q=q, l1=ax.sum(1, dtype=F), clip=clip, inf=F(ax.max()))


def q8_margin_raw(sa, l1a, ca, sb, l1b, cb, cpad):
    sa, l1a, ca, sb, l1b, cb, cpad = (np.asarray(v, F) for v in (sa, l1a, ca, sb, l1b, cb, cpad))
    clip = ca * (F(127.0) * sb + cb) + F(127.0) * sa * cb
    return (F(0.5) * sa * l1b + F(0.5) * sb * (l1a + F(0.5) * cpad * sa) + clip) * F(1.0001)


def margin_log2(m, inv_ct):
    return np.asarray(m, F) * inv_ct * LOG2E + F(1e-3)


def neg_stab(raw, m, inv_ct):
    mhat = (np.asarray(raw, F) - np.asarray(m, F)) * inv_ct - F(1e-6)
    return -mhat * LOG2E


def sig_threshold(nm, emu, inv_kss):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((-SKIP - np.asarray(emu, F) - np.asarray(nm, F)) * inv_kss) - F(1.0)
        t = np.fmin(np.fmax(t, F(-1.0e9)), F(1.0e9))
    return np.where(np.isnan(t), -1.0e9, t).astype(np.int64)


def sure_slack(emarg, kss, k, l1a_max, inf_b):
    p = k * l1a_max * inf_b
    dq = np.ceil((F(2.0) * emarg + F(7.62939453125e-6) * p + F(0.01)) * (F(1.0) / kss) * F(1.0001))
    return int(dq) + 2 if (emarg < F(60.0) and dq < F(1.0e9)) else 0x3FFFFFFF


def exact_dot(a, b):
    """[E, C] x [E, C] -> [E]: lane l of 16 takes the 4-vectors l, l + 16, l + 32, l + 48 (zero beyond C), one fma chain,
    then row_sum16: lane ^ 1, lane ^ 2, row_half_mirror (7 - l inside 8), row_mirror (15 - l)"""
    e, c = a.shape
    pa, pb = np.zeros((e, 256), F), np.zeros((e, 256), F)
    pa[:, :c], pb[:, :c] = a, b
    pa, pb = pa.reshape(e, 4, 16, 4), pb.reshape(e, 4, 16, 4)          # [entry][q][lane][element]
    sm = np.zeros((e, 16), F)
    for q in range(4):
        for el in range(4):
            sm = fma32(pa[:, q, :, el], pb[:, q, :, el], sm)
    lanes = np.arange(16)
    for perm in (lanes ^ 1, lanes ^ 2, (lanes & 8) | (7 - (lanes & 7)), 15 - lanes):
        sm = (sm + sm[:, perm]).astype(F)
    assert (sm == sm[:, :1]).all()
    return sm[:, 0]


def model(f0, f1, temp=0.1, thr=0.2):
    """one sample through prep, k_thresh and the parking rule; the exact filters of every parked entry"""
    f0, f1 = np.ascontiguousarray(f0, F), np.ascontiguousarray(f1, F)
    (l, c), s = f0.shape, f1.shape[0]
    cpad = F(64 if c <= 64 else (128 if c <= 128 else 256))
    inv_ct = F(1.0) / (F(c) * F(temp))
    k = inv_ct * LOG2E
    a, b = prep(f0), prep(f1)
    sa, sb = a['sigma'], b['sigma']
    ss = sa * sb
    kss = k * ss
    inv_kss = F(1.0) / kss
    qq = a['q'] @ b['q'].T
    l1a_max, l1b_max, ca, cb = a['l1'].max(), b['l1'].max(), a['clip'].max(), b['clip'].max()
    emarg = margin_log2(q8_margin_raw(sa, l1a_max, ca, sb, l1b_max, cb, cpad), inv_ct)

    def side(own, other_inf, mx, n_other, l1_own_first):
        l1 = own['l1']
        dead = F(2.002) * l1 * other_inf * inv_ct + F(1e-3) < (F(np.log2(thr)) + F(np.log2(float(n_other)))) * F(0.69314718)
        bl1 = np.repeat(np.maximum.reduceat(l1, np.arange(0, len(l1), 32)), 32)[:len(l1)]
        if l1_own_first:
            mraw = q8_margin_raw(sa, l1, ca, sb, l1b_max, cb, cpad)
            emu = margin_log2(q8_margin_raw(sa, bl1, ca, sb, l1b_max, cb, cpad), inv_ct)
        else:
            mraw = q8_margin_raw(sa, l1a_max, ca, sb, l1, cb, cpad)
            emu = margin_log2(q8_margin_raw(sa, l1a_max, ca, sb, bl1, cb, cpad), inv_ct)
        nm = np.where(dead, F(-np.inf), neg_stab(ss * mx.astype(F), mraw, inv_ct)).astype(F)
        return nm, sig_threshold(nm, emu, inv_kss), emu
    nmr, thr_r, emu_r = side(a, b['inf'], qq.max(1), s, True)
    nmc, thr_c, emu_c = side(b, a['inf'], qq.max(0), l, False)
    assert (emu_r <= emarg).all() and (emu_c <= emarg).all()          # (what the proof of D uses)
    d = sure_slack(emarg, kss, k, l1a_max, b['inf'])
    lo, hi = np.minimum(thr_r[:, None], thr_c[None, :]), np.maximum(thr_r[:, None], thr_c[None, :])
    parked = qq > lo
    sure = parked & (lo > -1000000000) & (qq > hi + d)
    i, j = np.nonzero(parked)
    x = exact_dot(f0[i], f1[j])
    pass_r, pass_c = fma32(x, k, nmr[i]) > -SKIP, fma32(x, k, nmc[j]) > -SKIP
    stand = (ss * qq[i, j].astype(F)).astype(F)
    return dict(i=i, j=j, q=qq[i, j], sure=sure[i, j], pass_r=pass_r, pass_c=pass_c, d=d, emarg=emarg, kss=kss,
                slack=qq[i, j] - (hi[i, j] + d), arg_r=fma32(stand, k, nmr[i]), arg_c=fma32(stand, k, nmc[j]), thr_r=thr_r, thr_c=thr_c)


def check(m):
    """every sure entry passes both exact filters; its stand-in's two exponentials are normal float32"""
    s = m['sure']
    assert (m['pass_r'][s] & m['pass_c'][s]).all(), "a sure entry fails an exact filter"
    for arg in (m['arg_r'][s], m['arg_c'][s]):
        assert ((arg > -SKIP) & (arg < F(61.0))).all()
    return int(s.sum()), int(len(s))


def peaked(seed, l, s, c, noise=0.4):
    z = synth.normal(seed, 1, (max(l, s), c)).astype(np.float64)
    z *= 4.0 * np.sqrt(c) / np.linalg.norm(z, axis=1, keepdims=True)
    idx = synth.permutation(seed, 3, max(l, s))[:s]
    return z[:l].astype(F), (z[idx] + noise * synth.normal(seed, 2, (s, c))).astype(F)


@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("seed", range(4))
def test_peaked_tiles_sure_entries_pass_both_filters_and_are_most_of_the_parked(seed, c):
    f0, f1 = peaked(500 + seed, 96, 96, c)
    m = model(f0, f1)
    nsure, npark = check(m)
    print(f"peaked C={c} seed={seed}: D={m['d']} emarg={m['emarg']:.3f} kss={m['kss']:.3e} sure {nsure} of {npark} parked")
    assert npark >= 90 and nsure >= 0.9 * npark          # measured: every parked entry of these tiles is sure


@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("factor", [2.5, 8.0])
def test_a_heavily_clipped_row_widens_the_slack_or_switches_the_rule_off(c, factor):
    """row 1 (not among the 32 sampled rows of a 96-row image) scaled: its clipped mass enters every margin"""
    f0, f1 = peaked(600 + c, 96, 96, c)
    base = model(f0, f1)
    f0[1] *= F(factor)
    m = model(f0, f1)
    nsure, npark = check(m)
    print(f"clipped x{factor} C={c}: D {base['d']} -> {m['d']} emarg {base['emarg']:.3f} -> {m['emarg']:.3f} sure {nsure} of {npark}")
    assert m['emarg'] > base['emarg'] and m['d'] > base['d']
    if not m['emarg'] < 60:
        assert nsure == 0


def _cross(seed, c, a_weak):
    """64 x 64: entry (3, 5) is the weak partner (a_weak) of row 3, whose strong partner is column 9, and of column 5,
    whose strong partner is row 7"""
    f0, f1 = peaked(seed, 64, 64, c, noise=0.05)
    f1[9] = f0[3]
    f1[5] = f0[7] + F(a_weak) * f0[3]
    return f0, f1


@pytest.mark.parametrize("c", [64, 256])
def test_entries_within_a_few_integer_steps_of_both_thresholds_plus_the_slack(c):
    seed = 700 + c

    def slack(a_weak):
        m = model(*_cross(seed, c, a_weak))
        sel = (m['i'] == 3) & (m['j'] == 5)
        return (int(m['slack'][sel][0]) if sel.any() else -10 ** 9), m
    lo, hi = 0.0, 1.0
    assert slack(hi)[0] > 0 and slack(lo)[0] <= 0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if slack(mid)[0] > 0 else (mid, hi)
    # one quantisation step of f1[5] in a channel where row 3's int8 value is +-1 moves q by exactly one
    f0, f1 = _cross(seed, c, hi)
    m0 = model(f0, f1)
    q3, sb = prep(f0)['q'][3], prep(f1)['sigma']
    ch = int(np.nonzero((np.abs(q3) == 1) & (np.abs(prep(f1)['q'][5]) < 100))[0][0])
    seen = set()
    for n in range(-8, 9):
        g1 = f1.copy()
        g1[5, ch] += F(n * int(q3[ch])) * sb
        m = model(f0, g1)
        check(m)
        sel = (m['i'] == 3) & (m['j'] == 5)
        assert sel.any()
        sl = int(m['slack'][sel][0])
        seen.add(sl)
        assert bool(m['sure'][sel][0]) == (sl > 0)
        # (3, 5) is near BOTH thresholds: row 3's and column 5's differ by the two strong partners' products only
        assert abs(int(m['thr_r'][3]) - int(m['thr_c'][5])) < 0.1 * abs(int(m['thr_r'][3]))
    print(f"cross C={c}: D={m0['d']} slacks seen {sorted(seen)}")
    assert any(0 < v <= 4 for v in seen) and any(-4 <= v <= 0 for v in seen)
