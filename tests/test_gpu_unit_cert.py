"""The unit certificate of the screening on the GPU: forced off against forced on (fm_debug_unit_cert), bit for bit.

With the certificate on, the max pass publishes every 32 x 32 unit's runner-up (umax2) and the place of its maximum
(upos), k_thresh the smallest integer threshold of every row block / column unit, and k_screen_rows resolves a unit with
umax2 <= Tmin without sweeping it (tests/test_unit_cert_model.py pins the rule on the CPU).  The parked set must be the
same entry for entry, so every output of the coarse stage must be IDENTICAL to the run with the certificate off: ids,
conf bits, keypoints, count, device flags, dense_cnt.  The `on` run is also held against the float64 yardstick of
tests/coarse_ref.py at the bars of tests/test_gpu_coarse_edges.py.

Pairs: descriptors of norm 4 sqrt(C) ('peaky' gain, partners = copies + 0.4 noise: peak similarity 160, everything else
below ~90 at C = 64 and ~45 at C = 256, the significance window is 32 ln 2 = 22), partners scattered by a seeded
permutation; lines without a partner are scaled by 1e-4 (dead lines: nothing is significant on their account).  Unit
(row block 0, column unit 0) of sample 0 is cleared of peaks and then planted:
  one      one peak at (3, 5)                                    -> certified, upos names (3, 5)
  two      peaks at (3, 5) and (10, 20)                          -> not certified
  row      columns 5 and 20 both partners of row 3 (20: 0.9 x)   -> not certified
  col      rows 3 and 10 both partners of column 5 (10: 0.9 x)   -> not certified
  tie      column 20 == column 5 exactly                         -> umax2 == umax, not certified
  above / below   column 20 = alpha x column 5, alpha bisected so that the second entry's INTEGER product is just above /
           just below row 3's integer threshold (read back from the workspace)   -> not certified either way
  negative every product of the unit negative (a common component of opposite sign)   -> unit not live, umax < 0
  tails    L = 70, S = 50 (last row block and unit partly padding, one peak planted in the corner unit; lines without
           partner dead) and L = 65, S = 129 with
           the peak of row 64 at column 128: a unit whose only valid entry is its maximum -> umax2 = kQMasked, certified;
           every unit with exactly one planted peak certifies.
The counter of certified live units (counted while the switch forces the certificate on) must be 0 with the switch off
and, with it on, lie between the certified units that surely hold a significant entry and all certified units (both
counted from the workspace's arrays); cases 'one', the tails and the headline-size pair demand that it is > 0: the test
cannot pass with the feature silently off."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, synth

import coarse_ref as cr
import test_gpu_coarse_edges as edges

pytestmark = pytest.mark.gpu
K_Q_MASKED = -(1 << 30)
OFF, ON = 1, 2
HW = {96: (8, 12), 70: (7, 10), 50: (5, 10), 65: (5, 13), 129: (3, 43), 4800: (60, 80)}


def _base(seed, n, l, s, c, idx=None):
    """f0, f1, idx [n][s] (column j is the partner of row idx[j], or has none when idx[j] >= l; idx given: that map)"""
    f0 = np.empty((n, l, c), np.float32)
    f1 = np.empty((n, s, c), np.float32)
    idx = np.stack([synth.permutation(seed + b, 3, max(l, s))[:s] for b in range(n)]) if idx is None else idx
    for b in range(n):
        z = synth.normal(seed + b, 1, (max(l, s), c)).astype(np.float64)
        z *= 4.0 * np.sqrt(c) / np.linalg.norm(z, axis=1, keepdims=True)
        f0[b] = z[:l]
        f1[b] = z[idx[b]] + 0.4 * synth.normal(seed + b, 2, (s, c))
    return f0, f1, idx


def _finish(f0, f1, idx):
    """lines without a partner become dead lines"""
    n, l, _ = f0.shape
    for b in range(n):
        has = np.zeros(max(l, f1.shape[1]), bool)
        has[idx[b]] = True
        f0[b, ~has[:l]] *= 1e-4
        f1[b, idx[b] >= l] *= 1e-4


def _clear_unit00(idx):
    """no partner pair inside rows 0..31 x columns 0..31 of sample 0 (swaps with pairs that lie outside both)"""
    p = idx[0]
    inside = [j for j in range(32) if p[j] < 32]
    outside = [j for j in range(32, len(p)) if p[j] >= 32]
    assert len(outside) >= len(inside)
    for j, k in zip(inside, outside):
        p[j], p[k] = p[k], p[j]


def _plant(idx, row, col):
    p = idx[0]
    k = int(np.nonzero(p == row)[0][0])
    p[col], p[k] = p[k], p[col]


@functools.lru_cache(maxsize=None)
def _pair(name, c, n, alpha=None):
    if name in ("tails70", "tails65"):
        l, s = (70, 50) if name == "tails70" else (65, 129)
        f0, f1, idx = _base(4100 + c, n, l, s, c)
        if name == "tails70":                          # the corner unit (rows 64..69 x columns 32..49) holds ONE peak: (66, 40)
            for b in range(n):
                p = idx[b]
                inside = [j for j in range(32, 50) if 64 <= p[j] < 70]
                outside = [k for k in range(32) if not 64 <= p[k] < 70]
                for j, k in zip(inside, outside):
                    p[j], p[k] = p[k], p[j]
                where = np.nonzero(p == 66)[0]
                if where.size:
                    p[40], p[where[0]] = p[where[0]], p[40]
                else:
                    p[40] = 66                         # (the row column 40 belonged to keeps no partner: a dead line)
            f0, f1, idx = _base(4100 + c, n, l, s, c, idx)
        if name == "tails65":
            for b in range(n):
                k = int(np.nonzero(idx[b] == 64)[0][0])
                idx[b][128], idx[b][k] = idx[b][k], idx[b][128]
            f0, f1, idx = _base(4100 + c, n, l, s, c, idx)
    else:
        l = s = 96
        f0, f1, idx = _base(4000 + c, n, l, s, c)
        _clear_unit00(idx)
        if name != "negative":
            _plant(idx, 3, 5)
        if name == "two":
            _plant(idx, 10, 20)
        f0, f1, idx = _base(4000 + c, n, l, s, c, idx)
        if name in ("row", "tie", "scaled"):          # column 20 joins row 3; its former partner row loses its own
            f0[0, idx[0][20]] *= 1e-4
            noise = 0.4 * synth.normal(77, 9, (c,))
            f1[0, 20] = {"row": 0.9 * f0[0, 3] + noise, "tie": f1[0, 5], "scaled": np.float32(alpha or 1) * f1[0, 5]}[name]
        if name == "col":                             # row 10 joins column 5; its former partner column loses its own
            f1[0, int(np.nonzero(idx[0] == 10)[0][0])] *= 1e-4
            f0[0, 10] = 0.9 * f0[0, 3] + 0.1 * synth.normal(78, 9, (c,))
        if name == "negative":
            e = synth.normal(79, 9, (c,)).astype(np.float64)
            e *= np.sqrt(3000.0 * np.sqrt(c / 256.0)) / np.linalg.norm(e)      # -|e|^2 outweighs 4.5 sigma of the rest
            f0[0, :32] += e
            f1[0, :32] -= e
    _finish(f0, f1, idx)
    cs = cr._case(f0, f1, HW[l], HW[s], border=0)
    cs['idx'] = idx
    return cs


@functools.lru_cache(maxsize=None)
def _yard(name, c, n, alpha=None):
    return cr.yardstick(_pair(name, c, n, alpha))


def _arrays(out):
    """the certificate's arrays of a finished call, from its workspace"""
    lib = _lib.load()
    n, l, s, c = out['shape']
    lay = (C.c_int64 * 9)()
    assert lib.fm_debug_unit_cert_layout(n, l, s, c, out['slots'], lay, 9) == 0
    gen = (C.c_int64 * 41)()
    assert lib.fm_debug_coarse_layout(n, l, s, c, out['slots'], gen, 41) == 0
    lp, sp = int(gen[4]), int(gen[5])
    o0 = out['base'] - out['ws'].data_ptr()

    def rd(off, count, dt):
        return out['ws'][o0 + off:o0 + off + 4 * count].view(dt).cpu().numpy()
    nu = (lp // 32) * (sp // 32)
    return dict(umax=rd(lay[0], n * nu, torch.float32).reshape(n, lp // 32, sp // 32),
                umax2=rd(lay[1], n * nu, torch.int32).reshape(n, lp // 32, sp // 32),
                upos=rd(lay[2], n * nu, torch.int32).reshape(n, lp // 32, sp // 32),
                thr_r=rd(lay[3], n * lp, torch.int32).reshape(n, lp), thr_c=rd(lay[4], n * sp, torch.int32).reshape(n, sp),
                tmin_r=rd(lay[5], n * lp // 32, torch.int32).reshape(n, lp // 32),
                tmin_c=rd(lay[6], n * sp // 32, torch.int32).reshape(n, sp // 32),
                count=int(rd(lay[7], 1, torch.int32)[0]), dense_cnt=rd(gen[34], n, torch.int32).copy())


def _certified(a, b, rb, u):
    return bool(a['umax2'][b, rb, u] <= min(a['tmin_r'][b, rb], a['tmin_c'][b, u]))


def _count_bounds(a, l):
    """what the kernel's counter of certified LIVE units must lie between: a certified unit whose maximum passes the two
    thresholds at its place holds a significant entry, so it is live for sure; no unit outside the certificate counts"""
    lo = hi = 0
    n, _, nu = a['umax2'].shape
    for b in range(n):
        for rb in range(-(-l // 32)):
            for u in range(nu):
                if not _certified(a, b, rb, u):
                    continue
                hi += 1
                g, lane = int(a['upos'][b, rb, u]) & 15, (int(a['upos'][b, rb, u]) >> 4) & 63
                i, j = rb * 32 + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), u * 32 + (lane & 31)
                lo += bool(a['umax'][b, rb, u] > min(a['thr_r'][b, i], a['thr_c'][b, j]))
    return lo, hi


def _run(cs, mode):
    lib = _lib.load()
    prev = lib.fm_debug_unit_cert(mode)
    try:
        out = edges._call(cs, 0)
        out['arrays'] = _arrays(out)
    finally:
        lib.fm_debug_unit_cert(prev)
    return out


def _off_on(cs, y=None, tag=""):
    """both runs; identical outputs; the `on` run against the yardstick; returns the `on` run"""
    off, on = _run(cs, OFF), _run(cs, ON)
    assert off['st'] == 0 and on['st'] == 0, (off['st'], off['info'], on['st'], on['info'])
    assert (off['m'], off['info']) == (on['m'], on['info'])
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c'):
        assert off[k].tobytes() == on[k].tobytes(), k
    assert np.array_equal(off['arrays']['dense_cnt'], on['arrays']['dense_cnt'])
    assert off['arrays']['umax'].tobytes() == on['arrays']['umax'].tobytes()      # (row blocks of padding: never written)
    lo, hi = _count_bounds(on['arrays'], cs['f0'].shape[1])
    assert off['arrays']['count'] == 0 and lo <= on['arrays']['count'] <= hi, (on['arrays']['count'], lo, hi)
    on['sure'] = lo
    if y is not None:
        on['mode'], on['first'] = 0, None
        bad = edges._list_errors(on, y) or edges._value_errors(tag, ("unit_cert", tag), on, cs, y)
        assert not bad, bad
    return on


SHAPES = [(256, 1), (64, 3)]


@pytest.mark.parametrize("c,n", SHAPES)
@pytest.mark.parametrize("name", ["one", "two", "row", "col", "tie", "negative"])
def test_planted_units_off_against_on(name, c, n):
    cs = _pair(name, c, n)
    on = _off_on(cs, _yard(name, c, n), f"{name} C={c} N={n}")
    a = on['arrays']
    m1, m2 = int(a['umax'][0, 0, 0]), int(a['umax2'][0, 0, 0])
    if name == "one":
        assert _certified(a, 0, 0, 0) and m2 < m1 and on['sure'] >= 1 and on['arrays']['count'] >= 1
        g, lane = int(a['upos'][0, 0, 0]) & 15, int(a['upos'][0, 0, 0]) >> 4
        assert ((g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), lane & 31) == (3, 5)
    elif name == "negative":
        assert m2 <= m1 < 0 and _certified(a, 0, 0, 0)          # (nothing to park: not live, whatever the certificate says)
    else:
        assert not _certified(a, 0, 0, 0)
        assert (m2 == m1) == (name == "tie")


@pytest.mark.parametrize("c,n", SHAPES)
def test_second_entry_just_above_and_just_below_the_row_threshold(c, n):
    """column 20 = alpha x column 5: alpha bisected on `runner-up > thr_r[3]` (12 steps from [0.3, 1])"""
    def above(alpha):
        a = _run(_pair("scaled", c, n, alpha), ON)['arrays']
        return int(a['umax2'][0, 0, 0]) > int(a['thr_r'][0, 3])
    lo, hi = 0.3, 1.0
    assert above(hi) and not above(lo)
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if above(mid) else (mid, hi)
    for alpha, want in ((lo, False), (hi, True)):
        cs = _pair("scaled", c, n, alpha)
        on = _off_on(cs, _yard("scaled", c, n, alpha), f"scaled {alpha:.5f} C={c} N={n}")
        a = on['arrays']
        assert (int(a['umax2'][0, 0, 0]) > int(a['thr_r'][0, 3])) == want
        assert not _certified(a, 0, 0, 0)


@pytest.mark.parametrize("c,n", SHAPES)
@pytest.mark.parametrize("name", ["tails70", "tails65"])
def test_tails_off_against_on(name, c, n):
    cs = _pair(name, c, n)
    on = _off_on(cs, _yard(name, c, n), f"{name} C={c} N={n}")
    a, idx = on['arrays'], cs['idx']
    l = cs['f0'].shape[1]
    for b in range(n):
        peaks = {}
        for j, i in enumerate(idx[b]):
            if i < l:
                peaks[(i // 32, j // 32)] = peaks.get((i // 32, j // 32), 0) + 1
        single = [k for k, v in peaks.items() if v == 1]
        assert single and all(_certified(a, b, rb, u) for rb, u in single), (b, single)
        assert on['sure'] >= len(single) and on['arrays']['count'] >= len(single)
        assert ((l - 1) // 32, (idx.shape[1] - 1) // 32) in single          # the corner unit, padded on both sides
        if name == "tails65":
            assert a['umax2'][b, 2, 4] == K_Q_MASKED and a['umax'][b, 2, 4] > 0 and _certified(a, b, 2, 4)
            g, lane = int(a['upos'][b, 2, 4]) & 15, int(a['upos'][b, 2, 4]) >> 4
            assert ((g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), lane & 31) == (0, 0)


def test_one_headline_size_pair_off_against_on():
    """one 640x480 'peaky' pair (L = S = 4800, C = 256): identical outputs, and most live units certify"""
    f0, f1 = synth.coarse_descriptors(1017, 1, 4800, 256, "peaky")
    on = _off_on(cr._case(f0, f1, HW[4800], HW[4800]))
    assert on['m'] > 3000 and on['arrays']['count'] > 2000
