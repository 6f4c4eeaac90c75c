"""GPU parity tests: the HIP path (through the C ABI) against the reference-generated golden
fixtures, the CPU oracle on fresh seeded inputs, and size-independent properties.

Bars: identical (b,i,j) inlier sets outside a guard band around thr,
mconf within 1e-5 (abs) of the reference, coarse keypoints bit-exact, fine keypoints within
1e-3 px (north star: 0.5 px).  Guard band: a reference/HIP disagreement is tolerated only when
the entry's conf lies within GUARD of thr, where float32 re-orderings of the reference's own
sums already flip the decision (hard part 3).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from featurematching_amd import modules, ops, synth
from featurematching_amd import _lib
from oracle import matcher_ref as orc
from helpers import load_golden, load_kats, case_inputs, compare_match_sets, net_tail_inputs, NET_TAIL, NET_TAIL_CFG2, epipolar_inputs, FLIPS

pytestmark = pytest.mark.gpu

GUARD = 2e-5
CONF_TOL = 1e-5
FINE_TOL_PX = 1e-3
DEV = "cuda:0"


def _np(d):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items() if not k.startswith('_')}


def _assert_coarse(got, ref, thr=0.2, conf_tol=CONF_TOL):
    got, ref = _np(got), _np(ref)
    only_g, only_r, err = compare_match_sets(got, ref)
    bad = [(k, v) for k, v in only_g + only_r if abs(v - thr) > GUARD]
    assert not bad, f"match sets differ outside the guard band: {bad[:5]} (+{len(bad) - 5 if len(bad) > 5 else 0})"
    assert err <= conf_tol, f"mconf differs by {err}"
    if not only_g and not only_r:
        assert np.array_equal(got['i_ids'], ref['i_ids']) and np.array_equal(got['j_ids'], ref['j_ids'])
        assert np.array_equal(got['b_ids'], ref['b_ids'])                      # same (b,i,j) order
        assert np.array_equal(got['mkpts0_c'], ref['mkpts0_c']) and np.array_equal(got['mkpts1_c'], ref['mkpts1_c'])
    assert got['i_ids'].dtype == np.int64 and got['mkpts0_c'].dtype == np.float32
    # every comparison reports how many entries flipped inside the guard band (the terminal summary lists them)
    FLIPS.append((os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0].split('::')[-1], len(only_g) + len(only_r),
                  len(ref['i_ids']), err))
    return len(only_g) + len(only_r)


def _run_coarse(f0, f1, hw_i, hw0_c, hw1_c, thr=0.2, border=2, temp=0.1, scale0=None, scale1=None):
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    s0 = None if scale0 is None else torch.as_tensor(scale0, device=DEV)
    s1 = None if scale1 is None else torch.as_tensor(scale1, device=DEV)
    return ops.coarse_match(t0, t1, hw0_c, hw1_c, hw_i[0] / hw0_c[0], thr, border, temp, s0, s1)


# ------------------------------------------------------------------ golden fixtures
@pytest.mark.parametrize("name,dist", [("cfg1_peaky", "peaky"), ("cfg1_borderline", "borderline"),
                                       ("cfg2_peaky", "peaky"), ("cfg2_borderline", "borderline"),
                                       ("cfg3_first2_peaky", "peaky"), ("cfg2_mixed", "mixed")])
def test_full_path_against_reference_fixture(name, dist):
    g = load_golden(name)
    inp = case_inputs(g['meta'], dist)
    out = _run_coarse(inp['f0'], inp['f1'], inp['hw_i'], inp['hw_c'], inp['hw_c'])
    ndiff = _assert_coarse(out, g)
    assert ndiff <= 4, f"{ndiff} guard-band flips"
    # crop and fine outputs are compared on the matches both sides hold (all of them unless a guard-band flip)
    gk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(out['b_ids'].tolist(), out['i_ids'].tolist(), out['j_ids'].tolist()))}
    rk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(g['b_ids'], g['i_ids'], g['j_ids']))}
    common = [k for k in gk if k in rk]
    gi = np.array([gk[k] for k in common])
    ri = np.array([rk[k] for k in common])
    assert len(common) >= len(rk) - 4
    ff0 = torch.as_tensor(inp['ff0'], device=DEV)
    ff1 = torch.as_tensor(inp['ff1'], device=DEV)
    wc = inp['hw_c'][1]
    win0 = ops.gather_windows(ff0, out['b_ids'], out['i_ids'], 7, 4, wc)
    win1 = ops.gather_windows(ff1, out['b_ids'], out['j_ids'], 7, 4, wc)
    pos = torch.arange(1, 50, dtype=torch.float64, device=DEV).view(1, 49, 1)
    ch = torch.arange(1, 65, dtype=torch.float64, device=DEV).view(1, 1, -1)
    np.testing.assert_allclose((win0.double() * pos * ch).sum((1, 2)).cpu().numpy()[gi], g['win0_sum'][ri], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose((win1.double() * pos * ch).sum((1, 2)).cpu().numpy()[gi], g['win1_sum'][ri], rtol=1e-12, atol=1e-9)
    w0, b0, w1, b1 = inp['mix']
    mix0 = torch.as_tensor(np.concatenate([w0, [b0]]).astype(np.float32), device=DEV)
    mix1 = torch.as_tensor(np.concatenate([w1, [b1]]).astype(np.float32), device=DEV)
    k0, k1 = ops.fine_match(win0, win1, mix0, mix1, out['mkpts0_c'], out['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0])
    assert np.abs(k0.cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max() <= FINE_TOL_PX
    assert np.abs(k1.cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max() <= FINE_TOL_PX
    np.testing.assert_allclose(k0.cpu().numpy()[gi, 2], g['mkpts0_f'][ri, 2], atol=1e-4)
    np.testing.assert_allclose(k1.cpu().numpy()[gi, 2], g['mkpts1_f'][ri, 2], atol=1e-4)


def _common_rows(out, g):
    gk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(out['b_ids'].tolist(), out['i_ids'].tolist(), out['j_ids'].tolist()))}
    rk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(g['b_ids'], g['i_ids'], g['j_ids']))}
    common = [k for k in gk if k in rk]
    return np.array([gk[k] for k in common]), np.array([rk[k] for k in common]), len(rk)


def _mix_tensors(mix):
    w0, b0, w1, b1 = mix
    return (torch.as_tensor(np.concatenate([w0, [b0]]).astype(np.float32), device=DEV),
            torch.as_tensor(np.concatenate([w1, [b1]]).astype(np.float32), device=DEV))


def _maps(inp, layout):
    ff0, ff1 = torch.as_tensor(inp['ff0'], device=DEV), torch.as_tensor(inp['ff1'], device=DEV)
    if layout == "nhwc":
        ff0, ff1 = ff0.contiguous(memory_format=torch.channels_last), ff1.contiguous(memory_format=torch.channels_last)
    return ff0, ff1


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name,dist", [("cfg2_peaky", "peaky"), ("cfg2_borderline", "borderline"),
                                       ("l9600_peaky", "peaky"), ("cfg5_peaky", "peaky")])
def test_bench_path_against_reference_fixture(name, dist, layout):
    """The entry points the bench times - fm_coarse_match, then crop + fine straight from the maps (fm_fine_match_maps;
    NCHW maps as the reference hands them over, and channels-last storage) - at the bench's sizes (640x480, 640x960 =
    the L = 9600 cost volume, 1024x1024) against the REFERENCE's own outputs, W = 7 (fine_matching_new.py fixes WW = 49)."""
    g = load_golden(name)
    inp = case_inputs(g['meta'], dist)
    out = _run_coarse(inp['f0'], inp['f1'], inp['hw_i'], inp['hw_c'], inp['hw_c'])
    ndiff = _assert_coarse(out, g)
    assert ndiff <= 4, f"{ndiff} guard-band flips"
    gi, ri, nref = _common_rows(out, g)
    assert len(gi) >= nref - 4
    ff0, ff1 = _maps(inp, layout)
    mix0, mix1 = _mix_tensors(inp['mix'])
    wc = inp['hw_c'][1]
    k0, k1 = ops.fine_match_maps(ff0, ff1, out['b_ids'], out['i_ids'], out['j_ids'], 7, 4, wc, wc, mix0, mix1,
                                 out['mkpts0_c'], out['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0])
    assert np.abs(k0.cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max() <= FINE_TOL_PX
    assert np.abs(k1.cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max() <= FINE_TOL_PX
    np.testing.assert_allclose(k0.cpu().numpy()[gi, 2], g['mkpts0_f'][ri, 2], atol=1e-4)
    np.testing.assert_allclose(k1.cpu().numpy()[gi, 2], g['mkpts1_f'][ri, 2], atol=1e-4)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name,dist", [("cfg2_peaky_w5", "peaky"), ("cfg2_borderline_w5", "borderline")])
def test_headline_step_w5_at_cfg2_against_reference_fixture(name, dist, layout):
    """What the metric times, pinned to the REFERENCE: one 640x480 pair, 5x5 fine window (BASELINE.json configs[1]).
    fine_matching_new.py:22-79 derives W from WW (:34); only the nn.Linear(49, 1) of :18-19 fix 49 - make_golden.py swaps
    them for Linear(25, 1) after construction and runs the reference's unmodified forward on its own W = 5 unfold
    (fine_preprocess.py:43-50).  fm_coarse_match + fm_fine_match_maps (NCHW and channels-last) against those outputs;
    the crops through fm_gather_windows against the per-window checksums."""
    g = load_golden(name)
    assert int(g['meta'][6]) == 5
    inp = case_inputs(g['meta'][:6], dist, ww=25)
    out = _run_coarse(inp['f0'], inp['f1'], inp['hw_i'], inp['hw_c'], inp['hw_c'])
    ndiff = _assert_coarse(out, g)
    assert ndiff <= 4, f"{ndiff} guard-band flips"
    gi, ri, nref = _common_rows(out, g)
    assert len(gi) >= nref - 4 and nref > 3000
    ff0, ff1 = _maps(inp, layout)
    mix0, mix1 = _mix_tensors(inp['mix'])
    wc = inp['hw_c'][1]
    k0, k1 = ops.fine_match_maps(ff0, ff1, out['b_ids'], out['i_ids'], out['j_ids'], 5, 4, wc, wc, mix0, mix1,
                                 out['mkpts0_c'], out['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0])
    assert k0.shape[1] == 3
    assert np.abs(k0.cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max() <= FINE_TOL_PX
    assert np.abs(k1.cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max() <= FINE_TOL_PX
    np.testing.assert_allclose(k0.cpu().numpy()[gi, 2], g['mkpts0_f'][ri, 2], atol=1e-4)
    np.testing.assert_allclose(k1.cpu().numpy()[gi, 2], g['mkpts1_f'][ri, 2], atol=1e-4)
    win0 = ops.gather_windows(ff0, out['b_ids'], out['i_ids'], 5, 4, wc)
    win1 = ops.gather_windows(ff1, out['b_ids'], out['j_ids'], 5, 4, wc)
    pos = torch.arange(1, 26, dtype=torch.float64, device=DEV).view(1, 25, 1)
    ch = torch.arange(1, 65, dtype=torch.float64, device=DEV).view(1, 1, -1)
    np.testing.assert_allclose((win0.double() * pos * ch).sum((1, 2)).cpu().numpy()[gi], g['win0_sum'][ri], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose((win1.double() * pos * ch).sum((1, 2)).cpu().numpy()[gi], g['win1_sum'][ri], rtol=1e-12, atol=1e-9)
    # ... and the two-call form on window tensors gives the fused call's numbers
    q0, q1 = ops.fine_match(win0, win1, mix0, mix1, out['mkpts0_c'], out['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0])
    assert torch.equal(q0, k0) and torch.equal(q1, k1)


@pytest.mark.parametrize("name,dist", [("cfg3_all64_peaky", "peaky"), ("cfg3_all64_borderline", "borderline")])
def test_cfg3_all_64_samples_against_the_reference_summary(name, dist):
    """BASELINE config #3 AT ITS SIZE against the reference: all 64 samples went through coarse_matching_new.py:43-143
    one at a time (make_golden.py:batch_summary_case) and left per-sample M, SHA-256 of the (i, j) ids in the
    reference's order, min / max / sum of mconf, sums of the coarse keypoints; matches within 1e-4 of thr are listed
    explicitly and excluded from the hashes (the guard band).  ONE batched fm_coarse_match_auto call is compared."""
    import hashlib
    g = load_golden(name)
    n, h, w, c, cf, seed = [int(v) for v in g['meta']]
    assert n == 64
    sh = synth.config_shapes(dict(h=h, w=w))
    hw_c = (sh['hc'], sh['wc'])
    f0 = torch.empty(n, sh['l'], c, device=DEV)
    f1 = torch.empty_like(f0)
    for b in range(n):                 # (sample b of the batch = seed + b: what coarse_descriptors(seed, 64, ...) returns)
        a0, a1 = synth.coarse_descriptors(seed + b, 1, sh['l'], c, dist)
        f0[b], f1[b] = torch.as_tensor(a0[0]), torch.as_tensor(a1[0])
    out = _np(ops.coarse_match(f0, f1, hw_c, hw_c, h / sh['hc']))
    band = {(int(b), int(i), int(j)): float(cv) for (b, i, j), cv in zip(g['band'], g['band_conf'])}
    flips = 0
    for b in range(n):
        sel = out['b_ids'] == b
        ij = np.stack([out['i_ids'][sel], out['j_ids'][sel]], 1)
        mc, kp0, kp1 = out['mconf'][sel], out['mkpts0_c'][sel], out['mkpts1_c'][sel]
        listed = np.array([(b, int(i), int(j)) in band for i, j in ij], bool)
        inside = (np.abs(mc - 0.2) < GUARD) & ~listed       # a flip INTO the set is only legal inside the guard band
        flips += int(inside.sum())
        for (i, j), cv in zip(ij[listed], mc[listed]):
            assert abs(cv - band[(b, int(i), int(j))]) <= CONF_TOL
        missing = [k for k in band if k[0] == b and not ((ij[:, 0] == k[1]) & (ij[:, 1] == k[2])).any()]
        for k in missing:                                   # a flip OUT of the set likewise
            assert abs(band[k] - 0.2) < GUARD, f"reference match {k} (conf {band[k]}) is missing"
        flips += len(missing)
        keep = ~(listed | inside)
        assert int(keep.sum()) == int(g['m'][b]), f"sample {b}: M {int(keep.sum())} vs reference {int(g['m'][b])}"
        assert hashlib.sha256(ij[keep].astype('<i4').tobytes()).hexdigest() == str(g['sha256'][b]), f"sample {b}: ids differ"
        assert abs(float(mc[keep].min()) - float(g['mconf_min'][b])) <= CONF_TOL
        assert abs(float(mc[keep].max()) - float(g['mconf_max'][b])) <= CONF_TOL
        assert abs(mc[keep].astype(np.float64).sum() - g['mconf_sum'][b]) <= CONF_TOL * max(1, int(keep.sum()))
        assert kp0[keep].astype(np.float64).sum() == g['kpts_sum'][b, 0] and kp1[keep].astype(np.float64).sum() == g['kpts_sum'][b, 1]
    FLIPS.append((f"test_cfg3_all_64_samples[{name}]", flips, int(g['m'].sum()) + len(band), 0.0))
    assert flips <= 4


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_headline_step_w5_at_cfg2_against_oracle(layout):
    """The metric's own configuration - one 640x480 pair, 5x5 fine window (BASELINE.json configs[1]) - through the
    calls bench.py times.  The reference's fine_matching_new.py cannot run W = 5 (nn.Linear(49, 1)); the oracle (pinned
    at W = 7 by the fixtures, W a parameter of the same code) is the checker."""
    cfg = synth.CONFIGS["cfg2"]
    sh = synth.config_shapes(cfg)
    f0, f1 = synth.coarse_descriptors(cfg['seed'], 1, sh['l'], cfg['c'], "peaky")
    ff0, ff1 = synth.fine_maps(cfg['seed'], 1, cfg['cf'], sh['hf'], sh['wf'])
    mix = synth.mix_weights(cfg['seed'], 25)
    hw_i, hw_c = (cfg['h'], cfg['w']), (sh['hc'], sh['wc'])
    ref = {k: v.numpy() for k, v in orc.match_features(f0, f1, ff0, ff1, hw_i, mix, w=5).items()}
    out = _run_coarse(f0, f1, hw_i, hw_c, hw_c)
    _assert_coarse(out, ref)
    gi, ri, nref = _common_rows(out, ref)
    assert len(gi) == nref and nref > 3000
    t0, t1 = _maps(dict(ff0=ff0, ff1=ff1), layout)
    mix0, mix1 = _mix_tensors(mix)
    k0, k1 = ops.fine_match_maps(t0, t1, out['b_ids'], out['i_ids'], out['j_ids'], 5, 4, hw_c[1], hw_c[1], mix0, mix1,
                                 out['mkpts0_c'], out['mkpts1_c'], hw_i[0] / sh['hf'])
    assert np.abs(k0.cpu().numpy()[gi] - ref['mkpts0_f'][ri]).max() <= FINE_TOL_PX
    assert np.abs(k1.cpu().numpy()[gi] - ref['mkpts1_f'][ri]).max() <= FINE_TOL_PX


@pytest.mark.parametrize("name,dist", [("cfg1_borderline", "borderline"), ("cfg2_borderline", "borderline"),
                                       ("cfg2_mixed", "mixed"), ("cfg2_peaky", "peaky"), ("cfg3_first2_borderline", "borderline"),
                                       ("l9600_borderline", "borderline")])
def test_flat_hint_against_reference_fixture(name, dist):
    """FM_MODE_FLAT (the caller's hint that every sample has flat similarity: no screening sweep, the float16 planes out
    of k_prep_split, k_stab, every sample to the dense sum kernel) against the REFERENCE's outputs - on flat data
    ('borderline': every conf in (0.2, 1)), on 'mixed' data (dead rows + rows without a peak; with the exact screening
    pass, as the bench runs it) and on PEAKED data, where the hint is wrong and must only cost time.  The call reports
    FM_DEV_ALL_DENSE (informational), which is how ops.coarse_match's mode memory learns the hint."""
    g = load_golden(name)
    inp = case_inputs(g['meta'], dist, with_fine=False)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    hw_c = inp['hw_c']
    buf = ops.coarse_match_async(t0, t1, hw_c, hw_c, inp['hw_i'][0] / hw_c[0], dense=True, flat=True,
                                 exact_screening=(dist == "mixed"))
    m = buf.read_count()
    assert buf.info & _lib.FM_DEV_ALL_DENSE
    ndiff = _assert_coarse(buf.sliced(m), g)
    assert ndiff <= 6, f"{ndiff} guard-band flips"
    # ... and the same call without the hint: the same matches (two float32-grade arithmetics may differ in the last bits
    # of conf for a sample that changes kernels - 'peaky' here - never in the set outside the guard band)
    buf2 = ops.coarse_match_async(t0, t1, hw_c, hw_c, inp['hw_i'][0] / hw_c[0], dense=True, exact_screening=(dist == "mixed"))
    m2 = buf2.read_count()
    assert bool(buf2.info & _lib.FM_DEV_ALL_DENSE) == (dist != "peaky")
    _assert_coarse(buf.sliced(m), {k: v for k, v in _np(buf2.sliced(m2)).items()}, conf_tol=2e-6)


def test_mode_memory_learns_the_wider_lists_on_mixed_data():
    """ops.coarse_match on 'mixed' data (peaked rows next to rows without a partner), nothing passed by the caller:
    FM_E_DENSE -> dense -> FM_E_CANDIDATES (rows with more near-candidates than 8 slots) -> 16 slots + the exact int8
    step; the shape's next call starts there, with the flat hint, in ONE coarse call - every time the reference's
    matches."""
    g = load_golden("cfg2_mixed")
    inp = case_inputs(g['meta'], "mixed", with_fine=False)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    ops.MODE_MEMORY.clear()
    key = ops.hint_key(t0.shape, t1.shape)
    outs = [ops.coarse_match(t0, t1, inp['hw_c'], inp['hw_c'], 8.0) for _ in range(3)]
    snap = ops.MODE_MEMORY.snapshot()[key]
    assert snap['dense'] and snap['flat'] and (snap['wide'] or snap['exact'])
    for o in outs:
        assert _assert_coarse(o, g) <= 4
    if snap['wide']:
        assert outs[2]['_coarse_buffers']._shape[4] == 16            # the steady state runs with 16 slots
    ops.MODE_MEMORY.clear()


def test_mode_memory_learns_the_flat_hint():
    """ops.coarse_match on flat data: FM_E_DENSE -> repeated with FM_MODE_DENSE -> that call reports FM_DEV_ALL_DENSE ->
    the shape's next call carries FM_MODE_FLAT; same matches every time."""
    g = load_golden("cfg1_borderline")
    inp = case_inputs(g['meta'], "borderline", with_fine=False)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    ops.MODE_MEMORY.clear()
    key = ops.hint_key(t0.shape, t1.shape)
    outs = [ops.coarse_match(t0, t1, inp['hw_c'], inp['hw_c'], 8.0) for _ in range(3)]
    snap = ops.MODE_MEMORY.snapshot()[key]
    assert snap['dense'] and snap['flat']
    for o in outs:
        _assert_coarse(o, g)
    assert np.array_equal(_np(outs[1])['mconf'], _np(outs[2])['mconf'])
    ops.MODE_MEMORY.clear()


def test_flat_hint_with_an_outlier_outside_the_sampled_rows():
    """The float16 planes k_prep_split writes under FM_MODE_FLAT are scaled from the SAMPLED rows' maximum: a descriptor
    ~6x beyond it would leave float16's range - k_stab compares the image's true maximum with the scale and reports
    FM_E_STEP; with FM_MODE_EXACT_STEP (scale from the true maximum) the call is served."""
    l, c, hw = 1200, 128, (30, 40)
    f0, f1 = synth.coarse_descriptors(92, 1, l, c, "borderline")
    sampled = sorted({(t * l) // 32 for t in range(32)})
    free = [r for r in range(l) if r not in sampled]
    f0[0, free[9]] *= 12.0
    ref = orc.coarse_match(f0, f1, (240, 320), hw, hw, 0.2, 2, 0.1)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    with pytest.raises(_lib.FMatchError) as e:
        ops.coarse_match_async(t0, t1, hw, hw, 8.0, dense=True, flat=True, exact_screening=True).read_count()
    assert e.value.status == _lib.FM_E_STEP
    buf = ops.coarse_match_async(t0, t1, hw, hw, 8.0, dense=True, flat=True, exact_screening=True, exact_step=True)
    m = buf.read_count()
    _assert_coarse(buf.sliced(m), ref)
    assert m == ref['i_ids'].shape[0] > 100


@pytest.mark.parametrize("name,w", [("cfg1_peaky", 7), ("cfg2_peaky", 5), ("cfg3_first2_peaky", 7)])
def test_assignment_launch_carries_the_map_copy(name, w):
    """fm_coarse_match_maps: the channels-last copy of image 1's NCHW fine map as a side job of the assignment kernel's
    launch, then fm_fine_match_maps with FM_LAYOUT_NCHW_PREPARED.  The coarse outputs are those of fm_coarse_match_dtype
    bit for bit, the scratch buffer is the permuted map bit for bit, and the fine keypoints equal the two-launch form's
    (ragged widths included: cfg1's 64-px rows are one piece, cfg2's 320-px rows five)."""
    g = load_golden(name)
    inp = case_inputs(g['meta'], "peaky", ww=w * w)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    ff0, ff1 = _maps(inp, "nchw")
    hw_c, scale = inp['hw_c'], inp['hw_i'][0] / inp['hw_c'][0]
    plain = ops.coarse_match_async(t0, t1, hw_c, hw_c, scale)
    m = plain.read_count()
    fused = ops.coarse_match_async(t0, t1, hw_c, hw_c, scale, side_map=ff1)
    assert fused.read_count() == m
    for k, v in plain.sliced(m).items():
        assert torch.equal(v, fused.sliced(m)[k]), k
    n, cf, hf, wf = ff1.shape
    got = fused.side_scratch[:ff1.numel() * 4].view(torch.float32).view(n, hf, wf, cf)
    assert torch.equal(got, ff1.permute(0, 2, 3, 1).contiguous())
    mix0, mix1 = _mix_tensors(inp['mix'])
    o = fused.sliced(m)
    a0, a1 = ops.fine_match_maps(ff0, ff1, o['b_ids'], o['i_ids'], o['j_ids'], w, 4, hw_c[1], hw_c[1], mix0, mix1,
                                 o['mkpts0_c'], o['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0], prepared=fused.side_scratch)
    b0, b1 = ops.fine_match_maps(ff0, ff1, o['b_ids'], o['i_ids'], o['j_ids'], w, 4, hw_c[1], hw_c[1], mix0, mix1,
                                 o['mkpts0_c'], o['mkpts1_c'], inp['hw_i'][0] / inp['hw_f'][0])
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    if w == 7:        # the reference's own fine keypoints
        gi, ri, nref = _common_rows(o, g)
        assert len(gi) == nref
        assert np.abs(a0.cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max() <= FINE_TOL_PX
        assert np.abs(a1.cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max() <= FINE_TOL_PX


@pytest.mark.parametrize("shape", [(3, 64, 17, 50), (1, 64, 9, 200), (2, 64, 33, 64)])
def test_map_copy_side_job_on_ragged_maps(shape):
    """The side job of fm_coarse_match_maps takes any [Nf, 64, Hf, Wf] float32 map (its shape is independent of the
    coarse problem): widths that are not multiples of 64 (a short last piece) or of 4 (the scalar loader), several
    samples - the scratch buffer is the permuted map bit for bit, the coarse outputs are untouched."""
    g = load_golden("cfg1_peaky")
    inp = case_inputs(g['meta'], "peaky", with_fine=False)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    side = torch.as_tensor(synth.normal(17, 3, shape), device=DEV)
    buf = ops.coarse_match_async(t0, t1, inp['hw_c'], inp['hw_c'], 8.0, side_map=side)
    m = buf.read_count()
    _assert_coarse(buf.sliced(m), g)
    n, c, hf, wf = shape
    got = buf.side_scratch[:side.numel() * 4].view(torch.float32).view(n, hf, wf, c)
    assert torch.equal(got, side.permute(0, 2, 3, 1).contiguous())


def test_flat_hint_on_a_batch_with_one_peaked_and_one_flat_sample():
    """FM_MODE_FLAT on a batch whose samples differ (sample 0 peaked, sample 1 flat): the hint is wrong for one of them
    and must only cost time - both samples against the oracle, and the same matches as the call without the hint."""
    l, c, hw = 1200, 128, (30, 40)
    a0, a1 = synth.coarse_descriptors(61, 1, l, c, "peaky")
    b0, b1 = synth.coarse_descriptors(62, 1, l, c, "borderline")
    f0, f1 = np.concatenate([a0, b0]), np.concatenate([a1, b1])
    ref = orc.coarse_match(f0, f1, (240, 320), hw, hw, 0.2, 2, 0.1)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    hint = ops.coarse_match_async(t0, t1, hw, hw, 8.0, dense=True, flat=True)
    mh = hint.read_count()
    assert hint.info & _lib.FM_DEV_ALL_DENSE
    _assert_coarse(hint.sliced(mh), ref)
    plain = ops.coarse_match_async(t0, t1, hw, hw, 8.0, dense=True)
    mp = plain.read_count()
    assert not (plain.info & _lib.FM_DEV_ALL_DENSE)            # sample 0 stayed with the screening kernel
    _assert_coarse(plain.sliced(mp), ref)
    assert mh == mp and int((hint.sliced(mh)['b_ids'] == 1).sum()) > 300


def test_cfg5_coarse_against_reference_fixture():
    g = load_golden("cfg5_peaky")                       # 1024x1024 -> L = S = 16384
    inp = case_inputs(g['meta'], "peaky", with_fine=False)
    out = _run_coarse(inp['f0'], inp['f1'], inp['hw_i'], inp['hw_c'], inp['hw_c'])
    _assert_coarse(out, g)


@pytest.mark.parametrize("name", ["cfg3_first2_borderline", "cfg5_borderline", "l9600_borderline"])
def test_coarse_on_non_degenerate_data_against_reference_fixture(name):
    """The reference's own outputs on 'borderline' data (conf spread over (0.2, 1)) for two samples of the cfg#3 batch
    and at S = 16384 (cfg#5), where the sparse kernel's S * 2^-32 truncation and the dense kernel's 22-bit products
    are largest relative to the 1e-5 bar."""
    g = load_golden(name)
    inp = case_inputs(g['meta'], "borderline", with_fine=False)
    out = _run_coarse(inp['f0'], inp['f1'], inp['hw_i'], inp['hw_c'], inp['hw_c'])
    # At S = 16384 the REFERENCE's float32 arithmetic is itself 1.0e-5 away from the exact value for some entries
    # (float64 evaluation of coarse_matching_new.py:64-68 on the same inputs: tools/diag_conf_f64.py), this path
    # 1.8e-6: against the fixture the bar is 2e-5 there, and the error against float64 is bounded below.
    ndiff = _assert_coarse(out, g, conf_tol=2e-5 if name == "cfg5_borderline" else CONF_TOL)
    assert ndiff <= 6, f"{ndiff} guard-band flips"
    # against the exact (float64) dual softmax: closer than the float32 reference is
    for b in range(int(g['meta'][0])):
        sim = (torch.as_tensor(inp['f0'][b], device=DEV).double() @ torch.as_tensor(inp['f1'][b], device=DEV).double().T) \
            / (inp['f0'].shape[2] * 0.1)
        conf64 = torch.softmax(sim, 0) * torch.softmax(sim, 1)
        sel = out['b_ids'] == b
        e_hip = (out['mconf'][sel].double() - conf64[out['i_ids'][sel], out['j_ids'][sel]]).abs().max().item()
        rs = torch.as_tensor(g['b_ids'] == b)
        e_ref = (torch.as_tensor(g['mconf'])[rs].double()
                 - conf64[torch.as_tensor(g['i_ids'].astype(np.int64))[rs].to(DEV), torch.as_tensor(g['j_ids'].astype(np.int64))[rs].to(DEV)].cpu()).abs().max().item()
        assert e_hip <= 5e-6, (e_hip, e_ref)
        del sim, conf64


def test_kats_against_reference_fixture():
    for name, k in load_kats().items():
        hw = [int(v) for v in k['hw']]
        thr, brm, temp = float(k['cfg'][0]), int(k['cfg'][1]), float(k['cfg'][2])
        out = _run_coarse(k['f0'], k['f1'], hw[0:2], hw[4:6], hw[6:8], thr, brm, temp, k.get('scale0'), k.get('scale1'))
        assert _assert_coarse(out, k, thr) == 0, name
        if name == "tie":       # both tied entries kept, same conf bits
            i = out['i_ids'].cpu().numpy()
            assert len(i) != len(set(i.tolist()))
        if 'fine_seed' in k and out['i_ids'].shape[0]:
            seed = int(k['fine_seed'])
            ff0, ff1 = synth.fine_maps(seed, k['f0'].shape[0], 64, hw[4] * 4, hw[5] * 4)
            w0, b0, w1, b1 = synth.mix_weights(seed, 49)
            win0 = ops.gather_windows(torch.as_tensor(ff0, device=DEV), out['b_ids'], out['i_ids'], 7, 4, hw[5])
            win1 = ops.gather_windows(torch.as_tensor(ff1, device=DEV), out['b_ids'], out['j_ids'], 7, 4, hw[7])
            mix0 = torch.as_tensor(np.concatenate([w0, [b0]]).astype(np.float32), device=DEV)
            mix1 = torch.as_tensor(np.concatenate([w1, [b1]]).astype(np.float32), device=DEV)
            k0, k1 = ops.fine_match(win0, win1, mix0, mix1, out['mkpts0_c'], out['mkpts1_c'], hw[0] / (hw[4] * 4))
            assert np.abs(k0.cpu().numpy() - k['mkpts0_f']).max() <= FINE_TOL_PX, name
            assert np.abs(k1.cpu().numpy() - k['mkpts1_f']).max() <= FINE_TOL_PX, name


def test_round2_kats_against_reference_fixture():
    """Per-sample scales with M >= 50 (keypoints bit-exact), and the constructed thr straddle: two inputs one ulp
    of one descriptor's scale apart, whose reference outputs differ by exactly the entry with conf = thr +- few ulp.
    The HIP path may place that ONE entry on either side (its conf is within 1e-6 of thr); nothing else may move."""
    cases = load_kats("kats_r2")
    k = cases["scale_big"]
    hw = [int(v) for v in k['hw']]
    out = _run_coarse(k['f0'], k['f1'], hw[0:2], hw[4:6], hw[6:8], 0.2, 2, 0.1, k['scale0'], k['scale1'])
    assert _assert_coarse(out, k) == 0 and out['i_ids'].shape[0] >= 50
    for name in ("thr_below", "thr_above"):
        k = cases[name]
        hw = [int(v) for v in k['hw']]
        i_s, j_s = [int(v) for v in k['straddle']]
        out = _np(_run_coarse(k['f0'], k['f1'], hw[0:2], hw[4:6], hw[6:8]))
        only_g, only_r, err = compare_match_sets(out, k)
        moved = {key for key, _ in only_g + only_r}
        assert moved <= {(0, i_s, j_s)}, (name, moved)       # a flip happens only at the constructed entry
        assert err <= CONF_TOL
        got = {(int(i), int(j)): float(c) for i, j, c in zip(out['i_ids'], out['j_ids'], out['mconf'])}
        if (i_s, j_s) in got:
            assert abs(got[(i_s, j_s)] - 0.2) < 2e-6


# ------------------------------------------------------------------ oracle on fresh inputs
@pytest.mark.parametrize("hc,wc,c,n,dist", [(7, 9, 64, 3, "peaky"), (15, 17, 128, 2, "borderline"),
                                            (33, 20, 256, 1, "borderline"), (16, 16, 256, 5, "peaky")])
def test_coarse_ragged_shapes_vs_oracle(hc, wc, c, n, dist):
    """L not a multiple of the 256-row panel, S not a multiple of the 64-column tile, each of the three channel counts
    the kernels are instantiated for (64, 128, 256).  Channel counts below and between them, and grids down to one
    cell: tests/test_gpu_coarse_edges.py."""
    f0, f1 = synth.coarse_descriptors(100 + hc, n, hc * wc, c, dist)
    ref = orc.coarse_match(f0, f1, (hc * 8, wc * 8), (hc, wc), (hc, wc), 0.2, 1, 0.1)
    out = _run_coarse(f0, f1, (hc * 8, wc * 8), (hc, wc), (hc, wc), border=1)
    _assert_coarse(out, ref)


def test_batched_screening_on_a_batch_of_small_pairs_vs_oracle():
    """k_thresh + k_screen_rows (the screening form a launch with >= 448 row blocks takes: batches, 1024x1024 pairs) on
    60 ragged 15x17-cell pairs of three kinds - peaked, flat ('borderline': every sample goes on to the dense sum
    kernel), peaked with textureless cells ('mixed': dead rows next to rows without a partner) - plus an exact tie
    (a duplicated descriptor in image 1: the reference keeps both entries, coarse_matching_new.py:105-106) inside one
    of the peaked samples.  Every sample against the oracle; the batch equals its samples run alone (those take the
    one-pair kernel k_screen)."""
    hc, wc, c, n = 15, 17, 128, 60
    l = hc * wc
    f0 = np.empty((n, l, c), np.float32)
    f1 = np.empty_like(f0)
    kinds = ["peaky", "borderline", "mixed"]
    for b in range(n):
        f0[b:b + 1], f1[b:b + 1] = synth.coarse_descriptors(700 + b, 1, l, c, kinds[b % 3])
    f1[3, 40] = f1[3, 41]                                   # sample 3 ('peaky'): columns 40 and 41 tie exactly
    hw_i = (hc * 8, wc * 8)
    ref = orc.coarse_match(f0, f1, hw_i, (hc, wc), (hc, wc), 0.2, 1, 0.1)
    out = _run_coarse(f0, f1, hw_i, (hc, wc), (hc, wc), border=1)
    assert out['_coarse_buffers']._shape[0] * 8 >= 448          # (the launch was large enough for the batched form)
    ndiff = _assert_coarse(out, ref)
    assert ndiff <= 4, f"{ndiff} guard-band flips"
    got = _np(out)
    tied = [(i, j) for b, i, j in zip(got['b_ids'], got['i_ids'], got['j_ids']) if b == 3 and j in (40, 41)]
    assert len(tied) == 2 and tied[0][0] == tied[1][0]
    for b in (0, 1, 2, 3):                                     # the same samples alone: same matches, conf within 2e-6
        alone = _np(_run_coarse(f0[b:b + 1], f1[b:b + 1], hw_i, (hc, wc), (hc, wc), border=1))
        sel = got['b_ids'] == b
        assert np.array_equal(got['i_ids'][sel], alone['i_ids']) and np.array_equal(got['j_ids'][sel], alone['j_ids'])
        assert np.abs(got['mconf'][sel] - alone['mconf']).max() <= 2e-6


def test_coarse_rectangular_l_ne_s():
    f0 = 3.0 * synth.normal(31, 1, (2, 40 * 50, 128))
    f1 = f0[:, synth.permutation(31, 3, 2000)[:1500]] + 0.3 * synth.normal(31, 2, (2, 1500, 128))
    ref = orc.coarse_match(f0, f1, (320, 400), (40, 50), (30, 50), 0.2, 2, 0.1)
    out = _run_coarse(f0, f1, (320, 400), (40, 50), (30, 50))
    _assert_coarse(out, ref)
    assert ref['i_ids'].shape[0] > 500


def test_small_magnitude_descriptors():
    """Descriptors far below 1: the float16 'lo' plane goes subnormal."""
    f0, f1 = synth.coarse_descriptors(41, 1, 400, 256, "borderline")
    f0, f1 = f0 * 0.02, f1 * 0.02
    ref = orc.coarse_match(f0, f1, (160, 160), (20, 20), (20, 20), 0.1, 2, 0.1 * 0.02 ** 2)
    out = _run_coarse(f0, f1, (160, 160), (20, 20), (20, 20), thr=0.1, temp=0.1 * 0.02 ** 2)
    _assert_coarse(out, ref, 0.1)
    assert ref['i_ids'].shape[0] > 50


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,dist", [((16, 16, 64), "peaky"), ((60, 80, 256), "peaky"), ((30, 40, 128), "borderline")])
def test_half_precision_descriptors(dtype, shape, dist):
    """fm_coarse_match_dtype: float16 / bfloat16 descriptors go to the kernels as they are.  Half-precision values
    and their pairwise products are exact in float32, so the oracle - the reference's float32 arithmetic - run on
    the up-cast tensors is the answer: identical ids outside the guard band, mconf within 1e-5."""
    hc, wc, c = shape
    f0, f1 = synth.coarse_descriptors(91, 2, hc * wc, c, dist)
    h0 = torch.as_tensor(f0).to(dtype)
    h1 = torch.as_tensor(f1).to(dtype)
    ref = orc.coarse_match(h0.float().numpy(), h1.float().numpy(), (hc * 8, wc * 8), (hc, wc), (hc, wc), 0.2, 2, 0.1)
    out = ops.coarse_match(h0.to(DEV), h1.to(DEV), (hc, wc), (hc, wc), 8.0)
    _assert_coarse(out, ref)
    assert ref['i_ids'].shape[0] > 50


def _repetitive_texture():
    """a quarter of the cells of BOTH images carry the same descriptor: every (repeated, repeated) entry ties with its
    row and its column maximum"""
    f0, f1 = synth.coarse_descriptors(43, 2, 30 * 40, 128, "peaky")
    f0[:, ::4] = f0[:, :1]
    f1[:, ::4] = f0[:, :1]
    return f0, f1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_textureless_cells_are_certified_dead(dtype):
    """Half of the cells of BOTH images carry almost no signal (near-zero descriptors).  Every entry of such a row is
    within e^-32 of the row's tiny maximum - formally significant, and every (textureless, textureless) entry passes
    the candidate test (360 k candidates against 8 slots per row: FM_E_CANDIDATES, the exact screening pass) - but
    ||a||_1 max|b| / (C T) bounds every softmax term of the row below thr: the sparse sum kernel drops such rows and
    columns (k_sum_sparse: DEAD rows), nothing overflows and no exact screening is needed.  The cells whose PARTNER is
    textureless are rows without a peak: those still need the dense sum kernel (FM_MODE_DENSE)."""
    f0, f1 = synth.coarse_descriptors(43, 2, 30 * 40, 128, "peaky")
    f0[:, ::2] *= 1e-4
    f1[:, ::2] *= 1e-4
    h0, h1 = torch.as_tensor(f0).to(dtype), torch.as_tensor(f1).to(dtype)      # (half precision: exact in float32)
    ref = orc.coarse_match(h0.float().numpy(), h1.float().numpy(), (240, 320), (30, 40), (30, 40), 0.2, 2, 0.1)
    assert 100 < ref['i_ids'].shape[0] < 900
    t0, t1 = h0.to(DEV), h1.to(DEV)
    buf = ops.coarse_match_async(t0, t1, (30, 40), (30, 40), 8.0, dense=True, exact_screening=False)
    m = buf.read_count()                 # (raises FM_E_CANDIDATES if a slot list had overflowed)
    assert m == ref['i_ids'].shape[0]
    _assert_coarse(buf.sliced(m), ref)


def test_flat_rows_take_the_exact_screening_pass():
    """Repetitive texture: every (repeated, repeated) entry is within ln(thr) of its row and its column maximum, the
    max-based screening of the sum pass overflows the candidate slots of those rows, and the exact screening pass
    (opt-in, decided on the device) must recover the exact set."""
    f0, f1 = _repetitive_texture()
    ref = orc.coarse_match(f0, f1, (240, 320), (30, 40), (30, 40), 0.2, 2, 0.1)
    out = _run_coarse(f0, f1, (240, 320), (30, 40), (30, 40))          # ops.coarse_match: retries with the exact pass
    _assert_coarse(out, ref)
    assert 100 < ref['i_ids'].shape[0] < 900
    # the asynchronous entry: without the exact pass the overflow is reported, with it one call suffices
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    with pytest.raises(_lib.FMatchError) as e:
        ops.coarse_match_async(t0, t1, (30, 40), (30, 40), 8.0).read_count()
    assert e.value.status in (_lib.FM_E_DENSE, _lib.FM_E_CANDIDATES)      # flat units / overflowing slots, whichever is met first
    with pytest.raises(_lib.FMatchError) as e:
        ops.coarse_match_async(t0, t1, (30, 40), (30, 40), 8.0, dense=True).read_count()
    assert e.value.status == _lib.FM_E_CANDIDATES
    buf = ops.coarse_match_async(t0, t1, (30, 40), (30, 40), 8.0, exact_screening=True)
    assert buf.read_count() == ref['i_ids'].shape[0]


def test_flat_rows_with_conf_matrix_run_the_coarse_stage_once(monkeypatch):
    """Training-shaped call (conf_matrix requested) on flat rows: the exact screening is on from the first attempt, so
    the coarse stage is enqueued once - not once to overflow and once more to recover.  And the hint word of
    fm_coarse_match_auto, kept per shape by ops.MODE_MEMORY: learnt, used, re-probed, forgotten."""
    f0, f1 = _repetitive_texture()
    ref = orc.coarse_match(f0, f1, (240, 320), (30, 40), (30, 40), 0.2, 2, 0.1)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    out = ops.coarse_match(t0, t1, (30, 40), (30, 40), 8.0, conf_matrix=True)
    assert out['_coarse_buffers'].attempts == 1
    _assert_coarse(out, ref)
    # a shape that overflowed once starts with the exact screening (and the dense sum kernel) the next time
    ops.MODE_MEMORY.clear()
    first = ops.coarse_match(t0, t1, (30, 40), (30, 40), 8.0)
    second = ops.coarse_match(t0, t1, (30, 40), (30, 40), 8.0)
    # (first call: common path -> + dense part -> [16 slots + exact step, which repetitive texture overflows too] -> exact screening)
    assert 2 <= first['_coarse_buffers'].attempts <= 4 and second['_coarse_buffers'].attempts == 1, first['_coarse_buffers'].attempts
    _assert_coarse(first, ref)
    _assert_coarse(second, ref)
    # the memory is visible, bounded and decays: the `reprobe`-th call of the shape starts on the common path again,
    # fails there for this data and ends with the flags again; peaked data of the same shape makes it forget them
    snap = ops.MODE_MEMORY.snapshot()
    assert len(snap) == 1 and list(snap.values())[0]['exact']
    monkeypatch.setattr(ops.MODE_MEMORY, "reprobe", 2)
    third = ops.coarse_match(t0, t1, (30, 40), (30, 40), 8.0)    # 2nd remembered call: a probe of the common path
    assert third['_coarse_buffers'].attempts >= 2 and list(ops.MODE_MEMORY.snapshot().values())[0]['exact']
    p0, p1 = synth.coarse_descriptors(77, f0.shape[0], 1200, f0.shape[2], "peaky")
    q0, q1 = torch.as_tensor(p0, device=DEV), torch.as_tensor(p1, device=DEV)
    pref = orc.coarse_match(p0, p1, (240, 320), (30, 40), (30, 40), 0.2, 2, 0.1)
    a = ops.coarse_match(q0, q1, (30, 40), (30, 40), 8.0)        # remembered flags: correct, only slower
    assert a['_coarse_buffers'].hint & _lib.FM_MODE_EXACT_SCREENING
    b = ops.coarse_match(q0, q1, (30, 40), (30, 40), 8.0)        # probe: succeeds on this data, the shape is forgotten
    c = ops.coarse_match(q0, q1, (30, 40), (30, 40), 8.0)
    assert b['_coarse_buffers'].hint == 0 and c['_coarse_buffers'].hint == 0 and not ops.MODE_MEMORY.snapshot()
    for o in (a, b, c):
        _assert_coarse(o, pref)
    ops.MODE_MEMORY.clear()


def _auto_call(f0, f1, hw0, hw1, scale_px, thr=0.2, border=2, temp=0.1, hint=0, mode=0, cap=None, max_slots=0,
               scale0=None, scale1=None):
    """fm_coarse_match_auto through ctypes, nothing else: returns (status, M, info, hint, outputs dict)"""
    lib = _lib.load()
    t0, t1 = torch.as_tensor(f0, device=DEV).contiguous(), torch.as_tensor(f1, device=DEV).contiguous()
    n, l, c = t0.shape
    s = t1.shape[1]
    nb = ctypes.c_size_t(0)
    assert lib.fm_coarse_workspace_bytes_auto(n, l, s, c, max_slots, ctypes.byref(nb)) == 0
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    cap = n * min(l, s) if cap is None else cap
    o = dict(b_ids=torch.empty(cap, dtype=torch.int64, device=DEV), i_ids=torch.empty(cap, dtype=torch.int64, device=DEV),
             j_ids=torch.empty(cap, dtype=torch.int64, device=DEV), mkpts0_c=torch.empty(cap, 2, device=DEV),
             mkpts1_c=torch.empty(cap, 2, device=DEV), mconf=torch.empty(cap, device=DEV))
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    s0 = None if scale0 is None else torch.as_tensor(scale0, device=DEV)
    s1 = None if scale1 is None else torch.as_tensor(scale1, device=DEV)
    h, m, info = ctypes.c_int32(hint), ctypes.c_int32(0), ctypes.c_int32(0)
    st = lib.fm_coarse_match_auto(p(t0), p(t1), _lib.FM_F32, n, l, s, c, hw0[0], hw0[1], hw1[0], hw1[1], temp, thr, border,
                                  scale_px, p(s0), p(s1), ctypes.c_void_p(base), nb.value, max_slots, mode,
                                  p(o['b_ids']), p(o['i_ids']), p(o['j_ids']), p(o['mkpts0_c']), p(o['mkpts1_c']),
                                  p(o['mconf']), cap, p(cnt), None, ctypes.byref(h), ctypes.byref(m), ctypes.byref(info),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    mm = max(0, min(int(m.value), cap))
    return st, int(m.value), int(info.value), int(h.value), {k: v[:mm] for k, v in o.items()}


@pytest.mark.parametrize("name,dist", [("cfg2_peaky", "peaky"), ("cfg2_mixed", "mixed"), ("cfg2_borderline", "borderline"),
                                       ("cfg1_borderline", "borderline")])
def test_one_c_call_serves_any_data(name, dist):
    """fm_coarse_match_auto - the ONE C entry point a drop-in caller needs (INTEGRATION.md option B) - driven through
    ctypes with NO retry on the Python side, on peaked, mixed (textureless cells + rows without a partner) and flat
    data, against the REFERENCE's fixtures; then once more from the hint word the first call left: one attempt."""
    g = load_golden(name)
    inp = case_inputs(g['meta'], dist, with_fine=False)
    hw = inp['hw_c']
    st, m, info, hint, out = _auto_call(inp['f0'], inp['f1'], hw, hw, inp['hw_i'][0] / hw[0])
    assert st == 0 and m == out['i_ids'].shape[0]
    assert _assert_coarse(out, g) <= 4
    attempts = (hint >> 24) & 0xff
    # (flat similarity alone is answered INSIDE the first attempt - the dense part is added to the common path's work;
    # 'mixed' overflows the default candidate slots on top of that and takes a second, wider attempt)
    assert attempts == 1 if dist != "mixed" else 2 <= attempts <= 4, attempts
    assert (hint & 0xffff) == 0 if dist == "peaky" else (hint & _lib.FM_MODE_DENSE)
    st2, m2, info2, hint2, out2 = _auto_call(inp['f0'], inp['f1'], hw, hw, inp['hw_i'][0] / hw[0], hint=hint & 0xffff)
    assert st2 == 0 and (hint2 >> 24) & 0xff == 1 and (hint2 & 0xff) == (hint & 0xff) | (_lib.FM_MODE_FLAT if dist != "peaky" else 0)
    assert _assert_coarse(out2, g) <= 4
    if dist != "peaky":          # ... and the third call runs with the flat hint (no screening sweep): same matches
        st3, m3, info3, hint3, out3 = _auto_call(inp['f0'], inp['f1'], hw, hw, inp['hw_i'][0] / hw[0], hint=hint2 & 0xffff)
        assert st3 == 0 and (hint3 >> 24) & 0xff == 1 and (hint3 & _lib.FM_MODE_FLAT) and (info3 & _lib.FM_DEV_ALL_DENSE)
        assert _assert_coarse(out3, g) <= 6


def test_one_c_call_on_the_known_answer_cases():
    """fm_coarse_match_auto on the reference's known-answer cases (exact two- and three-way ties, the thr straddle,
    per-sample scales, a batch with different M, M == 0), on an outlier descriptor outside the int8 step's sample
    (FM_E_STEP answered inside) and on output buffers that are too small (FM_E_CAPACITY: the needed capacity comes back,
    the second call with that capacity is served)."""
    for name, k in load_kats().items():
        hw = [int(v) for v in k['hw']]
        thr, brm, temp = float(k['cfg'][0]), int(k['cfg'][1]), float(k['cfg'][2])
        st, m, info, hint, out = _auto_call(k['f0'], k['f1'], hw[4:6], hw[6:8], hw[0] / hw[4], thr, brm, temp,
                                            scale0=k.get('scale0'), scale1=k.get('scale1'))
        if st == _lib.FM_E_CAPACITY:          # exact ties: more matches than N * min(L, S)
            st, m, info, hint, out = _auto_call(k['f0'], k['f1'], hw[4:6], hw[6:8], hw[0] / hw[4], thr, brm, temp, cap=m,
                                                scale0=k.get('scale0'), scale1=k.get('scale1'))
        assert st == 0, (name, st)
        assert _assert_coarse(out, k, thr) == 0, name
        if name == "empty":
            assert m == 0
    # an outlier row outside the sampled rows of the int8 step
    l, c, hw = 1200, 128, (30, 40)
    f0, f1 = synth.coarse_descriptors(91, 1, l, c, "peaky")
    sampled = sorted({(t * l) // 32 for t in range(32)})
    free = [r for r in range(l) if r not in sampled]
    f0[0, free[5]] *= 4.0
    ref = orc.coarse_match(f0, f1, (240, 320), hw, hw, 0.2, 2, 0.1)
    st, m, info, hint, out = _auto_call(f0, f1, hw, hw, 8.0)
    assert st == 0 and (hint & _lib.FM_MODE_EXACT_STEP) and m == ref['i_ids'].shape[0] > 700
    _assert_coarse(out, ref)
    # too small output buffers
    st, m, info, hint, out = _auto_call(f0, f1, hw, hw, 8.0, cap=100)
    assert st == _lib.FM_E_CAPACITY and m == ref['i_ids'].shape[0]
    st, m2, info, hint, out = _auto_call(f0, f1, hw, hw, 8.0, cap=m, hint=hint & 0xffff)
    assert st == 0 and m2 == m and (hint >> 24) & 0xff == 1
    _assert_coarse(out, ref)
    # bad input is the caller's: reported, not retried
    f0[0, 3, 7] = np.nan
    st, m, info, hint, out = _auto_call(f0, f1, hw, hw, 8.0)
    assert st == _lib.FM_E_RANGE


def test_alone_hint_changes_launch_geometry_only():
    """FM_MODE_ALONE (the caller has the GPU to itself: two max-pass workgroups per CU, 8-unit screening chunks) is a hint
    about the device - the outputs must be the bits of the call without it, on peaked, flat and mixed data, one pair and
    a small batch; and the synchronous ops.coarse_match passes it by default."""
    for name, dist, nb in (("cfg2_peaky", "peaky", 1), ("cfg2_mixed", "mixed", 1), ("cfg1_borderline", "borderline", 3)):
        g = load_golden(name)
        inp = case_inputs(g['meta'], dist, with_fine=False)
        f0 = torch.as_tensor(np.repeat(inp['f0'], nb, 0), device=DEV)
        f1 = torch.as_tensor(np.repeat(inp['f1'], nb, 0), device=DEV)
        a = _np(ops.coarse_match(f0, f1, inp['hw_c'], inp['hw_c'], 8.0, alone=True))
        b = _np(ops.coarse_match(f0, f1, inp['hw_c'], inp['hw_c'], 8.0, alone=False))
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)
        sel = a['b_ids'] == 0
        _assert_coarse({k: v[sel] for k, v in a.items()}, g)
    # the asynchronous form: the mode bit reaches the C call and the workspace size does not depend on it
    inp = case_inputs(load_golden("cfg2_peaky")['meta'], "peaky", with_fine=False)
    t0, t1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    x = ops.coarse_match_async(t0, t1, inp['hw_c'], inp['hw_c'], 8.0, alone=True)
    y = ops.coarse_match_async(t0, t1, inp['hw_c'], inp['hw_c'], 8.0, alone=False)
    mx, my = x.read_count(), y.read_count()
    assert mx == my and x.workspace.numel() == y.workspace.numel()
    assert torch.equal(x.i_ids[:mx], y.i_ids[:my]) and torch.equal(x.mconf[:mx], y.mconf[:my])


def test_coarse_without_cell_maps_gives_the_same_matches():
    """FM_MODE_NO_CELL_MAPS only drops the cell -> match maps (for callers that never run the cell-ordered crops)."""
    f0, f1 = synth.coarse_descriptors(44, 2, 20 * 30, 128, "peaky")
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    a = ops.coarse_match_async(t0, t1, (20, 30), (20, 30), 8.0)
    b = ops.coarse_match_async(t0, t1, (20, 30), (20, 30), 8.0, cell_maps=False)
    ma, mb = a.read_count(), b.read_count()
    assert ma == mb > 300
    for k, v in a.sliced(ma).items():
        assert torch.equal(v, b.sliced(mb)[k]), k
    a.cell_maps()
    with pytest.raises(RuntimeError):
        b.cell_maps()


@pytest.mark.parametrize("case", ["outlier_row", "outlier_row_both_images", "textureless_sample"])
def test_int8_step_survives_outliers_outside_the_sampled_rows(case):
    """The int8 screening step of an image comes from 32 sampled rows (k_prep_split); what it clips elsewhere widens
    every margin.  (a) ONE descriptor 4x larger than the rest, outside the sample; (b) one in each image (3x / 2.5x); (c)
    every SAMPLED row of image 0 nearly zero (a sample that fell on textureless cells).  The first call reports FM_E_STEP
    - not FM_E_RANGE: the inputs are fine; not a silent detour through the dense kernel - and FM_MODE_EXACT_STEP (the
    true maxima from one more small kernel) serves them; ops.coarse_match does that by itself and remembers the shape.
    (An outlier row's noise entries are as large as other columns' peaks, and the partners of near-zero cells are rows
    without a peak: such data legitimately needs the dense sum kernel as well - the explicit call below switches it on,
    ops.coarse_match finds out.)"""
    l, c, hw = 1200, 128, (30, 40)
    f0, f1 = synth.coarse_descriptors(91, 1, l, c, "peaky")
    sampled = sorted({(t * l) // 32 for t in range(32)})
    free = [r for r in range(l) if r not in sampled]
    if case == "outlier_row":
        f0[0, free[5]] *= 4.0
    elif case == "outlier_row_both_images":
        f0[0, free[5]] *= 3.0
        f1[0, free[77]] *= 2.5
    else:
        f0[0, sampled] *= 1e-3
    ref = orc.coarse_match(f0, f1, (240, 320), hw, hw, 0.2, 2, 0.1)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    with pytest.raises(_lib.FMatchError) as e:
        ops.coarse_match_async(t0, t1, hw, hw, 8.0, dense=True, exact_screening=True).read_count()
    assert e.value.status == _lib.FM_E_STEP
    buf = ops.coarse_match_async(t0, t1, hw, hw, 8.0, exact_step=True, dense=True, exact_screening=True)
    m = buf.read_count()
    _assert_coarse(buf.sliced(m), ref)
    assert m == ref['i_ids'].shape[0] > 700
    ops.MODE_MEMORY.clear()
    out = ops.coarse_match(t0, t1, hw, hw, 8.0)                  # retries by itself ...
    _assert_coarse(out, ref)
    snap = ops.MODE_MEMORY.snapshot()
    assert len(snap) == 1 and list(snap.values())[0]['step']
    ops.MODE_MEMORY.clear()
    # ... and the exact step changes nothing for ordinary data (finer codes, same matches)
    g0, g1 = synth.coarse_descriptors(92, 1, l, c, "borderline")
    a = ops.coarse_match(torch.as_tensor(g0, device=DEV), torch.as_tensor(g1, device=DEV), hw, hw, 8.0, exact_step=True)
    _assert_coarse(a, orc.coarse_match(g0, g1, (240, 320), hw, hw, 0.2, 2, 0.1))


def test_non_finite_input_is_reported():
    f0, f1 = synth.coarse_descriptors(42, 1, 64, 64, "peaky")
    f0[0, 3, 5] = np.inf
    with pytest.raises(_lib.FMatchError) as e:
        _run_coarse(f0, f1, (64, 64), (8, 8), (8, 8))
    assert e.value.status == _lib.FM_E_RANGE


@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("channels_last", [False, True])
def test_gather_windows_vs_oracle(w, channels_last):
    ff0, _ = synth.fine_maps(51, 2, 64, 48, 64)
    wc = 16
    ids = torch.tensor([0, 15, 11 * 16 + 15, 11 * 16, 37, 100, 191, 5, 16], dtype=torch.int64)
    b = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0, 0], dtype=torch.int64)
    ref = orc.crop_windows(ff0, b, ids, w, 4, wc)
    t = torch.as_tensor(ff0, device=DEV)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    got = ops.gather_windows(t, b.to(DEV), ids.to(DEV), w, 4, wc)
    assert torch.equal(got.cpu(), ref)                   # a gather is bit-exact


@pytest.mark.parametrize("w", [5, 7])
def test_fine_match_vs_oracle(w):
    m, ww = 1000, w * w
    win0 = synth.normal(61, 1, (m, ww, 64))
    win1 = synth.normal(61, 2, (m, ww, 64))
    win1[:200] = win0[:200] * 3.0                        # sharp heat-maps too
    w0, b0, w1, b1 = synth.mix_weights(61, ww)
    kc0 = (synth.uniform(61, 3, m * 2).reshape(m, 2) * 600).astype(np.float32)
    kc1 = (synth.uniform(61, 4, m * 2).reshape(m, 2) * 600).astype(np.float32)
    r0, r1 = orc.fine_match(win0, win1, w0, b0, w1, b1, kc0, kc1, 2.0)
    mix0 = torch.as_tensor(np.concatenate([w0, [b0]]).astype(np.float32), device=DEV)
    mix1 = torch.as_tensor(np.concatenate([w1, [b1]]).astype(np.float32), device=DEV)
    g0, g1 = ops.fine_match(torch.as_tensor(win0, device=DEV), torch.as_tensor(win1, device=DEV), mix0, mix1,
                            torch.as_tensor(kc0, device=DEV), torch.as_tensor(kc1, device=DEV), 2.0)
    assert (g0.cpu() - r0).abs().max().item() <= FINE_TOL_PX
    assert (g1.cpu() - r1).abs().max().item() <= FINE_TOL_PX


@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("channels_last", [False, True])
def test_fine_match_from_the_maps(w, channels_last):
    """fm_fine_match_maps (crop + fine in one call, no window tensors; channels-last maps read in place, NCHW maps
    through the tiled transpose) against the oracle's crop + fine (<= 1e-3 px) and against fm_gather_windows +
    fm_fine_match bit for bit.  Rectangular maps of different sizes whose widths (52, 40) are not multiples of the
    transpose's 64-pixel tile, cells on every border (zero padding on all four sides), N = 2."""
    n, (h0c, w0c), (h1c, w1c) = 2, (9, 13), (11, 10)
    ff0 = np.stack([synth.normal(171 + b, 1, (64, h0c * 4, w0c * 4)) for b in range(n)])
    ff1 = np.stack([synth.normal(171 + b, 2, (64, h1c * 4, w1c * 4)) for b in range(n)])
    m = 160
    b = np.sort((synth.uniform(171, 3, m) * n).astype(np.int64))
    i = (synth.uniform(171, 4, m) * h0c * w0c).astype(np.int64)
    j = (synth.uniform(171, 5, m) * h1c * w1c).astype(np.int64)
    i[:6] = [0, w0c - 1, (h0c - 1) * w0c, h0c * w0c - 1, 5, (h0c // 2) * w0c]           # corners and edges
    j[:6] = [h1c * w1c - 1, 0, w1c - 1, (h1c - 1) * w1c, (h1c // 2) * w1c + w1c - 1, 3]
    w0, b0, w1, b1 = synth.mix_weights(171, w * w)
    kc0 = np.stack([(i % w0c) * 8.0, (i // w0c) * 8.0], 1).astype(np.float32)
    kc1 = np.stack([(j % w1c) * 8.0, (j // w1c) * 8.0], 1).astype(np.float32)
    bt, it, jt = torch.as_tensor(b), torch.as_tensor(i), torch.as_tensor(j)
    r0, r1 = orc.fine_match(orc.crop_windows(ff0, bt, it, w, 4, w0c), orc.crop_windows(ff1, bt, jt, w, 4, w1c),
                            w0, b0, w1, b1, kc0, kc1, 2.0)
    t0, t1 = torch.as_tensor(ff0, device=DEV), torch.as_tensor(ff1, device=DEV)
    if channels_last:
        t0, t1 = t0.contiguous(memory_format=torch.channels_last), t1.contiguous(memory_format=torch.channels_last)
    mix0 = torch.as_tensor(np.concatenate([w0, [b0]]).astype(np.float32), device=DEV)
    mix1 = torch.as_tensor(np.concatenate([w1, [b1]]).astype(np.float32), device=DEV)
    bd, idv, jd = bt.to(DEV), it.to(DEV), jt.to(DEV)
    k0d, k1d = torch.as_tensor(kc0, device=DEV), torch.as_tensor(kc1, device=DEV)
    cnt = torch.tensor([m - 7, 0], dtype=torch.int32, device=DEV)                       # device-side count < capacity
    g0, g1 = ops.fine_match_maps(t0, t1, bd, idv, jd, w, 4, w0c, w1c, mix0, mix1, k0d, k1d, 2.0, count=cnt)
    assert (g0[:m - 7].cpu() - r0[:m - 7]).abs().max().item() <= FINE_TOL_PX
    assert (g1[:m - 7].cpu() - r1[:m - 7]).abs().max().item() <= FINE_TOL_PX
    win0 = ops.gather_windows(t0, bd, idv, w, 4, w0c)
    win1 = ops.gather_windows(t1, bd, jd, w, 4, w1c)
    assert torch.equal(win0.cpu(), orc.crop_windows(ff0, bt, it, w, 4, w0c))            # (the 16-byte-chunk crop is exact)
    h0, h1 = ops.fine_match(win0, win1, mix0, mix1, k0d, k1d, 2.0)
    assert torch.equal(g0[:m - 7], h0[:m - 7]) and torch.equal(g1[:m - 7], h1[:m - 7])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("w", [5, 7])
def test_half_precision_fine_maps_need_no_upcast(w, channels_last, dtype):
    """float16 / bfloat16 fine maps (an autocast backbone's hand-over, network/net.py:56-57) go to
    fm_fine_match_maps_dtype as they are: every such value is exact in float32 and the arithmetic is the float32
    call's, so the result equals the call on the up-cast maps bit for bit.  Odd map widths, cells on the borders."""
    n, (h0c, w0c), (h1c, w1c) = 2, (9, 13), (11, 10)
    ff0 = torch.as_tensor(np.stack([synth.normal(271 + b, 1, (64, h0c * 4, w0c * 4)) for b in range(n)]), device=DEV).to(dtype)
    ff1 = torch.as_tensor(np.stack([synth.normal(271 + b, 2, (64, h1c * 4, w1c * 4)) for b in range(n)]), device=DEV).to(dtype)
    m = 120
    b = torch.as_tensor(np.sort((synth.uniform(271, 3, m) * n).astype(np.int64)), device=DEV)
    i = (synth.uniform(271, 4, m) * h0c * w0c).astype(np.int64)
    j = (synth.uniform(271, 5, m) * h1c * w1c).astype(np.int64)
    i[:4] = [0, w0c - 1, (h0c - 1) * w0c, h0c * w0c - 1]
    j[:4] = [h1c * w1c - 1, 0, w1c - 1, (h1c - 1) * w1c]
    kc0 = torch.as_tensor(np.stack([(i % w0c) * 8.0, (i // w0c) * 8.0], 1).astype(np.float32), device=DEV)
    kc1 = torch.as_tensor(np.stack([(j % w1c) * 8.0, (j // w1c) * 8.0], 1).astype(np.float32), device=DEV)
    it, jt = torch.as_tensor(i, device=DEV), torch.as_tensor(j, device=DEV)
    mix0, mix1 = _mix_tensors(synth.mix_weights(271, w * w))
    if channels_last:
        ff0, ff1 = ff0.contiguous(memory_format=torch.channels_last), ff1.contiguous(memory_format=torch.channels_last)
    g0, g1 = ops.fine_match_maps(ff0, ff1, b, it, jt, w, 4, w0c, w1c, mix0, mix1, kc0, kc1, 2.0)
    h0, h1 = ops.fine_match_maps(ff0.float(), ff1.float(), b, it, jt, w, 4, w0c, w1c, mix0, mix1, kc0, kc1, 2.0)
    assert g0.dtype == torch.float32 and torch.equal(g0, h0) and torch.equal(g1, h1)
    assert torch.isfinite(g0).all() and (g0[:, :2] - kc0).abs().max() < 16


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("channels_last", [False, True])
def test_half_precision_maps_are_cropped_without_an_upcast(channels_last, dtype):
    """ops.gather_windows on float16 / bfloat16 maps (fm_gather_windows_dtype): read as they are - the crop of the up-cast
    map bit for bit, zero padding on the borders included."""
    n, (hc, wc) = 2, (9, 13)
    ff = torch.as_tensor(np.stack([synth.normal(281 + b, 1, (64, hc * 4, wc * 4)) for b in range(n)]), device=DEV).to(dtype)
    m = 90
    b = torch.as_tensor(np.sort((synth.uniform(281, 3, m) * n).astype(np.int64)), device=DEV)
    i = (synth.uniform(281, 4, m) * hc * wc).astype(np.int64)
    i[:4] = [0, wc - 1, (hc - 1) * wc, hc * wc - 1]
    it = torch.as_tensor(i, device=DEV)
    if channels_last:
        ff = ff.contiguous(memory_format=torch.channels_last)
    for w in (5, 7):
        got = ops.gather_windows(ff, b, it, w, 4, wc)
        ref = ops.gather_windows(ff.float(), b, it, w, 4, wc)
        assert got.dtype == torch.float32 and torch.equal(got, ref)
        assert torch.equal(got.cpu(), orc.crop_windows(ff.float().cpu().contiguous().numpy(), b.cpu(), it.cpu(), w, 4, wc))


# ------------------------------------------------------------------ drop-in modules
def test_modules_follow_the_data_dict_protocol():
    g = load_golden("cfg1_peaky")
    inp = case_inputs(g['meta'], "peaky")
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 64}, 'fine': {'d_model': 64}}
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1,
                                 'train_coarse_percent': 1.0, 'train_pad_num_gt_min': 200}).eval()
    fp = modules.FinePreprocess(cfg).to(DEV).eval()
    fm = modules.FineMatching({'d_model': 64}).to(DEV).eval()
    w0, b0, w1, b1 = inp['mix']
    with torch.no_grad():
        fm.mix_feat_0.weight.copy_(torch.as_tensor(w0).view(1, -1)); fm.mix_feat_0.bias.fill_(float(b0))
        fm.mix_feat_1.weight.copy_(torch.as_tensor(w1).view(1, -1)); fm.mix_feat_1.bias.fill_(float(b1))
        fp.down_proj.weight.zero_(); fp.down_proj.bias.zero_()          # identity context merge, as in the
        fp.merge_feat.weight.zero_(); fp.merge_feat.bias.zero_()        # fixture generator
        fp.merge_feat.weight[:, :64] = torch.eye(64)
    data = {'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i'], 'hw0_c': inp['hw_c'], 'hw1_c': inp['hw_c'],
            'hw0_f': inp['hw_f'], 'hw1_f': inp['hw_f'], 'bs': 1}
    fc0, fc1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    cm(fc0, fc1, data)
    for key in ('b_ids', 'i_ids', 'j_ids', 'gt_mask', 'm_bids', 'mkpts0_c', 'mkpts1_c', 'mconf'):
        assert key in data
    assert data['gt_mask'].dtype == torch.bool and data['b_ids'].dtype == torch.int64
    with torch.no_grad():
        u0, u1 = fp(torch.as_tensor(inp['ff0'], device=DEV), torch.as_tensor(inp['ff1'], device=DEV), fc0, fc1, data)
    assert data['W'] == 7 and u0.shape == (data['b_ids'].shape[0], 49, 64)
    fm(u0, u1, data)
    assert data['mkpts0_f'].shape == (u0.shape[0], 3)
    assert np.abs(data['mkpts0_f'].cpu().numpy()[:, :2] - g['mkpts0_f'][:, :2]).max() <= 2e-3
    assert np.abs(data['mkpts1_f'].cpu().numpy()[:, :2] - g['mkpts1_f'][:, :2]).max() <= 2e-3
    # M == 0 branch (fine_matching_new.py:40-48)
    d0 = dict(data, mkpts0_c=data['mkpts0_c'][:0], mkpts1_c=data['mkpts1_c'][:0], b_ids=data['b_ids'][:0],
              i_ids=data['i_ids'][:0], j_ids=data['j_ids'][:0])
    e0, e1 = fp(torch.as_tensor(inp['ff0'], device=DEV), torch.as_tensor(inp['ff1'], device=DEV), fc0, fc1, d0)
    assert e0.shape == (0, 49, 64)
    fm(e0, e1, d0)
    assert d0['expec_f'].shape == (0, 3) and d0['mkpts0_f'].shape == (0, 2)


# ------------------------------------------------------------------ properties at full size
def test_properties_at_cfg2_size():
    cfg = synth.CONFIGS['cfg2']
    sh = synth.config_shapes(cfg)
    f0, f1 = synth.coarse_descriptors(77, 2, sh['l'], 256, "peaky")
    hw_c = (sh['hc'], sh['wc'])
    a = _np(_run_coarse(f0, f1, (480, 640), hw_c, hw_c))
    b = _np(_run_coarse(f0, f1, (480, 640), hw_c, hw_c))
    for k in a:                                           # deterministic, bit for bit
        assert np.array_equal(a[k], b[k]), k
    key = a['b_ids'] * (1 << 40) + a['i_ids'] * (1 << 20) + a['j_ids']
    assert np.all(np.diff(key) > 0)                       # torch.where order, no duplicates
    assert a['mconf'].min() > 0.2
    # border cells never match
    for ids in (a['i_ids'], a['j_ids']):
        y, x = ids // sh['wc'], ids % sh['wc']
        assert y.min() >= 2 and y.max() < sh['hc'] - 2 and x.min() >= 2 and x.max() < sh['wc'] - 2
    # batch of two == the two pairs run alone
    s0 = _np(_run_coarse(f0[:1], f1[:1], (480, 640), hw_c, hw_c))
    s1 = _np(_run_coarse(f0[1:], f1[1:], (480, 640), hw_c, hw_c))
    m0 = (a['b_ids'] == 0).sum()
    assert np.array_equal(a['i_ids'][:m0], s0['i_ids']) and np.array_equal(a['j_ids'][m0:], s1['j_ids'])
    assert np.array_equal(a['mconf'][:m0], s0['mconf']) and np.array_equal(a['mconf'][m0:], s1['mconf'])
    # swapping the two images transposes the match set (dual softmax is symmetric)
    t = _np(_run_coarse(f1[:1], f0[:1], (480, 640), hw_c, hw_c))
    fwd = set(zip(s0['i_ids'].tolist(), s0['j_ids'].tolist()))
    bwd = set(zip(t['j_ids'].tolist(), t['i_ids'].tolist()))
    assert len(fwd ^ bwd) <= 2                            # conf differs in the last bits only


def test_properties_at_cfg3_size():
    """BASELINE config #3 at its size (batch of 64 pairs of 640x480, C = 256): the launch geometry of a batch that
    fills the chip by itself (one column split in the max pass, 64-unit ranges in the sparse sum kernel).  Inputs
    are generated on the device (same statistics as the 'peaky' distribution); checked: bitwise determinism,
    torch.where order, border exclusion, and batch == the single pairs run alone."""
    sh = synth.config_shapes(synth.CONFIGS['cfg2'])
    n, l, c = 64, sh['l'], 256
    g = torch.Generator(device=DEV).manual_seed(123)
    f0 = 4.0 * torch.randn(n, l, c, device=DEV, generator=g)
    f1 = torch.empty_like(f0)
    for b in range(n):
        f1[b] = f0[b, torch.randperm(l, device=DEV, generator=g)]
    f1 += 0.4 * torch.randn(n, l, c, device=DEV, generator=g)
    hw_c = (sh['hc'], sh['wc'])
    run = lambda a0, a1: _np(ops.coarse_match(a0, a1, hw_c, hw_c, 8.0))
    # the common path alone serves peaked data at this size too (four launches + k_thresh: no sample flagged for the
    # dense kernel - read_count would raise FM_E_DENSE - and ops.coarse_match below does not fall back silently)
    ops.MODE_MEMORY.clear()
    common = ops.coarse_match_async(f0, f1, hw_c, hw_c, 8.0)
    m_common = common.read_count()
    a = run(f0, f1)
    assert not ops.MODE_MEMORY.snapshot(), "the batch needed a retry of the coarse stage"
    assert m_common == a['i_ids'].shape[0]
    b2 = run(f0, f1)
    for k in a:                                           # deterministic, bit for bit
        assert np.array_equal(a[k], b2[k]), k
    key = a['b_ids'] * (1 << 40) + a['i_ids'] * (1 << 20) + a['j_ids']
    assert np.all(np.diff(key) > 0)                       # torch.where order, no duplicates
    assert set(np.unique(a['b_ids']).tolist()) == set(range(n))
    assert a['mconf'].min() > 0.2 and a['i_ids'].shape[0] > 0.7 * n * 56 * 76
    for ids in (a['i_ids'], a['j_ids']):                  # border cells never match
        y, x = ids // sh['wc'], ids % sh['wc']
        assert y.min() >= 2 and y.max() < sh['hc'] - 2 and x.min() >= 2 and x.max() < sh['wc'] - 2
    for b in (0, 31, 63):                                 # a sample of the batch == that pair run alone
        s = run(f0[b:b + 1], f1[b:b + 1])
        sel = a['b_ids'] == b
        assert np.array_equal(a['i_ids'][sel], s['i_ids']) and np.array_equal(a['j_ids'][sel], s['j_ids'])
        assert np.array_equal(a['mconf'][sel], s['mconf']) and np.array_equal(a['mkpts1_c'][sel], s['mkpts1_c'])


# ------------------------------------------------------------------ row a8: net.forward after the backbone
@pytest.mark.parametrize("name,meta", [("net_tail_small", NET_TAIL), ("net_tail_cfg2", NET_TAIL_CFG2)])
def test_matcher_tail_against_reference_fixture(name, meta):
    """Matcher.forward_features (network/net.py:66-83: HIP coarse context layers (fm_coarse_transformer, 8 layers,
    d_model 256) -> HIP coarse matching -> HIP window crop fused with the context merge -> HIP fine context layers
    (fm_fine_transformer) -> HIP fine matching) against the fixtures the REFERENCE's own five modules produced for the
    same seeded feature maps and weights: two 128x128 pairs, and ONE 640x480 PAIR - the size bench.py times
    forward_features at (L = S = 4800, 1624 matches with conf spread over (0.2, 1]).  The context layers are
    float32-equivalent products in another summation order than the fixture's, which moves the descriptors by ~1e-6
    relative: the conf tolerance of this chain test is 4e-5 (guard band likewise; measured 1.3e-5 / 2.0e-5), fine
    keypoints 5e-4 px (measured 6e-5)."""
    from featurematching_amd.matcher import Matcher
    g = load_golden(name)
    inp = net_tail_inputs(meta)
    m = Matcher().to(DEV).eval()
    t = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
    m.coarse.load_state_dict(t(inp['w_coarse']))
    m.fine.load_state_dict(t(inp['w_fine']))
    m.fine_preprocess.load_state_dict(t(inp['w_prep']))
    w0, b0, w1, b1 = inp['mix']
    with torch.no_grad():
        m.fine_matching.mix_feat_0.weight.copy_(torch.as_tensor(w0).view(1, -1)); m.fine_matching.mix_feat_0.bias.fill_(float(b0))
        m.fine_matching.mix_feat_1.weight.copy_(torch.as_tensor(w1).view(1, -1)); m.fine_matching.mix_feat_1.bias.fill_(float(b1))
    dev = lambda x: torch.as_tensor(x, device=DEV)
    data = {'bs': meta['n'], 'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i']}
    m.forward_features(dev(inp['feat_c0']), dev(inp['feat_c1']), dev(inp['feat_f0']), dev(inp['feat_f1']), data)
    np.testing.assert_allclose(data['feat_c0'].double().sum((1, 2)).cpu().numpy(), g['c0_sum'], rtol=1e-5)
    got = _np({k: data[k] for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c')})
    only_g, only_r, err = compare_match_sets(got, g)
    FLIPS.append((f"test_matcher_tail_against_reference_fixture[{name}]", len(only_g) + len(only_r), len(g['i_ids']), err))
    assert all(abs(v - 0.2) < 4e-5 for _, v in only_g + only_r), (only_g, only_r)
    assert err <= 4e-5, err
    gk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(got['b_ids'], got['i_ids'], got['j_ids']))}
    rk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(g['b_ids'], g['i_ids'], g['j_ids']))}
    common = [k for k in gk if k in rk]
    gi, ri = np.array([gk[k] for k in common]), np.array([rk[k] for k in common])
    assert len(common) >= len(rk) - 2 and len(rk) > 80
    assert np.array_equal(got['mkpts0_c'][gi], g['mkpts0_c'][ri])
    assert np.abs(data['mkpts0_f'].cpu().numpy()[gi, :2] - g['mkpts0_f'][ri, :2]).max() <= 5e-4
    assert np.abs(data['mkpts1_f'].cpu().numpy()[gi, :2] - g['mkpts1_f'][ri, :2]).max() <= 5e-4


def test_matcher_tail_redoes_the_fine_half_when_the_fine_kernel_reports_its_range():
    """Matcher.forward_features reads the fine kernel's range report BEHIND the launch of the fine matching (the host
    sync then waits behind work the GPU has).  A fine-layer weight of 20 lies outside the kernel's fixed weight scale
    (|w| < 16): the report must send the call through the float32 layers and the fine matching must be redone on their
    output - the same keypoints as a matcher whose fine layers never use the kernel."""
    from featurematching_amd.matcher import Matcher
    inp = net_tail_inputs()
    t = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
    dev = lambda x: torch.as_tensor(x, device=DEV)
    outs = []
    for use_hip in (True, False):
        torch.manual_seed(7)
        m = Matcher().to(DEV).eval()
        m.coarse.load_state_dict(t(inp['w_coarse']))
        m.fine.load_state_dict(t(inp['w_fine']))
        m.fine_preprocess.load_state_dict(t(inp['w_prep']))
        with torch.no_grad():
            m.fine.layers[0].q_proj.weight[0, 0] = 20.0
        m.fine.use_hip = use_hip
        data = {'bs': NET_TAIL['n'], 'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i']}
        m.forward_features(dev(inp['feat_c0']), dev(inp['feat_c1']), dev(inp['feat_f0']), dev(inp['feat_f1']), data)
        outs.append((data, m.fine.range_fallbacks))
    (d_hip, fb_hip), (d_ref, fb_ref) = outs
    assert fb_hip == 1 and fb_ref == 0
    assert torch.equal(d_hip['i_ids'], d_ref['i_ids']) and d_hip['i_ids'].numel() > 80
    assert torch.isfinite(d_hip['mkpts0_f']).all()
    assert torch.equal(d_hip['mkpts0_f'], d_ref['mkpts0_f']) and torch.equal(d_hip['mkpts1_f'], d_ref['mkpts1_f'])


# ------------------------------------------------------------------ match(img0, img1) facade
def test_matcher_end_to_end_on_warped_images():
    """Seeded-random backbone, image1 = image0 shifted by (16, 8) px: the matcher must run end to
    end, honour the API surface and recover the shift for the bulk of its matches."""
    from featurematching_amd.matcher import Matcher
    torch.manual_seed(3)
    m = Matcher().to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    img = torch.rand(1, 3, 480 + 32, 640 + 32, generator=g) * 255      # white noise: every cell is distinctive
    img0 = img[:, :, 0:480, 0:640].contiguous().to(DEV)
    img1 = img[:, :, 8:488, 16:656].contiguous().to(DEV)
    k0, k1, conf = m.match(img0, img1)
    assert k0.shape == k1.shape and k0.shape[1] == 2 and conf.shape[0] == k0.shape[0]
    assert k0.shape[0] > 100
    # coarse level: image1 = image0 shifted by exactly (2, 1) cells -> every coarse match has that shift
    dc = (m.last['mkpts0_c'] - m.last['mkpts1_c']).cpu().numpy()
    assert ((dc[:, 0] == 16) & (dc[:, 1] == 8)).mean() > 0.98
    # fine level (random weights): offsets stay inside the window, i.e. W//2 +- (W//2)*scale = 3 +- 6 px
    off0 = (k0 - m.last['mkpts0_c']).cpu().numpy()
    assert off0.min() >= -3.001 and off0.max() <= 9.001
    for key in ('mkpts0_f', 'mkpts1_f', 'mconf', 'm_bids', 'feat_c0', 'feat_f1', 'hw0_c', 'W'):
        assert key in m.last


# ------------------------------------------------------------------ dense conf_matrix + training ids
def test_dense_conf_matrix_keeps_the_rows_of_textureless_cells():
    """The dead-row certificate of the sparse sum kernel (no match possible -> nobody reads the row's denominator) must
    not be used when the dense conf_matrix is requested: the training loss reads EVERY entry, also the ~1/S^2 ones of
    near-zero descriptors."""
    f0, f1 = synth.coarse_descriptors(47, 1, 20 * 30, 128, "peaky")
    f0[:, ::3] *= 1e-4
    f1[:, 1::3] *= 1e-4
    ref = orc.coarse_match(f0, f1, (160, 240), (20, 30), (20, 30), 0.2, 2, 0.1, return_conf=True)
    out = ops.coarse_match(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), (20, 30), (20, 30), 8.0,
                           conf_matrix=True)
    _assert_coarse(out, ref)
    got = out['conf_matrix'].cpu()
    assert torch.isfinite(got).all()
    # the dense matrix comes from the hi/lo-split float16 product (22 significant bits: at similarities of ~160 an entry
    # with conf c carries 2 * 2^-22 |sim| c); round 5: every entry with conf > 0.1 of a sample the dense kernel served is
    # rewritten from its exact float32 dot product (k_conf_patch_dense), as the entries on a screened sample's lists are
    # - the bar is BASELINE.md's 1e-5 EVERYWHERE
    smax = float(np.abs(f0[0].astype(np.float64) @ f1[0].astype(np.float64).T).max()) / (128 * 0.1)
    assert smax > 100 and (got - ref['conf_matrix']).abs().max().item() <= 1e-5
    # relative accuracy where the certificate would have dropped the row: conf ~ 1 / (L S) there
    tiny = ref['conf_matrix'][0, 0]
    assert float(tiny.max()) < 1e-4 and ((got[0, 0] - tiny).abs() <= 1e-3 * tiny.abs() + 1e-12).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conf_matrix_of_a_batch_with_a_screened_and_a_flat_sample(dtype):
    """One call, two samples: sample 0 is served by the screening kernel (its conf sweep is the one-product CONF_LITE
    variant, its listed entries are rewritten from exact dot products), sample 1 has textureless cells and goes through
    the dense kernel (hi/lo-split sweep; k_exact_lists + k_fix_sums make its listed entries and their denominators exact
    together).  Both against the oracle on the same (for bfloat16: up-cast) descriptors at 1e-5, at similarities of ~200."""
    f0, f1 = synth.coarse_descriptors(53, 2, 20 * 30, 128, "peaky")
    f0[1, ::3] *= 1e-4
    f1[1, 1::3] *= 1e-4
    t0, t1 = torch.as_tensor(f0, device=DEV).to(dtype), torch.as_tensor(f1, device=DEV).to(dtype)
    g0, g1 = t0.float().cpu().numpy(), t1.float().cpu().numpy()
    ref = orc.coarse_match(g0, g1, (160, 240), (20, 30), (20, 30), 0.2, 2, 0.1, return_conf=True)
    out = ops.coarse_match(t0, t1, (20, 30), (20, 30), 8.0, conf_matrix=True)
    _assert_coarse(out, ref)
    got = out['conf_matrix'].cpu()
    smax = float(np.abs(g0[0].astype(np.float64) @ g1[0].astype(np.float64).T).max()) / (128 * 0.1)
    assert smax > 100
    for b in range(2):
        assert (got[b] - ref['conf_matrix'][b]).abs().max().item() <= 1e-5, b
    pick = got[out['b_ids'].cpu(), out['i_ids'].cpu(), out['j_ids'].cpu()]
    assert (pick - out['mconf'].cpu()).abs().max().item() <= 2e-6


def test_dense_conf_matrix_and_training_ids():
    f0, f1 = synth.coarse_descriptors(91, 2, 23 * 31, 256, "borderline")       # ragged L = S = 713
    hw_c, hw_i = (23, 31), (184, 248)
    ref = orc.coarse_match(f0, f1, hw_i, hw_c, hw_c, 0.2, 2, 0.1, return_conf=True)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    out = ops.coarse_match(t0, t1, hw_c, hw_c, 8.0, conf_matrix=True)
    _assert_coarse(out, ref)
    got = out['conf_matrix'].cpu()
    assert got.shape == ref['conf_matrix'].shape
    err = (got - ref['conf_matrix']).abs().max().item()
    assert err <= 1e-5, err
    # the emitted mconf are entries of the dense matrix
    pick = got[out['b_ids'].cpu(), out['i_ids'].cpu(), out['j_ids'].cpu()]
    assert (pick - out['mconf'].cpu()).abs().max().item() <= 2e-6
    # training mode: supervision ids select the windows (coarse_matching_new.py:113-116)
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}, conf_matrix=True).train()
    spv = dict(spv_b_ids=torch.tensor([0, 1, 1], device=DEV), spv_i_ids=torch.tensor([40, 7, 300], device=DEV),
               spv_j_ids=torch.tensor([41, 8, 5], device=DEV))
    data = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw_c, hw1_c=hw_c, **spv)
    cm(t0, t1, data)
    assert torch.equal(data['i_ids'], spv['spv_i_ids']) and data['conf_matrix'].shape == (2, 713, 713)
    assert data['mkpts0_c'].cpu().tolist() == [[(40 % 31) * 8.0, (40 // 31) * 8.0], [56.0, 0.0], [(300 % 31) * 8.0, 72.0]]
    assert data['mconf'].shape[0] == ref['mconf'].shape[0]
    with pytest.raises(RuntimeError):
        modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}).train()(t0, t1, dict(data))


def test_conf_matrix_carries_the_dual_softmax_gradient():
    """the reference's coarse loss reads data['conf_matrix'] (losses/loss.py:27-67, sparse focal
    loss on the ground-truth entries); the conf_matrix of the HIP forward must hand the same gradient to the
    descriptors as autograd through the reference's own expression (coarse_matching_new.py:64-68)."""
    f0, f1 = synth.coarse_descriptors(17, 2, 12 * 16, 64, "borderline")
    hw_c, hw_i = (12, 16), (96, 128)
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    g = torch.Generator(device="cpu").manual_seed(3)
    gt = torch.stack([torch.randint(2, (60,), generator=g), torch.randint(192, (60,), generator=g),
                      torch.randint(192, (60,), generator=g)], 1).to(DEV)

    def focal(conf):       # compute_coarse_loss, 'focal', sparse supervision (loss.py:53-60), alpha 0.25 gamma 2
        p = torch.clamp(conf, 1e-6, 1 - 1e-6)[gt[:, 0], gt[:, 1], gt[:, 2]]
        return (-0.25 * torch.pow(1 - p, 2.0) * p.log()).mean()

    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}, conf_matrix=True).train()
    spv = dict(spv_b_ids=gt[:, 0].contiguous(), spv_i_ids=gt[:, 1].contiguous(), spv_j_ids=gt[:, 2].contiguous())
    data = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw_c, hw1_c=hw_c, **spv)
    cm(a0, a1, data)
    assert data['conf_matrix'].requires_grad
    focal(data['conf_matrix']).backward()
    # the reference's expression under autograd
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    sim = torch.einsum("nlc,nsc->nls", b0 / 64 ** .5, b1 / 64 ** .5) / 0.1
    focal(torch.softmax(sim, 1) * torch.softmax(sim, 2)).backward()
    for got, ref in ((a0.grad, b0.grad), (a1.grad, b1.grad)):
        scale = ref.abs().max().item()
        assert scale > 0 and (got.double() - ref).abs().max().item() <= 2e-4 * scale


def _dense_losses(gt_mask):
    """the reference's coarse losses over ALL entries (losses/loss.py:44-50 cross entropy, :62-65 focal with dense
    supervision, alpha 0.25, gamma 2, c_pos_w = c_neg_w = 1)"""
    def focal(conf):
        c = torch.clamp(conf, 1e-6, 1 - 1e-6)
        lp = -0.25 * torch.pow(1 - c[gt_mask], 2.0) * c[gt_mask].log()
        ln = -0.25 * torch.pow(c[~gt_mask], 2.0) * (1 - c[~gt_mask]).log()
        return lp.mean() + ln.mean()

    def xent(conf):
        c = torch.clamp(conf, 1e-6, 1 - 1e-6)
        return (-torch.log(c[gt_mask])).mean() + (-torch.log(1 - c[~gt_mask])).mean()
    return {"focal": focal, "cross_entropy": xent}


@pytest.mark.parametrize("loss", ["focal", "cross_entropy", "weighted_sum"])
@pytest.mark.parametrize("hw0,hw1,c", [((12, 16), (12, 16), 64), ((15, 17), (11, 13), 128)])
def test_dense_conf_matrix_gradient_goes_through_the_hip_backward(hw0, hw1, c, loss):
    """A loss that reads EVERY entry of data['conf_matrix'] - the reference's terms over all negatives (losses/loss.py:
    44-50, 62-65; their clamp(conf, 1e-6, ..) zeroes the gradient of most entries, so what autograd hands back is sparse or
    dense depending on the data) and a plain weighted sum (dL/dconf dense for certain: fm_dual_softmax_backward_dense, three
    tiled sweeps, conf recomputed from exact dot products) - must give the descriptors the gradient float64 autograd gives
    through the reference's own expression (coarse_matching_new.py:64-68).  Ragged shapes (L != S, neither a multiple of
    32); the torch formula (three [N, L, S] temporaries, a warning) must not run."""
    l, s_ = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1 = synth.coarse_descriptors(19, 2, max(l, s_), c, "borderline")
    f0, f1 = np.ascontiguousarray(f0[:, :l]), np.ascontiguousarray(f1[:, :s_])
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    out = ops.coarse_match(a0.detach(), a1.detach(), hw0, hw1, 8.0, conf_matrix=True)
    # supervision at entries the matcher itself found (conf well inside the losses' clamp) + a few random ones
    gt_mask = torch.zeros(2, l, s_, dtype=torch.bool, device=DEV)
    gt_mask[out['b_ids'][::3], out['i_ids'][::3], out['j_ids'][::3]] = True
    g = torch.Generator(device=DEV).manual_seed(5)
    wts = torch.randn(2, l, s_, device=DEV, generator=g)
    fn = _dense_losses(gt_mask).get(loss, lambda conf: (conf * wts.to(conf.dtype)).sum())
    conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # the torch fallback warns: it must not run
        fn(conf).backward()
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    sim = torch.einsum("nlc,nsc->nls", b0 / c ** .5, b1 / c ** .5) / 0.1
    fn(torch.softmax(sim, 1) * torch.softmax(sim, 2)).backward()
    for got, ref in ((a0.grad, b0.grad), (a1.grad, b1.grad)):
        scale = ref.abs().max().item()
        assert scale > 1e-6 and (got.double() - ref).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("what", ["stats", "conf_matrix"])
def test_softmax_statistics_at_a_low_threshold_use_the_slot_count_the_call_ran_with(what):
    """thr = 0.05: fm_default_cand_slots is 32, ops.coarse_match caps the auto call at 16 slots - the workspace layout the
    statistics are read from (CoarseBuffers.softmax_stats -> fm_coarse_softmax_stats) must be the 16-slot one the serving
    attempt ran with (third byte of the hint word), not the default's; the gradient against float64 autograd through
    coarse_matching_new.py:64-68 (a layout for the wrong slot count reads past the workspace)."""
    hw = (12, 16)
    l, c = hw[0] * hw[1], 64
    f0, f1 = synth.coarse_descriptors(29, 2, l, c, "borderline")
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    lib = _lib.load()
    assert lib.fm_default_cand_slots(0.05) > 16
    out = ops.coarse_match(a0.detach(), a1.detach(), hw, hw, 8.0, thr=0.05, stats=(what == "stats"),
                           conf_matrix=(what == "conf_matrix"))
    assert out['_coarse_buffers']._shape[4] == 16
    g = torch.Generator(device="cpu").manual_seed(11)
    gt = torch.stack([torch.randint(2, (80,), generator=g), torch.randint(l, (80,), generator=g),
                      torch.randint(l, (80,), generator=g)], 1).to(DEV)
    wts = torch.randn(80, generator=g).to(DEV)
    if what == "stats":
        conf = ops.dual_softmax_at(a0, a1, gt[:, 0], gt[:, 1], gt[:, 2], out['_coarse_buffers'])
    else:
        conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])[gt[:, 0], gt[:, 1], gt[:, 2]]
    (conf * wts).sum().backward()
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    sim = torch.einsum("nlc,nsc->nls", b0 / c ** .5, b1 / c ** .5) / 0.1
    conf64 = (torch.softmax(sim, 1) * torch.softmax(sim, 2))[gt[:, 0], gt[:, 1], gt[:, 2]]
    (conf64 * wts.double()).sum().backward()
    assert (conf.detach().double() - conf64.detach()).abs().max().item() <= 1e-5
    for got, ref in ((a0.grad, b0.grad), (a1.grad, b1.grad)):
        scale = ref.abs().max().item()
        assert scale > 0 and (got.double() - ref).abs().max().item() <= 2e-4 * scale
    # the oracle's matches at this threshold too
    ref = orc.coarse_match(torch.as_tensor(f0), torch.as_tensor(f1), (96, 128), hw, hw, thr=0.05)
    _assert_coarse(out, ref, thr=0.05)


def test_dense_conf_matrix_gradient_at_cfg2_size_without_an_LxS_temporary():
    """The same at the metric's size - one 640x480 pair, L = S = 4800, C = 256 - with an assert on the allocator: the
    backward of a dense dL/dconf [1, 4800, 4800] (92 MB) may not allocate anything of that size (the torch formula it
    replaces holds three such temporaries); against float64 autograd."""
    cfg = synth.CONFIGS["cfg2"]
    sh = synth.config_shapes(cfg)
    l, c = sh['l'], cfg['c']
    hw_c = (sh['hc'], sh['wc'])
    f0, f1 = synth.coarse_descriptors(23, 1, l, c, "borderline")
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    g = torch.Generator(device=DEV).manual_seed(7)
    G = torch.randn(1, l, l, device=DEV, generator=g)
    # float64 autograd first (its temporaries are freed before the measurement)
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    sim = torch.einsum("nlc,nsc->nls", b0 / c ** .5, b1 / c ** .5) / 0.1
    ((torch.softmax(sim, 1) * torch.softmax(sim, 2)) * G.double()).sum().backward()
    del sim
    out = ops.coarse_match(a0.detach(), a1.detach(), hw_c, hw_c, 8.0, conf_matrix=True)
    conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    d0, d1 = torch.autograd.grad(conf, (a0, a1), grad_outputs=G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 0.5 * G.numel() * 4, f"backward allocated {peak / 1e6:.0f} MB next to a {G.numel() * 4 / 1e6:.0f} MB gradient"
    for got, ref in ((d0, b0.grad), (d1, b1.grad)):
        scale = ref.abs().max().item()
        assert scale > 0 and (got.double() - ref).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("dist", ["borderline", "peaky"])
def test_dual_softmax_at_supervised_entries_and_its_backward_without_an_LxS_array(dist):
    """SURVEY 8(f) row 3 at the metric's size (640x480: L = S = 4800, C = 256): the reference's coarse loss with sparse
    supervision reads conf_matrix at the ground-truth entries only (losses/loss.py:57-61).  ops.dual_softmax_at gives
    those entries - and, through fm_dual_softmax_backward, their gradient w.r.t. the descriptors - from the softmax
    statistics of a coarse call (stats=True) and tile-wise recomputed similarities: no [N, L, S] array is ever
    allocated (asserted on torch's allocator), against float64 autograd through coarse_matching_new.py:64-68."""
    cfg = synth.CONFIGS["cfg2"]
    sh = synth.config_shapes(cfg)
    l, c = sh['l'], cfg['c']
    f0, f1 = synth.coarse_descriptors(cfg['seed'] + 40, 1, l, c, dist)
    hw_c = (sh['hc'], sh['wc'])
    # supervised entries: 2500 true partners (row i of image 0 sits at column perm^-1(i) of image 1) + 500 wrong pairs
    perm = synth.permutation(cfg['seed'] + 40, 3, l)             # f1[q] = f0[perm[q]] + noise
    inv = np.empty(l, np.int64); inv[perm] = np.arange(l)
    rows = synth.permutation(9, 1, l)[:3000]
    cols = inv[rows].copy()
    cols[2500:] = synth.permutation(9, 2, l)[:500]
    gi, gj = torch.as_tensor(rows, device=DEV), torch.as_tensor(cols, device=DEV)
    gb = torch.zeros_like(gi)

    def focal(p):          # compute_coarse_loss 'focal' with sparse supervision (loss.py:53-60), alpha 0.25 gamma 2
        p = torch.clamp(p, 1e-6, 1 - 1e-6)
        return (-0.25 * torch.pow(1 - p, 2.0) * p.log()).mean()

    # the reference's expression under float64 autograd (this one DOES build the L x S matrices)
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    sim = torch.einsum("nlc,nsc->nls", b0 / c ** .5, b1 / c ** .5) / 0.1
    conf64 = (torch.softmax(sim, 1) * torch.softmax(sim, 2))[gb, gi, gj]
    focal(conf64).backward()
    ref0, ref1, conf64 = b0.grad.clone(), b1.grad.clone(), conf64.detach().clone()
    del sim, b0, b1
    torch.cuda.empty_cache()

    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.coarse_match(a0.detach(), a1.detach(), hw_c, hw_c, 8.0, stats=True, dense=(dist != "peaky"))
    conf = ops.dual_softmax_at(a0, a1, gb, gi, gj, out['_coarse_buffers'])
    focal(conf).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 0.75 * l * l * 4, f"peak {peak / 1e6:.1f} MB: an L x S float32 array is {l * l * 4 / 1e6:.1f} MB"
    # (against float64: the float32 reference's own sums are up to ~5e-6 away at S = 4800, tools/diag_conf_f64.py)
    assert (conf.detach().double() - conf64).abs().max().item() <= 1.5e-5
    for got, ref in ((a0.grad, ref0), (a1.grad, ref1)):
        scale = ref.abs().max().item()
        # ('peaky': every supervised conf is beyond the loss's clamp at 1e-6 / 1 - 1e-6 - the gradient is exactly zero)
        assert (scale > 0) == (dist == "borderline")
        assert (got.double() - ref).abs().max().item() <= 2e-4 * scale


def test_dense_conf_matrix_entries_that_matter_take_the_exact_route():
    """data['conf_matrix'] on peaked data (|sim| ~ 160): the dense sweep's hi/lo-split products carry 22 bits (2e-4 in a
    conf near 1 there); every entry with a non-negligible row term is rewritten from its exact float32 dot product
    (k_conf_patch), so the matrix is within 1e-5 of the reference everywhere."""
    f0, f1 = synth.coarse_descriptors(58, 2, 30 * 40, 256, "peaky")
    hw_c = (30, 40)
    ref = orc.coarse_match(f0, f1, (240, 320), hw_c, hw_c, 0.2, 2, 0.1, return_conf=True)
    out = ops.coarse_match(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), hw_c, hw_c, 8.0, conf_matrix=True)
    _assert_coarse(out, ref)
    err = (out['conf_matrix'].cpu() - ref['conf_matrix']).abs().max().item()
    assert err <= 1e-5, err
    smax = float(np.abs(f0[0].astype(np.float64) @ f1[0].astype(np.float64).T).max()) / (256 * 0.1)
    assert smax > 100            # (where the 22-bit route alone would be ~2^-22 * 160 = 4e-5 off)


def test_conf_matrix_at_the_bench_size_one_product_sweep():
    """The conf sweep of a sample the screening kernel served is ONE float16 product (k_dense<C, CONF_LITE>): everything
    that matters is on a row's list and rewritten exactly, the rest is below 2^-32 of its row's largest term.  At the
    bench's size (one 640x480 pair, L = S = 4800, C = 256, |sim| ~ 200) against the oracle's float32 matrix: 1e-5 in
    every entry; the listed entries (conf > 1e-6 here) also RELATIVE to 1e-4; no entry that the reference has below
    1e-9 comes out above 1e-8."""
    cfg = dict(synth.CONFIGS["cfg2"], n=1)
    sh = synth.config_shapes(cfg)
    f0, f1 = synth.coarse_descriptors(4711, 1, sh['l'], cfg['c'], "peaky")
    hw_c, hw_i = (sh['hc'], sh['wc']), (cfg['h'], cfg['w'])
    ref = orc.coarse_match(f0, f1, hw_i, hw_c, hw_c, 0.2, 2, 0.1, return_conf=True)
    out = ops.coarse_match(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), hw_c, hw_c, 8.0, conf_matrix=True)
    _assert_coarse(out, ref)
    got, want = out['conf_matrix'].cpu(), ref['conf_matrix']
    assert (got - want).abs().max().item() <= 1e-5
    big = want > 1e-6
    assert int(big.sum()) >= ref['mconf'].shape[0]
    assert ((got[big] - want[big]).abs() <= 1e-4 * want[big] + 1e-7).all()
    assert float(got[want < 1e-9].max()) < 1e-8


def test_gt_padding_sampler():
    """The older training sampler (network/utils/coarse_matching.py:114-141): predicted matches (sub-sampled when
    there are too many) followed by randomly drawn ground-truth matches with mconf = 0; gt_mask marks them and
    data['mconf'] drops them (:137-141)."""
    f0, f1 = synth.coarse_descriptors(19, 2, 12 * 16, 64, "peaky")
    hw_c, hw_i = (12, 16), (96, 128)
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    spv = dict(spv_b_ids=torch.tensor([0, 1, 1], device=DEV), spv_i_ids=torch.tensor([40, 7, 100], device=DEV),
               spv_j_ids=torch.tensor([41, 8, 5], device=DEV))
    cfg = {'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1, 'train_coarse_percent': 1.0, 'train_pad_num_gt_min': 20}
    ev = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw_c, hw1_c=hw_c)
    modules.CoarseMatching(cfg).eval()(t0, t1, ev)
    m_pred = ev['b_ids'].shape[0]
    data = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw_c, hw1_c=hw_c, **spv)
    modules.CoarseMatching(cfg, conf_matrix=True, gt_pad_sampler=True).train()(t0, t1, data)
    num_train = 2 * 192
    n_gt = max(num_train - m_pred, 20)
    assert data['b_ids'].shape[0] == m_pred + n_gt and m_pred <= num_train - 20
    assert torch.equal(data['i_ids'][:m_pred], ev['i_ids']) and torch.equal(data['j_ids'][:m_pred], ev['j_ids'])
    gtp = torch.stack([data['b_ids'][m_pred:], data['i_ids'][m_pred:], data['j_ids'][m_pred:]], 1).cpu().tolist()
    assert all(tuple(r) in {(0, 40, 41), (1, 7, 8), (1, 100, 5)} for r in gtp)
    assert data['gt_mask'].sum().item() == n_gt and not data['gt_mask'][:m_pred].any()
    assert data['mconf'].shape[0] == m_pred and torch.equal(data['mconf'], ev['mconf'])
    assert data['mkpts0_c'].shape == (m_pred + n_gt, 2)
    assert data['mkpts0_c'][m_pred:].cpu().tolist() == [[(r[1] % 16) * 8.0, (r[1] // 16) * 8.0] for r in gtp]


# ------------------------------------------------------------------ cell-ordered window crops
@pytest.mark.parametrize("w", [5, 7])
def test_cell_ordered_gather_equals_list_ordered_gather(w):
    """Same windows from the cell-ordered kernel (one wave per cell of the image) as from the list-ordered
    one, incl. map borders, unmatched cells, a cell count that is not a multiple of the grid granule, and
    exact ties (two- and three-way, in either image) whose losers come from the tie list."""
    hc, wc = 11, 13
    f0, f1 = synth.coarse_descriptors(71, 2, hc * wc, 64, "peaky")
    # exact ties built from fresh descriptors (the cells' original partners simply stay unmatched)
    va, vb, vc = (4.0 * synth.normal(71, k, (64,)) for k in (9, 10, 11))
    f0[0, 30] = va
    f1[0, 40] = f1[0, 41] = va + 0.4 * synth.normal(71, 12, (64,))            # cell 30 -> cells 40 and 41
    f0[1, 33] = vb
    f1[1, 50] = f1[1, 51] = f1[1, 52] = vb + 0.4 * synth.normal(71, 13, (64,))    # three-way tie in sample 1
    f1[1, 70] = vc
    f0[1, 60] = f0[1, 61] = vc + 0.4 * synth.normal(71, 14, (64,))            # two image-0 cells -> one image-1 cell
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    # (cells without a partner have flat similarity rows: the dense sum kernel's job, FM_MODE_DENSE)
    buf = ops.coarse_match_async(t0, t1, (hc, wc), (hc, wc), 8.0, border_rm=0, dense=True)
    m = buf.read_count()
    o = buf.sliced(m)
    pairs0 = list(zip(o['b_ids'].tolist(), o['i_ids'].tolist()))
    pairs1 = list(zip(o['b_ids'].tolist(), o['j_ids'].tolist()))
    assert m > 150 and len(set(pairs0)) <= m - 3 and len(set(pairs1)) <= m - 1      # the ties are there
    ff0, ff1 = synth.fine_maps(71, 2, 64, hc * 4, wc * 4)
    c0, c1 = buf.cell_maps()
    for ff, ids, cells in ((ff0, o['i_ids'], c0), (ff1, o['j_ids'], c1)):
        t = torch.as_tensor(ff, device=DEV)
        ref = ops.gather_windows(t, o['b_ids'], ids, w, 4, wc)
        got = ops.gather_windows(t, o['b_ids'], ids, w, 4, wc, cells=cells, h_c=hc)
        assert torch.equal(got, ref)
        assert torch.equal(ref.cpu(), orc.crop_windows(ff, o['b_ids'].cpu(), ids.cpu(), w, 4, wc))


# ------------------------------------------------------------------ crop fused with the context merge (row a5)
@pytest.mark.parametrize("gain", [1e-6, 1.0, 300.0, 3e5])
def test_fused_context_merge_follows_the_magnitude_of_the_maps(gain):
    """The fused crop + merge kernel splits the window values into float16 halves at a power-of-two scale that follows
    every window's largest magnitude: fine maps of magnitude 1e-6 .. 3e5 (a fixed 2^8 scale returned inf beyond 255.9,
    silently) against the oracle, relative to the magnitude of the output."""
    g = load_golden("merge_cfg1_w7")
    c = case_inputs(g['meta'][:6], "peaky")
    hc, wc = c['hw_c']
    dw, db, mw, mb = (torch.as_tensor(a, device=DEV) for a in synth.merge_weights(c['cfg']['seed'], c['cfg']['c'], 64))
    w_c = mw[:, 64:]
    e_w, e_b = (w_c @ dw).contiguous(), (w_c @ db + mb).contiguous()
    packed = ops.pack_merge_weights(mw)
    ff0 = (c['ff0'] * np.float32(gain)).astype(np.float32)
    ff0[0, :, 40:44, 40:44] *= np.float32(1e-3)               # one cell's window three orders of magnitude smaller
    ref0, _ = orc.fine_preprocess(ff0, ff0, c['f0'], c['f1'], g['b_ids'], g['i_ids'], g['i_ids'], 7, 4, wc, wc,
                                  down_proj=(dw.cpu(), db.cpu()), merge_feat=(mw.cpu(), mb.cpu()))
    ctx = torch.nn.functional.linear(torch.as_tensor(c['f0'], device=DEV), e_w, e_b)
    ids = torch.as_tensor(g['i_ids'].astype(np.int64), device=DEV)
    bids = torch.as_tensor(g['b_ids'].astype(np.int64), device=DEV)
    got = ops.gather_merge_windows(torch.as_tensor(ff0, device=DEV), packed, ctx, bids, ids, 7, 4, hc, wc).cpu()
    assert torch.isfinite(got).all()
    # per window: 2^-20 of the window's own largest output (float32-equivalent product of 64 terms + the context term)
    scale = ref0.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)
    assert ((got - ref0).abs() / scale).max().item() <= 2.0 ** -20


@pytest.mark.parametrize("name,dist", [("merge_cfg1_w7", "peaky"), ("merge_cfg2_w5", "borderline")])
def test_fused_crop_and_context_merge(name, dist):
    """fm_gather_merge_windows (crop + merge_feat(cat[window, down_proj(feat_c)]), fine_preprocess.py:43-60) against
    the reference module's own output (fixture) and the oracle, in list order and in cell order."""
    g = load_golden(name)
    w = int(g['meta'][6])
    c = case_inputs(g['meta'][:6], dist)
    hc, wc = c['hw_c']
    dw, db, mw, mb = (torch.as_tensor(a, device=DEV) for a in synth.merge_weights(c['cfg']['seed'], c['cfg']['c'], 64))
    fc0, fc1 = torch.as_tensor(c['f0'], device=DEV), torch.as_tensor(c['f1'], device=DEV)
    buf = ops.coarse_match_async(fc0, fc1, c['hw_c'], c['hw_c'], 8.0, dense=(dist == "borderline"))
    m = buf.read_count()
    o = buf.sliced(m)
    assert np.array_equal(o['i_ids'].cpu().numpy(), g['i_ids']) and np.array_equal(o['j_ids'].cpu().numpy(), g['j_ids'])
    packed = ops.pack_merge_weights(mw)
    w_c = mw[:, 64:]
    e_w, e_b = (w_c @ dw).contiguous(), (w_c @ db + mb).contiguous()
    ref0, ref1 = orc.fine_preprocess(c['ff0'], c['ff1'], c['f0'], c['f1'], g['b_ids'], g['i_ids'], g['j_ids'], w, 4, wc, wc,
                                     down_proj=(dw.cpu(), db.cpu()), merge_feat=(mw.cpu(), mb.cpu()))
    pos = torch.arange(1, w * w + 1, dtype=torch.float64).view(1, w * w, 1)
    ch = torch.arange(1, 65, dtype=torch.float64).view(1, 1, -1)
    cells = buf.cell_maps()
    for ff, fc, ids, ref, key, cm in ((c['ff0'], fc0, o['i_ids'], ref0, 'merged0', cells[0]),
                                      (c['ff1'], fc1, o['j_ids'], ref1, 'merged1', cells[1])):
        ctx = torch.nn.functional.linear(fc, e_w, e_b)
        t = torch.as_tensor(ff, device=DEV)
        for use_cells in (None, cm):
            got = ops.gather_merge_windows(t, packed, ctx, o['b_ids'], ids, w, 4, hc, wc, cells=use_cells).cpu()
            assert (got - ref).abs().max().item() <= 4e-6
            np.testing.assert_allclose(got[:3].numpy(), g[key + '_head'], rtol=0, atol=2e-5)
            # weighted checksum of all windows against the reference's: 1e-6 of the total weight (elementwise
            # errors of ~1e-6 add up over W*W*64 weighted terms)
            np.testing.assert_allclose((got.double() * pos * ch).sum((1, 2)).numpy(), g[key + '_sum'], rtol=0,
                                       atol=1e-6 * float((pos * ch).sum()))


def test_fine_preprocess_module_fused_equals_two_step():
    """modules.FinePreprocess in eval mode (fused HIP crop+merge) against its own two-step path (HIP crop, then
    the two nn.Linear layers), random weights, W = 7 with a tie-free cfg1 case."""
    g = load_golden("cfg1_peaky")
    inp = case_inputs(g['meta'], "peaky")
    cfg = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 64}, 'fine': {'d_model': 64}}
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}).eval()
    torch.manual_seed(3)
    fp = modules.FinePreprocess(cfg).to(DEV).eval()
    data = {'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i'], 'hw0_c': inp['hw_c'], 'hw1_c': inp['hw_c'],
            'hw0_f': inp['hw_f'], 'hw1_f': inp['hw_f'], 'bs': 1}
    fc0, fc1 = torch.as_tensor(inp['f0'], device=DEV), torch.as_tensor(inp['f1'], device=DEV)
    ff0, ff1 = torch.as_tensor(inp['ff0'], device=DEV), torch.as_tensor(inp['ff1'], device=DEV)
    cm(fc0, fc1, data)
    with torch.no_grad():
        a0, a1 = fp(ff0, ff1, fc0, fc1, data)
        fp.fused_merge = False
        b0, b1 = fp(ff0, ff1, fc0, fc1, data)
        fp.fused_merge = True
        with torch.no_grad():
            fp.merge_feat.bias.add_(1.0)            # an in-place weight update must invalidate the cached constants
        c0, _ = fp(ff0, ff1, fc0, fc1, data)
    scale = max(1.0, b0.abs().max().item())
    assert (a0 - b0).abs().max().item() <= 2e-5 * scale and (a1 - b1).abs().max().item() <= 2e-5 * scale
    assert (c0 - (b0 + 1.0)).abs().max().item() <= 2e-5 * scale


@pytest.mark.parametrize("w", [5, 7])
def test_pair_gather_equals_two_single_gathers(w):
    """fm_gather_windows_pair (both images in one launch, plain and fused with the merge) against the per-image
    entry points, on a rectangular case (L != S, different map sizes) with exact ties."""
    h0, w0, h1, w1 = 9, 12, 11, 10
    f0 = 4.0 * synth.normal(81, 1, (2, h0 * w0, 64))
    perm = synth.permutation(81, 3, h1 * w1)
    f1 = 4.0 * synth.normal(81, 2, (2, h1 * w1, 64))
    k = min(h0 * w0, h1 * w1) - 10
    f1[:, perm[:k]] = f0[:, :k] + 0.4 * synth.normal(81, 4, (2, k, 64))
    f1[0, perm[k]] = f1[0, perm[0]]                                  # tie: cell 0 of image 0 -> two cells of image 1
    t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
    buf = ops.coarse_match_async(t0, t1, (h0, w0), (h1, w1), 8.0, border_rm=0, dense=True)
    m = buf.read_count()
    o = buf.sliced(m)
    assert m > 100
    ff0 = torch.as_tensor(synth.fine_maps(81, 2, 64, h0 * 4, w0 * 4)[0], device=DEV)
    ff1 = torch.as_tensor(synth.fine_maps(82, 2, 64, h1 * 4, w1 * 4)[1], device=DEV)
    cells = buf.cell_maps()
    a0, a1 = ops.gather_windows_pair(ff0, ff1, o['b_ids'], o['i_ids'], o['j_ids'], w, 4, (h0, w0), (h1, w1), cells)
    assert torch.equal(a0, ops.gather_windows(ff0, o['b_ids'], o['i_ids'], w, 4, w0))
    assert torch.equal(a1, ops.gather_windows(ff1, o['b_ids'], o['j_ids'], w, 4, w1))
    packed = ops.pack_merge_weights(torch.as_tensor(synth.merge_weights(81, 64, 64)[2], device=DEV))
    ctx0 = torch.as_tensor(synth.normal(81, 7, (2, h0 * w0, 64)), device=DEV)
    ctx1 = torch.as_tensor(synth.normal(81, 8, (2, h1 * w1, 64)), device=DEV)
    b0, b1 = ops.gather_windows_pair(ff0, ff1, o['b_ids'], o['i_ids'], o['j_ids'], w, 4, (h0, w0), (h1, w1), cells,
                                     packed_w=packed, ctx0=ctx0, ctx1=ctx1)
    assert torch.equal(b0, ops.gather_merge_windows(ff0, packed, ctx0, o['b_ids'], o['i_ids'], w, 4, h0, w0))
    assert torch.equal(b1, ops.gather_merge_windows(ff1, packed, ctx1, o['b_ids'], o['j_ids'], w, 4, h1, w1, cells=cells[1]))


# ------------------------------------------------------------------ the step after the path (8(f) row 4)
def test_epipolar_errors_against_reference_fixture():
    """fm_epipolar_errors vs the fixture the reference's compute_symmetrical_epipolar_errors (utils/metrics.py:60-81)
    produced; the per-pair inlier score against the oracle's distances; drop-in form on a data dict."""
    from featurematching_amd import post
    g = load_golden("epi_small")
    inp = epipolar_inputs()
    t = {k: torch.as_tensor(v, device=DEV) for k, v in inp.items()}
    epi, inl, per = post.epipolar_errors(t['mkpts0_f'], t['mkpts1_f'], t['m_bids'], t['T_0to1'], t['K0'], t['K1'],
                                         inlier_thr=1e-2)
    np.testing.assert_allclose(epi.cpu().numpy(), g['epi_errs'], rtol=2e-4, atol=1e-9)
    ref_in = g['epi_errs'] < 1e-2
    far = np.abs(g['epi_errs'] - 1e-2) > 1e-5
    assert np.array_equal(inl.cpu().numpy()[far], ref_in[far])
    per = per.cpu().numpy()
    assert per[:, 0].tolist() == np.bincount(inp['m_bids'], minlength=3).tolist()
    assert np.abs(per[:, 1] - np.bincount(inp['m_bids'], weights=ref_in, minlength=3)).max() <= (~far).sum()
    data = dict(t)
    post.compute_symmetrical_epipolar_errors(data)
    assert torch.equal(data['epi_errs'], epi)
    e0, i0, p0 = post.epipolar_errors(t['mkpts0_f'][:0], t['mkpts1_f'][:0], t['m_bids'][:0], t['T_0to1'], t['K0'], t['K1'])
    assert e0.shape == (0,) and int(p0.sum()) == 0


# ------------------------------------------------------------------ fine context layers in HIP (8(f) row 1)
@pytest.mark.parametrize("w", [7, 5])
def test_fine_transformer_vs_oracle(w):
    """fm_fine_transformer (one wave per match, 32-token slices in registers, hi/lo-split MFMAs) against the oracle's
    restatement of the reference's LocalFeatureTransformer (pinned by net_tail_small) on seeded windows/weights."""
    ww, m = w * w, 37
    wts = synth.transformer_weights(77, 64, 2)
    x0 = synth.normal(78, 1, (m, ww, 64)).astype(np.float32)
    x1 = synth.normal(78, 2, (m, ww, 64)).astype(np.float32)
    r0, r1 = orc.local_feature_transformer(x0, x1, wts, 8, ['self', 'cross'])
    packed = ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in wts.items()}, DEV)
    g0, g1 = ops.fine_transformer(torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV), packed)
    e0 = (g0.cpu() - r0).abs().max().item()
    e1 = (g1.cpu() - r1).abs().max().item()
    assert e0 <= 2e-5 and e1 <= 2e-5, (e0, e1)
    # the module takes the kernel by itself in eval mode - also under the reference's own inference call, which leaves
    # grad mode on (demo/demo.py:105-108: matcher.eval()(data)) - and its torch ops when a gradient is asked for
    from featurematching_amd.transformer import LocalFeatureTransformer
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV).eval()
    tf.load_state_dict({k: torch.as_tensor(v) for k, v in wts.items()})
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    with torch.no_grad():
        a0, _ = tf(t0, t1)
    assert torch.equal(a0, g0)
    assert torch.is_grad_enabled()
    b0, _ = tf(t0, t1, None, None)           # grad mode on, eval, the reference's four-argument call: still the HIP kernel
    assert torch.equal(b0, g0) and not b0.requires_grad
    c0, _ = tf(t0.clone().requires_grad_(), t1)      # an input that wants a gradient: torch ops
    assert c0.requires_grad and not torch.equal(c0, g0) and (c0.detach() - g0).abs().max().item() <= 2e-5
    d0, _ = tf.train()(t0, t1)               # training mode: torch ops
    assert d0.requires_grad and (d0.detach() - g0).abs().max().item() <= 2e-5
    # padding masks (transformer.py:89-95): the module's torch layers (all-ones masks change nothing)
    e0, _ = tf.eval()(t0, t1, torch.ones(m, ww, dtype=torch.bool, device=DEV), None)
    assert (e0.detach() - g0).abs().max().item() <= 2e-5


@pytest.mark.parametrize("gain,expect_flag,ww", [(1e-3, False, 49), (8.0, False, 49), (120.0, False, 49), (300.0, False, 49),
                                                 (3e5, True, 49), (300.0, False, 25), (3e5, True, 25)])
def test_fine_transformer_follows_the_data_and_reports_what_it_cannot_hold(gain, expect_flag, ww):
    """fm_fine_transformer splits its operands into float16 halves at a power-of-two activation scale: 2^8 at first
    (|activation| < 255.9); a match whose operands leave float16 there is recomputed inside the kernel with 2^4, 2^0,
    2^-4 (k_fine_tf), and only beyond that (|activation| ~ 1e6) does the call SAY so (FM_DEV_RANGE in the status word)
    instead of clamping silently - the module then answers with its float32 layers.  Window values of magnitude
    `gain` x N(0,1): 8 -> |x| up to ~35, projections up to ~60: first attempt; 120 and 300: a smaller scale; 3e5: out."""
    from featurematching_amd.transformer import LocalFeatureTransformer
    m = 21
    wts = synth.transformer_weights(77, 64, 2)
    x0 = (gain * synth.normal(79, 1, (m, ww, 64))).astype(np.float32)
    x1 = (gain * synth.normal(79, 2, (m, ww, 64))).astype(np.float32)
    r0, r1 = orc.local_feature_transformer(x0, x1, wts, 8, ['self', 'cross'])
    tw = {k: torch.as_tensor(v) for k, v in wts.items()}
    packed = ops.pack_fine_transformer(tw, DEV)
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    g0, g1 = ops.fine_transformer(t0, t1, packed, status=status)
    flagged = bool(int(status.item()) & _lib.FM_DEV_RANGE)
    assert flagged == expect_flag, (gain, float(np.abs(x0).max()))
    tol = 2e-5 * max(1.0, float(r0.abs().max()))
    if not flagged:
        assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
        assert (g0.cpu() - r0).abs().max().item() <= tol and (g1.cpu() - r1).abs().max().item() <= tol
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV).eval()
    tf.load_state_dict(tw)
    a0, a1 = tf(t0, t1)                       # the module: HIP kernel inside the range, float32 layers beyond it
    assert tf.range_fallbacks == (1 if expect_flag else 0)
    assert (a0.cpu() - r0).abs().max().item() <= tol and (a1.cpu() - r1).abs().max().item() <= tol


def test_fine_transformer_starts_where_the_previous_call_ended():
    """fm_fine_transformer_start: windows whose activations leave the first scale (2^8) make the kernel repeat its passes
    at 2^4; the call reports the lowering, the module starts the next call there (no lowering reported any more) and the
    outputs of both calls agree with the oracle within the tolerance of a lowered scale; an explicit start below what
    the data needs only costs precision."""
    from featurematching_amd.transformer import LocalFeatureTransformer
    ww, m = 49, 600
    wnp = synth.transformer_weights(5, 64, 2)
    wts = {k: torch.as_tensor(v) for k, v in wnp.items()}
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV).eval()
    tf.load_state_dict(wts)
    x0 = (120.0 * synth.normal(11, 1, (m, ww, 64))).astype(np.float32)     # beyond 255.9: every match lowers its scale
    x1 = (120.0 * synth.normal(11, 2, (m, ww, 64))).astype(np.float32)
    r0, r1 = orc.local_feature_transformer(x0, x1, wnp, 8, ['self', 'cross'])
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    tol = 2e-5 * max(1.0, float(r0.abs().max()))
    a0, a1 = tf(t0, t1)
    first = tf.last_status.tolist()
    assert first[0] == 0 and first[1] in (4, 8, 12) and tf._fine_start == 8 - first[1]
    b0, b1 = tf(t0, t1)
    assert tf.last_status.tolist() == [0, 0]                # started where the first call ended: nothing to lower
    for g in (a0, a1, b0, b1):
        assert torch.isfinite(g).all()
    assert (a0.cpu() - r0).abs().max().item() <= tol and (b0.cpu() - r0).abs().max().item() <= tol
    assert (a1.cpu() - r1).abs().max().item() <= tol and (b1.cpu() - r1).abs().max().item() <= tol
    # the C entry point refuses a scale it does not have
    packed = ops.pack_fine_transformer(wts, DEV)
    with pytest.raises(_lib.FMatchError):
        ops.fine_transformer(t0, t1, packed, start_scale=6)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_fine_transformer_reports_non_finite_windows(bad):
    """fmatch.h: NaN / Inf activations are reported as FM_DEV_RANGE.  NaN never wins the kernel's running maximum, so
    the outputs themselves are checked; the module answers with its float32 layers (NaN there too, as in the reference),
    counts the call, and check_range=False leaves the report in `last_status` without a host sync."""
    from featurematching_amd.transformer import LocalFeatureTransformer
    m, ww = 9, 49
    x0 = synth.normal(83, 1, (m, ww, 64)).astype(np.float32)
    x1 = synth.normal(83, 2, (m, ww, 64)).astype(np.float32)
    x1[4, 17, 5] = bad
    wts = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(77, 64, 2).items()}
    packed = ops.pack_fine_transformer(wts, DEV)
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    g0, g1 = ops.fine_transformer(t0, t1, packed, status=status)
    assert int(status.item()) & _lib.FM_DEV_RANGE
    ok = [k for k in range(m) if k != 4]
    assert torch.isfinite(g0[ok]).all() and torch.isfinite(g1[ok]).all()      # the other matches are untouched
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV).eval()
    tf.load_state_dict(wts)
    a0, _ = tf(t0, t1)
    assert tf.range_fallbacks == 1 and not torch.isfinite(a0[4]).all() and torch.isfinite(a0[ok]).all()
    tf.check_range = False
    tf(t0, t1)
    assert tf.range_fallbacks == 1 and int(tf.last_status[0].item()) & _lib.FM_DEV_RANGE


def test_fine_transformer_weights_beyond_the_scale_are_reported_and_large_sums_are_held():
    """The two other limits of the first attempt's scales: a weight of magnitude >= 16 (fixed weight scale: caught when
    the weights are packed, reported) and per-head sums of elu(k)+1 >= 2047 with activations inside the range - the
    sum's scale follows the activation scale, so the kernel repeats such a match at a smaller scale and holds it."""
    ww, m = 49, 9
    x0 = synth.normal(80, 1, (m, ww, 64)).astype(np.float32)
    x1 = synth.normal(80, 2, (m, ww, 64)).astype(np.float32)
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    for what in ("weight", "sum"):
        wts = synth.transformer_weights(77, 64, 2)
        if what == "weight":
            wts["layers.1.mlp.0.weight"] = wts["layers.1.mlp.0.weight"].copy()
            wts["layers.1.mlp.0.weight"][5, 7] = 17.0                     # one weight beyond the scale
        else:
            # all-positive tokens against an all-ones k projection: k = sum_c x_c ~ 51 for every token (inside the
            # activation range) but sum_s (elu(k)+1) ~ 49 x 52 = 2550 > 2047 for every head feature
            wts["layers.0.k_proj.weight"] = np.ones_like(wts["layers.0.k_proj.weight"])
            t0, t1 = t0.abs(), t1.abs()
        packed = ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in wts.items()}, DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        g0, g1 = ops.fine_transformer(t0, t1, packed, status=status)
        if what == "weight":
            assert int(status.item()) & _lib.FM_DEV_RANGE, what
        else:
            assert int(status.item()) == 0
            r0, r1 = orc.local_feature_transformer(t0.cpu().numpy(), t1.cpu().numpy(), wts, 8, ['self', 'cross'])
            tol = 2e-5 * max(1.0, float(r0.abs().max()))
            assert (g0.cpu() - r0).abs().max().item() <= tol and (g1.cpu() - r1).abs().max().item() <= tol


# ------------------------------------------------------------------ coarse context layers in HIP (8(f) row 1)
def test_coarse_transformer_padding_masks_against_reference_fixture():
    """fm_coarse_transformer_masked: the reference's optional padding masks (transformer.py:78-96, attentions.py:35-40) in
    the HIP context layers - padded query tokens get Q = 0, padded source tokens K = 0 - against the outputs of the
    REFERENCE's LocalFeatureTransformer(d_model 256, ['self', 'cross'] x 2) with masks, every position (the padded ones
    too: their message is zero there and here).  The module hands masked calls of its coarse configuration to the kernels."""
    g = load_golden("tf_masked_coarse")
    seed, n, l, s_, d = [int(v) for v in g['meta']]
    layers = ['self', 'cross', 'self', 'cross']
    tw = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(seed, d, len(layers)).items()}
    x0 = torch.as_tensor((2.0 * synth.normal(seed, 1, (n, l, d))).astype(np.float32), device=DEV)
    x1 = torch.as_tensor((2.0 * synth.normal(seed, 2, (n, s_, d))).astype(np.float32), device=DEV)
    m0, m1 = torch.as_tensor(g['mask0'], device=DEV), torch.as_tensor(g['mask1'], device=DEV)
    packed = ops.pack_coarse_transformer(tw, len(layers), DEV)
    y0, y1 = ops.coarse_transformer(x0, x1, packed, layers, mask0=m0, mask1=m1)
    e0 = np.abs(y0.cpu().numpy() - g['out0']).max()
    e1 = np.abs(y1.cpu().numpy() - g['out1']).max()
    assert e0 <= 5e-5 and e1 <= 5e-5, (e0, e1)
    u0, u1 = ops.coarse_transformer(x0, x1, packed, layers)
    assert (u0 - y0).abs().max().item() > 1e-2                      # the masks matter
    z0, z1 = ops.coarse_transformer(x0, x1, packed, layers, mask1=m1)      # one mask only
    assert (z0 - y0).abs().max().item() > 1e-3 and (z0 - u0).abs().max().item() > 1e-3
    from featurematching_amd.transformer import LocalFeatureTransformer
    tf = LocalFeatureTransformer(dict(d_model=d, nhead=8, layer_names=layers, attention='linear')).to(DEV).eval()
    tf.load_state_dict(tw)
    with torch.no_grad():
        a0, a1 = tf(x0, x1, m0, m1)
        t0, t1 = tf._torch_layers(x0, x1, m0, m1)
    assert torch.equal(a0, y0) and torch.equal(a1, y1)              # the module took the kernels
    assert (t0 - y0).abs().max().item() <= 5e-5 and (t1 - y1).abs().max().item() <= 5e-5


@pytest.mark.parametrize("n,l,s,layers", [(1, 300, 300, ['self', 'cross'] * 4),      # the reference's 8 layers
                                          (2, 77, 130, ['self', 'cross']),           # ragged tiles, L != S, batch
                                          (1, 32, 5, ['cross', 'self', 'self'])])    # one tile; fewer tokens than a tile
def test_coarse_transformer_vs_oracle(n, l, s, layers):
    """fm_coarse_transformer (K/V partials + fused query-side layer on the float32 matrix cores) against the
    oracle's restatement of the reference's LocalFeatureTransformer (pinned by net_tail_small), d_model 256."""
    wts = synth.transformer_weights(91, 256, len(layers))
    x0 = (2.0 * synth.normal(92, 1, (n, l, 256))).astype(np.float32)
    x1 = (2.0 * synth.normal(92, 2, (n, s, 256))).astype(np.float32)
    r0, r1 = orc.local_feature_transformer(x0, x1, wts, 8, layers)
    tw = {k: torch.as_tensor(v) for k, v in wts.items()}
    packed = ops.pack_coarse_transformer(tw, len(layers), DEV)
    t0, t1 = torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV)
    g0, g1 = ops.coarse_transformer(t0, t1, packed, layers)
    e0 = (g0.cpu() - r0).abs().max().item()
    e1 = (g1.cpu() - r1).abs().max().item()
    # float32 products in another summation order than torch-CPU's; |x| reaches ~10 after eight residual layers
    assert e0 <= 5e-5 and e1 <= 5e-5, (e0, e1)
    assert torch.equal(t0.cpu(), torch.as_tensor(x0)) and torch.equal(t1.cpu(), torch.as_tensor(x1))    # inputs untouched
    h0, h1 = ops.coarse_transformer(t0, t1, packed, layers)
    assert torch.equal(g0, h0) and torch.equal(g1, h1)               # deterministic (no float atomics)
    # the module takes the kernels by itself in eval mode (grad mode on or off, as the reference's demo calls it), its
    # torch ops when a gradient is asked for
    from featurematching_amd.transformer import LocalFeatureTransformer
    tf = LocalFeatureTransformer(dict(d_model=256, nhead=8, layer_names=layers, attention='linear')).to(DEV).eval()
    tf.load_state_dict(tw)
    with torch.no_grad():
        a0, a1 = tf(t0, t1)
    assert torch.equal(a0, g0) and torch.equal(a1, g1)
    b0, b1 = tf(t0, t1)                      # grad mode on: still the HIP kernels
    assert torch.equal(b0, g0) and torch.equal(b1, g1)
    c0, c1 = tf(t0.clone().requires_grad_(), t1)     # a gradient is wanted: torch ops
    assert c0.requires_grad
    assert (c0.detach() - g0).abs().max().item() <= 5e-5 and (c1.detach() - g1).abs().max().item() <= 5e-5


def test_context_layers_at_the_bench_s_sizes():
    """The sizes bench.py runs the context layers at: the coarse layers on one 640x480 pair (N = 1, L = S = 4800, the
    reference's 8 layers: k_ctx_kv_sum folds 150 partials per image, 150 tiles per launch) and the fine layers on
    M = 3100 windows of 49 tokens (388 workgroups) - against the oracle, tolerances as at the small sizes."""
    layers = ['self', 'cross'] * 4
    wts = synth.transformer_weights(91, 256, len(layers))
    x0 = (2.0 * synth.normal(95, 1, (1, 4800, 256))).astype(np.float32)
    x1 = (2.0 * synth.normal(95, 2, (1, 4800, 256))).astype(np.float32)
    torch.set_num_threads(16)
    r0, r1 = orc.local_feature_transformer(x0, x1, wts, 8, layers)
    packed = ops.pack_coarse_transformer({k: torch.as_tensor(v) for k, v in wts.items()}, len(layers), DEV)
    g0, g1 = ops.coarse_transformer(torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV), packed, layers)
    e0, e1 = (g0.cpu() - r0).abs().max().item(), (g1.cpu() - r1).abs().max().item()
    assert e0 <= 5e-5 and e1 <= 5e-5, (e0, e1)
    m, ww = 3100, 49
    wf = synth.transformer_weights(77, 64, 2)
    w0 = synth.normal(96, 1, (m, ww, 64)).astype(np.float32)
    w1 = synth.normal(96, 2, (m, ww, 64)).astype(np.float32)
    q0, q1 = orc.local_feature_transformer(w0, w1, wf, 8, ['self', 'cross'])
    pf = ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in wf.items()}, DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    cnt = torch.tensor([m - 3, 0], dtype=torch.int32, device=DEV)         # device-side count: the last workgroup is ragged
    h0, h1 = ops.fine_transformer(torch.as_tensor(w0, device=DEV), torch.as_tensor(w1, device=DEV), pf, count=cnt, status=status)
    assert int(status.item()) == 0
    e0, e1 = (h0[:m - 3].cpu() - q0[:m - 3]).abs().max().item(), (h1[:m - 3].cpu() - q1[:m - 3]).abs().max().item()
    assert e0 <= 2e-5 and e1 <= 2e-5, (e0, e1)


@pytest.mark.parametrize("gain", [1e-3, 300.0])
def test_coarse_transformer_operand_scales_follow_the_data(gain):
    """The split products carry one power-of-two scale per token, taken from the data: token sets far below / above
    unit magnitude (where a fixed float16 scale would flush or overflow) keep float32-level accuracy."""
    layers = ['self', 'cross']
    wts = synth.transformer_weights(93, 256, len(layers))
    x0 = (gain * synth.normal(94, 1, (1, 70, 256))).astype(np.float32)
    x1 = (gain * synth.normal(94, 2, (1, 45, 256))).astype(np.float32)
    x1[0, 7] = 0.0                                                       # an all-zero token (scale falls back to 1)
    r0, r1 = orc.local_feature_transformer(x0, x1, wts, 8, layers)
    packed = ops.pack_coarse_transformer({k: torch.as_tensor(v) for k, v in wts.items()}, len(layers), DEV)
    g0, g1 = ops.coarse_transformer(torch.as_tensor(x0, device=DEV), torch.as_tensor(x1, device=DEV), packed, layers)
    for g, r in ((g0, r0), (g1, r1)):
        assert torch.isfinite(g).all()
        err = (g.cpu() - r).abs().max().item()
        assert err <= 2e-5 * max(1.0, float(r.abs().max())), (err, float(r.abs().max()))
