"""The coarse stage below its padded channel counts (64 / 128 / 256), on tiny and lopsided grids and at the edges of its
arguments, against the float64 yardstick of tests/coarse_ref.py (pinned on the CPU by tests/test_coarse_ref.py).

Every call goes through ctypes into a workspace filled with 0xFF bytes and into outputs filled with -1 / NaN: the library
keeps no state and asks nothing of the workspace's contents (include/fmatch.h), so a padded lane that was never zeroed
or an output row that was never written shows up as a failure instead of as luck.

Match lists.  Every case is seeded so that its undecided set is empty (coarse_ref.yardstick), so the id lists must EQUAL
the yardstick's, in order; keypoints bit for bit; rows at or beyond M untouched.

Values (conf, the log-denominators).  With e32 = the float32 reference's own largest error against float64 on the case:
    conf:            |got - conf64| <= min(4 e32_conf + 4 ulp(conf64), 1e-5)        (1e-5: BASELINE.md section 4)
    log-denominator: |ln(sum) - nm ln 2 - lse64| <= 4 e32_lse + 4 ulp(largest |sim| of the row / column)
(+ 2^-126 for conf: the kernels' exponentials flush float32 subnormals, the CPU reference keeps them.  e32 is computed
on the host that runs the test: its float32 BLAS sums in an order that depends on the thread count, so e32 - and the
bar with it - moves by tens of percent between hosts.)  Where the
measurements do not support the first form the case keeps the 1e-5 ceiling alone: CEILING_ONLY below names them,
profiles/coarse_edges_accuracy.txt is condensed from the lines this file prints before it asserts (`pytest -s`: ACC = a
comparison, ANS = an explicit mode that answered with a data-dependent status).

Statuses.  fm_coarse_match_auto must serve every case, and so must the first call of every explicit mode - except on the
(case, route, variant) triples expected_answer() pins, where the data is not what the mode is made for and
include/fmatch.h documents another answer.  There the first call must return exactly that status and the mode the header
names must then serve the call:
  FM_E_DENSE       mode 0 / FM_MODE_EXACT_STEP, plain.  The screening resolves at most 24 significant entries per
                   32 x 32 unit of the matrix (kMaxExact, coarse_screen.hip) and cand_slots per row / column:
                   'peaky' at C = 4 and 12 (too few channels for peaks); the C = 256 grids 1x1 | 5x7, 5x7 | 1x1 (35
                   significant entries in one row / column), 1x40 | 40x1 (40 matches, ~26 of them in the first unit),
                   5x7 | 16x20 and 16x20 | 3x3 (every partner-less row / column owns a significant entry: its maximum);
                   the 6x7 | 9x5 'peaky' cases (42 matches and three partner-less columns in two units).  2x2 | 3x3 and
                   1x1 | 1x1 stay below both limits and must be served;
  FM_E_CANDIDATES  FM_MODE_DENSE without FM_MODE_EXACT_SCREENING when every row's statistics are wanted (FM_MODE_STATS, a
                   conf_matrix) of 'mixed' data: its textureless rows hold ~99 equal candidates.
The set is a property of the seeded data (the same on every run).  Mode 0, FM_MODE_EXACT_STEP and the flat hint must
serve 'peaky' at C = 36 .. 252 (9x11 cells: ~10 matches per unit) at the first call.  The training
entry points keep the bars they have elsewhere: 2e-4 max|ref| for gradients (test_gpu_parity.py), 4 e_ref + FLOOR |loss|
for the loss values (test_gpu_coarse_loss.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from featurematching_amd import _lib
from helpers import compare_match_sets

import coarse_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CEILING = 1e-5
GUARD = 2e-5
LOSS_FLOOR = 2 * 1.6e-7           # tests/test_gpu_coarse_loss.py
FTZ = 2.0 ** -126                 # the exponentials flush float32 subnormals (v_exp_f32): a conf below the smallest normal is 0
M0, EXACT, DENSE, STEP, STATS, FLAT = 0, _lib.FM_MODE_EXACT_SCREENING, _lib.FM_MODE_DENSE, _lib.FM_MODE_EXACT_STEP, \
    _lib.FM_MODE_STATS, _lib.FM_MODE_FLAT
# Conf values held to the 1e-5 ceiling alone, (what, case key): the full conf_matrix of the two cases whose measurement
# exceeds 4 e32 + 4 ulp - 'mixed' float32 at C = 100 (1.45e-6 against 1.04e-6, ratio 1.40) and at C = 68 (6.8e-7 against
# 6.2e-7, ratio 1.10).  Entries off the lists of significant entries come from the dense sweep's hi/lo-split float16
# products (22 significant bits against float32's 24, include/fmatch.h).  Every other case is held to the tighter bar;
# the next largest conf_matrix ratio is 0.66 (C = 36 'mixed' float32: profiles/coarse_edges_accuracy.txt).
CEILING_ONLY = {("conf_matrix", ("channel", 100, "mixed", "float32")), ("conf_matrix", ("channel", 68, "mixed", "float32"))}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(nbytes):
    """(tensor, 256-byte aligned base address) of nbytes bytes, every byte 0xFF"""
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def _dev(cs):
    dt = cr.DTYPES[cs.get('dtype', 'float32')]
    return (torch.as_tensor(cs['f0']).to(dt).to(DEV).contiguous(), torch.as_tensor(cs['f1']).to(dt).to(DEV).contiguous(),
            {torch.float32: _lib.FM_F32, torch.float16: _lib.FM_F16, torch.bfloat16: _lib.FM_BF16}[dt])


def _call(cs, mode=0, auto=False, conf=False, slots=None, cap=None, hint=0):
    """One coarse call: fm_coarse_match_dtype + fm_read_count_info, or fm_coarse_match_auto.  Returns a dict: st (the
    status of the call or of the count), m, info, hint, slots (what the serving attempt ran with), the capacity-sized
    outputs as numpy arrays, conf (numpy or None) and ws / base (the workspace, alive)."""
    lib = _lib.load()
    t0, t1, dt = _dev(cs)
    n, l, c = t0.shape
    s = t1.shape[1]
    thr, border, temp = cs.get('thr', 0.2), cs.get('border', 2), cs.get('temp', 0.1)
    if slots is None:      # flat data and conf_matrix requests: >= 16 (include/fmatch.h, fm_coarse_match)
        slots = lib.fm_default_cand_slots(thr)
        if conf or (mode & (DENSE | FLAT | EXACT | STATS)):
            slots = max(slots, 16)
    nb = C.c_size_t(0)
    if auto:
        assert lib.fm_coarse_workspace_bytes_auto(n, l, s, c, 0, C.byref(nb)) == 0
    else:
        assert lib.fm_coarse_workspace_bytes_mode(n, l, s, c, slots, mode, int(conf), C.byref(nb)) == 0
    ws, base = _workspace(nb.value)
    cap = n * min(l, s) + 8 if cap is None else cap
    i64 = lambda: torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    f32 = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float32, device=DEV)
    o = dict(b_ids=i64(), i_ids=i64(), j_ids=i64(), mkpts0_c=f32(cap, 2), mkpts1_c=f32(cap, 2), mconf=f32(cap))
    cnt = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    cm = f32(n, l, s) if conf else None
    s0 = None if cs.get('scale0') is None else torch.as_tensor(cs['scale0'], device=DEV)
    s1 = None if cs.get('scale1') is None else torch.as_tensor(cs['scale1'], device=DEV)
    outs = [(_ptr(o[k]) if cap else None) for k in ('b_ids', 'i_ids', 'j_ids', 'mkpts0_c', 'mkpts1_c', 'mconf')]
    head = (_ptr(t0), _ptr(t1), dt, n, l, s, c, *cs['hw0'], *cs['hw1'], temp, thr, border, cs['scale_px'], _ptr(s0), _ptr(s1),
            C.c_void_p(base), nb.value)
    m, info, h = C.c_int32(-7), C.c_int32(0), C.c_int32(hint)
    if auto:
        st = lib.fm_coarse_match_auto(*head, 0, mode, *outs, cap, _ptr(cnt), _ptr(cm), C.byref(h), C.byref(m), C.byref(info),
                                      _stream())
        slots = (h.value >> 16) & 0xff
    else:
        st = lib.fm_coarse_match_dtype(*head, slots, mode, *outs, cap, _ptr(cnt), _ptr(cm), _stream())
        if st == 0:
            st = lib.fm_read_count_info(_ptr(cnt), cap, C.byref(m), C.byref(info), _stream())
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res.update(st=st, m=int(m.value), info=int(info.value), hint=int(h.value), slots=slots, cap=cap, ws=ws, base=base,
               conf=None if cm is None else cm.cpu().numpy(), shape=(n, l, s, c), dev=(t0, t1))
    return res


# include/fmatch.h: the two data-dependent answers of an explicit mode and the bit the header tells the caller to add
REMEDY = {_lib.FM_E_DENSE: DENSE, _lib.FM_E_CANDIDATES: DENSE | EXACT}


def expected_answer(key, route, var):
    """The status the FIRST call of an explicit route must return: FM_OK, except on the pinned triples of the module
    docstring (a property of the seeded case, not of a run)."""
    plain_common = var == "plain" and route in ("mode0", "exact_step")
    if key[0] == "channel" and key[2] == "peaky" and key[1] in (4, 12) and plain_common:
        return _lib.FM_E_DENSE
    if key[0] == "channel" and key[2] == "mixed" and route in ("dense", "dense+exact_step") and var in ("stats", "conf"):
        return _lib.FM_E_CANDIDATES
    if key[0] == "grid" and key[1] == 256 and plain_common:              # all but 1x1 | 1x1 (0) and 2x2 | 3x3 (4)
        return _lib.FM_E_DENSE if key[2] in (1, 2, 3, 5, 6) else 0
    if key[0] == "arg" and cr.ARG_CASES[key[1]]['kind'] == "peaky" and plain_common:
        return _lib.FM_E_DENSE                                         # 42 against 45 cells in two 32-column units
    return 0


def _served(tag, cs, mode=0, auto=False, conf=False, cap=None, expect=0):
    """_call; its status must be `expect` (FM_E_CAPACITY aside, which the capacity test asks for).  Where `expect` is one
    of the two documented data-dependent answers, the call the header prescribes follows - once more with the bit it
    names - and that one must serve.  out['first'] = None or what is wrong with the first call's status; out['mode'] =
    the mode that served; the ANS lines record the second calls."""
    out = _call(cs, mode, auto=auto, conf=conf, cap=cap)
    first = None if out['st'] in (expect, _lib.FM_E_CAPACITY if expect == 0 else expect) else \
        f"first call: status {out['st']} (info {out['info']:#x}), expected {expect}"
    if not auto and first is None and expect in REMEDY:
        print(f"ANS {tag}: mode {mode} answered {out['st']} (info {out['info']:#x}): once more with mode | {REMEDY[expect]}")
        mode |= REMEDY[expect]
        out = _call(cs, mode, conf=conf, cap=cap)
    out['mode'], out['first'] = mode, first
    return out


def _list_errors(out, y):
    """status OK; ids equal to the yardstick's in order; keypoints bit-exact; dtypes and count; rows beyond M untouched"""
    if out.get('first'):
        return [out['first']]
    if out['st'] != 0:
        return [f"status {out['st']} (info {out['info']:#x})"]
    m, bad = out['m'], []
    if m != len(y['i_ids']):
        bad.append(f"M {m} != {len(y['i_ids'])}")
    else:
        for k in ('b_ids', 'i_ids', 'j_ids'):
            if out[k].dtype != np.int64 or not np.array_equal(out[k][:m], y[k]):
                bad.append(f"{k} differ")
        for k in ('mkpts0_c', 'mkpts1_c'):
            if out[k].dtype != np.float32 or out[k][:m].tobytes() != y[k].tobytes():
                bad.append(f"{k} not bit-exact")
        if out['mconf'].dtype != np.float32 or not np.all(np.isfinite(out['mconf'][:m])):
            bad.append("mconf not finite")
    m = max(0, min(m, out['cap']))
    if not (np.all(out['b_ids'][m:] == -1) and np.all(out['i_ids'][m:] == -1) and np.all(out['j_ids'][m:] == -1)):
        bad.append("id rows beyond M written")
    if not (np.isnan(out['mkpts0_c'][m:]).all() and np.isnan(out['mkpts1_c'][m:]).all() and np.isnan(out['mconf'][m:]).all()):
        bad.append("float rows beyond M written")
    return bad


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _conf_errors(tag, key, what, got, want, e32):
    """conf values against float64 under the bar of the module docstring; prints the ACC line first"""
    if got.size == 0:
        return []
    err = np.abs(got.astype(np.float64) - want)
    intended = 4 * e32 + 4 * _ulp(want) + FTZ
    bar = np.full_like(err, CEILING) if (what, key) in CEILING_ONLY else np.minimum(intended, CEILING)
    print(f"ACC {tag:58s} {what:11s} n {got.size:6d}  max err {err.max():.3e}  e32 {e32:.3e}  max err/(4 e32 + 4 ulp) "
          f"{(err / intended).max():8.3f}  bar {'1e-5' if (what, key) in CEILING_ONLY else 'min(4 e32 + 4 ulp, 1e-5)'}")
    if not np.all(np.isfinite(got)):
        return [f"{what}: not finite / not written"]
    k = int(np.argmax(err - bar))
    return [] if np.all(err <= bar) else [f"{what}: err {err.flat[k]:.3e} > bar {bar.flat[k]:.3e} (value {want.flat[k]:.6e})"]


def _stats(out):
    """the statistics of fm_coarse_softmax_stats as natural-log denominators (lse_r [N, L], lse_c [N, S]) + raw pointers"""
    lib = _lib.load()
    n, l, s, c = out['shape']
    nr, sr, nc, sc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    qr, qc = C.c_int(), C.c_int()
    assert lib.fm_coarse_softmax_stats(C.c_void_p(out['base']), n, l, s, c, out['slots'], C.byref(nr), C.byref(sr), C.byref(qr),
                                       C.byref(nc), C.byref(sc), C.byref(qc)) == 0
    assert qr.value >= l and qc.value >= s

    def read(p, pitch, k):
        o = p.value - out['ws'].data_ptr()
        return out['ws'][o:o + n * pitch * 4].view(torch.float32).view(n, pitch)[:, :k].cpu().numpy().astype(np.float64)
    lse_r = np.log(read(sr, qr.value, l)) - read(nr, qr.value, l) * np.log(2.0)
    lse_c = np.log(read(sc, qc.value, s)) - read(nc, qc.value, s) * np.log(2.0)
    return lse_r, lse_c, (nr, sr, qr.value, nc, sc, qc.value)


def _stats_errors(tag, out, y):
    lse_r, lse_c, _ = _stats(out)
    bad = []
    for name, got, want, amax in (("lse_rows", lse_r, y['lse_r'].numpy(), y['amax_r'].numpy()),
                                  ("lse_cols", lse_c, y['lse_c'].numpy(), y['amax_c'].numpy())):
        err = np.abs(got - want)
        bar = 4 * y['e32_lse'] + 4 * _ulp(amax)
        print(f"ACC {tag:58s} {name:11s} n {got.size:6d}  max err {np.nanmax(err):.3e}  e32 {y['e32_lse']:.3e}  max err/(4 e32 + 4 ulp) "
              f"{np.nanmax(err / bar):8.3f}  bar 4 e32 + 4 ulp(max|sim|)")
        if not np.all(np.isfinite(got)):
            bad.append(f"{name}: not finite / not written")
        elif not np.all(err <= bar):
            k = int(np.argmax(err - bar))
            bad.append(f"{name}: err {err.flat[k]:.3e} > bar {bar.flat[k]:.3e}")
    return bad


def _conf_at(out, cs, ids, stats):
    """fm_dual_softmax_conf_at at ids [K, 3] (float32 descriptors) into a NaN-filled buffer"""
    n, l, s, c = out['shape']
    t0, t1 = out['dev'][0].float().contiguous(), out['dev'][1].float().contiguous()
    b, i, j = (torch.as_tensor(np.ascontiguousarray(ids[:, k]), device=DEV) for k in range(3))
    got = torch.full((ids.shape[0],), float("nan"), dtype=torch.float32, device=DEV)
    st = _lib.load().fm_dual_softmax_conf_at(_ptr(t0), _ptr(t1), n, l, s, c, cs.get('temp', 0.1), *stats, _ptr(b), _ptr(i), _ptr(j),
                                             ids.shape[0], _ptr(got), _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    return got.cpu().numpy()


def _probe_ids(y, shape, seed, k=200):
    """about 200 random entries plus every matched one"""
    n, l, s, _ = shape
    u = cr.synth.uniform(seed, 5, 3 * k).reshape(3, k)
    rnd = np.stack([(u[0] * n).astype(np.int64), (u[1] * l).astype(np.int64), (u[2] * s).astype(np.int64)], 1)
    return np.concatenate([rnd, np.stack([y['b_ids'], y['i_ids'], y['j_ids']], 1)], 0)


def _value_errors(tag, key, out, cs, y, seed=3):
    """mconf; with statistics: the log-denominators and fm_dual_softmax_conf_at; with a conf_matrix: every entry"""
    bad = _conf_errors(tag, key, "mconf", out['mconf'][:out['m']], y['mconf64'], y['e32_conf'])
    if out['conf'] is not None or (out['mode'] & STATS):
        bad += _stats_errors(tag, out, y)
        ids = _probe_ids(y, out['shape'], seed)
        got = _conf_at(out, cs, ids, _stats(out)[2])
        bad += _conf_errors(tag, key, "conf_at", got, y['conf64'][ids[:, 0], ids[:, 1], ids[:, 2]].numpy(), y['e32_conf'])
    if out['conf'] is not None:
        bad += _conf_errors(tag, key, "conf_matrix", out['conf'], y['conf64'].numpy(), y['e32_conf'])
    return bad


def _run_routes(key, routes, variants=("plain", "stats", "conf")):
    """every (name, mode or 'auto') route, plain, with FM_MODE_STATS and with a conf_matrix request: all failures listed"""
    cs, y = cr.case(key), cr.yard(key)
    failures = []
    for name, mode in routes:
        for var in variants:
            auto = mode == "auto"
            bits = (0 if auto else mode) | (STATS if var == "stats" else 0)
            tag = f"{key} {name}/{var}"
            out = _served(tag, cs, bits, auto=auto, conf=(var == "conf"), expect=0 if auto else expected_answer(key, name, var))
            bad = _list_errors(out, y)
            if not bad:
                bad = _value_errors(tag, key, out, cs, y)
            failures += [f"{tag}: {b}" for b in bad]
    return failures


# ------------------------------------------------------------------------------------------------ a. channel counts
ROUTES = {"peaky": (("mode0", M0), ("flat", FLAT), ("exact_step", STEP), ("auto", "auto")),
          "borderline": (("dense", DENSE), ("flat", FLAT), ("exact_screening", EXACT), ("auto", "auto")),
          "mixed": (("dense", DENSE), ("exact_screening", EXACT), ("dense+exact_step", DENSE | STEP), ("auto", "auto"))}


@pytest.mark.parametrize("dtype", list(cr.DTYPES))
@pytest.mark.parametrize("c", cr.CHANNELS)
def test_partial_channel_counts_on_every_route(c, dtype):
    """C below / between the padded counts, float32 / float16 / bfloat16 descriptors, 9x11 against 9x11 cells, N = 2:
    mode 0, FM_MODE_EXACT_STEP and the flat hint on 'peaky'; FM_MODE_DENSE, FM_MODE_FLAT and FM_MODE_EXACT_SCREENING on
    'borderline'; FM_MODE_DENSE (with and without the exact step) and the exact screening on 'mixed';
    fm_coarse_match_auto from hint 0 on all three - each plain, with FM_MODE_STATS and with a conf_matrix request."""
    failures = []
    for kind in cr.KINDS:
        failures += _run_routes(("channel", c, kind, dtype), ROUTES[kind])
    assert not failures, "\n".join(failures)


def test_batched_screening_at_a_partial_channel_count():
    """60 pairs of 5x7 cells at C = 100, kinds alternating: at least 448 row blocks, the launch size at which the
    screening takes its batched form (k_thresh + k_screen_rows).  The batch against the yardstick, and every sample
    equal to the same sample run alone (same ids, conf within 2e-6: the bar of the C = 128 test of this kind)."""
    key = ("batch",)
    cs, y = cr.case(key), cr.yard(key)
    n, l = cs['f0'].shape[:2]
    assert n * (-(-l // 256) * 256 // 32) >= 448
    out = _served(str(key), cs, 0, auto=True)
    failures = _list_errors(out, y) or _value_errors(str(key), key, out, cs, y)
    assert not failures, failures
    for b in range(n):
        one = dict(cs, f0=cs['f0'][b:b + 1], f1=cs['f1'][b:b + 1])
        alone = _call(one, 0, auto=True)
        sel = out['b_ids'][:out['m']] == b
        assert alone['st'] == 0 and alone['m'] == sel.sum(), b
        assert np.array_equal(alone['i_ids'][:alone['m']], out['i_ids'][:out['m']][sel]), b
        assert np.array_equal(alone['j_ids'][:alone['m']], out['j_ids'][:out['m']][sel]), b
        if alone['m']:
            assert np.abs(alone['mconf'][:alone['m']] - out['mconf'][:out['m']][sel]).max() <= 2e-6, b


@pytest.mark.parametrize("name", cr.KATS_R3)
def test_partial_channel_known_answers_against_the_reference(name):
    """kats_r3.npz (C = 36 with per-sample scales, C = 100 with an exact tie, C = 192), the reference's own outputs:
    identical match sets outside the guard band around thr, mconf within 1e-5, same order, keypoints bit-exact"""
    key = ("kat", "kats_r3", name)
    cs, k = cr.case(key), cr.case(key)['fixture']
    for mode in (DENSE | EXACT, "auto"):
        out = _served(f"{key} {mode}", cs, 0 if mode == "auto" else mode, auto=(mode == "auto"))
        assert out['first'] is None and out['st'] == 0, (mode, out['first'], out['st'])
        got = {f: out[f][:out['m']] for f in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c')}
        only_g, only_r, err = compare_match_sets(got, k)
        assert not [e for e in only_g + only_r if abs(e[1] - 0.2) > GUARD], (mode, only_g, only_r)
        assert err <= CEILING, (mode, err)
        assert not only_g and not only_r          # (the yardstick's undecided set of these inputs is empty)
        assert all(np.array_equal(got[f], k[f]) for f in ('b_ids', 'i_ids', 'j_ids'))
        assert got['mkpts0_c'].tobytes() == k['mkpts0_c'].tobytes() and got['mkpts1_c'].tobytes() == k['mkpts1_c'].tobytes()
        if 'tie' in k:       # both tied entries, the same conf bits
            b, i, j, j2 = [int(v) for v in k['tie']]
            sel = (got['b_ids'] == b) & (got['i_ids'] == i)
            assert sorted(got['j_ids'][sel].tolist()) == sorted([j, j2])
            assert got['mconf'][sel][0].tobytes() == got['mconf'][sel][1].tobytes()


# ---------------------------------------------------------------------------------------- c. small and lopsided grids
@pytest.mark.parametrize("g", range(len(cr.GRIDS)), ids=[f"{a[0]}x{a[1]}_{b[0]}x{b[1]}" for a, b in cr.GRIDS])
@pytest.mark.parametrize("c", [256, 100])
def test_small_and_lopsided_grids(c, g):
    """L or S below the 32-row sample, the 32x32 screening unit and the 256 / 64 padding (down to one cell), very
    lopsided L : S; border_rm = 0; image 1 = noisy permuted copies of image 0.  'peaky' at C = 256 on mode 0,
    'borderline' at C = 100 on FM_MODE_DENSE, both on fm_coarse_match_auto; lists, statistics, conf_at, conf_matrix."""
    routes = (("mode0", M0) if cr.grid_kind(c) == "peaky" else ("dense", DENSE), ("auto", "auto"))
    failures = _run_routes(("grid", c, g), routes)
    assert not failures, "\n".join(failures)


# -------------------------------------------------------------------------------------------------- d. argument edges
@pytest.mark.parametrize("name", [k for k in cr.ARG_CASES if k != "cap"])
def test_argument_edges(name):
    """6x7 against 9x5 cells, C = 100: border_rm 0 .. 3 (at 3 nothing survives: M = 0, status OK; at 2 the two images keep
    different numbers of cells), thr 0.02 (the lowest 64 slots serve) / 0.5 / 0.9, temperature 0.05 / 1.0, non-integer
    per-sample scales with N = 3"""
    kind = cr.ARG_CASES[name]['kind']
    routes = (("mode0", M0) if kind == "peaky" else ("dense+exact", DENSE | EXACT), ("auto", "auto"))
    failures = _run_routes(("arg", name), routes)
    assert not failures, "\n".join(failures)
    if cr.built_empty(("arg", name)):
        assert len(cr.yard(("arg", name))['i_ids']) == 0


@pytest.mark.parametrize("auto", [False, True], ids=["explicit", "auto"])
def test_capacity_is_reported_and_the_second_call_is_served(auto):
    """cap = 0 and cap = M - 1 answer FM_E_CAPACITY with the required M; a call with that capacity is served"""
    key = ("arg", "cap")
    cs, y = cr.case(key), cr.yard(key)
    m = len(y['i_ids'])
    # (mode 0 answers FM_E_DENSE on this pair first, capacity or not - expected_answer();
    # the status word reports the capacity once FM_MODE_DENSE serves)
    expect = 0 if auto else expected_answer(key, "mode0", "plain")
    for cap in (0, m - 1):
        out = _served(f"cap {cap}", cs, 0, auto=auto, cap=cap, expect=expect)
        assert out['first'] is None and out['st'] == _lib.FM_E_CAPACITY and out['m'] == m, (cap, out['first'], out['st'], out['m'])
    out = _served(f"cap {m}", cs, 0, auto=auto, cap=m, expect=expect)
    assert not _list_errors(out, y)


# ------------------------------------------------------------------------- e. training entry points at partial C
def _train_setup(c):
    key = ("train", c)
    cs, y, ref = cr.case(key), cr.yard(key), cr.train_reference(key)
    out = _served(f"train {c}", cs, DENSE | STATS)
    assert not _list_errors(out, y)
    return cs, y, ref, out, _stats(out)[2]


def _grad_errors(tag, got, want):
    bad = []
    for name, g, r in zip(("d_feat0", "d_feat1"), got, want):
        g = g.cpu().numpy()
        scale = np.abs(r).max()
        if not np.all(np.isfinite(g)):
            bad.append(f"{tag} {name}: {np.count_nonzero(~np.isfinite(g))} elements not finite / not written")
            continue
        err = np.abs(g.astype(np.float64) - r).max()
        print(f"ACC {tag:58s} {name:11s} max|ref| {scale:.3e}  err/max|ref| {err / scale:.3e}  bar 2e-4")
        if not (scale > 1e-6 and err <= 2e-4 * scale):
            bad.append(f"{tag} {name}: err {err:.3e} > 2e-4 * {scale:.3e}")
    return bad


def _nan_like(t):
    return torch.full_like(t, float("nan"))


@pytest.mark.parametrize("c", cr.TRAIN_CHANNELS)
def test_dual_softmax_backward_at_partial_channel_counts(c):
    """fm_dual_softmax_conf_at, fm_dual_softmax_backward and _backward_dense at 15x17 against 11x13 cells, N = 2, against
    float64 autograd through coarse_matching_new.py:64-68; d_feat pre-filled with NaN, workspaces with 0xFF"""
    lib = _lib.load()
    cs, y, ref, out, stats = _train_setup(c)
    n, l, s, _ = out['shape']
    t0, t1 = out['dev']
    ids = ref['ids']
    failures = _conf_errors(f"train {c}", ("train", c), "conf_at", _conf_at(out, cs, ids, stats), ref['conf_at'], y['e32_conf'])
    need = int(lib.fm_dual_softmax_backward_workspace_bytes(n, l, s, c))
    b, i, j = (torch.as_tensor(np.ascontiguousarray(ids[:, k]), device=DEV) for k in range(3))
    gc = torch.as_tensor((ref['g_sparse'].astype(np.float64) * ref['conf_at']).astype(np.float32), device=DEV)
    ws, base = _workspace(need)
    d0, d1 = _nan_like(t0), _nan_like(t1)
    st = lib.fm_dual_softmax_backward(_ptr(t0), _ptr(t1), n, l, s, c, 0.1, *stats, _ptr(b), _ptr(i), _ptr(j), _ptr(gc),
                                      ids.shape[0], C.c_void_p(base), need, _ptr(d0), _ptr(d1), _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    failures += _grad_errors(f"train {c} backward", (d0, d1), ref['sparse'])
    G = torch.as_tensor(ref['g_dense'], device=DEV).contiguous()
    ws, base = _workspace(need)
    d0, d1 = _nan_like(t0), _nan_like(t1)
    st = lib.fm_dual_softmax_backward_dense(_ptr(t0), _ptr(t1), n, l, s, c, 0.1, *stats, _ptr(G), C.c_void_p(base), need,
                                            _ptr(d0), _ptr(d1), _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    failures += _grad_errors(f"train {c} backward_dense", (d0, d1), ref['dense'])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["focal", "cross_entropy"])
@pytest.mark.parametrize("c", cr.TRAIN_CHANNELS)
def test_coarse_loss_at_partial_channel_counts(c, kind):
    """fm_coarse_loss_forward / _backward on the same shapes: loss, positive and negative mean within 4 e_ref + FLOOR |x|
    of float64 (the bar of tests/test_gpu_coarse_loss.py), gradients within 2e-4 max|ref|; outputs pre-filled with NaN,
    the workspace with 0xFF"""
    lib = _lib.load()
    cs, y, ref, out, stats = _train_setup(c)
    n, l, s, _ = out['shape']
    t0, t1 = out['dev']
    ids = ref['ids']
    b, i, j = (torch.as_tensor(np.ascontiguousarray(ids[:, k]), device=DEV) for k in range(3))
    need = int(lib.fm_coarse_loss_workspace_bytes(n, l, s, c, ids.shape[0]))
    assert need > 0
    ws, base = _workspace(need)
    loss = torch.full((3,), float("nan"), device=DEV)
    problem = (_ptr(t0), _ptr(t1), n, l, s, c, 0.1, *stats, {"cross_entropy": _lib.FM_LOSS_CROSS_ENTROPY,
               "focal": _lib.FM_LOSS_FOCAL}[kind], 0.25, 2.0, 1.0, 1.0, _ptr(b), _ptr(i), _ptr(j), ids.shape[0], C.c_void_p(base), need)
    st = lib.fm_coarse_loss_forward(*problem, _ptr(loss), _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    failures = []
    r = ref[kind]
    for what, got, want, w32 in zip(("loss", "pos_mean", "neg_mean"), loss.tolist(), r['loss64'], r['loss32']):
        e_ref = abs(w32 - want)
        print(f"ACC train {c} {kind:13s} {what:9s} loss64 {want:.9e}  e_ref/|loss64| {e_ref / abs(want):.3e}  "
              f"e_hip/|loss64| {abs(got - want) / abs(want):.3e}")
        if not abs(got - want) <= 4 * e_ref + LOSS_FLOOR * abs(want):
            failures.append(f"{what}: {got!r} against {want!r} (e_ref {e_ref:.3e})")
    d_loss = torch.ones(1, device=DEV)
    d0, d1 = _nan_like(t0), _nan_like(t1)
    st = lib.fm_coarse_loss_backward(*problem, _ptr(d_loss), _ptr(d0), _ptr(d1), _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    failures += _grad_errors(f"train {c} loss {kind}", (d0, d1), r['grads'])
    assert not failures, "\n".join(failures)
