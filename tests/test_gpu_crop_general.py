"""The window crop (fm_gather_windows*) and its adjoint (fm_gather_windows_backward) on every path the C ABI dispatches:
general Cf / W / stride / pad (the generic kernels, every k_crop_bwd<NCH> instantiation), both layouts, three element
types, the device-side count on every crop entry point, backward rows outside the grid, and the cell-ordered crop
with hand-built cell maps (tie list short, and overflowed).  The yardsticks are index arithmetic
(tests/fine_grad_ref.py, pinned against torch's unfold by tests/test_crop_ref.py); a gather is compared bit for bit."""
import functools

import pytest
import torch

from featurematching_amd import _lib, ops, synth

from fine_grad_ref import CROP_CASES, CROP_MAP, crop_adjoint, crop_ref, crop_unfold, unfold_grid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HF, WF = CROP_MAP
FM_E_UNSUPPORTED = -3
DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# (Cf, W, stride, pad, h_c, w_c): the shared table on unfold's own grid, plus a coarse grid that overhangs the map
# (12 * 4 = 48 > 37 rows, 14 * 4 = 56 > 45 columns: windows partly and wholly in the padding)
CASES = [(cf, w, s, p, *unfold_grid(HF, WF, w, s, p)) for cf, w, s, p in CROP_CASES] + [(64, 7, 4, 2, 12, 14)]
CASE_IDS = [f"Cf{cf}-W{w}-s{s}-p{p}" for cf, w, s, p in CROP_CASES] + ["Cf64-W7-s4-p2-overhang"]
by_case = pytest.mark.parametrize("case", CASES, ids=CASE_IDS)


def _case(cf, w, s, p):
    return CASES[CROP_CASES.index((cf, w, s, p))]


def _ids(seed, h_c, w_c, m=None):
    """(b_ids, ids) int64: random cells of both samples, the four corners and edge cells (windows reaching into the
    padding), one cell repeated 1, 2 and 300 times, in shuffled list order (the recipe of test_gpu_fine_grad._ids).
    By default a quarter of the cells is drawn (at most 400 draws), so that some pixels stay unread"""
    g = torch.Generator().manual_seed(seed)
    cells = h_c * w_c
    m = min(400, max(8, N * cells // 4)) if m is None else m
    b = torch.randint(N, (m,), generator=g)
    i = torch.randint(cells, (m,), generator=g)
    border = torch.tensor([0, w_c - 1, (h_c - 1) * w_c, cells - 1, w_c // 2, (h_c // 2) * w_c, (h_c // 2) * w_c + w_c - 1])
    rep = [torch.full((k,), c % cells) for k, c in ((1, w_c + 3), (2, 2 * w_c + 5), (300, 3 * w_c + 7))]
    ii = torch.cat([i, border, *rep])
    bb = torch.cat([b, torch.randint(N, (len(border),), generator=g), *[torch.full_like(r, N - 1) for r in rep]])
    p = torch.randperm(len(ii), generator=g)
    return bb[p].contiguous(), ii[p].contiguous()


def _map(seed, cf, dtype=torch.float32):
    return torch.randn(N, cf, HF, WF, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _store(feat, layout):
    """the device buffer of a logical [N, Cf, Hf, Wf] map in `layout` (1: an explicit [N, Hf, Wf, Cf] array)"""
    t = feat.to(DEV)
    return t.contiguous() if layout == 0 else t.permute(0, 2, 3, 1).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _count(k):
    return torch.tensor([k, 0], dtype=torch.int32, device=DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _stream():
    return ops._stream(torch.device(DEV))


def _crop(store, layout, cf, b, i, w, stride, pad, w_c, count=None, out=None):
    """(status, out): fm_gather_windows (float32) / fm_gather_windows_dtype straight through ctypes, `out` pre-filled
    with NaN unless given"""
    lib = _lib.load()
    m = b.shape[0]
    out = _nan(m, w * w, cf) if out is None else out
    tail = (N, cf, HF, WF, layout, w, stride, pad, w_c, ops._ptr(b), ops._ptr(i), ops._ptr(count), m, ops._ptr(out),
            _stream())
    if store.dtype == torch.float32:
        st = lib.fm_gather_windows(ops._ptr(store), *tail)
    else:
        st = lib.fm_gather_windows_dtype(ops._ptr(store), ops._DTYPES[store.dtype], *tail)
    torch.cuda.synchronize()
    return st, out


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("layout", [0, 1])
@by_case
def test_forward_equals_index_arithmetic(case, layout):
    cf, w, stride, pad, h_c, w_c = case
    b, i = _ids(11, h_c, w_c)
    bd, idev = b.to(DEV), i.to(DEV)
    for dtype in DTYPES:
        feat = _map(100 + cf + w, cf, dtype)
        store = _store(feat, layout)
        before = store.clone()
        st, out = _crop(store, layout, cf, bd, idev, w, stride, pad, w_c)
        if layout == 1 and cf % 4:
            assert st == FM_E_UNSUPPORTED and torch.isnan(out).all()
            continue
        assert st == 0, f"{dtype}: status {st}"
        ref = crop_ref(feat.float(), b, i, w, stride, pad, w_c)
        assert _same_bits(out, ref), f"{dtype}: {(out.cpu() != ref).sum().item()} elements differ"
        assert torch.equal(store, before), "the map was written"
        # the same through ops.gather_windows, which reads the layout off the tensor
        t = feat.to(DEV)
        if layout == 1:
            t = t.contiguous(memory_format=torch.channels_last)
        assert _same_bits(ops.gather_windows(t, bd, idev, w, stride, w_c, pad=pad), ref)


# ------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def _backward_case(case):
    """(b, i, d_win, float64 adjoint, reads, e32): e32 = the error of torch's float32 autograd through unfold against
    the float64 adjoint, relative to max |adjoint| - computed on the CPU, never from the HIP result"""
    cf, w, stride, pad, h_c, w_c = case
    b, i = _ids(7, h_c, w_c)
    d_win = torch.randn(b.shape[0], w * w, cf, generator=torch.Generator().manual_seed(1))
    ref, reads = crop_adjoint(d_win, b, i, (N, cf, HF, WF), w, stride, w_c, pad)
    leaf = torch.zeros(N, cf, HF, WF, requires_grad=True)
    crop_unfold(leaf, b, i, w, stride, pad, h_c, w_c).backward(d_win)
    scale = ref.abs().max().item()
    assert scale > 0
    return b, i, d_win, ref, reads, (leaf.grad.double() - ref).abs().max().item() / scale


def _bar(e32):
    """relative bar of the float32 backward: the project's 1e-6, or twice the error of torch's own float32 sum of the
    same terms where that is larger (both are float32 sums in different orders)"""
    return max(1e-6, 2 * e32)


def _crop_backward(d_win, b, i, cf, layout, w, stride, pad, h_c, w_c, count=None):
    """(status, d_feat as the logical [N, Cf, Hf, Wf] view): fm_gather_windows_backward straight through ctypes into a
    buffer pre-filled with NaN"""
    lib = _lib.load()
    m = b.shape[0]
    buf = _nan(N, cf, HF, WF) if layout == 0 else _nan(N, HF, WF, cf)
    need = int(lib.fm_gather_windows_backward_workspace_bytes(N, h_c, w_c, m))
    ws, wsp = ops._aligned_workspace(need, DEV)
    st = lib.fm_gather_windows_backward(ops._ptr(d_win), ops._ptr(b), ops._ptr(i), ops._ptr(count), m, N, cf, HF, WF,
                                        layout, w, stride, pad, h_c, w_c, wsp, need, ops._ptr(buf), _stream())
    torch.cuda.synchronize()
    return st, (buf if layout == 0 else buf.permute(0, 3, 1, 2))


@pytest.mark.parametrize("layout", [0, 1])
@by_case
def test_backward_against_float64(case, layout):
    cf, w, stride, pad, h_c, w_c = case
    b, i, d_win, ref, reads, e32 = _backward_case(case)
    g, bd, idev = d_win.to(DEV), b.to(DEV), i.to(DEV)
    got = [ops.gather_windows_backward(g, bd, idev, (N, cf, HF, WF), w, stride, w_c, h_c, pad=pad, layout=layout)
           for _ in range(2)]
    torch.cuda.synchronize()
    assert _same_bits(got[0], got[1]), "two calls differ"
    assert got[0].is_contiguous(memory_format=torch.channels_last if layout else torch.contiguous_format)
    # EVERY element is written: the same call into a buffer full of NaN
    st, direct = _crop_backward(g, bd, idev, cf, layout, w, stride, pad, h_c, w_c)
    assert st == 0 and not torch.isnan(direct).any()
    assert _same_bits(direct.contiguous(), got[0].contiguous())
    hip = got[0].double().cpu()
    scale = ref.abs().max().item()
    err = (hip - ref).abs().max().item() / scale
    print(f"crop backward {CASE_IDS[CASES.index(case)]} layout {layout}: rel err hip {err:.2e}, torch f32 {e32:.2e}, "
          f"bar {_bar(e32):.2e}")
    assert err <= _bar(e32)
    unread = (reads == 0).expand_as(hip)
    assert unread.any() and (hip[unread] == 0).all() and not torch.signbit(hip[unread]).any()


@pytest.mark.parametrize("cf,w,stride,pad", [(32, 3, 2, 1), (200, 7, 3, 2)])
def test_autograd_route_at_general_shapes(cf, w, stride, pad):
    case = _case(cf, w, stride, pad)
    h_c, w_c = case[4:]
    b, i, d_win, ref, _, e32 = _backward_case(case)
    bd, idev = b.to(DEV), i.to(DEV)
    scale = ref.abs().max().item()
    for dtype in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            feat = _map(5, cf).to(DEV).to(dtype)
            if cl:
                feat = feat.contiguous(memory_format=torch.channels_last)
            feat.requires_grad_(True)
            win = ops.gather_windows_grad(feat, bd, idev, w, stride, w_c, h_c, pad=pad)
            with torch.no_grad():
                assert _same_bits(win, ops.gather_windows(feat, bd, idev, w, stride, w_c, pad=pad))
            assert _same_bits(win, crop_ref(feat.detach().float(), b, i, w, stride, pad, w_c))
            win.backward(d_win.to(DEV))
            assert feat.grad.dtype == dtype and feat.grad.shape == feat.shape
            assert feat.grad.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            tol = _bar(e32) if dtype == torch.float32 else 1e-2
            assert (feat.grad.double().cpu() - ref).abs().max().item() <= tol * scale


# ------------------------------------------------------------------ the device-side count
def _check_counted(run, m, shapes):
    """run(count or None, outs) fills the [m, ...] outputs (and raises on a status).  With d_count = {k, 0}: rows
    < min(k, m) equal the call without a count bit for bit, rows beyond still hold the NaN they were pre-filled with"""
    full = [_nan(*s) for s in shapes]
    run(None, full)
    torch.cuda.synchronize()
    for t in full:
        assert not torch.isnan(t).any()
    for k in (0, 1, m // 2 + 1, m - 1, m + 1000):
        outs = [_nan(*s) for s in shapes]
        run(_count(k), outs)
        torch.cuda.synchronize()
        kk = min(k, m)
        for o, f in zip(outs, full):
            assert _same_bits(o[:kk], f[:kk]), f"count {k}: counted rows differ"
            assert torch.isnan(o[kk:]).all(), f"count {k}: a row beyond the count was written"


@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("layout", [0, 1])
def test_count_on_the_64_channel_list_kernels(w, layout):
    cf, _, stride, pad, h_c, w_c = _case(64, 7, 4, 2)
    b, i = (t.to(DEV) for t in _ids(3, h_c, w_c))
    store = _store(_map(1, cf), layout)
    m = b.shape[0]

    def run(count, outs):
        assert _crop(store, layout, cf, b, i, w, stride, pad, w_c, count=count, out=outs[0])[0] == 0
    _check_counted(run, m, [(m, w * w, cf)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", [0, 1])
def test_count_on_the_generic_kernels(dtype, layout):
    cf, w, stride, pad, h_c, w_c = _case(32, 3, 2, 1)
    b, i = (t.to(DEV) for t in _ids(3, h_c, w_c))
    store = _store(_map(1, cf, dtype), layout)
    m = b.shape[0]

    def run(count, outs):
        assert _crop(store, layout, cf, b, i, w, stride, pad, w_c, count=count, out=outs[0])[0] == 0
    _check_counted(run, m, [(m, w * w, cf)])


def _cell_maps(b, i, cells, pitch, seed=0):
    """(cell_to_match int32 [N * pitch], ties int32 [1024]) as the coarse stage leaves them (coarse_select.hip): the
    largest match index + 1 of every cell (0 = unmatched); every other match of a cell is a tie loser: ties[0] counts
    ALL of them, ties[1..1023] lists the first 1023 in arrival order (any order: shuffled here), the rest stays zero"""
    m = b.shape[0]
    key = b * pitch + i
    cell = torch.zeros(N * pitch, dtype=torch.int64).scatter_reduce(0, key, torch.arange(1, m + 1), "amax")
    losers = torch.nonzero(cell[key] != torch.arange(1, m + 1)).flatten()
    losers = losers[torch.randperm(len(losers), generator=torch.Generator().manual_seed(seed))]
    ties = torch.zeros(1024, dtype=torch.int32)
    ties[0] = len(losers)
    ties[1:1 + min(1023, len(losers))] = losers[:1023].to(torch.int32)
    return cell.to(torch.int32).to(DEV), ties.to(DEV)


def _cells_call(feat, w, stride, pad, h_c, w_c, cell, pitch, ties, b, i, count, out):
    st = _lib.load().fm_gather_windows_cells(ops._ptr(feat), N, 64, HF, WF, w, stride, pad, h_c, w_c, ops._ptr(cell), pitch,
                                             ops._ptr(ties), ops._ptr(b), ops._ptr(i), ops._ptr(count), b.shape[0],
                                             ops._ptr(out), _stream())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("w", [5, 7])
@pytest.mark.parametrize("repeat", [1, 200, 1500], ids=["no_ties", "ties_listed", "tie_list_overflowed"])
def test_cell_ordered_crop_with_hand_built_maps(w, repeat):
    """fm_gather_windows_cells with the cell map and the tie list built here as the coarse stage would: no ties, some
    hundred tie losers (listed), and 2 x 1499 losers of one cell per sample (more than the 1023 the list holds: every
    wave scans a slice of the match list).  Equal to the list-ordered crop and to the yardstick, with and without a
    count"""
    cf, _, stride, pad, h_c, w_c = _case(64, 7, 4, 2)
    cells, pitch = h_c * w_c, h_c * w_c + 5
    g = torch.Generator().manual_seed(repeat)
    if repeat == 1:             # distinct cells only
        key = torch.randperm(N * cells, generator=g)[:N * cells * 2 // 3]
        b, i = key // cells, key % cells
    else:
        b, i = _ids(repeat, h_c, w_c, m=60)
        extra = [(torch.full((repeat,), s), torch.full((repeat,), (4 + s) * w_c + 2 + 3 * s)) for s in range(N)]
        b, i = torch.cat([b] + [e[0] for e in extra]), torch.cat([i] + [e[1] for e in extra])
        p = torch.randperm(b.shape[0], generator=g)
        b, i = b[p].contiguous(), i[p].contiguous()
    cell, ties = _cell_maps(b, i, cells, pitch)
    nties = int(ties[0].item())
    assert {1: nties == 0, 200: 0 < nties <= 1023, 1500: nties > 1023}[repeat]
    feat = _map(2, cf)
    store, bd, idev = feat.to(DEV), b.to(DEV), i.to(DEV)
    m = b.shape[0]
    ref = crop_ref(feat, b, i, w, stride, pad, w_c)
    out = _nan(m, w * w, cf)
    assert _cells_call(store, w, stride, pad, h_c, w_c, cell, pitch, ties, bd, idev, None, out) == 0
    assert _same_bits(out, ref)
    st, listed = _crop(store, 0, cf, bd, idev, w, stride, pad, w_c)
    assert st == 0 and _same_bits(out, listed)

    def run(count, outs):
        assert _cells_call(store, w, stride, pad, h_c, w_c, cell, pitch, ties, bd, idev, count, outs[0]) == 0
    _check_counted(run, m, [(m, w * w, cf)])
    # ops.gather_windows(cells=...) takes the same route
    assert _same_bits(ops.gather_windows(store, bd, idev, w, stride, w_c, pad=pad, h_c=h_c,
                                         cells=(cell.data_ptr(), pitch, ties.data_ptr())), ref)


@pytest.fixture(scope="module")
def coarse():
    """a rectangular coarse case (L != S, different map sizes) with an exact tie, its matches and cell maps (the setup
    of test_gpu_parity.test_pair_gather_equals_two_single_gathers)"""
    h0, w0, h1, w1 = 9, 12, 11, 10
    f0 = 4.0 * synth.normal(81, 1, (2, h0 * w0, 64))
    perm = synth.permutation(81, 3, h1 * w1)
    f1 = 4.0 * synth.normal(81, 2, (2, h1 * w1, 64))
    k = min(h0 * w0, h1 * w1) - 10
    f1[:, perm[:k]] = f0[:, :k] + 0.4 * synth.normal(81, 4, (2, k, 64))
    f1[0, perm[k]] = f1[0, perm[0]]                                  # tie: cell 0 of image 0 -> two cells of image 1
    buf = ops.coarse_match_async(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), (h0, w0), (h1, w1), 8.0,
                                 border_rm=0, dense=True)
    m = buf.read_count()
    assert m > 100
    ff0 = torch.as_tensor(synth.fine_maps(81, 2, 64, h0 * 4, w0 * 4)[0], device=DEV)
    ff1 = torch.as_tensor(synth.fine_maps(82, 2, 64, h1 * 4, w1 * 4)[1], device=DEV)
    packed = ops.pack_merge_weights(torch.as_tensor(synth.merge_weights(81, 64, 64)[2], device=DEV))
    ctx0 = torch.as_tensor(synth.normal(81, 7, (2, h0 * w0, 64)), device=DEV)
    ctx1 = torch.as_tensor(synth.normal(81, 8, (2, h1 * w1, 64)), device=DEV)
    return dict(buf=buf, m=m, o=buf.sliced(m), cells=buf.cell_maps(), hw0=(h0, w0), hw1=(h1, w1), ff0=ff0, ff1=ff1,
                packed=packed, ctx0=ctx0, ctx1=ctx1)


@pytest.mark.parametrize("w", [5, 7])
def test_count_on_the_cell_ordered_and_merging_crops(coarse, w):
    c, o, m = coarse, coarse["o"], coarse["m"]
    (h0, w0), (h1, w1) = c["hw0"], c["hw1"]
    shape = (m, w * w, 64)
    pair = (c["ff0"], c["ff1"], o["b_ids"], o["i_ids"], o["j_ids"], w, 4, c["hw0"], c["hw1"], c["cells"])
    merge1 = (c["ff1"], c["packed"], c["ctx1"], o["b_ids"], o["j_ids"], w, 4, h1, w1)
    # image 1 (its list order is scattered over the map; it holds the tie): plain cell order, merge in list and in
    # cell order
    _check_counted(lambda cnt, outs: ops.gather_windows(c["ff1"], o["b_ids"], o["j_ids"], w, 4, w1, count=cnt, out=outs[0],
                                                        cells=c["cells"][1], h_c=h1), m, [shape])
    _check_counted(lambda cnt, outs: ops.gather_merge_windows(*merge1, count=cnt, out=outs[0]), m, [shape])
    _check_counted(lambda cnt, outs: ops.gather_merge_windows(*merge1, count=cnt, out=outs[0], cells=c["cells"][1]), m,
                   [shape])
    # both images in one launch, plain and merged
    _check_counted(lambda cnt, outs: ops.gather_windows_pair(*pair, count=cnt, out0=outs[0], out1=outs[1]), m,
                   [shape, shape])
    _check_counted(lambda cnt, outs: ops.gather_windows_pair(*pair, count=cnt, out0=outs[0], out1=outs[1],
                                                             packed_w=c["packed"], ctx0=c["ctx0"], ctx1=c["ctx1"]), m,
                   [shape, shape])
    # and without a count the plain crops are the yardstick's
    a0, a1 = ops.gather_windows_pair(*pair)
    for got, ff, ids, wc in ((a0, c["ff0"], o["i_ids"], w0), (a1, c["ff1"], o["j_ids"], w1)):
        assert _same_bits(got, crop_ref(ff, o["b_ids"], ids, w, 4, 2, wc))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("cf,w,stride,pad", [(64, 7, 4, 2), (20, 9, 8, 4), (200, 7, 3, 2)])
def test_backward_count_and_rows_outside_the_grid(cf, w, stride, pad, layout):
    case = _case(cf, w, stride, pad)
    h_c, w_c = case[4:]
    b, i, d_win, ref, _, _ = _backward_case(case)
    g, bd, idev = d_win.to(DEV), b.to(DEV), i.to(DEV)
    m = b.shape[0]
    args = (cf, layout, w, stride, pad, h_c, w_c)
    st, full = _crop_backward(g, bd, idev, *args)
    assert st == 0
    # a count: the first k rows alone, bit for bit; 0 -> all zero; beyond m_max -> clamped
    for k in (m // 2 + 1, 1, m - 1):
        st, got = _crop_backward(g, bd, idev, *args, count=_count(k))
        st2, alone = _crop_backward(g[:k].contiguous(), bd[:k].contiguous(), idev[:k].contiguous(), *args)
        assert st == 0 and st2 == 0 and _same_bits(got.contiguous(), alone.contiguous()), f"count {k}"
        assert not _same_bits(got.contiguous(), full.contiguous())
    st, got = _crop_backward(g, bd, idev, *args, count=_count(0))
    assert st == 0 and (got == 0).all() and not torch.signbit(got).any()
    st, got = _crop_backward(g, bd, idev, *args, count=_count(m + 1000))
    assert st == 0 and _same_bits(got.contiguous(), full.contiguous())
    k = m // 2 + 1
    by_ops = ops.gather_windows_backward(g, bd, idev, (N, cf, HF, WF), w, stride, w_c, h_c, pad=pad, layout=layout,
                                         count=_count(k))
    st, alone = _crop_backward(g[:k].contiguous(), bd[:k].contiguous(), idev[:k].contiguous(), *args)
    assert st == 0 and _same_bits(by_ops.contiguous(), alone.contiguous())
    # rows whose (b, id) is outside [0, N) x [0, h_c * w_c) are skipped before any read: the result is the list's
    # without them
    cells = h_c * w_c
    bad = [(-1, 3), (N, 3), (0, -1), (1, cells), (N + 7, cells + 9), (-2 ** 40, 1), (0, 2 ** 40), (2 ** 31, 0),
           (0, 2 ** 32 + 1)]
    gen = torch.Generator().manual_seed(8)
    pos = torch.sort(torch.randperm(m, generator=gen)[:len(bad)]).values.tolist()
    bb, ii, at = b.tolist(), i.tolist(), 0
    mixed_b, mixed_i, rows = [], [], []
    for j in range(m):
        if at < len(pos) and pos[at] == j:
            mixed_b.append(bad[at][0])
            mixed_i.append(bad[at][1])
            rows.append(torch.randn(1, w * w, cf, generator=gen))
            at += 1
        mixed_b.append(bb[j])
        mixed_i.append(ii[j])
        rows.append(d_win[j:j + 1])
    mb, mi = torch.tensor(mixed_b, dtype=torch.int64, device=DEV), torch.tensor(mixed_i, dtype=torch.int64, device=DEV)
    assert mb.shape[0] == m + len(bad)
    st, got = _crop_backward(torch.cat(rows).to(DEV), mb, mi, *args)
    assert st == 0 and _same_bits(got.contiguous(), full.contiguous())


# ------------------------------------------------------------------ shapes outside the cell-ordered path
@pytest.mark.parametrize("cf,w,stride,pad", [(32, 3, 2, 1), (64, 5, 2, 2), (64, 15, 4, 7)])
def test_gather_windows_with_cells_falls_through_to_the_list_kernels(cf, w, stride, pad):
    """ops.gather_windows(cells=...) at Cf != 64 or W outside {5, 7} runs the list kernel (the cell-ordered entry
    points answer FM_E_UNSUPPORTED there, tests/test_abi.py); at Cf = 64, W = 5 it takes the cell-ordered one"""
    h_c, w_c = _case(cf, w, stride, pad)[4:]
    b, i = _ids(13, h_c, w_c, m=50)
    cells, pitch = h_c * w_c, h_c * w_c
    cell, ties = _cell_maps(b, i, cells, pitch)
    feat = _map(3, cf)
    got = ops.gather_windows(feat.to(DEV), b.to(DEV), i.to(DEV), w, stride, w_c, pad=pad, h_c=h_c,
                             cells=(cell.data_ptr(), pitch, ties.data_ptr()))
    assert _same_bits(got, crop_ref(feat, b, i, w, stride, pad, w_c))
    if cf != 64 or w not in (5, 7):
        out = _nan(b.shape[0], w * w, cf)
        store, bd, idev = feat.to(DEV), b.to(DEV), i.to(DEV)
        st = _lib.load().fm_gather_windows_cells(ops._ptr(store), N, cf, HF, WF, w, stride, pad, h_c, w_c, ops._ptr(cell),
                                                 pitch, ops._ptr(ties), ops._ptr(bd), ops._ptr(idev), None, b.shape[0],
                                                 ops._ptr(out), _stream())
        torch.cuda.synchronize()
        assert st == FM_E_UNSUPPORTED and torch.isnan(out).all()
