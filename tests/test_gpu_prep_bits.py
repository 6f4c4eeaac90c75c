"""k_prep_split, bit for bit: everything the descriptor quantisation pass writes against a numpy float32 model of the
documented formulas (csrc/coarse_prep.hip).

  sigma    = kPrepHeadroom * (largest |x| of the kPrepSampleRows rows t * rows / ns of the image) / 127, one per image;
             FM_MODE_EXACT_STEP: (largest |x| of the image) * (1 + 1e-5) / kPrepHeadroom in its place
  code     = clamp(rint(x * (1 / sigma)), +-127); a NaN product (NaN, or Inf * 0) gives -127
  address  = (((row / 32 * KS8 + ks) * 2 + h) * 32 + row % 32) * 16 + k % 16, chunk k / 16 = h * KS8 + ks, KS8 = C / 32
  L1 norm / clipped mass of a row: eight partial sums (partial g takes the 16-channel chunks g and g + 8, elements in
             order), then the partials in g order; all in float32
  block    = {largest L1 norm (+inf: the block holds a NaN, an Inf or |x| >= 32768), largest clipped mass, largest |x|, 0}
  planes   (fm_debug_launch_flat): y = x * 2^k with 127 sigma * 2^k in [2^13, 2^14); hi = f16(y), lo = f16(y - hi) at
             (((row / 32 * KSTEPS + ks) * 2 + h) * 32 + row % 32) * 8 + k % 8, chunk k / 8 = h * KSTEPS + ks, KSTEPS = C / 16
  and the span of per-call counters in front of the int8 planes is cleared.

float32 rows go through fm_debug_launch_prep and fm_debug_launch_flat(which = 0) on a workspace filled with 0xA5;
float16 / bfloat16 rows and FM_MODE_EXACT_STEP through the complete call (the diagnostic launchers take float32 rows and
no mode), whose later kernels only read these regions.  The regions are found through fm_debug_coarse_layout; l1_1 and
the block statistics, which it does not name, follow l1_0 with every region on the next 256-byte boundary.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPES = [(33, 70), (64, 31), (1, 257)]
GRIDS = {33: (3, 11), 70: (7, 10), 64: (8, 8), 31: (1, 31), 1: (1, 1), 257: (1, 257)}
HEADROOM, SAMPLE_ROWS = np.float32(1.5), 32
F32 = np.float32


def _up(x, m):
    return (x + m - 1) // m * m


def _regions(n, l, s, c):
    lib = _lib.load()
    slots = lib.fm_default_cand_slots(0.2)
    lay = (C.c_int64 * 41)()
    assert lib.fm_debug_coarse_layout(n, l, s, c, slots, lay, 41) == 0
    lp, sp, cp = int(lay[4]), int(lay[5]), int(lay[3])
    l1_0 = int(lay[21])
    l1_1 = _up(l1_0 + n * lp * 4, 256)
    bstat0 = _up(l1_1 + n * sp * 4, 256)
    bstat1 = _up(bstat0 + n * lp // 32 * 16, 256)
    reg = {"prep_zero": (int(lay[10]), int(lay[18]) - int(lay[10])), "q0": (int(lay[18]), n * lp * cp),
           "q1": (int(lay[19]), n * sp * cp), "sigimg": (int(lay[20]), n * 8), "l1_0": (l1_0, n * lp * 4),
           "l1_1": (l1_1, n * sp * 4), "bstat0": (bstat0, n * lp // 32 * 16), "bstat1": (bstat1, n * sp // 32 * 16),
           "hi0": (int(lay[14]), n * lp * cp * 2), "lo0": (int(lay[15]), n * lp * cp * 2),
           "hi1": (int(lay[16]), n * sp * cp * 2), "lo1": (int(lay[17]), n * sp * cp * 2)}
    assert lp >= l and sp >= s and lp % 64 == 0 and sp % 64 == 0 and cp == (64 if c <= 64 else 128 if c <= 128 else 256)
    return reg, slots, lp, sp


def _model_image(x, rp, exact_step, planes):
    """x float32 [N, rows, c_in], rp = rows of the padded planes -> the bytes of one image's regions"""
    n, rows, c_in = x.shape
    cp = 64 if c_in <= 64 else 128 if c_in <= 128 else 256
    X = np.zeros((n, rp, cp), F32)
    X[:, :rows, :c_in] = x
    A = np.abs(X)
    sig = np.zeros(n, F32)
    with np.errstate(all="ignore"):
        for b in range(n):
            if exact_step:
                am = np.fmax.reduce(A[b].ravel(), initial=F32(0))
                am = F32(F32(am * (F32(1.0) + F32(1e-5))) / HEADROOM)
            else:
                ns = min(SAMPLE_ROWS, rows)
                am = np.fmax.reduce(A[b, [t * rows // ns for t in range(ns)], :c_in].ravel(), initial=F32(0))
            sig[b] = F32(am * F32(HEADROOM / F32(127.0))) if am < np.inf else F32(1.0)
        inv = np.where(sig > 0, F32(1.0) / np.where(sig > 0, sig, F32(1.0)), F32(0.0)).astype(F32)
        clip_at = (F32(127.0) * sig).astype(F32)
        t = (X * inv[:, None, None]).astype(F32)
        codes = np.where(np.isnan(t), F32(-127.0), np.clip(np.rint(t), -127.0, 127.0)).astype(np.int8)
        # fragment-major addresses
        R = (np.arange(n)[:, None] * rp + np.arange(rp)[None, :])[:, :, None]          # global padded row
        k = np.arange(cp)[None, None, :]
        ks8 = cp // 32
        q16 = k // 16
        addr = (((R // 32 * ks8 + q16 % ks8) * 2 + q16 // ks8) * 32 + R % 32) * 16 + k % 16
        q = np.zeros(n * rp * cp, np.int8)
        q[addr.ravel()] = codes.ravel()
        # L1 norm and clipped mass: eight partials (chunks g, g + 8), then the partials in g order
        term = np.fmax(A - clip_at[:, None, None], F32(0.0)).astype(F32)
        l1, ce = np.zeros((n, rp), F32), np.zeros((n, rp), F32)
        for g in range(8):
            s1, c1 = np.zeros((n, rp), F32), np.zeros((n, rp), F32)
            for ch in (g, g + 8):
                if ch < cp // 16:
                    for e in range(16):
                        s1 = (s1 + A[:, :, ch * 16 + e]).astype(F32)
                        c1 = (c1 + term[:, :, ch * 16 + e]).astype(F32)
            l1, ce = (l1 + s1).astype(F32), (ce + c1).astype(F32)
        nb = n * rp // 32
        Ab, l1b, ceb = A.reshape(nb, 32 * cp), l1.reshape(nb, 32), ce.reshape(nb, 32)
        bstat = np.zeros((nb, 4), F32)
        bad = (~(Ab < F32(32768.0))).any(axis=1)
        bstat[:, 0] = np.where(bad, F32(np.inf), np.fmax.reduce(l1b, axis=1))
        bstat[:, 1] = np.fmax.reduce(ceb, axis=1)
        bstat[:, 2] = np.fmax.reduce(Ab, axis=1, initial=F32(0))
        out = {"q": q, "l1": l1.ravel(), "bstat": bstat.ravel(), "sig": sig}
        if planes:
            sc = np.ones(n, F32)
            for b in range(n):
                if clip_at[b] > 0 and clip_at[b] < np.inf:
                    sc[b] = np.ldexp(F32(1.0), 14 - int(np.frexp(clip_at[b])[1]))
            Y = (X * sc[:, None, None]).astype(F32)
            hi = Y.astype(np.float16)
            lo = (Y - hi.astype(F32)).astype(F32).astype(np.float16)
            kst = cp // 16
            q8 = k // 8
            addr2 = (((R // 32 * kst + q8 % kst) * 2 + q8 // kst) * 32 + R % 32) * 8 + k % 8
            for name, pl in (("hi", hi), ("lo", lo)):
                flat = np.zeros(n * rp * cp, np.float16)
                flat[addr2.ravel()] = pl.ravel()
                out[name] = flat
    return out


def _model(x0, x1, lp, sp, exact_step=False, planes=False):
    m0, m1 = _model_image(x0, lp, exact_step, planes), _model_image(x1, sp, exact_step, planes)
    want = {"q0": m0["q"], "q1": m1["q"], "l1_0": m0["l1"], "l1_1": m1["l1"], "bstat0": m0["bstat"], "bstat1": m1["bstat"],
            "sigimg": np.stack([m0["sig"], m1["sig"]], axis=1).ravel()}
    if planes:
        want.update(hi0=m0["hi"], lo0=m0["lo"], hi1=m1["hi"], lo1=m1["lo"])
    return want


def _compare(ws, off, reg, want, what):
    for name, w in want.items():
        o, nb = reg[name]
        got = ws[off + o: off + o + nb].cpu().numpy()
        assert w.nbytes == nb, (what, name)
        if w.dtype == np.float16:       # (a NaN's payload is not part of the contract: NaN where the model has NaN)
            g16, nan = got.view(np.float16), np.isnan(w)
            assert np.array_equal(np.isnan(g16), nan), (what, name)
            gb, wb = g16.view(np.uint16), w.view(np.uint16)
            assert np.array_equal(gb[~nan], wb[~nan]), (what, name, int((gb[~nan] != wb[~nan]).sum()))
        elif name.startswith("l1"):     # (likewise for the L1 norm of a row that holds a NaN)
            g32, nan = got.view(F32), np.isnan(w)
            assert np.array_equal(np.isnan(g32), nan), (what, name)
            assert np.array_equal(g32.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), (what, name)
        else:
            wb = w.view(np.uint8)
            assert np.array_equal(got, wb), (what, name, int((got != wb).sum()), np.flatnonzero(got != wb)[:8])


def _inputs(seed, n, l, s, c_in):
    r = np.random.default_rng(seed)
    x0 = (4.0 * r.standard_normal((n, l, c_in))).astype(F32)
    x1 = (4.0 * r.standard_normal((n, s, c_in))).astype(F32)
    return x0, x1


def _debug_launches(x0, x1, what):
    """fm_debug_launch_prep and fm_debug_launch_flat(which = 0) on float32 rows against the model"""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    (n, l, c_in), s = x0.shape, x1.shape[1]
    reg, slots, lp, sp = _regions(n, l, s, c_in)
    nbytes = C.c_size_t()
    assert lib.fm_coarse_workspace_bytes(n, l, s, c_in, slots, C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    ptr = C.c_void_p(ws.data_ptr() + off)
    t0, t1 = torch.as_tensor(x0, device=dev), torch.as_tensor(x1, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    model = _model(x0, x1, lp, sp, planes=True)
    for planes in (False, True):
        want = {k: v for k, v in model.items() if planes or k[:2] not in ("hi", "lo")}
        ws.fill_(0xA5)
        f0p, f1p = C.c_void_p(t0.data_ptr()), C.c_void_p(t1.data_ptr())
        if planes:
            rc = lib.fm_debug_launch_flat(ptr, f0p, f1p, n, l, s, c_in, slots, 0.1, 0.2, 0, st)
        else:
            rc = lib.fm_debug_launch_prep(ptr, f0p, f1p, n, l, s, c_in, slots, st)
        assert rc == 0
        torch.cuda.synchronize()
        _compare(ws, off, reg, want, (what, "flat" if planes else "prep"))
        o, nb = reg["prep_zero"]
        assert nb > 0 and int(ws[off + o: off + o + nb].max()) == 0, (what, "per-call counters not cleared")


def _complete_call(x0, x1, dtype, exact_step, what):
    dev = torch.device("cuda:0")
    (n, l, c_in), s = x0.shape, x1.shape[1]
    t0, t1 = torch.as_tensor(x0, device=dev).to(dtype), torch.as_tensor(x1, device=dev).to(dtype)
    buf = ops.coarse_match_async(t0, t1, GRIDS[l], GRIDS[s], 8.0, border_rm=0, exact_step=exact_step)
    torch.cuda.synchronize()
    reg, _, lp, sp = _regions(n, l, s, c_in)
    ws = buf.workspace
    off = (-ws.data_ptr()) % 256
    want = _model(t0.float().cpu().numpy(), t1.float().cpu().numpy(), lp, sp, exact_step=exact_step)
    _compare(ws, off, reg, want, what)


@pytest.mark.parametrize("cdrop", [0, 4])
@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("ls", SHAPES)
def test_prep_bits_float32(ls, n, c, cdrop):
    """(33, 70): tail blocks; (1, 257) and (x, 70): a sample whose padding is a whole block; c - 4: the row-wise loads"""
    l, s = ls
    x0, x1 = _inputs(7 + l + n + c + cdrop, n, l, s, c - cdrop)
    _debug_launches(x0, x1, (ls, n, c - cdrop))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cdrop", [0, 4])
@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("ls", SHAPES)
def test_prep_bits_half(ls, n, c, cdrop, dtype):
    l, s = ls
    x0, x1 = _inputs(11 + l + n + c + cdrop, n, l, s, c - cdrop)
    _complete_call(x0, x1, dtype, False, (ls, n, c - cdrop, dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("c", [64, 124, 256])
@pytest.mark.parametrize("ls", SHAPES)
def test_prep_bits_exact_step(ls, c, dtype):
    """FM_MODE_EXACT_STEP: k_prep_amax + the step from the block maxima; an element 8x beyond the sampled rows' maximum
    then is not clipped"""
    l, s = ls
    x0, x1 = _inputs(13 + l + c, 2, l, s, c)
    x1[1, s - 1, c - 1] = 128.0          # (the last row is not one of the sampled rows when s > 32; exact in bfloat16)
    _complete_call(x0, x1, dtype, True, (ls, c, dtype))


def _unsampled_row(rows):
    ns = min(SAMPLE_ROWS, rows)
    free = sorted(set(range(rows)) - {t * rows // ns for t in range(ns)})
    assert free
    return free[len(free) // 2]


@pytest.mark.parametrize("c", [64, 124, 256])
@pytest.mark.parametrize("ls", [(33, 70), (1, 257)])
def test_prep_bits_outlier(ls, c):
    """one element of 1e5 outside the sampled rows of image 1 (and of image 0 where it has such rows): codes clamp at
    127, the clipped mass of its row and block is > 0"""
    l, s = ls
    x0, x1 = _inputs(17 + l + c, 2, l, s, c)
    x1[1, _unsampled_row(s), 5] = 1e5
    x1[0, _unsampled_row(s), c - 1] = -1e5
    if l > SAMPLE_ROWS:
        x0[0, _unsampled_row(l), 17] = 1e5
    want = _model(x0, x1, _up(l, 64), _up(s, 64))
    assert want["bstat1"].reshape(-1, 4)[:, 1].max() > 0
    _debug_launches(x0, x1, ("outlier", ls, c))


@pytest.mark.parametrize("c", [64, 124, 256])
@pytest.mark.parametrize("ls", [(33, 70), (64, 31)])
def test_prep_bits_bad_values(ls, c):
    """one NaN and one Inf (and one finite value out of range): the +inf marker of their blocks and of no other; NaN and
    Inf in sampled and in unsampled rows"""
    l, s = ls
    x0, x1 = _inputs(19 + l + c, 2, l, s, c)
    x0[0, l - 1, 3] = np.nan             # L = 33: row 32, not sampled; L = 64: sampled (t * 2 hits 62 only: row 63 is not)
    x0[1, 0, c - 2] = np.inf             # row 0 is always sampled: the step falls back to 1
    x1[0, s // 2, 9] = -np.inf
    x1[1, s - 1, 0] = np.nan
    x1[1, 1, 1] = 40000.0
    want = _model(x0, x1, _up(l, 64), _up(s, 64))
    assert np.isinf(want["bstat0"].reshape(-1, 4)[:, 0]).sum() == 2
    _debug_launches(x0, x1, ("bad", ls, c))
