"""The coarse level's training kernels (k_conf_at, k_dsm_uv, k_dsm_bwd in its three modes, the coarse loss's sweep,
k_sweep_combine, k_dsm_entries) through the C ABI with the softmax statistics HANDED IN by the test, against the float64
closed form of tests/dsm_grad_ref.py (pinned on the CPU by tests/test_dsm_grad_ref.py), at the smallest shapes that reach
every tile, split and pitch edge of the sweep (the table: dsm_grad_ref.CASES).

Bar.  With T the per-element sum of the magnitudes of the terms a gradient element is made of (dsm_grad_ref.term_bound):
    e_hip = max |hip - ref64| / T  <=  4 e_ref + FLOOR + 4 delta,         and exactly 0 where T == 0
(|hip - ref64| less dsm_grad_ref.flush_bound, about 1e-36: float32 subnormals are flushed, which is all there is to the
gradients of the unmatched columns of 'peaky' data; e_ref is taken the same way)
e_ref = the same figure of float32 torch autograd through the reference's expression with the same dL/dconf, on the
device; delta = the largest relative error of the handed denominators against a float64 log-sum-exp (computed per case);
4 = this project's allowance for another summation order and recomputed softmaxes (test_gpu_linear_attention.py,
test_gpu_coarse_loss.py, test_gpu_window_merge.py).  FLOOR = twice the largest e_ref over the 'regular' cases of this
file (dsm_grad_ref.REGULAR: every case on 'borderline' or 'soft' data), measured on the MI355X: profiles/dsm_grad_accuracy.txt,
which holds every ACC line this file prints (`pytest -s`).  A bar relative to max|grad| measures the conditioning of the
input on small saturated problems; this one does not care how much the terms cancel.

Canaries.  Every buffer handed over - descriptors, statistics, G, ids, gc, d_loss, the outputs, the workspace - is a slice
of a larger allocation filled with NaN (ids: 0; the workspace and its surroundings: 0xFF bytes).  After each call the
surroundings are unchanged and every output element is finite: a read outside a buffer shows up as a NaN in a result.
No case hands the kernels an id outside its range (test_dsm_grad_ref.py).

fm_dual_softmax_conf_at keeps the bar of test_gpu_coarse_edges.py in the form its statistics have there, 4 e32 +
4 ulp(max|sim|): the handed offsets come from float64 dot products, the kernel's exponent from its own float32 one.
Loss values keep the bar of test_gpu_coarse_loss.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, ops

import dsm_grad_ref as dr
from test_gpu_coarse_edges import FTZ, LOSS_FLOOR, _stream, _ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2 * 5.502e-6      # profiles/dsm_grad_accuracy.txt: the largest e_ref over dsm_grad_ref.REGULAR ('temp0.05 sparse', d_feat1)
PAD = 64                  # elements either side of every buffer
KINDS = {"cross_entropy": _lib.FM_LOSS_CROSS_ENTROPY, "focal": _lib.FM_LOSS_FOCAL}
PAIRS = [(n, m) for n, c in dr.CASES.items() for m in c.modes]


class Guarded:
    """a buffer that is a slice of a larger allocation: PAD elements of `fill` either side"""

    def __init__(self, data=None, shape=None, dtype=torch.float32, fill=float("nan")):
        if data is not None:
            data = torch.as_tensor(np.ascontiguousarray(data))
            shape, dtype = tuple(data.shape), data.dtype
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.raw = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device=DEV)
        self.view = self.raw[PAD:PAD + self.n]
        if data is not None and self.n:
            self.view.copy_(data.reshape(-1))
        assert self.raw.data_ptr() % 256 == 0
        self.address = self.raw.data_ptr() + PAD * self.raw.element_size()        # (an empty slice has no data_ptr)
        self.before = self._surroundings()

    def _surroundings(self):
        b, e = self.raw.view(torch.uint8), self.raw.element_size()
        return torch.cat([b[:PAD * e], b[(PAD + self.n) * e:]]).clone()

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    def intact(self):
        return torch.equal(self._surroundings(), self.before)

    def numpy(self):
        return self.view.cpu().numpy().reshape(self.shape)


class GuardedWorkspace(Guarded):
    """nbytes bytes at a 256-byte aligned address, 0xFF inside and for 256 bytes either side"""

    def __init__(self, nbytes):
        self.n, self.shape = nbytes, (nbytes,)
        self.raw = torch.full((nbytes + 512,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.address = self.raw.data_ptr() + 256
        self.before = self._surroundings()

    def _surroundings(self):
        return torch.cat([self.raw[:256], self.raw[256 + self.n:]]).clone()


@functools.lru_cache(maxsize=None)
def _handed(name):
    """(ofs_r, sum_r, ofs_c, sum_c, delta) at the case's pitches"""
    c, d = dr.CASES[name], dr.build(name)
    return dr.stats(d['f0'], d['f1'], c.temp, c.L + c.dr, c.S + c.dc)


def _run(name, mode, scale=1.0, swap=False, forward_stats=False):
    """One call of the mode's entry point(s) on the case.  Returns dict(d=(d_feat0, d_feat1) numpy, conf_at, loss, delta,
    bad=[what is wrong with canaries / finiteness / statuses])."""
    lib = _lib.load()
    c, d = dr.CASES[name], dr.build(name)
    f0, f1, ids = d['f0'], d['f1'], d['ids']
    gc = d['gc'] * np.float32(scale)
    G = d['G'] * np.float32(0.0 if mode == "dense0" else scale)
    n, l, s = c.N, c.L, c.S
    out = dict(bad=[])
    if forward_stats:
        t0, t1 = torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)
        fwd = ops.coarse_match(t0, t1, dr.GRIDS[l], dr.GRIDS[s], 8.0, border_rm=0, temperature=c.temp, stats=True)
        bufs = fwd['_coarse_buffers']
        nr, sr, qr, nc, sc, qc = bufs.softmax_stats()
        torch.cuda.synchronize()
        raw = bufs.workspace.view(torch.uint8)

        def read(p, pitch, k):
            o = p.value - raw.data_ptr()
            return raw[o:o + n * pitch * 4].view(torch.float32).view(n, pitch)[:, :k].cpu().numpy()
        out['delta'] = max(dr.stats_delta(read(nr, qr, l), read(sr, qr, l), d['sm']['lse_r']),
                           dr.stats_delta(read(nc, qc, s), read(sc, qc, s), d['sm']['lse_c']))
        held, stats = [bufs], (nr, sr, qr, nc, sc, qc)
    else:
        ofs_r, sum_r, ofs_c, sum_c, out['delta'] = _handed(name)
        held = [Guarded(v) for v in (ofs_r, sum_r, ofs_c, sum_c)]
        if swap:
            held = held[2:] + held[:2]
        stats = (held[0].ptr, held[1].ptr, held[0].shape[1], held[2].ptr, held[3].ptr, held[2].shape[1])
    if swap:
        f0, f1, l, s = f1, f0, s, l
        ids, G = ids[:, [0, 2, 1]], np.ascontiguousarray(G.transpose(0, 2, 1))
    g0, g1 = Guarded(f0), Guarded(f1)
    b, i, j = (Guarded(ids[:, k], fill=0) for k in range(3))
    k = len(ids)
    d0, d1 = Guarded(shape=f0.shape), Guarded(shape=f1.shape)
    bufs_ = held + [g0, g1, b, i, j, d0, d1]
    head = (g0.ptr, g1.ptr, n, l, s, c.C, c.temp, *stats)

    def call(fn, *args):
        st = getattr(lib, fn)(*args, _stream())
        torch.cuda.synchronize()
        if st != 0:
            out['bad'].append(f"{fn}: status {st}")

    if mode == "sparse":
        need = int(lib.fm_dual_softmax_backward_workspace_bytes(n, l, s, c.C))
        ws, ggc, conf = GuardedWorkspace(need), Guarded(gc), Guarded(shape=(k,))
        bufs_ += [ws, ggc, conf]
        call("fm_dual_softmax_conf_at", *head, b.ptr, i.ptr, j.ptr, k, conf.ptr)
        call("fm_dual_softmax_backward", *head, b.ptr, i.ptr, j.ptr, ggc.ptr, k, ws.ptr, need, d0.ptr, d1.ptr)
        out['conf_at'] = conf.numpy()
    elif mode in ("dense", "dense0"):
        need = int(lib.fm_dual_softmax_backward_workspace_bytes(n, l, s, c.C))
        ws, gg = GuardedWorkspace(need), Guarded(G)
        bufs_ += [ws, gg]
        call("fm_dual_softmax_backward_dense", *head, gg.ptr, ws.ptr, need, d0.ptr, d1.ptr)
    else:
        need = int(lib.fm_coarse_loss_workspace_bytes(n, l, s, c.C, k))
        ws, loss, d_loss = GuardedWorkspace(need), Guarded(shape=(3,)), Guarded(np.full(1, scale, np.float32))
        bufs_ += [ws, loss, d_loss]
        problem = (*head, KINDS[mode], 0.25, 2.0, 1.0, 1.0, b.ptr, i.ptr, j.ptr, k, ws.ptr, need)
        call("fm_coarse_loss_forward", *problem, loss.ptr)
        call("fm_coarse_loss_backward", *problem, d_loss.ptr, d0.ptr, d1.ptr)
        out['loss'] = loss.numpy()
    assert need > 0
    if not all(g.intact() for g in bufs_ if isinstance(g, Guarded)):
        out['bad'].append("bytes outside a buffer were written")
    out['d'] = (d0.numpy(), d1.numpy())
    for what in ('conf_at', 'loss'):
        if what in out and not np.all(np.isfinite(out[what])):
            out['bad'].append(f"{what}: not finite / not written")
    for side in range(2):
        if not np.all(np.isfinite(out['d'][side])):
            out['bad'].append(f"d_feat{side}: {np.count_nonzero(~np.isfinite(out['d'][side]))} elements not finite / not written")
    return out


@functools.lru_cache(maxsize=None)
def _e_ref(name, mode):
    """(e_ref of d_feat0, of d_feat1, e32 of conf): float32 torch autograd on the device with the same dL/dconf"""
    c, d, r = dr.CASES[name], dr.build(name), dr.reference(name, mode)
    a0, a1, conf = dr.autograd(d['f0'], d['f1'], c.temp, r['g_dense'].astype(np.float32), torch.float32, DEV)
    e = [_normalised(a, r['ref'][side], r['T'][side], r['U'][side])[0] for side, a in enumerate((a0, a1))]
    return e[0], e[1], float(np.abs(conf.double().cpu().numpy() - d['sm']['conf']).max())


def _normalised(got, ref, T, U):
    """(max (|got - ref| - U) / T over T > 0, every element with T == 0 is exactly 0); U: dsm_grad_ref.flush_bound"""
    live = T > 0
    e = float((np.maximum(np.abs(got.astype(np.float64) - ref) - U, 0.0)[live] / T[live]).max()) if live.any() else 0.0
    return e, bool(np.all(got[~live] == 0))


def _grad_errors(tag, name, mode, got, delta):
    """the bar of the module docstring on both gradients; prints the ACC lines first"""
    r = dr.reference(name, mode)
    ref, bad = r['ref'], []
    for side in range(2):
        e_hip, zeros = _normalised(got[side], ref[side], r['T'][side], r['U'][side])
        e_ref = _e_ref(name, mode)[side]
        bar = 4 * e_ref + FLOOR + 4 * delta
        cancel = np.abs(ref[side]).max() / max(r['T'][side].max(), 1e-300)
        print(f"ACC {tag:34s} d_feat{side}  e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  delta {delta:.3e}  e_hip/bar "
              f"{e_hip / bar if bar else 0:6.3f}  max|ref|/max T {cancel:.1e}  {'regular' if name in dr.REGULAR else dr.CASES[name].kind}")
        if not zeros:
            bad.append(f"{tag} d_feat{side}: nonzero where no term is")
        if not e_hip <= bar:
            bad.append(f"{tag} d_feat{side}: e_hip {e_hip:.3e} > 4 * {e_ref:.3e} + {FLOOR:.3e} + 4 * {delta:.3e}")
    return bad


def _conf_at_errors(tag, name, got):
    c, d = dr.CASES[name], dr.build(name)
    if got.size == 0:
        return []
    k = d['ids']
    want = d['sm']['conf'][k[:, 0], k[:, 1], k[:, 2]]
    e32 = _e_ref(name, "sparse")[2]
    err = np.abs(got.astype(np.float64) - want).max()
    bar = 4 * e32 + 4 * float(_ulp(np.abs(d['sm']['sim']).max())) + FTZ
    print(f"ACC {tag:34s} conf_at  max err {err:.3e}  e32 {e32:.3e}  err/bar {err / bar:6.3f}  bar 4 e32 + 4 ulp(max|sim|)")
    return [] if err <= bar else [f"{tag} conf_at: err {err:.3e} > {bar:.3e}"]


def _loss_errors(tag, name, mode, got):
    r = dr.reference(name, mode)
    l32, _ = dr.loss_dconf(name, mode, torch.float32)
    bad = []
    for what, g, want, w32 in zip(("loss", "pos_mean", "neg_mean"), got.tolist(), r['loss64'], l32):
        e_ref = abs(w32 - want)
        print(f"ACC {tag:34s} {what:9s} loss64 {want:.9e}  e_ref/|loss64| {e_ref / abs(want):.3e}  e_hip/|loss64| "
              f"{abs(g - want) / abs(want):.3e}")
        if not abs(g - want) <= 4 * e_ref + LOSS_FLOOR * abs(want):
            bad.append(f"{tag} {what}: {g!r} against {want!r} (e_ref {e_ref:.3e})")
    return bad


@pytest.mark.parametrize("name,mode", PAIRS, ids=[f"{n}-{m}" for n, m in PAIRS])
def test_gradients_against_float64_with_handed_statistics(name, mode):
    """every case of the table in every mode it lists: statuses, canaries, finite outputs, exact zeros where no term is
    (K = 0, G = 0, a sample without an entry), the normalised bar; conf_at and the loss values under their own bars"""
    out = _run(name, mode)
    bad = out['bad']
    if not bad:
        bad = _grad_errors(f"{name} {mode}", name, mode, out['d'], out['delta'])
        if mode == "sparse":
            bad += _conf_at_errors(f"{name} {mode}", name, out['conf_at'])
        if mode in dr.LOSSES:
            bad += _loss_errors(f"{name} {mode}", name, mode, out['loss'])
    assert not bad, "\n".join(bad)


# one add per atomic target (listed entries with distinct rows and columns; dense: L <= 32 gives one row tile per column
# sum, S <= 64 at most two z slices per row sum, and a + b = b + a): the bits do not depend on the arrival order.
# ('peaky' data is not in the list: its softmax tails sit at the float32 underflow threshold, where the exponentials
# flush and a product that is flushed at g may be kept at 2 g.)
BITS_SPARSE = ["tile33x97", "tile1x65", "split33x33", "split_n86", "chan252", "data_scaled", "pitch_r7_c1"]
BITS_DENSE = ["tile2x2", "tile31x31", "tile32x32"]


@pytest.mark.parametrize("name,mode", [(n, "sparse") for n in BITS_SPARSE] + [(n, "dense") for n in BITS_DENSE])
def test_twice_the_upstream_gradient_is_exactly_twice_the_gradients_and_two_calls_give_the_same_bits(name, mode):
    assert dr.CASES[name].bits and (mode == "sparse" or (dr.CASES[name].L <= 32 and dr.CASES[name].S <= 64))
    one, again, two = _run(name, mode), _run(name, mode), _run(name, mode, scale=2.0)
    assert not one['bad'] + again['bad'] + two['bad']
    for side in range(2):
        assert one['d'][side].tobytes() == again['d'][side].tobytes(), f"d_feat{side}: two calls differ"
        assert np.array_equal(two['d'][side], 2.0 * one['d'][side]), f"d_feat{side}: not exactly twice"
        assert np.abs(one['d'][side]).max() > 0


@pytest.mark.parametrize("name", ["tile65x65", "split_n128", "chan128", "pitch_r7_c1"])
def test_dense_mode_twice_within_the_rounding_of_its_column_sums(name):
    """u takes one float atomic per 32-row tile of the owner image in arrival order, v one per z slice (dsm_grad.hip):
    two calls agree to 4 * 2^-23 T"""
    one, again = _run(name, "dense"), _run(name, "dense")
    assert not one['bad'] + again['bad']
    T = dr.reference(name, "dense")['T']
    for side in range(2):
        diff = np.abs(one['d'][side].astype(np.float64) - again['d'][side])
        print(f"ACC {name + ' dense twice':34s} d_feat{side}  max |a - b| / T {(diff / T[side]).max():.3e}  bar 4.8e-07  "
              f"bitwise {one['d'][side].tobytes() == again['d'][side].tobytes()}")
        assert np.all(diff <= 4 * 2.0 ** -23 * T[side])


@pytest.mark.parametrize("name,mode", [(n, m) for n in ("tile33x97", "tile97x33", "tile1x65", "chan68", "pitch_r7_c1")
                                       for m in ("sparse", "dense")])
def test_swapped_roles_return_the_two_gradients_swapped(name, mode):
    """f1, f0 with the statistics swapped, the ids swapped and G transposed: (d_feat1, d_feat0) of the plain call, under
    the bar against float64; whether also bit for bit is recorded, not asserted"""
    plain, swapped = _run(name, mode), _run(name, mode, swap=True)
    assert not plain['bad'] + swapped['bad']
    ref = dr.reference(name, mode)['ref']
    got = (swapped['d'][1], swapped['d'][0])
    bad = _grad_errors(f"{name} {mode} swapped", name, mode, got, swapped['delta'])
    same = all(got[side].tobytes() == plain['d'][side].tobytes() for side in range(2))
    print(f"ACC {name + ' ' + mode + ' swapped':34s} bitwise equal to the plain call: {same}")
    assert got[0].shape == ref[0].shape and not bad, "\n".join(bad)


@pytest.mark.parametrize("name", [n for n, c in dr.CASES.items() if c.kind == "saturated"])
def test_saturated_shapes_with_the_statistics_the_forward_call_left(name):
    """ops.coarse_match(..., stats=True) in place of the handed statistics, the same bar with delta measured from what the
    forward left in its workspace: what the dense backward owes on the small saturated problems DESIGN.md section 2
    counts beyond 2e-4 of max|grad|"""
    out = _run(name, "dense", forward_stats=True)
    bad = out['bad'] or _grad_errors(f"{name} dense forward-stats", name, "dense", out['d'], out['delta'])
    assert not bad, "\n".join(bad)
