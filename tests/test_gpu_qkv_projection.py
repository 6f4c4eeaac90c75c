"""ops.qkv_projection (fm_qkv_projection_forward / _backward, csrc/qkv_proj.hip) and the `hip_proj` switch of the context
layers, on the GPU.

The yardstick is float64 autograd through qkv_projection_ref.proj64 - the three projection lines of EncoderLayer.forward -
on the up-cast inputs, on the device.  For each of q, k, v, dx (dsrc) and the three weight gradients:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through the same three lines
    assert e_hip <= 4 e_ref + FLOOR
- the form and the factor of tests/test_gpu_encoder_tail.py and tests/test_gpu_linear_attention.py.  FLOOR is twice the
largest e_ref over this file's REGULAR lines, measured on the MI355X from the float32 torch path, never from the kernels
(profiles/qkv_projection_accuracy.txt holds every ACC and MEM line these tests print and the figure).  Left out of that
maximum, but held to the same bar: the module-level lines and any line with max|ref64| < 1e-6.

Sizes of the implementation (csrc/qkv_proj.hip): a wave's tile kQpTile = 32 tokens; a workgroup's chunk kQpFwdChunk = 256
tokens forward, kQpBwdChunk = 128 backward; at most kQpMaxGroups = 256 workgroups, so in self mode the forward's grid takes
a second round above 65 536 tokens and the backward's above 32 768; cross mode walks the chunks of x, then those of src, in
the same grid; k_qp_fold adds the slabs in 8 slices (more than one slab per slice from 9 workgroups = 1025 tokens in self
mode).  The token counts are not chunked on the host."""
import pytest
import torch

from featurematching_amd import _lib, ops, synth

import qkv_projection_ref as qref
import train_layers_yardstick as yard

pytestmark = pytest.mark.gpu

FLOOR = 2 * 4.470e-6        # profiles/qkv_projection_accuracy.txt: the largest e_ref over the regular lines of this file
DEV = "cuda:0"
FINE = {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}


def _case(seed, tx, ts=None, **kw):
    """(x, src or None, (gq, gk, gv), [wq, wk, wv]) float32 on the device"""
    x, src, g, w = qref.inputs(seed, tx, ts, **kw)
    dev = lambda t: None if t is None else torch.as_tensor(t, device=DEV)
    return dev(x), dev(src), tuple(dev(t) for t in g), [dev(w[k]) for k in qref.WEIGHTS]


def _three(x, src, g, weights, **kw):
    """(hip, ref32, ref64): each the tuple of qref.autograd"""
    hip = qref.autograd(ops.qkv_projection, x, src, g, weights, **kw)
    ref32 = qref.autograd(qref.proj, x, src, g, weights, **kw)
    ref64 = qref.autograd(qref.proj64, x, src, tuple(t.double() for t in g), weights, **kw)
    return hip, ref32, ref64


def _names(src):
    return qref.NAMES_SELF if src is None else qref.NAMES_CROSS


def _hold(tag, hip, ref32, ref64, names):
    """print every figure, then hold every tensor to the bar, at this file's floor"""
    yard.hold(tag, names, hip, ref32, ref64, FLOOR)


def _check(tag, seed, x_shape, s_shape=None, **kw):
    """self mode (s_shape None) or cross mode at the given shapes [..., 64]"""
    count = lambda shape: int(torch.Size(shape[:-1]).numel())
    x, src, g, weights = _case(seed, count(x_shape), None if s_shape is None else count(s_shape), **kw)
    x = x.view(x_shape)
    if src is not None:
        src = src.view(s_shape)
    g = (g[0].view(x_shape),) + tuple(t.view(x_shape if s_shape is None else s_shape) for t in g[1:])
    hip, ref32, ref64 = _three(x, src, g, weights)
    _hold(tag, hip, ref32, ref64, _names(src))
    return hip


# ---- token counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1025])
def test_token_counts_self(T):
    """both sides of kQpTile = 32, kQpBwdChunk = 128 and kQpFwdChunk = 256; 1025 tokens = 9 slabs, one fold slice with two"""
    _check(f"regular self T{T}", 100 + T, (T, 64))


@pytest.mark.parametrize("Tx,Ts", [(75, 130), (130, 75), (1, 257), (257, 1), (31, 33), (33, 32), (32, 2), (127, 129),
                                   (128, 255), (129, 256), (256, 127), (1025, 2), (2, 1025)])
def test_token_counts_cross(Tx, Ts):
    """the same edges with Tx != Ts: the q side and the k / v side end their chunks independently, and either side may be
    the one with more than one slab per fold slice"""
    _check(f"regular cross T{Tx}x{Ts}", 1000 + 7 * Tx + Ts, (Tx, 64), (Ts, 64))


def test_more_than_one_round_of_the_grid():
    """65 569 tokens in self mode: 257 chunks of kQpFwdChunk = 256 and 513 of kQpBwdChunk = 128 over kQpMaxGroups = 256
    workgroups - a second round forward, a second and a third backward, the last tile ragged"""
    _check("regular self T65569", 90, (256 * 256 + 32 + 1, 64))


# ---- shapes as the module hands them over --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 25, 64), (130, 49, 64)])
def test_module_shapes_self(shape):
    hip = _check(f"regular self {list(shape)}", 200 + shape[0], shape)
    assert all(t.shape == shape for t in hip[:4])


@pytest.mark.parametrize("shape", [(3, 25, 64), (130, 49, 64)])
def test_module_shapes_cross(shape):
    s_shape = (shape[0], 74 - shape[1], 64)                          # 25 against 49 tokens and the other way round
    hip = _check(f"regular cross {list(shape)}", 220 + shape[0], shape, s_shape)
    assert hip[0].shape == shape and hip[3].shape == shape
    assert all(hip[i].shape == s_shape for i in (1, 2, 4))


def test_non_contiguous_inputs():
    """x = every other row of a [2 T, 64] tensor, src = the left half of a [T, 128] one"""
    x, src, g, weights = _case(210, 75, 75)
    wide_x = torch.stack([x, torch.full_like(x, 7.0)], 1).reshape(150, 64)
    wide_s = torch.cat([src, torch.full_like(src, -7.0)], 1)

    def run(self_mode):
        """the op on strided views of leaf tensors (qref.autograd's clone would make them contiguous); the gradients
        come back through the views: the rows and columns outside them get zeros"""
        wx, ws = wide_x.clone().requires_grad_(True), wide_s.clone().requires_grad_(True)
        w = [t.detach().clone().requires_grad_(True) for t in weights]
        xs, ss = wx[::2], ws[:, :64]
        assert not xs.is_contiguous() and torch.equal(xs, x)
        assert not ss.is_contiguous() and torch.equal(ss, src)
        out = ops.qkv_projection(xs, xs if self_mode else ss, *w)
        assert all(t.is_contiguous() for t in out)
        torch.autograd.backward(list(out), list(g))
        assert not wx.grad[1::2].any() and (self_mode or not ws.grad[:, 64:].any())
        data = (wx.grad[::2],) if self_mode else (wx.grad[::2], ws.grad[:, :64])
        return tuple(t.detach() for t in out) + data + tuple(t.grad for t in w)

    ref32 = qref.autograd(qref.proj, x, src, g, weights)
    ref64 = qref.autograd(qref.proj64, x, src, tuple(t.double() for t in g), weights)
    _hold("regular cross T75 non-contiguous", run(False), ref32, ref64, qref.NAMES_CROSS)
    ref32 = qref.autograd(qref.proj, x, None, g, weights)            # and in self mode: x alone
    ref64 = qref.autograd(qref.proj64, x, None, tuple(t.double() for t in g), weights)
    _hold("regular self T75 non-contiguous", run(True), ref32, ref64, qref.NAMES_SELF)


# ---- value ranges --------------------------------------------------------------------------------------------------
def test_scale_30():
    _check("regular self [130, 49, 64] x30", 300, (130, 49, 64), scale=30.0)
    _check("regular cross [130, 49, 64] x30", 301, (130, 49, 64), (130, 25, 64), scale=30.0)


# ---- what is asked for ---------------------------------------------------------------------------------------------
def _record_backward(monkeypatch):
    """the arguments of every fm_qkv_projection_backward call, as ctypes receives them"""
    lib = _lib.load()
    real, seen = lib.fm_qkv_projection_backward, []
    monkeypatch.setattr(lib, "fm_qkv_projection_backward", lambda *a: (seen.append(a), real(*a))[1])
    return seen


@pytest.mark.parametrize("cross", [False, True])
def test_data_gradients_only(monkeypatch, cross):
    """no weight requires grad: dx (and dsrc) hold the bar, no weight gets a .grad (qref.autograd asserts it) and the
    backward is handed NULL weight-gradient pointers"""
    x, src, g, weights = _case(400, 130 * 49, 130 * 25 if cross else None)
    seen = _record_backward(monkeypatch)
    hip, ref32, ref64 = _three(x, src, g, weights, weight_grads=False)
    assert len(hip) == (5 if cross else 4)
    assert len(seen) == 1 and seen[0][15:18] == (None, None, None) and seen[0][13] is not None
    assert (seen[0][14] is not None) == cross                        # d_src: cross mode only
    _hold("regular data only " + ("cross" if cross else "self"), hip, ref32, ref64, _names(src))
    hip = qref.autograd(ops.qkv_projection, x, src, g, weights)      # and with the weights: all three pointers
    assert len(seen) == 2 and all(p is not None for p in seen[1][15:18])


def test_forward_only():
    for x, src, g, weights in (_case(410, 333), _case(411, 333, 200)):
        s = x if src is None else src
        with torch.no_grad():
            hip = ops.qkv_projection(x, s, *weights)
            r32, r64 = qref.proj(x, s, *weights), qref.proj64(x, s, *weights)
        assert not any(t.requires_grad for t in hip)
        _hold("regular forward only " + ("self" if src is None else "cross"), hip, r32, r64, ("q", "k", "v"))


def test_self_mode_is_the_sum_of_cross_mode():
    """the gradient self mode returns for x = dx + dsrc of the cross-mode call on a copy of x; a view of x's memory with
    x's offset, shape and strides is self mode too"""
    x, _, g, weights = _case(430, 130 * 49)
    self_ = qref.autograd(ops.qkv_projection, x, None, g, weights)
    cross = qref.autograd(ops.qkv_projection, x, x.clone(), g, weights)
    ref64 = qref.autograd(qref.proj64, x, None, tuple(t.double() for t in g), weights)
    ref32 = qref.autograd(qref.proj, x, None, g, weights)
    summed = cross[:3] + (cross[3] + cross[4],) + cross[5:]
    _hold("regular self T6370", self_, ref32, ref64, qref.NAMES_SELF)
    _hold("regular self = cross dx + dsrc", summed, ref32, ref64, qref.NAMES_SELF)
    apart = yard.rel_err(self_[3], summed[3].double())               # and the two against each other, at the same bar
    assert apart <= 4 * yard.rel_err(ref32[3], ref64[3]) + FLOOR, apart
    for u, v in zip(self_[:3], cross[:3]):                           # q, k, v: the same k-ordered chains in either mode
        assert torch.equal(u, v)
    xg = x.detach().clone().requires_grad_(True)
    q, k, v = ops.qkv_projection(xg, xg.view(-1, 64), *weights)
    torch.autograd.backward([q, k, v], list(g))
    assert torch.equal(xg.grad, self_[3])


@pytest.mark.parametrize("cross", [False, True])
def test_same_bits_on_every_call(cross):
    x, src, g, weights = _case(420, 130 * 49, 130 * 49 if cross else None)
    x = x.view(130, 49, 64)
    src = None if src is None else src.view(130, 49, 64)
    g = tuple(t.view(130, 49, 64) for t in g)
    first = qref.autograd(ops.qkv_projection, x, src, g, weights)
    second = qref.autograd(ops.qkv_projection, x, src, g, weights)
    assert len(first) == (8 if cross else 7)
    for u, v in zip(first, second):
        assert torch.equal(u, v)


# ---- the modules ---------------------------------------------------------------------------------------------------
_module, _module_run = yard.module, yard.module_run


@pytest.mark.parametrize("masked", [False, True])
def test_module_training_step(monkeypatch, masked):
    """a training-mode fine LocalFeatureTransformer with hip_attention=True, hip_tail=True at the inputs of
    tests/test_gpu_encoder_tail.py's module case: hip_proj on against a float64 copy, e_ref from hip_proj off in float32.
    Both outputs, both input gradients, every parameter's gradient; masked = a ragged padding mask on image 0."""
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(900, i, (130, 49, 64)), device=DEV) for i in (1, 2, 3, 4))
    kw = {}
    if masked:
        mask0 = torch.zeros(130, 49, dtype=torch.bool, device=DEV)
        for b in range(130):
            mask0[b, :max(1, 49 - (3 * b + 4) % 49)] = True
        kw = {'mask0': mask0}
    calls = yard.count_calls(monkeypatch, "qkv_projection")
    switches = dict(hip_attention=True, hip_tail=True)
    names, hip = _module_run(_module(FINE, hip_proj=True, **switches), x0, x1, g0, g1, torch.float32, **kw)
    assert calls == {"qkv_projection": 4}                            # self x 2, cross x 2: every layer call took the HIP op
    _, ref32 = _module_run(_module(FINE, **switches), x0, x1, g0, g1, torch.float32, **kw)
    assert calls == {"qkv_projection": 4}
    _, ref64 = _module_run(_module(FINE, dtype=torch.float64, hip_proj=True, **switches), x0, x1, g0, g1, torch.float64, **kw)
    assert calls == {"qkv_projection": 4}                            # float64 tensors: the torch lines
    _hold("module fine" + (" masked" if masked else ""), hip, ref32, ref64, names)


def test_module_d256_takes_the_torch_lines(monkeypatch):
    cfg = {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross']}
    x0, x1 = (torch.as_tensor(synth.normal(910, i, (2, 60, 256)), device=DEV) for i in (1, 2))
    calls = yard.count_calls(monkeypatch, "qkv_projection")
    _, on = _module_run(_module(cfg, hip_proj=True), x0, x1, x1, x0, torch.float32)
    _, off = _module_run(_module(cfg), x0, x1, x1, x0, torch.float32)
    assert calls == {"qkv_projection": 0}
    for u, v in zip(on, off):
        assert torch.equal(u, v)


# ---- memory --------------------------------------------------------------------------------------------------------
def test_peak_memory():
    """forward + backward in self mode at [2000 * 49, 64] allocate q, k, v, dx, the three weight gradients and one workspace
    per call, and nothing of the tensors' size besides (torch saves only the inputs here too: no ratio is asserted)"""
    T = 2000 * 49
    gen = torch.Generator(device=DEV).manual_seed(5)
    x, gq, gk, gv = (torch.randn(T, 64, device=DEV, generator=gen) for _ in range(4))
    _, _, _, weights = _case(500, 64)
    qref.autograd(ops.qkv_projection, x[:64], None, (gq[:64], gk[:64], gv[:64]), weights)     # (library loaded, attributes set)
    # blocks for the results are then cut to size from one cached segment; a fresh segment of its own would round each
    # of them up to a multiple of 2 MiB, which max_memory_allocated counts
    spare = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)
    del spare
    ws = _lib.load().fm_qkv_projection_workspace_bytes(T, T, 64)
    assert 0 < ws <= 64 << 20
    # q, k, v and dx; the weight gradients; the forward's workspace is released before the backward takes its own
    allowed = 4 * T * 64 * 4 + 3 * 64 * 64 * 4 + ws + (1 << 20)
    self_mode = lambda fn: lambda x, *w: fn(x, x, *w)
    peak_hip = yard.peak_above_inputs(self_mode(ops.qkv_projection), [x] + weights, (gq, gk, gv))
    peak_torch = yard.peak_above_inputs(self_mode(qref.proj), [x] + weights, (gq, gk, gv))
    print(f"MEM  qkv T{T}  hip {peak_hip} B  allowed {allowed} B  torch {peak_torch} B  ({peak_torch / max(peak_hip, 1):.2f} x)")
    assert peak_hip <= allowed, (peak_hip, allowed)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    """256 channels, float64, a mismatched batch dimension and zero tokens raise before anything launches"""
    _, _, _, weights = _case(600, 64)
    x = torch.zeros(3, 25, 64, device=DEV)
    for bad_x, bad_s in ((torch.zeros(3, 25, 256, device=DEV),) * 2, (x, torch.zeros(4, 25, 64, device=DEV)),
                         (x.double(), x.double()), (x, x.double()), (torch.zeros(0, 64, device=DEV),) * 2,
                         (x, torch.zeros(3, 0, 64, device=DEV))):
        assert not ops.qkv_projection_supported(bad_x, bad_s)
        with pytest.raises(ValueError):
            ops.qkv_projection(bad_x, bad_s, *weights)
    with pytest.raises(ValueError):
        ops.qkv_projection(x, x, *[w.double() for w in weights])
    with pytest.raises(RuntimeError):
        ops.qkv_projection(x.cpu(), x.cpu(), *weights)
    with pytest.raises(_lib.FMatchError) as err:                     # the ABI's own check, through the library
        lib = _lib.load()
        _lib.check(lib.fm_qkv_projection_forward(*[x.data_ptr()] * 5, 75, 75, 32, None, 0, *[x.data_ptr()] * 3, None), "x")
    assert err.value.status == _lib.FM_E_UNSUPPORTED
    assert ops.qkv_projection_supported(x, x) and ops.qkv_projection_supported(x, torch.zeros(3, 49, 64, device=DEV))
