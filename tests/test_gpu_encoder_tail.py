"""ops.encoder_tail (fm_encoder_tail_forward / _backward, csrc/encoder_tail.hip) and the `hip_tail` switch of the context
layers, on the GPU.

The yardstick is float64 autograd through encoder_tail_ref.tail64 - the three torch lines of EncoderLayer.forward behind
the attention - on the up-cast inputs, on the device (tests/test_modules_cpu.py pins the torch layers to the reference's
fixtures).  For each of y, dx, da and the seven parameter gradients:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through the same three lines
    assert e_hip <= 4 e_ref + FLOOR
- the form and the factor of tests/test_gpu_linear_attention.py.  FLOOR is twice the largest e_ref over this file's REGULAR
lines, measured on the MI355X from the float32 torch path, never from the kernels (profiles/encoder_tail_accuracy.txt holds
every ACC and MEM line these tests print and the figure).  Left out of that maximum, but held to the same bar: the
`zero_share` lines, the module-level lines and any line with max|ref64| < 1e-6.

Sizes of the implementation (csrc/encoder_tail.hip): a wave's tile kEtTile = 32 tokens; a workgroup's chunk kEtFwdChunk =
256 tokens forward, kEtBwdChunk = 128 backward; at most kEtMaxGroups = 256 workgroups, so the forward's grid takes a second
round above 65 536 tokens and the backward's above 32 768; k_et_fold adds the slabs in 8 slices (more than one slab per
slice from 9 workgroups = 1025 tokens).  T is not chunked on the host."""
import pytest
import torch

from featurematching_amd import _lib, ops, synth

import encoder_tail_ref as tref
import train_layers_yardstick as yard

pytestmark = pytest.mark.gpu

FLOOR = 2 * 4.244e-6        # profiles/encoder_tail_accuracy.txt: the largest e_ref over the regular lines of this file
DEV = "cuda:0"
FINE = {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}


def _hip(x, a, *params):
    return ops.encoder_tail(x, a, *params, tref.EPS, tref.EPS)


def _case(seed, T, **kw):
    """(x, a, gy [T, 64], [the seven parameters]) float32 on the device; the ReLU guard's first-round share is held here"""
    x, a, gy, p, share = tref.inputs(seed, T, **kw)
    assert share <= 0.05, share
    dev = lambda t: torch.as_tensor(t, device=DEV)
    return dev(x), dev(a), dev(gy), [dev(p[k]) for k in tref.PARAMS]


def _three(x, a, gy, params, **kw):
    """(hip, ref32, ref64): each the tuple of tref.autograd"""
    hip = tref.autograd(_hip, x, a, gy, params, **kw)
    ref32 = tref.autograd(tref.tail, x, a, gy, params, **kw)
    ref64 = tref.autograd(tref.tail64, x, a, gy.double(), params, **kw)
    return hip, ref32, ref64


def _hold(tag, hip, ref32, ref64, names=tref.NAMES):
    """print every figure, then hold every tensor to the bar, at this file's floor"""
    yard.hold(tag, names, hip, ref32, ref64, FLOOR)


def _check(tag, seed, shape, **kw):
    t = 1
    for s in shape[:-1]:
        t *= s
    x, a, gy, params = _case(seed, t, **kw)
    x, a, gy = (v.view(shape) for v in (x, a, gy))
    hip, ref32, ref64 = _three(x, a, gy, params)
    _hold(tag, hip, ref32, ref64)
    return hip


# ---- token counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025])
def test_token_counts(T):
    """both sides of kEtTile = 32, kEtBwdChunk = 128 and kEtFwdChunk = 256; 1025 tokens = 9 slabs, one fold slice with two"""
    _check(f"regular T{T}", 100 + T, (T, 64))


def test_more_than_one_round_of_the_grid():
    """65 569 tokens: 257 chunks of kEtFwdChunk = 256 and 513 of kEtBwdChunk = 128 over kEtMaxGroups = 256 workgroups - a
    second round forward, a second and a third backward, the last tile ragged"""
    _check("regular T65569", 90, (65536 + 33, 64))


# ---- shapes as the module hands them over --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 25, 64), (130, 49, 64)])
def test_module_shapes(shape):
    hip = _check(f"regular {list(shape)}", 200 + shape[0], shape)
    assert hip[0].shape == shape and hip[1].shape == shape and hip[2].shape == shape


def test_non_contiguous_x():
    """x = every other row of a [2 T, 64] tensor, a = the left half of a [T, 128] one"""
    x, a, gy, params = _case(210, 75)
    wide_x = torch.stack([x, torch.full_like(x, 7.0)], 1).reshape(150, 64)
    wide_a = torch.cat([a, torch.full_like(a, -7.0)], 1)
    xs = wide_x[::2]
    assert not xs.is_contiguous() and torch.equal(xs, x)
    a_nc = wide_a[:, :64]
    assert not a_nc.is_contiguous() and torch.equal(a_nc, a)
    hip = tref.autograd(_hip, xs, a_nc, gy, params)
    ref32 = tref.autograd(tref.tail, x, a, gy, params)
    ref64 = tref.autograd(tref.tail64, x, a, gy.double(), params)
    _hold("regular T75 non-contiguous", hip, ref32, ref64)


# ---- value ranges --------------------------------------------------------------------------------------------------
def test_scale_30():
    """x and a at scale 30: LayerNorm's invariance (a) and a large hidden layer (x)"""
    _check("regular [130, 49, 64] x30", 300, (130, 49, 64), scale=30.0)


def test_zero_tokens():
    """a tenth of the tokens with x = a = 0, b1 = 0 - what a fully masked query gives: m = 0, variance 0, n1 = 0, p = 0
    exactly, the ReLU mask 0.  Everything stays finite and holds the bar."""
    hip = _check("zero_share [130, 49, 64]", 310, (130, 49, 64), zero_share=0.1)
    assert all(bool(torch.isfinite(t).all()) for t in hip)


# ---- what is asked for ---------------------------------------------------------------------------------------------
def test_data_gradients_only():
    """no parameter requires grad: dx and da hold the bar, no parameter gets a .grad (tref.autograd asserts it) and the
    backward is handed NULL parameter-gradient pointers"""
    x, a, gy, params = _case(400, 130 * 49)
    hip, ref32, ref64 = _three(x, a, gy, params, param_grads=False)
    assert len(hip) == 3
    _hold("regular T6370 data only", hip, ref32, ref64)


def test_forward_only():
    x, a, gy, params = _case(410, 333)
    with torch.no_grad():
        y = _hip(x, a, *params)
        r32, r64 = tref.tail(x, a, *params), tref.tail64(x, a, *params)
    assert not y.requires_grad
    _hold("regular T333 forward only", (y,), (r32,), (r64,))


def test_same_bits_on_every_call():
    x, a, gy, params = _case(420, 130 * 49)
    x, a, gy = (v.view(130, 49, 64) for v in (x, a, gy))
    first = tref.autograd(_hip, x, a, gy, params)
    second = tref.autograd(_hip, x, a, gy, params)
    assert len(first) == 10
    for u, v in zip(first, second):
        assert torch.equal(u, v)


# ---- the modules ---------------------------------------------------------------------------------------------------
_module, _module_run = yard.module, yard.module_run


@pytest.mark.parametrize("masked", [False, True])
def test_module_training_step(monkeypatch, masked):
    """a training-mode fine LocalFeatureTransformer with hip_attention=True at the inputs of
    tests/test_gpu_linear_attention.py's module case: hip_tail on against a float64 copy, e_ref from hip_tail off in
    float32.  Both outputs, both input gradients, every parameter's gradient; masked = a ragged padding mask on image 0."""
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(900, i, (130, 49, 64)), device=DEV) for i in (1, 2, 3, 4))
    kw = {}
    if masked:
        mask0 = torch.zeros(130, 49, dtype=torch.bool, device=DEV)
        for b in range(130):
            mask0[b, :max(1, 49 - (3 * b + 4) % 49)] = True
        kw = {'mask0': mask0}
    calls = yard.count_calls(monkeypatch, "encoder_tail")
    names, hip = _module_run(_module(FINE, hip_attention=True, hip_tail=True), x0, x1, g0, g1, torch.float32, **kw)
    assert calls == {"encoder_tail": 4}                              # self x 2, cross x 2: every layer call took the HIP tail
    _, ref32 = _module_run(_module(FINE, hip_attention=True), x0, x1, g0, g1, torch.float32, **kw)
    assert calls == {"encoder_tail": 4}
    _, ref64 = _module_run(_module(FINE, dtype=torch.float64, hip_attention=True, hip_tail=True), x0, x1, g0, g1,
                           torch.float64, **kw)
    assert calls == {"encoder_tail": 4}                              # float64 tensors: the torch lines
    _hold("module fine" + (" masked" if masked else ""), hip, ref32, ref64, names)


def test_module_d256_takes_the_torch_lines(monkeypatch):
    cfg = {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross']}
    x0, x1 = (torch.as_tensor(synth.normal(910, i, (2, 60, 256)), device=DEV) for i in (1, 2))
    calls = yard.count_calls(monkeypatch, "encoder_tail")
    _, on = _module_run(_module(cfg, hip_tail=True), x0, x1, x1, x0, torch.float32)
    _, off = _module_run(_module(cfg), x0, x1, x1, x0, torch.float32)
    assert calls == {"encoder_tail": 0}
    for u, v in zip(on, off):
        assert torch.equal(u, v)


# ---- memory --------------------------------------------------------------------------------------------------------
def test_peak_memory():
    """forward + backward at [2000 * 49, 64] allocate y, dx, da, the seven parameter gradients, the state and one workspace,
    and nothing of the tensors' size besides: none of the six tensors torch's autograd keeps per call"""
    T = 2000 * 49
    gen = torch.Generator(device=DEV).manual_seed(5)
    x, a, gy = (torch.randn(T, 64, device=DEV, generator=gen) for _ in range(3))
    _, _, _, params = _case(500, 64)
    tref.autograd(_hip, x[:64], a[:64], gy[:64], params)             # (library loaded, kernels' attributes set)
    # blocks for the results are then cut to size from one cached segment; a fresh segment of its own would round each
    # of them up to a multiple of 2 MiB, which max_memory_allocated counts
    spare = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)
    del spare
    lib = _lib.load()
    state, ws = lib.fm_encoder_tail_state_bytes(T, 64), lib.fm_encoder_tail_workspace_bytes(T, 64)
    assert state <= 16 * T and 0 < ws <= 64 << 20
    allowed = 3 * T * 64 * 4 + sum(p.numel() * 4 for p in params) + state + ws + (1 << 20)
    peak_hip = yard.peak_above_inputs(_hip, [x, a] + params, gy)
    peak_torch = yard.peak_above_inputs(tref.tail, [x, a] + params, gy)
    print(f"MEM  tail T{T}  hip {peak_hip} B  allowed {allowed} B  torch {peak_torch} B  ({peak_torch / max(peak_hip, 1):.2f} x)")
    assert peak_hip <= allowed, (peak_hip, allowed)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    """256 channels, mismatched shapes and float64 raise before anything launches"""
    _, _, _, params = _case(600, 64)
    x = torch.zeros(3, 25, 64, device=DEV)
    for bad_x, bad_a in ((torch.zeros(3, 25, 256, device=DEV),) * 2, (x, torch.zeros(3, 49, 64, device=DEV)),
                         (x.double(), x.double()), (x, x.double()), (torch.zeros(0, 64, device=DEV),) * 2):
        assert not ops.encoder_tail_supported(bad_x, bad_a)
        with pytest.raises(ValueError):
            ops.encoder_tail(bad_x, bad_a, *params, tref.EPS, tref.EPS)
    with pytest.raises(ValueError):
        ops.encoder_tail(x, x, *[p.double() for p in params], tref.EPS, tref.EPS)
    with pytest.raises(RuntimeError):
        ops.encoder_tail(x.cpu(), x.cpu(), *params, tref.EPS, tref.EPS)
    with pytest.raises(_lib.FMatchError) as err:                     # the ABI's own check, through the library
        lib = _lib.load()
        _lib.check(lib.fm_encoder_tail_forward(*[x.data_ptr()] * 9, 75, 32, 1e-5, 1e-5, None, 0, None, x.data_ptr(), None), "x")
    assert err.value.status == _lib.FM_E_UNSUPPORTED
    assert ops.encoder_tail_supported(x, x)
