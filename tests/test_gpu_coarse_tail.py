"""ops.coarse_tail (fm_coarse_tail_forward / _backward, csrc/coarse_tail.hip), the `hip_coarse_tail` switch of the context
layers and the Matcher's `hip_train_coarse`, on the GPU.

The yardstick is float64 autograd through coarse_tail_ref.tail64 - the three torch lines of EncoderLayer.forward behind
the attention, d_model 256 - on the up-cast inputs, on the device.  For each of y, dx, da and the seven parameter gradients:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through the same three lines
    assert e_hip <= 4 e_ref + FLOOR
(train_layers_yardstick.hold).  FLOOR is twice the largest e_ref over this file's REGULAR lines, measured on the MI355X
from the float32 torch path, never from the kernels (profiles/coarse_tail_accuracy.txt holds every ACC and MEM line these
tests print and the figure).  Left out of that maximum, but held to the same bar: the `zero_share` lines, the
module-level lines and any line with max|ref64| < 1e-6.

Sizes of the implementation (csrc/coarse_tail.hip): the product kernel's tile is 64 tokens (kCtBM) and a LayerNorm
workgroup takes kCtLnTok = 64 tokens, 16 per wave, and writes one row of partial LayerNorm gradients; a slab of partial
weight gradients covers kCtSplit = 512 tokens; the C call walks T in equal chunks of at most kCtChunk = 8192 tokens (8193
tokens = chunks of 4160 and 4033, 16385 = 5504, 5504 and 5377), and from the second chunk on the fold ADDS to the gradients.
k_ct_fold adds slabs and rows in 8 slices: more than one row per slice from 9 rows = 513 tokens of a chunk.  Every grid
covers its chunk wholly - no kernel takes a second round of its grid; what takes that place here is the second chunk."""
import pytest
import torch

from featurematching_amd import _lib, ops, synth

import coarse_tail_ref as tref
import matcher_train_ref as mref
import train_layers_yardstick as yard

pytestmark = pytest.mark.gpu

FLOOR = 2 * 3.608e-6        # profiles/coarse_tail_accuracy.txt: the largest e_ref over the regular lines of this file
DEV = "cuda:0"
COARSE = {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross']}
OPS = mref.OPS + ("coarse_tail",)


def _hip(x, a, *params):
    return ops.coarse_tail(x, a, *params, tref.EPS, tref.EPS)


def _case(seed, T, **kw):
    """(x, a, gy [T, 256], [the seven parameters]) float32 on the device; the ReLU guard's first-round share is held here"""
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
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 511, 512, 513, 1025, 8192, 8193, 16385])
def test_token_counts(T):
    """both sides of the tile and the LayerNorm workgroup (64), of a slab (512) and of a chunk (8192); 1025 tokens = 3
    slabs and 17 rows, fold slices with three; 8193 = two chunks, 16385 = three: the folds add to the first chunk's sums"""
    _check(f"regular T{T}", 100 + T, (T, 256))


# ---- shapes as the module hands them over --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 60, 256), (1, 4800, 256)])
def test_module_shapes(shape):
    hip = _check(f"regular {list(shape)}", 200 + shape[0], shape)
    assert hip[0].shape == shape and hip[1].shape == shape and hip[2].shape == shape


def test_non_contiguous_inputs():
    """x = every other row of a [2 T, 256] tensor, a = the left half of a [T, 512] one"""
    x, a, gy, params = _case(210, 75)
    wide_x = torch.stack([x, torch.full_like(x, 7.0)], 1).reshape(150, 256)
    wide_a = torch.cat([a, torch.full_like(a, -7.0)], 1)
    xs = wide_x[::2]
    assert not xs.is_contiguous() and torch.equal(xs, x)
    a_nc = wide_a[:, :256]
    assert not a_nc.is_contiguous() and torch.equal(a_nc, a)
    hip = tref.autograd(_hip, xs, a_nc, gy, params)
    ref32 = tref.autograd(tref.tail, x, a, gy, params)
    ref64 = tref.autograd(tref.tail64, x, a, gy.double(), params)
    _hold("regular T75 non-contiguous", hip, ref32, ref64)


# ---- value ranges --------------------------------------------------------------------------------------------------
def test_scale_30():
    """x and a at scale 30: LayerNorm's invariance (a) and a large hidden layer (x)"""
    _check("regular [1, 4800, 256] x30", 300, (1, 4800, 256), scale=30.0)


def test_zero_tokens():
    """a tenth of the tokens with x = a = 0, b1 = 0 - what a fully masked query gives: m = 0, variance 0, n1 = 0, p = 0
    exactly, the ReLU mask 0.  Everything stays finite and holds the bar."""
    hip = _check("zero_share [1, 4800, 256]", 310, (1, 4800, 256), zero_share=0.1)
    assert all(bool(torch.isfinite(t).all()) for t in hip)


# ---- what is asked for ---------------------------------------------------------------------------------------------
def test_data_gradients_only():
    """no parameter requires grad: dx and da hold the bar, no parameter gets a .grad (tref.autograd asserts it) and the
    backward is handed NULL parameter-gradient pointers; two chunks"""
    x, a, gy, params = _case(400, 9000)
    hip, ref32, ref64 = _three(x, a, gy, params, param_grads=False)
    assert len(hip) == 3
    _hold("regular T9000 data only", hip, ref32, ref64)


def test_forward_only():
    x, a, gy, params = _case(410, 333)
    with torch.no_grad():
        y = _hip(x, a, *params)
        r32, r64 = tref.tail(x, a, *params), tref.tail64(x, a, *params)
    assert not y.requires_grad
    _hold("regular T333 forward only", (y,), (r32,), (r64,))


def test_same_bits_on_every_call():
    x, a, gy, params = _case(420, 9000)
    x, a, gy = (v.view(1, 9000, 256) for v in (x, a, gy))
    first = tref.autograd(_hip, x, a, gy, params)
    second = tref.autograd(_hip, x, a, gy, params)
    assert len(first) == 10
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def test_same_bits_whatever_the_workspace_held(monkeypatch):
    """every workspace handed to the two calls prefilled with 0xFF bytes - NaN bit patterns - against workspaces as the
    allocator hands them out: the same bits in all ten outputs, all finite.  (The op keeps no state: the state query
    answers 0 and no state buffer exists to prefill.)  Two chunks, so the second chunk meets what the first one left."""
    x, a, gy, params = _case(430, 9000)
    assert _lib.load().fm_coarse_tail_state_bytes(9000, 256) == 0
    plain = tref.autograd(_hip, x, a, gy, params)
    real, handed = ops._aligned_workspace, []

    def filled(nbytes, device):
        ws, ptr = real(nbytes, device)
        ws.fill_(0xFF)
        handed.append(nbytes)
        return ws, ptr
    monkeypatch.setattr(ops, "_aligned_workspace", filled)
    dirty = tref.autograd(_hip, x, a, gy, params)
    assert len(handed) == 2 and len(dirty) == 10                     # one workspace forward, one backward
    for u, v in zip(plain, dirty):
        assert bool(torch.isfinite(v).all()) and torch.equal(u, v)


# ---- the modules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_module_training_step(monkeypatch, masked):
    """a training-mode coarse LocalFeatureTransformer (self + cross) with hip_attention=True on [2, 60, 256]:
    hip_coarse_tail on against a float64 copy, e_ref from hip_coarse_tail off in float32.  Both outputs, both input
    gradients, every parameter's gradient; masked = a ragged padding mask on image 0."""
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(900, i, (2, 60, 256)), device=DEV) for i in (1, 2, 3, 4))
    kw = {}
    if masked:
        mask0 = torch.zeros(2, 60, dtype=torch.bool, device=DEV)
        mask0[0, :41] = True
        mask0[1, :60] = True
        kw = {'mask0': mask0}
    calls = yard.count_calls(monkeypatch, "coarse_tail", "encoder_tail")
    names, hip = yard.module_run(yard.module(COARSE, hip_attention=True, hip_coarse_tail=True), x0, x1, g0, g1,
                                 torch.float32, **kw)
    assert calls == {"coarse_tail": 4, "encoder_tail": 0}            # self x 2, cross x 2: every layer call took the HIP tail
    _, ref32 = yard.module_run(yard.module(COARSE, hip_attention=True), x0, x1, g0, g1, torch.float32, **kw)
    assert calls == {"coarse_tail": 4, "encoder_tail": 0}
    _, ref64 = yard.module_run(yard.module(COARSE, dtype=torch.float64, hip_attention=True, hip_coarse_tail=True), x0, x1,
                               g0, g1, torch.float64, **kw)
    assert calls == {"coarse_tail": 4, "encoder_tail": 0}            # float64 tensors: the torch lines
    _hold("module coarse" + (" masked" if masked else ""), hip, ref32, ref64, names)


# ---- memory --------------------------------------------------------------------------------------------------------
def test_peak_memory():
    """forward + backward at [64 * 4800, 256] allocate y, dx, da, the seven parameter gradients, the state and one
    workspace, and nothing of the tensors' size besides: none of the tensors torch's autograd keeps per call"""
    T = 64 * 4800
    gen = torch.Generator(device=DEV).manual_seed(5)
    x, a, gy = (torch.randn(T, 256, device=DEV, generator=gen) for _ in range(3))
    _, _, _, params = _case(500, 64)
    tref.autograd(_hip, x[:64], a[:64], gy[:64], params)             # (library loaded)
    # blocks for the results are then cut to size from one cached segment; a fresh segment of its own would round each
    # of them up to a multiple of 2 MiB, which max_memory_allocated counts
    spare = torch.empty(1536 << 20, dtype=torch.uint8, device=DEV)
    del spare
    lib = _lib.load()
    state, ws = lib.fm_coarse_tail_state_bytes(T, 256), lib.fm_coarse_tail_workspace_bytes(T, 256)
    assert state <= 16 * T and 0 < ws <= 128 << 20
    allowed = 3 * T * 256 * 4 + sum(p.numel() * 4 for p in params) + state + ws + (1 << 20)
    peak_hip = yard.peak_above_inputs(_hip, [x, a] + params, gy)
    peak_torch = yard.peak_above_inputs(tref.tail, [x, a] + params, gy)
    print(f"MEM  tail T{T}  hip {peak_hip} B  allowed {allowed} B  torch {peak_torch} B  ({peak_torch / max(peak_hip, 1):.2f} x)")
    assert peak_hip <= allowed, (peak_hip, allowed)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    """64 channels, mismatched shapes, float64 and no tokens raise before anything launches"""
    _, _, _, params = _case(600, 64)
    x = torch.zeros(2, 60, 256, device=DEV)
    for bad_x, bad_a in ((torch.zeros(2, 60, 64, device=DEV),) * 2, (x, torch.zeros(2, 61, 256, device=DEV)),
                         (x.double(), x.double()), (x, x.double()), (torch.zeros(0, 256, device=DEV),) * 2):
        assert not ops.coarse_tail_supported(bad_x, bad_a)
        with pytest.raises(ValueError):
            ops.coarse_tail(bad_x, bad_a, *params, tref.EPS, tref.EPS)
    with pytest.raises(ValueError):
        ops.coarse_tail(x, x, *[p.double() for p in params], tref.EPS, tref.EPS)
    with pytest.raises(RuntimeError):
        ops.coarse_tail(x.cpu(), x.cpu(), *params, tref.EPS, tref.EPS)
    with pytest.raises(_lib.FMatchError) as err:                     # the ABI's own check, through the library
        lib = _lib.load()
        _lib.check(lib.fm_coarse_tail_forward(*[x.data_ptr()] * 9, 120, 64, 1e-5, 1e-5, None, 0, None, x.data_ptr(), None), "x")
    assert err.value.status == _lib.FM_E_UNSUPPORTED
    assert ops.coarse_tail_supported(x, x)


# ---- the Matcher ---------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic_torch():
    """torch's own scatter-adds (the backward of feat_c[b_ids, ids]) in a fixed order while two runs are compared"""
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])


def test_matcher_hip_train_coarse_on_against_off(monkeypatch, deterministic_torch):
    """the default configuration (8 coarse layers) on matcher_train_ref's seeded batch, patch backbone, fixture_merge:
    with hip_train_coarse every coarse layer call takes ops.coarse_tail (8 layers x 2 images) and nothing else changes
    its count; loss and every gradient within tests/test_gpu_matcher_train.py's wiring bar of the hip_train_coarse=False
    run, 1e-3 of max|g_off|."""
    off = mref.matcher(hip_train=True, patches=True, fixture_merge=True)
    on = mref.matcher(hip_train=True, hip_train_coarse=True, patches=True, fixture_merge=True)
    on.load_state_dict(off.state_dict())
    calls = yard.count_calls(monkeypatch, *OPS)
    loss_off, g_off = mref.step(off, mref.batch(62, grad=True))
    base = {"window_merge": 2, "linear_attention": 20, "encoder_tail": 4, "qkv_projection": 4}
    assert calls == {**base, "coarse_tail": 0}
    for k in calls:
        calls[k] = 0
    loss_on, g_on = mref.step(on, mref.batch(62, grad=True))
    assert calls == {**base, "coarse_tail": 16}
    d_loss = abs(loss_on.item() - loss_off.item())
    print(f"ACC  matcher coarse tail on/off  loss off {loss_off.item():.9e}  on {loss_on.item():.9e}  |diff| / |off| "
          f"{d_loss / abs(loss_off.item()):.3e}")
    rows = []
    for name, g in g_off.items():
        top = g.abs().max().item()
        diff = (g_on[name].double() - g.double()).abs().max().item()
        print(f"ACC  matcher coarse tail on/off  {name:44s} max|g_off| {top:.3e}  max|g_on - g_off| / max|g_off| {diff / top:.3e}")
        rows.append((name, diff, top))
    assert d_loss <= 1e-3 * abs(loss_off.item())
    for name, diff, top in rows:
        assert diff <= 1e-3 * top, (name, diff, top)


def test_eval_after_training_mode_is_the_eval_matcher():
    never = mref.matcher(seed=5, hip_train=False, patches=True).eval()
    m = mref.matcher(seed=5, hip_train=True, hip_train_coarse=True, patches=True)
    assert m.coarse.hip_coarse_tail
    mref.step(m, mref.batch(65, grad=True))                          # a training step ...
    m.load_state_dict(never.state_dict())                            # ... and the weights of before
    img0, img1 = (torch.as_tensor(synth.normal(64, k, (1, 3, mref.HC * 8, mref.WC * 8)), device=DEV) for k in (1, 2))
    m.eval()
    assert not m.coarse.hip_coarse_tail
    want, got = never.match(img0, img1), m.match(img0, img1)
    assert not any(t.requires_grad for t in got)
    for u, v in zip(got, want):
        assert u.shape == v.shape and torch.equal(u, v)
