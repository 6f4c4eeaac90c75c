"""ops.full_attention (fm_full_attention_forward / _backward, csrc/full_attn.hip) and the 'full' attention core of the
context layers, on the GPU.

The yardstick is float64 autograd through transformer.full_attention on the up-cast inputs, on the device
(tests/test_full_attention_ref.py pins that function to the reference's FullAttention, gradients included).  For each of
out, dq, dk, dv:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through transformer.full_attention
    assert e_hip <= 4 e_ref + FLOOR
(train_layers_yardstick.hold).  FLOOR is twice the largest e_ref over this file's REGULAR lines - plain normals at scale 1
and 3 (profiles/full_attention_accuracy.txt holds every ACC line these tests print and the figure); the `shifted` and ramp
lines are left out of that maximum, which can only make the floor smaller.  It comes from torch's float32 path, not from
the kernels.  At S = 1 the exact dq and dk are zero (p = 1, dS = 0), so those two tensors are held by absolute error, to
FLOOR times the natural size of the terms that cancel.

The kernels' own sizes (csrc/full_attn.hip): tiles of 32 tokens on either side; a sweep's launch has at most 2^20
workgroups of one wave (N * 8 * ceil(L or S / 32) units, the rest by grid stride), k_fa_delta's at most 4096 of 256 threads
(N * L * 8 rows): N = 2^17 at L = 2 is the last batch below both caps, 2^17 + 1 the first above."""
import ctypes as C

import pytest
import torch

from featurematching_amd import _lib, ops, synth, transformer

import full_attention_ref as fref
import train_layers_yardstick as yard

pytestmark = pytest.mark.gpu

FLOOR = 2 * 2.337e-6        # profiles/full_attention_accuracy.txt: the largest e_ref over the regular lines of this file
DEV = "cuda:0"
NAMES = ("out", "dq", "dk", "dv")


def _hip(q, k, v, q_mask=None, kv_mask=None):
    return ops.full_attention(q, k, v, q_mask=q_mask, kv_mask=kv_mask)


def _case(dims, seed, scale=1.0, kind=None):
    """(q, k, v, g) float32 on the device"""
    data = fref.inputs(seed, dims, scale) if kind is None else fref.hard_inputs(kind, seed, dims)
    return tuple(torch.as_tensor(t, device=DEV) for t in data)


def _three(case):
    """(hip, ref32, ref64): each (out, dq, dk, dv)"""
    q, k, v, g = case
    hip = fref.autograd(_hip, q, k, v, g)
    ref32 = fref.autograd(transformer.full_attention, q, k, v, g)
    ref64 = fref.autograd(transformer.full_attention, q.double(), k.double(), v.double(), g.double())
    return hip, ref32, ref64


def _check(tag, dims, seed, **kw):
    case = _case(dims, seed, **kw)
    hip, ref32, ref64 = _three(case)
    if dims[2] > 1:
        yard.hold(tag, NAMES, hip, ref32, ref64, FLOOR)
        return case, hip
    # S = 1: out and dv to the bar; dq and dk, exactly 0, by absolute error
    pick = lambda t: (t[0], t[3])
    yard.hold(tag, ("out", "dv"), pick(hip), pick(ref32), pick(ref64), FLOOR)
    q, k, v, g = case
    top = lambda t: t.abs().max().item()
    for name, got, ref, other in (("dq", hip[1], ref64[1], k), ("dk", hip[2], ref64[2], q)):
        bound = FLOOR * top(g) * top(v) * top(other) / dims[4] ** .5
        print(f"ACC  {tag:34s} {name:22s} max|ref64| {top(ref):.3e}  max|hip| {top(got):.3e}  bound {bound:.3e}")
        assert top(ref) == 0 and bool(torch.isfinite(got).all()) and top(got) <= bound, (tag, name, top(got), bound)
    return case, hip


# ---- lengths and shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 32])
@pytest.mark.parametrize("n_tok", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_lengths(n_tok, d):
    """both sides of every multiple of the 32-token tile up to 64, and of 128 and 256; one key alone"""
    _check(f"D{d} N2 L{n_tok} S{n_tok}", (2, n_tok, n_tok, 8, d), 400 + n_tok + d)


@pytest.mark.parametrize("d", [8, 32])
@pytest.mark.parametrize("l,s", [(33, 700), (700, 33), (25, 49), (49, 25), (5, 1)])
def test_cross_shapes(l, s, d):
    """L != S both ways: a cross layer between images of different size"""
    _check(f"D{d} N2 L{l} S{s}", (2, l, s, 8, d), 500 + l + d)


@pytest.mark.parametrize("d", [8, 32])
@pytest.mark.parametrize("ww", [25, 49])
def test_fine_windows(ww, d):
    _check(f"D{d} N130 L{ww} S{ww}", (130, ww, ww, 8, d), 520 + ww + d)


@pytest.mark.parametrize("n", [70000, 1 << 17, (1 << 17) + 1])
def test_batch_beyond_a_grid_dimension(n):
    """more samples than a grid's y or z may have, and either side of both launch caps (the grid-stride loops' second round)"""
    _check(f"D8 N{n} L2 S3", (n, 2, 3, 8, 8), 530)


@pytest.mark.parametrize("d", [8, 32])
@pytest.mark.parametrize("l,s", [(130, 97), (300, 300)])
def test_scale_3(l, s, d):
    """q and k at scale 3: scores of a few tens, probabilities from 1 down to underflow"""
    _check(f"D{d} N2 L{l} S{s} x3", (2, l, s, 8, d), 540 + l + d, scale=3.0)


@pytest.mark.parametrize("d", [8, 32])
@pytest.mark.parametrize("dims", [(2, 130, 97), (1, 300, 300)])
@pytest.mark.parametrize("kind", fref.KINDS)
def test_hard_inputs(kind, dims, d):
    """scores that overflow exp without the maximum subtracted; a maximum that rises through the whole sweep; one that
    sits in the first tile (full_attention_ref.hard_inputs)"""
    n, l, s = dims
    _, hip = _check(f"D{d} N{n} L{l} S{s} {kind}", (n, l, s, 8, d), 560 + l + d, kind=kind)


# ---- determinism ---------------------------------------------------------------------------------------------------
SAME_BITS = [(130, 49, 49, 8, 8), (2, 700, 300, 8, 32)]


@pytest.mark.parametrize("dims", SAME_BITS)
def test_same_bits_on_every_call(dims):
    q, k, v, g = _case(dims, 800)
    first = fref.autograd(_hip, q, k, v, g)
    second = fref.autograd(_hip, q, k, v, g)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def _abi(case, fill):
    """forward + backward through ctypes with the workspace, state and every output prefilled with `fill` bytes"""
    q, k, v, g = case
    n, l, h, d = q.shape
    dims = (n, l, k.shape[1], h, d)
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    buf = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    like = lambda t: torch.full((t.numel() * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(t.shape)
    need, state_bytes = lib.fm_full_attention_workspace_bytes(*dims), lib.fm_full_attention_state_bytes(*dims)
    assert need > 0 and state_bytes > 0
    ws, state = buf(need + 256), buf(state_bytes).view(torch.float32)
    wsp = C.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    out, dq, dk, dv = like(q), like(q), like(k), like(k)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.fm_full_attention_forward(p(q), p(k), p(v), *dims, wsp, need, p(state), p(out), st), "forward")
    ws.fill_(fill)                                   # nothing is kept in it between the calls
    _lib.check(lib.fm_full_attention_backward(p(q), p(k), p(v), p(out), p(g), p(state), *dims, wsp, need, p(dq), p(dk), p(dv),
                                              st), "backward")
    torch.cuda.synchronize()
    return out, dq, dk, dv, state[:n * l * h]


@pytest.mark.parametrize("dims", [(5, 49, 25, 8, 8), (2, 70, 45, 8, 32)])
def test_same_bits_whatever_the_memory_held(dims):
    """every output element is written and no region of the workspace is read before it is written: 0xFF bytes (NaNs) in
    the workspace, the state and the outputs leave the bits of a call on zeroed buffers, and those of the op"""
    case = _case(dims, 810)
    clean, dirty = _abi(case, 0), _abi(case, 0xFF)
    for name, a, b in zip(NAMES + ("state",), clean, dirty):
        assert torch.equal(a, b), name
        assert bool(torch.isfinite(b).all()), name
    for name, a, b in zip(NAMES, fref.autograd(_hip, *case), dirty):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("dims", SAME_BITS)
def test_side_stream_and_graph_replay(dims):
    """forward + backward on a non-default stream, and captured once on that stream and replayed twice (the second time on
    other inputs and back): the default stream's bits.  The capture is of one stream and holds kernel launches only, each
    ordered behind the one before: a chain, no parallel branches."""
    sets = [_case(dims, 820), _case(dims, 821, scale=3.0)]
    want = [fref.autograd(_hip, *s) for s in sets]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    q, k, v, g = (t.clone() for t in sets[0])
    q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)

    def step():
        out = ops.full_attention(q, k, v)
        return (out,) + torch.autograd.grad(out, (q, k, v), g)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]
    side.synchronize()
    for name, a, b in zip(NAMES, eager, want[0]):
        assert torch.equal(a, b), ("side stream", name)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = step()
    got = []
    with torch.cuda.stream(side):
        for i in (0, 1, 0):
            with torch.no_grad():
                for dst, src in zip((q, k, v, g), sets[i]):
                    dst.copy_(src)
            graph.replay()
            got.append((i, [t.detach().clone() for t in res]))
    side.synchronize()
    for r, (i, tensors) in enumerate(got):
        for name, a, b in zip(NAMES, tensors, want[i]):
            assert torch.equal(a, b), ("replay", r, name)
    assert not torch.equal(want[0][0], want[1][0])


def test_inference_call():
    """under no_grad the op hands a NULL state and saves nothing: the same `out` bits"""
    for dims in SAME_BITS:
        q, k, v, g = _case(dims, 830)
        with_grad = fref.autograd(_hip, q, k, v, g)[0]
        with torch.no_grad():
            out = ops.full_attention(q, k, v)
        assert out.grad_fn is None and torch.equal(out, with_grad)
        plain = ops.full_attention(q, k, v)                          # grad mode on, nothing requires grad
        assert plain.grad_fn is None and torch.equal(plain, with_grad)


# ---- refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 30, 30, 4, 32), (2, 30, 30, 8, 16)])
def test_unsupported_shapes_raise(dims):
    n, l, s, h, d = dims
    q = torch.zeros(n, l, h, d, device=DEV)
    k = torch.zeros(n, s, h, d, device=DEV)
    assert not ops.full_attention_supported(q, k)
    with pytest.raises(_lib.FMatchError) as err:
        ops.full_attention(q, k, k)
    assert err.value.status == _lib.FM_E_UNSUPPORTED


def test_supported_and_masks():
    for (n, l, s, h, d), served in (((1, 1, 1, 8, 8), True), ((3, 25, 49, 8, 8), True), ((2, 300, 200, 8, 32), True),
                                    ((70000, 2, 3, 8, 8), True), ((2, 30, 30, 8, 64), False), ((2, 30, 30, 16, 8), False)):
        q, k = torch.empty(n, l, h, d, device=DEV), torch.empty(n, s, h, d, device=DEV)
        assert ops.full_attention_supported(q, k) is served, (n, l, s, h, d)
    q = torch.zeros(2, 30, 8, 32, device=DEV)
    assert not ops.full_attention_supported(q, torch.empty(3, 30, 8, 32, device=DEV))         # another batch size
    assert not ops.full_attention_supported(q.double(), q.double()) and not ops.full_attention_supported(q.cpu(), q.cpu())
    mask = torch.ones(2, 30, device=DEV)
    for kw in (dict(q_mask=mask), dict(kv_mask=mask), dict(q_mask=mask, kv_mask=mask)):
        with pytest.raises(ValueError):
            ops.full_attention(q, q, q, **kw)


# ---- the modules ---------------------------------------------------------------------------------------------------
MODULES = [("fine", 64, (130, 49), (130, 49)), ("coarse", 256, (2, 300), (2, 200))]


def _cfg(d_model):
    return {'d_model': d_model, 'nhead': 8, 'layer_names': ['self', 'cross'], 'attention': 'full'}


def _features(seed, d_model, shape0, shape1):
    return tuple(torch.as_tensor(synth.normal(seed, i, (*s, d_model)), device=DEV)
                 for i, s in ((1, shape0), (2, shape1), (3, shape0), (4, shape1)))


@pytest.mark.parametrize("name,d_model,shape0,shape1", MODULES)
def test_module_training_step(monkeypatch, name, d_model, shape0, shape1):
    """LocalFeatureTransformer(attention='full') in training mode with hip_attention=True against a float64 copy; e_ref
    from hip_attention=False in float32.  Outputs, input gradients and every parameter's gradient.  At d_model 64 once more
    with the HIP tail and the HIP projections around the core."""
    cfg = _cfg(d_model)
    x0, x1, g0, g1 = _features(900, d_model, shape0, shape1)
    calls = yard.count_calls(monkeypatch, "full_attention")
    names, hip = yard.module_run(yard.module(cfg, hip_attention=True), x0, x1, g0, g1, torch.float32)
    assert calls == {"full_attention": 4}                            # self x 2, cross x 2: every layer call took the HIP op
    _, ref32 = yard.module_run(yard.module(cfg), x0, x1, g0, g1, torch.float32)
    assert calls == {"full_attention": 4}
    _, ref64 = yard.module_run(yard.module(cfg, dtype=torch.float64, hip_attention=True), x0, x1, g0, g1, torch.float64)
    assert calls == {"full_attention": 4}                            # float64 tensors: the torch function
    yard.hold(f"module {name} full", names, hip, ref32, ref64, FLOOR)
    if d_model == 64:
        _, all_on = yard.module_run(yard.module(cfg, hip_attention=True, hip_tail=True, hip_proj=True), x0, x1, g0, g1,
                                    torch.float32)
        assert calls == {"full_attention": 8}
        yard.hold(f"module {name} full tail proj", names, all_on, ref32, ref64, FLOOR)


@pytest.mark.parametrize("name,d_model,shape0,shape1", MODULES)
def test_module_eval(monkeypatch, name, d_model, shape0, shape1):
    """eval mode under no_grad: use_hip=True (the default) takes the op in all four layer calls and meets the bar;
    use_hip=False, or padding masks, never call it and give the torch layers' bits"""
    cfg = _cfg(d_model)
    x0, x1, _, _ = _features(910, d_model, shape0, shape1)
    ones0, ones1 = (torch.ones(t.shape[:2], dtype=torch.bool, device=DEV) for t in (x0, x1))
    calls = yard.count_calls(monkeypatch, "full_attention")
    with torch.no_grad():
        hip = yard.module(cfg).eval()(x0, x1)
        assert calls == {"full_attention": 4}
        off = yard.module(cfg, use_hip=False).eval()
        ref32 = off(x0, x1)
        masked_off = off(x0, x1, ones0, ones1)
        masked_on = yard.module(cfg).eval()(x0, x1, ones0, ones1)
        masked_switch = yard.module(cfg, hip_attention=True).eval()(x0, x1, ones0, ones1)
        ref64 = yard.module(cfg, dtype=torch.float64).eval()(x0.double(), x1.double())
        assert calls == {"full_attention": 4}
    for a, b, c in zip(masked_off, masked_on, masked_switch):
        assert torch.equal(a, b) and torch.equal(a, c)
    yard.hold(f"module {name} full eval", ("out0", "out1"), hip, ref32, ref64, FLOOR)


# ---- memory --------------------------------------------------------------------------------------------------------
def test_memory_is_not_of_order_l_times_s():
    """forward + backward at (1, 2400, 2400, 8, 32) allocate the four results, the state and the workspace: about 10 MB,
    where the scores alone are 184 MB"""
    dims = (1, 2400, 2400, 8, 32)
    q, k, v, g = _case(dims, 950)
    fref.autograd(_hip, q[:, :64], k[:, :64], v[:, :64], g[:, :64])  # (library loaded)
    # blocks for the results are then cut to size from one cached segment; a fresh segment of its own would round each
    # of them up to a multiple of 2 MiB, which max_memory_allocated counts
    spare = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)
    del spare
    lib = _lib.load()
    state, ws = lib.fm_full_attention_state_bytes(*dims), lib.fm_full_attention_workspace_bytes(*dims)
    assert state > 0 and ws > 0
    allowed = 2 * q.numel() * 4 + 2 * k.numel() * 4 + state + ws + (1 << 20)     # out, dq, dk, dv
    peak_hip = yard.peak_above_inputs(_hip, (q, k, v), g)
    peak_torch = yard.peak_above_inputs(transformer.full_attention, (q, k, v), g)
    print(f"MEM  full N1 L2400 S2400 D32  hip {peak_hip} B  allowed {allowed} B  torch {peak_torch} B  "
          f"({peak_torch / max(peak_hip, 1):.1f} x)")
    assert peak_hip <= allowed, (peak_hip, allowed)
