"""ops.linear_attention (fm_linear_attention_forward / _backward, csrc/linear_attn.hip) and the `hip_attention` switch of the
context layers, on the GPU.

The yardstick is float64 autograd through transformer.linear_attention on the up-cast inputs, on the device
(tests/test_linear_attention_ref.py pins that function to the reference's LinearAttention, gradients included).  For each of
out, dq, dk, dv:
    e_hip = max|hip - ref64| / max|ref64|,   e_ref = the same for float32 torch autograd through transformer.linear_attention
    assert e_hip <= 4 e_ref + FLOOR
- the form of tests/test_gpu_fine_loss.py.  The factor 4 allows another summation order and a recomputed `out` in the
backward; FLOOR is twice the largest e_ref over this file's REGULAR inputs (profiles/linear_attention_accuracy.txt holds
every ACC line these tests print and the figure).  Two kinds of line are left out of that maximum, which makes the floor
smaller, never larger: the `sink` inputs, where the reference's own float32 arithmetic is the weak side (elu(-30) + 1 is
(e^-30 - 1) + 1 = 0 or 6e-8 in float32, not 9.4e-14: e_ref reaches 8.8e-4 there, e_hip stays at 4e-7), and dq / dk at
S = 1, which are O(eps) cancellations (with one source token out = V up to eps, so the exact gradients are ~1e-7 of
float32's rounding of their terms and e_ref is of order 1).  Both kinds are held to the same bar with that floor; the
module-level lines (e_ref up to 4.7e-6 through the float32 GEMMs) likewise."""
import pytest
import torch

from featurematching_amd import _lib, ops, synth, transformer

import linear_attention_ref as lref
import train_layers_yardstick as yard

pytestmark = pytest.mark.gpu

FLOOR = 2 * 1.582e-6        # profiles/linear_attention_accuracy.txt: the largest e_ref over the regular inputs of this file
DEV = "cuda:0"
NAMES = ("out", "dq", "dk", "dv")


def _hip(q, k, v, q_mask=None, kv_mask=None):
    return ops.linear_attention(q, k, v, q_mask=q_mask, kv_mask=kv_mask)


def _case(dims, seed, scale=1.0, sink=False, masked=False, empty_kv=None):
    """(q, k, v, g) float32 on the device and the two masks (bool, or None)"""
    q, k, v, g = (torch.as_tensor(t, device=DEV) for t in lref.inputs(seed, dims, scale, sink))
    qm = km = None
    if masked:
        qm, km = (torch.as_tensor(m, device=DEV) for m in lref.ragged_masks(dims, empty_kv))
    return q, k, v, g, qm, km


def _three(case):
    """(hip, ref32, ref64): each (out, dq, dk, dv)"""
    q, k, v, g, qm, km = case
    as_t = lambda m, dt: None if m is None else m.to(dt)
    hip = lref.autograd(_hip, q, k, v, g, qm, km)
    ref32 = lref.autograd(transformer.linear_attention, q, k, v, g, as_t(qm, torch.float32), as_t(km, torch.float32))
    ref64 = lref.autograd(transformer.linear_attention, q.double(), k.double(), v.double(), g.double(),
                          as_t(qm, torch.float64), as_t(km, torch.float64))
    return hip, ref32, ref64


def _hold(tag, hip, ref32, ref64, names=NAMES):
    """print every figure, then hold every tensor to the bar, at this file's floor"""
    yard.hold(tag, names, hip, ref32, ref64, FLOOR)


def _check(tag, dims, seed, **kw):
    case = _case(dims, seed, **kw)
    hip, ref32, ref64 = _three(case)
    _hold(tag, hip, ref32, ref64)
    return case, hip


# ---- the window route: H = 8, D = 8, 1 <= L, S <= 64 --------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 130])
@pytest.mark.parametrize("ww", [25, 49])
def test_window_sizes(m, ww):
    """one workgroup per sequence: 130 is more than one workgroup, and ragged at any packing up to 128 per workgroup"""
    _check(f"window M{m} L{ww} S{ww}", (m, ww, ww, 8, 8), 100 + m + ww)


@pytest.mark.parametrize("l,s", [(1, 1), (64, 64), (25, 49), (49, 25)])
@pytest.mark.parametrize("masked", [False, True])
def test_window_shapes(l, s, masked):
    """the smallest and the largest window, L != S both ways; q and k at scale 3: both branches of phi, values near
    exp(-10).  Masked: ragged lengths, and sample 1's kv mask all zero - out is 0 there and the gradients finite"""
    dims = (3, l, s, 8, 8)
    (q, k, v, g, qm, km), hip = _check(f"window L{l} S{s} x3" + (" masked" if masked else ""), dims, 200 + l + s, scale=3.0,
                                       masked=masked, empty_kv=1 if masked else None)
    if masked:
        assert not km[1].any() and not hip[0][1].any()
        assert not hip[0][~qm].any() and not hip[1][~qm].any() and not hip[2][~km].any() and not hip[3][~km].any()


@pytest.mark.parametrize("masked", [False, True])
def test_window_underflow(masked):
    """a tenth of the tokens at q, k = -30: phi underflows towards 0 and everything stays finite"""
    _check("window M130 L25 S49 sink" + (" masked" if masked else ""), (130, 25, 49, 8, 8), 300, sink=True, masked=masked,
           empty_kv=7 if masked else None)


def test_window_grid_stride():
    """more sequences than the launch has workgroups (kLaWinGrid = 2048): the grid-stride loop's second round"""
    _check("window M2050 L5 S7", (2050, 5, 7, 8, 8), 310)


# ---- the long route: H = 8, D = 32 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tok", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025])
def test_long_lengths(n_tok):
    """both sides of every power of two up to 1024: the 16-row tile (kLaTile), the 32-row work unit (kLaUnit), the fold's 8
    slices of slabs"""
    _check(f"long N1 L{n_tok} S{n_tok}", (1, n_tok, n_tok, 8, 32), 400 + n_tok)


@pytest.mark.parametrize("l,s", [(33, 700), (700, 33), (300, 300)])
@pytest.mark.parametrize("masked", [False, True])
def test_long_batched(l, s, masked):
    """cross layers between images of different size, ragged masks; q and k at scale 3"""
    dims = (2, l, s, 8, 32)
    (q, k, v, g, qm, km), hip = _check(f"long N2 L{l} S{s} x3" + (" masked" if masked else ""), dims, 500 + l, scale=3.0,
                                       masked=masked)
    if masked:
        assert not hip[0][~qm].any() and not hip[1][~qm].any() and not hip[2][~km].any() and not hip[3][~km].any()


def test_long_underflow_and_empty_kv():
    (q, k, v, g, qm, km), hip = _check("long N2 L300 S300 sink masked", (2, 300, 300, 8, 32), 600, sink=True, masked=True,
                                       empty_kv=1)
    assert not km[1].any() and not hip[0][1].any()
    _check("long N2 L300 S300 sink", (2, 300, 300, 8, 32), 601, sink=True)


def test_long_workload_size():
    """N = 1, L = S = 4800: 150 slabs to fold"""
    _check("long N1 L4800 S4800", (1, 4800, 4800, 8, 32), 700)


def test_long_unit_cap():
    """more than kLaMaxUnits = 256 units of 32 rows (515 here): workgroups take a second and a third unit, the last one ragged"""
    n_tok = 256 * 64 + 65
    _check(f"long N1 L{n_tok} S{n_tok}", (1, n_tok, n_tok, 8, 32), 710)


# ---- determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(130, 49, 49, 8, 8), (1, 4800, 4800, 8, 32)])
def test_same_bits_on_every_call(dims):
    q, k, v, g, qm, km = _case(dims, 800)
    first = lref.autograd(_hip, q, k, v, g)
    second = lref.autograd(_hip, q, k, v, g)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---- refusals ------------------------------------------------------------------------------------------------------
REFUSED = [(2, 30, 30, 8, 16), (2, 30, 30, 4, 32), (2, 65, 49, 8, 8)]


@pytest.mark.parametrize("dims", REFUSED)
def test_unsupported_shapes_raise(dims):
    n, l, s, h, d = dims
    q = torch.zeros(n, l, h, d, device=DEV)
    k = torch.zeros(n, s, h, d, device=DEV)
    assert not ops.linear_attention_supported(q, k)
    with pytest.raises(_lib.FMatchError) as err:
        ops.linear_attention(q, k, k)
    assert err.value.status == _lib.FM_E_UNSUPPORTED
    assert not ops.linear_attention_supported(q.double(), k.double()) and not ops.linear_attention_supported(q.cpu(), k.cpu())


def test_supported_mirrors_the_route_table():
    """la_route of csrc/linear_attn.hip (tests/test_linear_attention_abi.py holds the ABI's statuses for the same shapes)"""
    table = [((1, 1, 1, 8, 8), True), ((3, 64, 64, 8, 8), True), ((3, 25, 49, 8, 8), True), ((2, 64, 65, 8, 8), False),
             ((1, 1, 1, 8, 32), True), ((2, 300, 200, 8, 32), True), ((2, 30, 30, 8, 64), False), ((2, 30, 30, 16, 8), False),
             ((2, 30, 30, 16, 32), False)] + [(dims, False) for dims in REFUSED]
    for (n, l, s, h, d), served in table:
        q, k = torch.empty(n, l, h, d, device=DEV), torch.empty(n, s, h, d, device=DEV)
        assert ops.linear_attention_supported(q, k) is served, (n, l, s, h, d)
    q = torch.empty(2, 30, 8, 32, device=DEV)
    assert not ops.linear_attention_supported(q, torch.empty(3, 30, 8, 32, device=DEV))       # another batch size
    assert not ops.linear_attention_supported(q, torch.empty(2, 30, 8, 8, device=DEV))        # another head size


# ---- the modules ---------------------------------------------------------------------------------------------------
_module, _module_run = yard.module, yard.module_run


@pytest.mark.parametrize("name,d_model,shape0,shape1", [("fine", 64, (130, 49), (130, 49)), ("coarse", 256, (2, 300), (2, 200))])
def test_module_training_step(monkeypatch, name, d_model, shape0, shape1):
    """LocalFeatureTransformer in training mode with hip_attention=True against a float64 copy; e_ref from
    hip_attention=False in float32.  Outputs, input gradients and every parameter's gradient."""
    cfg = {'d_model': d_model, 'nhead': 8, 'layer_names': ['self', 'cross']}
    x0, x1 = (torch.as_tensor(synth.normal(900, i, (*s, d_model)), device=DEV) for i, s in ((1, shape0), (2, shape1)))
    g0, g1 = (torch.as_tensor(synth.normal(900, i, (*s, d_model)), device=DEV) for i, s in ((3, shape0), (4, shape1)))
    calls = yard.count_calls(monkeypatch, "linear_attention")
    names, hip = _module_run(_module(cfg, hip_attention=True), x0, x1, g0, g1, torch.float32)
    assert calls == {"linear_attention": 4}                          # self x 2, cross x 2: every layer call took the HIP op
    _, ref32 = _module_run(_module(cfg), x0, x1, g0, g1, torch.float32)
    assert calls == {"linear_attention": 4}
    _, ref64 = _module_run(_module(cfg, dtype=torch.float64, hip_attention=True), x0, x1, g0, g1, torch.float64)
    assert calls == {"linear_attention": 4}                          # float64 tensors: the torch function
    _hold(f"module {name}", hip, ref32, ref64, names)


@pytest.mark.parametrize("d_model,tokens", [(128, 30), (64, 65)])
def test_module_takes_the_torch_function_for_unsupported_shapes(monkeypatch, d_model, tokens):
    """D = 16, and 65 tokens at D = 8: hip_attention=True computes what hip_attention=False computes, bit for bit"""
    cfg = {'d_model': d_model, 'nhead': 8, 'layer_names': ['self', 'cross']}
    x0, x1 = (torch.as_tensor(synth.normal(910, i, (3, tokens, d_model)), device=DEV) for i in (1, 2))
    calls = yard.count_calls(monkeypatch, "linear_attention")
    _, on = _module_run(_module(cfg, hip_attention=True), x0, x1, x1, x0, torch.float32)
    _, off = _module_run(_module(cfg), x0, x1, x1, x0, torch.float32)
    assert calls == {"linear_attention": 0}
    for a, b in zip(on[:4], off[:4]):
        assert torch.equal(a, b)


# ---- memory --------------------------------------------------------------------------------------------------------
def test_window_route_memory():
    """forward + backward at M = 2000, WW = 49 allocate the four results and nothing of their size besides"""
    dims = (2000, 49, 49, 8, 8)
    q, k, v, g, _, _ = _case(dims, 950)
    lref.autograd(_hip, q[:2], k[:2], v[:2], g[:2])                  # (library loaded, kernels' attributes set)
    # blocks for the results are then cut to size from one cached segment; a fresh segment of its own would round each
    # of them up to a multiple of 2 MiB, which max_memory_allocated counts
    spare = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)
    del spare
    lib = _lib.load()
    state, ws = lib.fm_linear_attention_state_bytes(*dims), lib.fm_linear_attention_workspace_bytes(*dims)
    assert state == 0 and ws == 0
    allowed = q.numel() * 4 + q.numel() * 4 + 2 * k.numel() * 4 + state + ws + 4 * 512     # out, dq, dk, dv
    peak_hip = yard.peak_above_inputs(_hip, (q, k, v), g)
    peak_torch = yard.peak_above_inputs(transformer.linear_attention, (q, k, v), g)
    print(f"MEM  window M2000 WW49  hip {peak_hip} B  allowed {allowed} B  torch {peak_torch} B  "
          f"({peak_torch / max(peak_hip, 1):.2f} x)")
    assert peak_hip <= allowed, (peak_hip, allowed)
