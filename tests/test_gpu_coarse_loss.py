"""The matrix-free coarse loss on the GPU (ops.coarse_loss, modules.CoarseLoss; fm_coarse_loss_forward / _backward):
gradients against float64 autograd through the reference's own expression (coarse_matching_new.py:64-68, then
losses/loss.py:27-67 - restated in tests/coarse_loss_ref.py and pinned there against the reference), the loss value
against the float64 formula with the float32-rounded clamp bounds, the allocator bound, today's conf_matrix route, the
drop-in modules and the edges.

Loss bar (FLOOR): |loss_hip - loss64| <= 4 e_ref + FLOOR |loss64| with e_ref = |loss_ref32 - loss64| of the reference's
expression evaluated by torch in float32 on the same input; FLOOR = twice the largest e_ref / |loss64| measured over this
file's inputs (profiles/coarse_loss_accuracy.txt)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from featurematching_amd import modules, ops, synth

import coarse_loss_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2 * 1.6e-7          # profiles/coarse_loss_accuracy.txt: the largest e_ref / |loss64| of the loss over the cases below
KINDS = ("focal", "cross_entropy")
SMALL = {"a": ((12, 16), (12, 16), 64, "borderline"), "b": ((15, 17), (11, 13), 128, "borderline")}
CASES = {**SMALL, "pair640": ((60, 80), (60, 80), 256, "borderline"), "peaky": ((12, 16), (12, 16), 64, "peaky")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarse_loss_small.npz")
CFG = {'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(f0, f1 numpy float32, ids int64 [K, 3] on the device with repeated triples, hw0, hw1)"""
    hw0, hw1, c, dist = CASES[case]
    l, s = hw0[0] * hw0[1], hw1[0] * hw1[1]
    n, seed = (1, 23) if case == "pair640" else (2, 19)
    f0, f1 = synth.coarse_descriptors(seed, n, max(l, s), c, dist)
    f0, f1 = np.ascontiguousarray(f0[:, :l]), np.ascontiguousarray(f1[:, :s])
    if case in SMALL:
        ids = torch.as_tensor(np.load(GOLDEN)[f"{case}_ids"], device=DEV)
    else:      # every third match the matcher found + random triples + 5 repeats
        out = ops.coarse_match(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV), hw0, hw1, 8.0)
        g = torch.Generator().manual_seed(41)
        k = 500 if case == "pair640" else 20
        rnd = torch.stack([torch.randint(n, (k,), generator=g), torch.randint(l, (k,), generator=g),
                           torch.randint(s, (k,), generator=g)], 1).to(DEV)
        ids = torch.cat([torch.stack([out['b_ids'][::3], out['i_ids'][::3], out['j_ids'][::3]], 1), rnd], 0)
        ids = torch.cat([ids, ids[:5]], 0)
        assert ids.shape[0] > k + 5 + 10          # the matcher found something
    return f0, f1, ids.contiguous(), hw0, hw1


@functools.lru_cache(maxsize=None)
def _reference(case, kind):
    """float64 with the float32-rounded bounds: (loss64, pos mean, neg mean, d_feat0, d_feat1), and the float32
    evaluation's three numbers.  The float64 gradients do not depend on which of the two bound pairs is used unless an
    entry lies between them."""
    f0, f1, ids, _, _ = _inputs(case)
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    conf = ref.conf_matrix(b0, b1)
    mask = ref.gt_mask(conf.shape, *ids.T)
    l64 = ref.masked_loss(conf, mask, kind, lo=ref.LO32, hi=ref.HI32)
    l64[0].backward()
    del conf
    with torch.no_grad():
        c32 = ref.conf_matrix(torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV))
        l32 = ref.masked_loss(c32, mask, kind)
    return tuple(v.item() for v in l64) + (b0.grad, b1.grad), tuple(v.item() for v in l32)


def _leaves(case, dtype=torch.float32):
    f0, f1 = _inputs(case)[:2]
    return (torch.as_tensor(f0, device=DEV, dtype=dtype).requires_grad_(True),
            torch.as_tensor(f1, device=DEV, dtype=dtype).requires_grad_(True))


def _hip(case, kind, scale=1.0, ids=None, leaves=None, **kw):
    """(loss tensor, d_feat0, d_feat1) of ops.coarse_match(stats=True) + ops.coarse_loss + backward"""
    _, _, spv, hw0, hw1 = _inputs(case)
    ids = spv if ids is None else ids
    a0, a1 = leaves or _leaves(case)
    out = ops.coarse_match(a0.detach(), a1.detach(), hw0, hw1, 8.0, stats=True)
    loss = ops.coarse_loss(a0, a1, ids[:, 0], ids[:, 1], ids[:, 2], out['_coarse_buffers'], kind, **kw)
    (scale * loss).backward()
    return loss, a0.grad, a1.grad


def _assert_loss(case, kind, what, got, want, e_ref):
    print(f"ACC {case:8s} {kind:13s} {what:9s} loss64 {want:.9e}  e_ref/|loss64| {e_ref / abs(want):.3e}  "
          f"e_hip/|loss64| {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= 4 * e_ref + FLOOR * abs(want), (case, kind, what, got, want, e_ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["a", "b", "pair640"])
def test_gradients_match_float64_autograd_through_the_references_expression(case, kind):
    """max|got - ref| <= 2e-4 max|ref| per image: the bar of the dense-gradient test of test_gpu_parity.py"""
    (_, _, _, r0, r1), _ = _reference(case, kind)
    _, d0, d1 = _hip(case, kind)
    for name, got, want in (("d_feat0", d0, r0), ("d_feat1", d1, r1)):
        scale = want.abs().max().item()
        err = (got.double() - want).abs().max().item()
        print(f"GRAD {case:8s} {kind:13s} {name} max|ref| {scale:.3e} err/max|ref| {err / scale:.3e}")
        assert scale > 1e-6 and err <= 2e-4 * scale, (case, kind, name, err, scale)


@pytest.mark.parametrize("kind", KINDS)
def test_peaky_descriptors_every_entry_outside_the_clamp_gives_exactly_zero_gradients(kind):
    (_, _, _, r0, r1), _ = _reference("peaky", kind)
    assert r0.abs().max().item() == 0 and r1.abs().max().item() == 0
    _, d0, d1 = _hip("peaky", kind)
    assert d0.abs().max().item() == 0 and d1.abs().max().item() == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_loss_value_against_float64_with_float32_bounds(case, kind):
    (l64, p64, n64, _, _), (l32, p32, n32) = _reference(case, kind)
    loss, _, _ = _hip(case, kind)
    pos, neg = (v.item() for v in loss.means)
    _assert_loss(case, kind, "loss", loss.item(), l64, abs(l32 - l64))
    _assert_loss(case, kind, "pos_mean", pos, p64, abs(p32 - p64))
    _assert_loss(case, kind, "neg_mean", neg, n64, abs(n32 - n64))
    if case in SMALL:       # the reference's own float32 number in place of torch's evaluation here
        l32_fix = float(np.load(GOLDEN)[f"{case}_{'focal' if kind == 'focal' else 'xent'}_loss32"])
        _assert_loss(case, kind, "fixture32", loss.item(), l64, abs(l32_fix - l64))


@pytest.mark.parametrize("kind", KINDS)
def test_no_LxS_array_from_the_coarse_call_to_the_gradients(kind):
    """from before ops.coarse_match(stats=True) to after backward(): the condition of the dense-gradient test of
    test_gpu_parity.py at this size"""
    leaves = _leaves("pair640")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, d0, d1 = _hip("pair640", kind, leaves=leaves)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    l = 4800
    assert peak < 0.5 * l * l * 4, f"coarse call + loss + backward allocated {peak / 1e6:.0f} MB ([L, S] is {l * l * 4 / 1e6:.0f} MB)"
    assert torch.isfinite(loss) and d0.abs().max().item() > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(SMALL))
def test_same_answer_as_the_conf_matrix_route(case, kind):
    """loss and gradients against attach_conf_matrix_grad + the torch loss on the HIP conf_matrix"""
    f0, f1, ids, hw0, hw1 = _inputs(case)
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    out = ops.coarse_match(a0.detach(), a1.detach(), hw0, hw1, 8.0, conf_matrix=True)
    conf = ops.attach_conf_matrix_grad(a0, a1, out['conf_matrix'], 0.1, out['_coarse_buffers'])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        old = ref.masked_loss(conf, ref.gt_mask(conf.shape, *ids.T), kind)[0]
        old.backward()
    loss, d0, d1 = _hip(case, kind)
    assert abs(loss.item() - old.item()) <= 2e-6 * abs(old.item())
    for got, want in ((d0, a0.grad), (d1, a1.grad)):
        scale = want.abs().max().item()
        assert scale > 1e-6 and (got - want).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("kind", KINDS)
def test_modules_train_without_conf_matrix_and_conf_matrix_gt(kind):
    f0, f1, ids, hw0, hw1 = _inputs("a")
    fixture = np.load(GOLDEN)
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    spv = dict(spv_b_ids=ids[:, 0].contiguous(), spv_i_ids=ids[:, 1].contiguous(), spv_j_ids=ids[:, 2].contiguous())
    hw_i = (hw0[0] * 8, hw0[1] * 8)
    data = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw0, hw1_c=hw1, **spv)
    modules.CoarseMatching(CFG, loss_stats=True).train()(a0, a1, data)
    assert 'conf_matrix' not in data and 'conf_matrix_gt' not in data
    loss = modules.CoarseLoss({'coarse_type': kind, 'focal_alpha': 0.25, 'focal_gamma': 2.0, 'pos_weight': 1.0,
                               'neg_weight': 1.0})(data)
    loss.backward()
    want = float(fixture[f"a_{'focal' if kind == 'focal' else 'xent'}_loss64"])
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    assert a0.grad is not None and a1.grad is not None and a0.grad.abs().max().item() > 0 and a1.grad.abs().max().item() > 0
    with pytest.raises(RuntimeError):
        modules.CoarseMatching(CFG).train()(a0, a1, dict(data))


def test_sparse_supervision_goes_through_dual_softmax_at():
    f0, f1, ids, hw0, hw1 = _inputs("a")
    fixture = np.load(GOLDEN)
    a0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    a1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    hw_i = (hw0[0] * 8, hw0[1] * 8)
    data = dict(hw0_i=hw_i, hw1_i=hw_i, hw0_c=hw0, hw1_c=hw1, spv_b_ids=ids[:, 0].contiguous(),
                spv_i_ids=ids[:, 1].contiguous(), spv_j_ids=ids[:, 2].contiguous())
    modules.CoarseMatching(CFG, loss_stats=True).train()(a0, a1, data)
    loss = modules.CoarseLoss({'coarse_type': 'focal', 'focal_alpha': 0.25, 'focal_gamma': 2.0, 'pos_weight': 1.0,
                               'neg_weight': 1.0}, sparse_spvs=True)(data)
    loss.backward()
    n, l, c = a0.shape
    want = float(fixture["a_focal_sparse_loss64"])
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    # the same numbers as calling dual_softmax_at on the distinct entries directly
    b0 = torch.as_tensor(f0, device=DEV).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV).requires_grad_(True)
    d = ref.distinct(ids[:, 0], ids[:, 1], ids[:, 2], l, a1.shape[1])
    p = torch.clamp(ops.dual_softmax_at(b0, b1, *d, data['_fm_coarse_loss'][0]), 1e-6, 1 - 1e-6)
    direct = (-0.25 * torch.pow(1 - p, 2.0) * p.log()).mean()
    direct.backward()
    assert loss.item() == direct.item()
    assert (a0.grad - b0.grad).abs().max().item() <= 1e-6 * b0.grad.abs().max().item()
    # at the 640x480 pair: nothing of the matrix's size from the loss call to the gradients
    g0, g1, spv, hw0, hw1 = _inputs("pair640")
    c0 = torch.as_tensor(g0, device=DEV).requires_grad_(True)
    c1 = torch.as_tensor(g1, device=DEV).requires_grad_(True)
    out = ops.coarse_match(c0.detach(), c1.detach(), hw0, hw1, 8.0, stats=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.coarse_loss(c0, c1, spv[:, 0], spv[:, 1], spv[:, 2], out['_coarse_buffers'], 'focal', sparse_spvs=True).backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 0.5 * 4800 * 4800 * 4
    assert c0.grad.abs().max().item() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_the_same_bits_of_loss(kind):
    for case in ("b", "pair640"):
        a, _, _ = _hip(case, kind)
        b, _, _ = _hip(case, kind)
        assert a.item() == b.item() and torch.equal(a.means, b.means)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_supervision(kind):
    """loss.py:37-39: entry (0, 0, 0) stands in with weight 0; against the fixture's K = 0 case and float64 autograd"""
    none = torch.zeros(0, 3, dtype=torch.int64, device=DEV)
    loss, d0, d1 = _hip("a", kind, ids=none)
    want = float(np.load(GOLDEN)[f"k0_{'focal' if kind == 'focal' else 'xent'}_loss64"])
    assert abs(loss.item() - want) <= 1e-4 * abs(want)        # (the reference's own float32 loss is 8e-6 from this float64 one)
    grads = {}
    for dt in (torch.float64, torch.float32):
        b0, b1 = _leaves("a", dt)
        conf = ref.conf_matrix(b0, b1)
        val = ref.masked_loss(conf, torch.zeros_like(conf, dtype=torch.bool), kind, lo=ref.LO32, hi=ref.HI32)[0]
        val.backward()
        grads[dt] = (val.item(), b0.grad.double(), b1.grad.double())
    l64 = grads[torch.float64][0]
    assert abs(loss.item() - l64) <= 4 * abs(grads[torch.float32][0] - l64) + FLOOR * abs(l64)
    # Every term of this gradient is a negative's, 1 / (1 - c) at the matches: a float32 conf near 1 moves it by
    # eps / (1 - c), whoever computes it.  The bar is therefore the reference's own float32 error on this input (times 4,
    # as for the loss) where that is above the 2e-4 of the other cases.
    for got, r, r32 in zip((d0, d1), grads[torch.float64][1:], grads[torch.float32][1:]):
        scale = r.abs().max().item()
        e_ref = (r32 - r).abs().max().item()
        err = (got.double() - r).abs().max().item()
        print(f"K0 {kind:13s} max|ref| {scale:.3e} e_ref32/max|ref| {e_ref / scale:.3e} err/max|ref| {err / scale:.3e}")
        assert scale > 1e-6 and err <= max(2e-4 * scale, 4 * e_ref)


@pytest.mark.parametrize("kind", KINDS)
def test_all_supervised_entries_in_one_row(kind):
    """every positive shares row 7 of sample 1 (their v contributions meet in one float atomic target)"""
    f0, f1, _, hw0, hw1 = _inputs("b")
    s = hw1[0] * hw1[1]
    ids = torch.stack([torch.ones(40, dtype=torch.int64), torch.full((40,), 7), torch.arange(0, 3 * 40, 3) % s], 1).to(DEV)
    loss, d0, d1 = _hip("b", kind, ids=ids)
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    conf = ref.conf_matrix(b0, b1)
    l64 = ref.masked_loss(conf, ref.gt_mask(conf.shape, *ids.T), kind, lo=ref.LO32, hi=ref.HI32)[0]
    l64.backward()
    assert abs(loss.item() - l64.item()) <= 2e-6 * abs(l64.item())
    for got, r in ((d0, b0.grad), (d1, b1.grad)):
        scale = r.abs().max().item()
        assert scale > 1e-6 and (got.double() - r).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("kind", KINDS)
def test_upstream_gradient_and_id_formats(kind):
    """(3 * loss).backward() triples the gradients; int32 ids and non-contiguous ids give the same loss and gradients"""
    _, _, ids, _, _ = _inputs("b")
    loss, d0, d1 = _hip("b", kind)
    _, t0, t1 = _hip("b", kind, scale=3.0)
    for one, three in ((d0, t0), (d1, t1)):
        assert (three - 3 * one).abs().max().item() <= 2e-6 * three.abs().max().item()
    wide = torch.zeros(ids.shape[0], 6, dtype=torch.int64, device=DEV)
    wide[:, ::2] = ids
    for other in (ids.to(torch.int32), wide[:, ::2]):
        assert not (other.dtype == torch.int64 and other[:, 1].is_contiguous())
        l2, e0, e1 = _hip("b", kind, ids=other)
        assert l2.item() == loss.item()
        assert (e0 - d0).abs().max().item() <= 2e-6 * d0.abs().max().item()
        assert (e1 - d1).abs().max().item() <= 2e-6 * d1.abs().max().item()


def test_general_gamma_matches_float64():
    """gamma = 1.5 takes the exp2(gamma log2 x) form"""
    f0, f1, ids, _, _ = _inputs("a")
    loss, d0, d1 = _hip("a", "focal", gamma=1.5, alpha=0.4, pos_weight=2.0, neg_weight=0.5)
    b0 = torch.as_tensor(f0, device=DEV, dtype=torch.float64).requires_grad_(True)
    b1 = torch.as_tensor(f1, device=DEV, dtype=torch.float64).requires_grad_(True)
    conf = ref.conf_matrix(b0, b1)
    l64 = ref.masked_loss(conf, ref.gt_mask(conf.shape, *ids.T), "focal", 0.4, 1.5, 2.0, 0.5, lo=ref.LO32, hi=ref.HI32)[0]
    l64.backward()
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())
    for got, r in ((d0, b0.grad), (d1, b1.grad)):
        scale = r.abs().max().item()
        assert scale > 1e-6 and (got.double() - r).abs().max().item() <= 2e-4 * scale
