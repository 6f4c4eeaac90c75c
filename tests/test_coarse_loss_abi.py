"""The matrix-free coarse loss through the C ABI without a GPU: the entry points load, refuse bad arguments before
anything launches and size their workspace; and the split the kernels implement (tests/coarse_loss_ref.py) is pinned,
on the CPU in float64, against a fixture written by the reference's own Loss.compute_coarse_loss
(tests/golden/make_golden_coarse_loss.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, synth

import coarse_loss_ref as ref

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_coarse_loss_workspace_bytes", "fm_coarse_loss_forward", "fm_coarse_loss_backward")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything
CASES = {"a": ((12, 16), (12, 16), 64), "b": ((15, 17), (11, 13), 128), "k0": ((12, 16), (12, 16), 64)}
LOSSES = {"focal": ("focal", False), "focal_sparse": ("focal", True), "xent": ("cross_entropy", False)}


def test_symbols_load():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES
    assert lib.fm_version() == 100


def _problem(n=1, l=100, s=90, c=64, t=0.1, pitch_r=128, pitch_c=128, kind=_lib.FM_LOSS_FOCAL, gamma=2.0, k=8, ptr=FAKE,
             ids=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return (ptr, ptr, n, l, s, c, t, ptr, ptr, pitch_r, ptr, ptr, pitch_c, kind, 0.25, gamma, 1.0, 1.0, ids, ids, ids, k, ws,
            ws_bytes)


def _calls(lib):
    return (lambda out=FAKE, **kw: lib.fm_coarse_loss_forward(*_problem(**kw), out, None),
            lambda out=FAKE, **kw: lib.fm_coarse_loss_backward(*_problem(**kw), out, out, out, None))


def test_argument_checks():
    lib = _lib.load()
    for call in _calls(lib):
        assert call(ptr=None) == FM_E_NULL
        assert call(out=None) == FM_E_NULL
        assert call(ws=None) == FM_E_NULL
        assert call(ids=None) == FM_E_NULL                         # K > 0 needs the id lists
        assert call(k=-1) == FM_E_SHAPE
        assert call(k=100 * 90 + 1) == FM_E_SHAPE                  # more distinct entries than the matrix has
        assert call(k=100 * 90 + 1, kind=2) == FM_E_UNSUPPORTED    # ... which is looked at behind the kind
        for bad in (dict(n=0), dict(l=0), dict(s=-3), dict(pitch_r=99), dict(pitch_c=89)):
            assert call(**bad) == FM_E_SHAPE, bad
        for bad in (dict(c=6), dict(c=260), dict(c=0), dict(t=0.0), dict(t=-1.0), dict(kind=2), dict(kind=-1), dict(gamma=0.0),
                    dict(gamma=-2.0)):
            assert call(**bad) == FM_E_UNSUPPORTED, bad
        need = lib.fm_coarse_loss_workspace_bytes(1, 100, 90, 64, 8)
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE
        assert call(ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
        # an empty supervision is a valid call: its NULL id lists get as far as the workspace check
        assert call(k=0, ids=None, ws_bytes=16) == FM_E_WORKSPACE


def test_workspace_bytes():
    lib = _lib.load()
    for bad in ((0, 10, 10, 64, 1), (1, 0, 10, 64, 1), (1, 10, -1, 64, 1), (1, 10, 10, 6, 1), (1, 10, 10, 300, 1),
                (1, 10, 10, 64, -1)):
        assert lib.fm_coarse_loss_workspace_bytes(*bad) == 0, bad
    for n, l, s, c in ((1, 4800, 4800, 256), (2, 255, 143, 128), (64, 4800, 4800, 256), (1, 1, 1, 4)):
        base = lib.fm_dual_softmax_backward_workspace_bytes(n, l, s, c)
        sizes = [lib.fm_coarse_loss_workspace_bytes(n, l, s, c, k) for k in (0, 1, 100, 5000)]
        assert sizes[0] >= base > 0 and sizes[0] == sizes[1]       # K = 0: the stand-in entry's room
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= base + 4 * 5000 * 4
        assert sizes[-1] - base < (1 << 20)                         # nothing of the matrix's size


def _descriptors(hw0, hw1, c, dtype):
    l, s = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1 = synth.coarse_descriptors(19, 2, max(l, s), c, "borderline")
    return (torch.as_tensor(np.ascontiguousarray(f0[:, :l]), dtype=dtype),
            torch.as_tensor(np.ascontiguousarray(f1[:, :s]), dtype=dtype))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "coarse_loss_small.npz"))


@pytest.mark.parametrize("case", list(CASES))
def test_fixture_has_the_cases_it_should(golden, case):
    ids = golden[f"{case}_ids"]
    hw0, hw1, c = CASES[case]
    f0, f1 = _descriptors(hw0, hw1, c, torch.float64)
    assert np.allclose(golden[f"{case}_desc_sums"], [f0.sum().item(), f1.sum().item()], rtol=0, atol=1e-9)
    if case == "k0":
        assert ids.shape == (0, 3)
    else:
        assert len(np.unique(ids, axis=0)) == len(ids) - 5 > 25     # 5 repeated triples
        assert ids[:, 1].max() < f0.shape[1] and ids[:, 2].max() < f1.shape[1]


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("case", list(CASES))
def test_split_and_masked_forms_are_the_references_loss(golden, case, loss):
    """float64, double clamp bounds: what the reference's code computes when handed float64.  Loss and gradients of the
    masked form (the reference's expression restated) and of the split form (what the kernels implement) against the
    reference's own numbers; the float32 loss of the reference is the float64 one to float32 accuracy."""
    hw0, hw1, c = CASES[case]
    kind, sparse = LOSSES[loss]
    ids = torch.as_tensor(golden[f"{case}_ids"])
    want = float(golden[f"{case}_{loss}_loss64"])
    forms = {"masked": lambda conf: ref.masked_loss(conf, ref.gt_mask(conf.shape, *ids.T), kind, sparse=sparse)[0]}
    if not sparse:
        forms["split"] = lambda conf: ref.split_loss(conf, *ids.T, kind)[0]
    for name, fn in forms.items():
        a0, a1 = (t.requires_grad_(True) for t in _descriptors(hw0, hw1, c, torch.float64))
        val = fn(ref.conf_matrix(a0, a1))
        assert abs(val.item() - want) <= 1e-12 * max(abs(want), 1e-3), (name, val.item(), want)
        if val.requires_grad:
            val.backward()
        for got, key in ((a0.grad, "g0"), (a1.grad, "g1")):
            g = torch.as_tensor(golden[f"{case}_{loss}_{key}"]).double()
            got = torch.zeros_like(a0 if key == "g0" else a1) if got is None else got
            scale = max(g.abs().max().item(), 1e-30)
            # (the fixture keeps every 4th row as float32: 6e-8 relative)
            assert (got[:, ::4] - g).abs().max().item() <= 2e-7 * scale, (name, key)
    assert abs(float(golden[f"{case}_{loss}_loss32"]) - want) <= 1e-5 * abs(want) + 1e-12


def test_float32_bounds_are_what_the_float32_reference_clamps_to(golden):
    """the reference run in float32 is closer to its float64 formula with the float32-rounded bounds than to the one with
    double bounds wherever entries sit on the upper bound; here: the bounds themselves"""
    assert ref.HI32 < 1 - 1e-6 and abs(ref.HI32 - 0.99999899) < 1e-8 and abs(ref.LO32 - 1e-6) < 1e-13
    c = torch.clamp(torch.tensor([0.0, 1.0], dtype=torch.float32), 1e-6, 1 - 1e-6)
    assert c[0].item() == ref.LO32 and c[1].item() == ref.HI32


def test_split_form_degenerate_cases():
    """loss.py:37-42 in the split form: no positive (entry (0,0,0) stands in with weight 0 and - neg_mask was taken before -
    stays among the negatives), no negative (weight 0)"""
    g = torch.Generator().manual_seed(2)
    conf = torch.rand(2, 3, 4, generator=g, dtype=torch.float64)
    none = torch.zeros(0, dtype=torch.long)
    for kind in ("focal", "cross_entropy"):
        a = ref.masked_loss(conf, torch.zeros(2, 3, 4, dtype=torch.bool), kind)
        b = ref.split_loss(conf, none, none, none, kind)
        assert abs(a[0].item() - b[0].item()) < 1e-14 and abs(a[2].item() - b[2].item()) < 1e-14
        every = torch.nonzero(torch.ones(2, 3, 4)).T
        a = ref.masked_loss(conf, torch.ones(2, 3, 4, dtype=torch.bool), kind)
        b = ref.split_loss(conf, *every, kind)
        assert abs(a[0].item() - b[0].item()) < 1e-14
