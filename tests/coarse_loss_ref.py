"""Plain-torch statements of the reference's coarse loss (losses/loss.py:27-67) for the tests of ops.coarse_loss.

`masked_loss` is the reference's expression itself (two boolean masks over the whole conf_matrix), `split_loss` the form
the HIP kernels implement (include/fmatch.h, fm_coarse_loss_forward): the negatives' term summed over EVERY entry, a
sparse correction at the distinct supervised entries.  Both take the clamp bounds as arguments: the reference's float32
clamp uses the float32 roundings of 1e-6 and 1 - 1e-6 (LO32, HI32; HI32 is 0.99999899, not 0.999999), handed a float64
conf it uses the doubles.  tests/test_coarse_loss_abi.py pins both against a fixture written by the reference's own
Loss.compute_coarse_loss."""
import numpy as np
import torch

LO32 = float(np.float32(1e-6))
HI32 = float(np.float32(1 - 1e-6))


def conf_matrix(f0, f1, temperature=0.1):
    """coarse_matching_new.py:64-68 (the descriptors are divided by sqrt(C) each, the similarity by the temperature)"""
    c = f0.shape[-1]
    sim = torch.einsum("nlc,nsc->nls", f0 / c ** .5, f1 / c ** .5) / temperature
    return torch.softmax(sim, 1) * torch.softmax(sim, 2)


def terms(c, kind, alpha=0.25, gamma=2.0):
    """(l_pos, l_neg) of a clamped conf"""
    if kind == 'cross_entropy':
        return -torch.log(c), -torch.log(1 - c)
    return -alpha * torch.pow(1 - c, gamma) * c.log(), -alpha * torch.pow(c, gamma) * (1 - c).log()


def distinct(b, i, j, l, s):
    key = torch.unique((b.long() * l + i.long()) * s + j.long())
    rows = torch.div(key, s, rounding_mode='floor')
    return torch.div(rows, l, rounding_mode='floor'), rows % l, key % s


def gt_mask(shape, b, i, j):
    m = torch.zeros(shape, dtype=torch.bool, device=b.device)
    m[b.long(), i.long(), j.long()] = True
    return m


def masked_loss(conf, pos_mask, kind='focal', alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, sparse=False,
                lo=1e-6, hi=1 - 1e-6):
    """loss.py:27-67 -> (loss, mean positive term, mean negative term)"""
    pos_mask = pos_mask.clone()
    neg_mask = ~pos_mask
    if not pos_mask.any():
        pos_mask[0, 0, 0] = True
        pos_weight = 0.
    if not neg_mask.any():
        neg_mask[0, 0, 0] = True
        neg_weight = 0.
    c = torch.clamp(conf, lo, hi)
    lp = terms(c[pos_mask], kind, alpha, gamma)[0].mean()
    if kind == 'focal' and sparse:
        return pos_weight * lp, lp, None
    ln = terms(c[neg_mask], kind, alpha, gamma)[1].mean()
    return pos_weight * lp + neg_weight * ln, lp, ln


def split_loss(conf, b, i, j, kind='focal', alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, lo=1e-6, hi=1 - 1e-6):
    """the same numbers without a mask: sum of l_neg over all entries minus its value at the distinct supervised
    entries, plus their l_pos"""
    n, l, s = conf.shape
    b, i, j = distinct(b, i, j, l, s)
    n_neg = n * l * s - b.numel()
    leave = 1.
    if b.numel() == 0:          # loss.py:37-39 sets pos_mask[0, 0, 0] only: the stand-in stays among the negatives
        b = i = j = torch.zeros(1, dtype=torch.long, device=conf.device)
        pos_weight, leave = 0., 0.
    if n_neg == 0:
        neg_weight = 0.
    c = torch.clamp(conf, lo, hi)
    lp_e, ln_e = terms(c[b, i, j], kind, alpha, gamma)
    pos_mean = lp_e.sum() / b.numel()
    neg_mean = (terms(c, kind, alpha, gamma)[1].sum() - leave * ln_e.sum()) / n_neg if n_neg else conf.new_zeros(())
    return pos_weight * pos_mean + neg_weight * neg_mean, pos_mean, neg_mean
