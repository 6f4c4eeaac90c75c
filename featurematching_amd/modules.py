"""Drop-in stage modules with the reference's names, signatures and ``data``-dict protocol.

    CoarseMatching.forward(feat_c0, feat_c1, data, mask_c0=None, mask_c1=None) -> None
        (network/utils/coarse_matching_new.py:43)
    FinePreprocess.forward(feat_f0, feat_f1, feat_c0, feat_c1, data) -> (Tensor, Tensor)
        (network/module/fine_preprocess.py:32)
    FineMatching.forward(feat_f0, feat_f1, data) -> None
        (network/utils/fine_matching_new.py:22)
    CoarseLoss.forward(data) -> Tensor
        (Loss.compute_coarse_loss, losses/loss.py:27, from the supervision ids instead of two [N,L,S] arrays)
    FineLoss.forward(data) -> Tensor
        (Loss.compute_fine_loss, losses/loss.py:70)
    Loss.forward(data) -> None
        (losses/loss.py:116)

Constructors take the same lower-cased config sub-dicts as network/net.py:29-32.  The
computation runs in the HIP kernels of libfmatch_hip.so (see ops.py); only the learned
``nn.Linear`` layers of FinePreprocess stay on PyTorch-ROCm.
"""
from __future__ import annotations

import logging
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

logger = logging.getLogger("featurematching_amd")


def _wants_grad(*tensors, training: bool = False) -> bool:
    """autograd will ask for a gradient through these tensors (or the module trains) - the kernels with a HIP backward"""
    return torch.is_grad_enabled() and (training or any(t.requires_grad for t in tensors))


class CoarseMatching(nn.Module):
    """`conf_matrix=True` also materialises the dense data['conf_matrix'] [N,L,S] the reference
    always writes (coarse_matching_new.py:70; only its training loss reads it) - one more sweep and
    N*L*S*4 bytes, so it is opt-in; it is required in training mode, where it carries the gradient of the dual
    softmax back to the descriptors (ops.attach_conf_matrix_grad).
    `gt_pad_sampler=True` selects the older training sampler (network/utils/coarse_matching.py:114-141: predicted
    matches sub-sampled to train_coarse_percent and padded with ground-truth matches up to train_pad_num_gt_min)
    instead of coarse_matching_new.py's plain substitution of the supervision ids (:113-116).
    `loss_stats=True` trains without the matrix: the coarse call keeps its softmax statistics (stats=True) and
    data['_fm_coarse_loss'] = (buffers, feat_c0, feat_c1) - the descriptors as handed in, with their autograd history -
    is what CoarseLoss reads; no data['conf_matrix'] is written unless conf_matrix=True asks for it as well."""

    def __init__(self, config, conf_matrix: bool = False, gt_pad_sampler: bool = False, loss_stats: bool = False):
        super().__init__()
        self.config = config
        self.thr = config['thr']
        self.border_rm = config['border_rm']
        self.train_coarse_percent = config.get('train_coarse_percent', 1.0)
        self.train_pad_num_gt_min = config.get('train_pad_num_gt_min', 200)
        self.temperature = config['dsmax_temperature']
        self.conf_matrix = conf_matrix
        self.gt_pad_sampler = gt_pad_sampler
        self.loss_stats = loss_stats

    def forward(self, feat_c0, feat_c1, data, mask_c0=None, mask_c1=None):
        """Writes b_ids, i_ids, j_ids, gt_mask, m_bids, mkpts0_c, mkpts1_c, mconf (and conf_matrix on
        request) into ``data`` (coarse_matching_new.py:70,118-141).  mask_c0/mask_c1 are accepted and
        ignored, as in the reference.  In training mode the ids that select the fine windows are the
        supervision ids data['spv_*_ids'] (:113-116); data['conf_matrix'] then carries the gradient of the dual
        softmax (the match lists themselves are not differentiable, as in the reference's @torch.no_grad
        get_coarse_match)."""
        if self.training and not (self.conf_matrix or self.loss_stats):
            raise RuntimeError("training-mode CoarseMatching needs conf_matrix=True (the loss reads data['conf_matrix']) "
                               "or loss_stats=True (CoarseLoss reads the softmax statistics)")
        scale = data['hw0_i'][0] / data['hw0_c'][0]
        with torch.no_grad():
            out = ops.coarse_match(feat_c0, feat_c1, data['hw0_c'], data['hw1_c'], scale, self.thr, self.border_rm,
                                   self.temperature, data.get('scale0'), data.get('scale1'),
                                   conf_matrix=self.conf_matrix, stats=self.loss_stats)
        if self.loss_stats:
            data['_fm_coarse_loss'] = (out['_coarse_buffers'], feat_c0, feat_c1)
        if self.conf_matrix:
            conf = out['conf_matrix']
            if _wants_grad(feat_c0, feat_c1):
                conf = ops.attach_conf_matrix_grad(feat_c0, feat_c1, conf, self.temperature, out['_coarse_buffers'])
            data.update({'conf_matrix': conf})
        mconf = out['mconf']
        b_ids, i_ids, j_ids = out['b_ids'], out['i_ids'], out['j_ids']
        mkpts0_c, mkpts1_c = out['mkpts0_c'], out['mkpts1_c']
        if self.training and self.gt_pad_sampler:                            # coarse_matching.py:114-141
            n, l, s = feat_c0.shape[0], feat_c0.shape[1], feat_c1.shape[1]
            num_train = int(n * max(l, s) * self.train_coarse_percent)
            num_pred = b_ids.shape[0]
            assert self.train_pad_num_gt_min < num_train, "min-num-gt-pad should be less than num-train-matches"
            dev = b_ids.device
            if num_pred <= num_train - self.train_pad_num_gt_min:
                pred_idx = torch.arange(num_pred, device=dev)
            else:
                pred_idx = torch.randint(num_pred, (num_train - self.train_pad_num_gt_min,), device=dev)
            gt_idx = torch.randint(len(data['spv_b_ids']), (max(num_train - num_pred, self.train_pad_num_gt_min),), device=dev)
            pick = lambda pred, gt: torch.cat([pred[pred_idx], gt[gt_idx]], dim=0)
            b_ids, i_ids, j_ids = pick(b_ids, data['spv_b_ids']), pick(i_ids, data['spv_i_ids']), pick(j_ids, data['spv_j_ids'])
            mconf = pick(mconf, torch.zeros(len(data['spv_b_ids']), device=dev))    # padded ground truth: mconf == 0
        elif self.training:                                                  # :113-116, :126-134
            b_ids, i_ids, j_ids = data['spv_b_ids'], data['spv_i_ids'], data['spv_j_ids']
        if self.training:                                                    # keypoints of the ids in use
            scale0 = scale * data['scale0'][b_ids] if 'scale0' in data else scale
            scale1 = scale * data['scale1'][b_ids] if 'scale1' in data else scale
            w0c, w1c = data['hw0_c'][1], data['hw1_c'][1]
            mkpts0_c = torch.stack([i_ids % w0c, torch.div(i_ids, w0c, rounding_mode='floor')], dim=1) * scale0
            mkpts1_c = torch.stack([j_ids % w1c, torch.div(j_ids, w1c, rounding_mode='floor')], dim=1) * scale1
        if not self.training:     # cell -> match maps for the cell-ordered window crop of FinePreprocess
            data['_fm_coarse'] = out['_coarse_buffers']
        # :137-141.  Only the GT-padding sampler produces entries with mconf == 0; every predicted match has
        # conf > thr > 0, so without it `mconf[mconf != 0]` is mconf itself - and the boolean indexing (a nonzero
        # with its host sync, three launches) is skipped
        padded = self.training and self.gt_pad_sampler
        data.update({'b_ids': b_ids, 'i_ids': i_ids, 'j_ids': j_ids,
                     'gt_mask': mconf == 0, 'm_bids': b_ids,
                     'mkpts0_c': mkpts0_c, 'mkpts1_c': mkpts1_c, 'mconf': mconf[mconf != 0] if padded else mconf})


class CoarseLoss(nn.Module):
    """Loss.compute_coarse_loss (losses/loss.py:27-67) without conf_matrix and conf_matrix_gt: forward(data) reads the
    supervision ids data['spv_b_ids' | 'spv_i_ids' | 'spv_j_ids'] (compute_supervision_coarse writes them next to
    conf_matrix_gt) and what CoarseMatching(..., loss_stats=True) left under data['_fm_coarse_loss'], and returns the
    loss the reference computes from the two [N, L, S] arrays (ops.coarse_loss).  `config`: the reference's loss section
    (coarse_type, focal_alpha, focal_gamma, pos_weight, neg_weight); `sparse_spvs`: config['module']['match_coarse']
    ['sparse_spvs'] of the reference."""

    def __init__(self, config, sparse_spvs: bool = False):
        super().__init__()
        self.coarse_type = config['coarse_type']
        self.alpha = config.get('focal_alpha', 0.25)
        self.gamma = config.get('focal_gamma', 2.0)
        self.pos_weight = config.get('pos_weight', 1.0)
        self.neg_weight = config.get('neg_weight', 1.0)
        self.sparse_spvs = sparse_spvs

    def forward(self, data):
        if '_fm_coarse_loss' not in data:
            raise RuntimeError("CoarseLoss needs the statistics of CoarseMatching(..., loss_stats=True)")
        buffers, feat_c0, feat_c1 = data['_fm_coarse_loss']
        return ops.coarse_loss(feat_c0, feat_c1, data['spv_b_ids'], data['spv_i_ids'], data['spv_j_ids'], buffers,
                               self.coarse_type, self.alpha, self.gamma, self.pos_weight, self.neg_weight, self.sparse_spvs)


def _fine_term(expec, gt):
    """one image's share of the fine loss: squared offset in units of the 7-pixel window, weighted by the inverse std
    (normalised to mean 1 over ALL rows and detached: a larger std must not pay), averaged over the rows whose ground
    truth is set (gt x != 0); without such a row the mean of nothing, NaN"""
    inv = expec[:, 2].clamp(min=1e-10).reciprocal()
    weight = (inv / inv.mean()).detach()
    sq = (expec[:, :2] - gt).square().sum(-1) / 49
    return (sq * weight)[gt[:, 0] != 0].mean()


def fine_loss_torch(expec0, expec1, gt0, gt1):
    """The fine loss of the reference's training mode (Loss.compute_fine_loss, losses/loss.py:70-98) in torch ops, on
    any device and dtype: what FineLoss computes on CPU tensors and, evaluated in float64 / float32, the yardstick of the
    HIP kernels (pinned to the reference's own numbers by tests/test_supervision_ref.py).  Syncs the host twice."""
    if expec0.sum() == 0:            # the reference's stand-in loss for a step without fine predictions
        return torch.zeros((), dtype=expec0.dtype, device=expec0.device)
    return _fine_term(expec0, gt0) + _fine_term(expec1, gt1)


def coarse_loss_torch(conf, conf_gt, coarse_type, alpha, gamma, pos_weight, neg_weight, sparse_spvs):
    """The coarse loss of the reference (Loss.compute_coarse_loss, losses/loss.py:27-67) on the dense conf_matrix and its
    0 / 1 ground truth: pos_weight * mean over the positives + neg_weight * mean over the negatives of the focal
    (-alpha (1 - p)^gamma log p, p the clamped probability of the right answer) or cross-entropy (-log p) term; focal
    with sparse_spvs keeps the positives only.  A side without entries contributes 0 (the reference lets entry
    (0, 0, 0) stand in with weight 0)."""
    if coarse_type not in ('focal', 'cross_entropy'):
        raise ValueError(f"coarse_type {coarse_type!r}: 'focal' or 'cross_entropy'")
    c = conf.clamp(1e-6, 1 - 1e-6)

    def side(mask, p, weight):
        if not bool(mask.any()):
            return conf.new_zeros(())
        p = p[mask]
        term = -p.log() if coarse_type == 'cross_entropy' else -alpha * (1 - p).pow(gamma) * p.log()
        return weight * term.mean()

    loss = side(conf_gt == 1, c, pos_weight)
    if coarse_type == 'focal' and sparse_spvs:
        return loss
    return loss + side(conf_gt == 0, 1 - c, neg_weight)


class FineLoss(nn.Module):
    """Loss.compute_fine_loss (losses/loss.py:70-98): forward(data) reads mkpts0_f / mkpts1_f [M, 3] = (x, y, std) and
    expec_f_gt_0 / expec_f_gt_1 [M, 2] (compute_supervision_fine) and returns the training-mode loss.  On the GPU it is
    ops.fine_loss (HIP forward and backward, no host sync); CPU tensors evaluate the same loss in torch ops (fine_loss_torch)."""

    def forward(self, data):
        e0, e1, g0, g1 = data['mkpts0_f'], data['mkpts1_f'], data['expec_f_gt_0'], data['expec_f_gt_1']
        if e0.is_cuda:
            return ops.fine_loss(e0, e1, g0, g1)
        return fine_loss_torch(e0, e1, g0, g1)


class Loss(nn.Module):
    """The reference's Loss (losses/loss.py:9-172) with its constructor and data-dict protocol: `config` is the
    reference's dict (config['module']['loss'][...], config['module']['match_coarse']['sparse_spvs']); forward(data)
    writes data['loss'] = coarse_weight * loss_c + fine_weight * loss_f and data['loss_scalars'] = {loss_c, loss_f,
    loss_pose, loss}: 0-dim CPU tensors, fetched by ONE copy of one small device tensor (the reference calls .cpu() per
    scalar).  The coarse term is CoarseLoss when CoarseMatching(loss_stats=True) left data['_fm_coarse_loss'], else the
    reference's dense expression on data['conf_matrix'] / data['conf_matrix_gt'].  In eval mode loss_scalars['loss_f']
    reads tensor(1.) (:137-141).  loss_pose is 0 and not part of the loss (the reference's `loss += loss_pose` is
    commented out); the pose losses ('old' / 'new') are not implemented."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.loss_config = config['module']['loss']
        self.sparse_spvs = config['module']['match_coarse']['sparse_spvs']
        self.pose_loss_cal_flag = self.loss_config.get('pose_loss_cal_flag', False)
        if self.pose_loss_cal_flag in ('old', 'new'):
            raise NotImplementedError(f"pose_loss_cal_flag {self.pose_loss_cal_flag!r}: the pose losses are not implemented")
        self.coarse_loss = CoarseLoss(self.loss_config, sparse_spvs=self.sparse_spvs)
        self.fine_loss = FineLoss()

    def compute_coarse_loss(self, data):
        if '_fm_coarse_loss' in data:
            return self.coarse_loss(data)
        c = self.coarse_loss
        return coarse_loss_torch(data['conf_matrix'], data['conf_matrix_gt'], c.coarse_type, c.alpha, c.gamma, c.pos_weight,
                                 c.neg_weight, self.sparse_spvs)

    def forward(self, data):
        loss_c = self.compute_coarse_loss(data)
        loss_f = self.fine_loss(data)
        loss = loss_c * self.loss_config['coarse_weight'] + loss_f * self.loss_config['fine_weight']
        loss_pose = torch.zeros((), dtype=loss.dtype, device=loss.device)
        names = ('loss_c', 'loss_f', 'loss_pose', 'loss')
        vals = torch.stack([v.detach().reshape(()).to(loss.dtype) for v in (loss_c, loss_f, loss_pose, loss)]).cpu()
        loss_scalars = {k: v.clone() for k, v in zip(names, vals.unbind(0))}
        if self.training is False:
            loss_scalars['loss_f'] = torch.tensor(1.)
        data.update({"loss": loss, "loss_scalars": loss_scalars})


class FinePreprocess(nn.Module):
    """fused_merge=False keeps crop and context merge apart in eval mode too, cell_ordered=False takes the list-ordered
    crop kernel (tools that time one variant against the other; both default to the fast path).
    hip_merge=True: a call that wants a gradient runs crop + context merge as ops.window_merge (HIP forward and backward,
    once per image; the windows and the [.., 128] concatenation never reach memory) where ops.window_merge_supported
    holds - float32 GPU maps of 64 channels, W in (5, 7).  Every other call runs the torch lines."""

    def __init__(self, config, fused_merge: bool = True, cell_ordered: bool = True, hip_merge: bool = False):
        super().__init__()
        self.config = config
        self.fused_merge, self.cell_ordered, self.hip_merge = fused_merge, cell_ordered, hip_merge
        self.cat_c_feat = config['fine_concat_coarse_feat']
        self.W = config['fine_window_size']
        d_model_c = config['coarse']['d_model']
        d_model_f = config['fine']['d_model']
        self.d_model_f = d_model_f
        if self.cat_c_feat:
            self.down_proj = nn.Linear(d_model_c, d_model_f, bias=True)
            self.merge_feat = nn.Linear(2 * d_model_f, d_model_f, bias=True)
        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")

    def _fused_ok(self, feat_f0, feat_f1, feat_c0, feat_c1, W) -> bool:
        """The fused crop+merge kernel serves eval mode (no autograd through the two Linear layers: inputs that
        require grad under grad mode take the torch layers) on maps with 64 fine channels and W in {5,7}: both maps
        NCHW-contiguous, or both channels-last with one element type out of float32 / float16 / bfloat16 (read in
        place: no layout copy, no up-cast pass)."""
        wants_grad = _wants_grad(feat_f0, feat_f1, feat_c0, feat_c1)
        nchw = feat_f0.is_contiguous() and feat_f1.is_contiguous()
        return self.fused_merge and not self.training and not wants_grad and self.d_model_f == 64 and W in (5, 7) \
            and feat_f0.shape[1] == 64 and (nchw or ops.maps_read_in_place(feat_f0, feat_f1))

    def _hip_merge_ok(self, feat_f0, feat_f1, feat_c0, feat_c1, W) -> bool:
        """hip_merge serves the calls that want a gradient (the eval-mode fused kernel keeps the rest): float32
        everywhere, both maps as ops.window_merge_supported asks"""
        if not (self.hip_merge and self.cat_c_feat and self.d_model_f == 64):
            return False
        params = (self.down_proj.weight, self.down_proj.bias, self.merge_feat.weight, self.merge_feat.bias)
        if not _wants_grad(feat_f0, feat_f1, feat_c0, feat_c1, *params):
            return False
        return all(t.is_cuda and t.dtype == torch.float32 for t in (feat_c0, feat_c1) + params) \
            and ops.window_merge_supported(feat_f0, W) and ops.window_merge_supported(feat_f1, W)

    def _merge_constants(self):
        """(packed W_w fragments, E = W_c . down_proj.weight [64, C], e = W_c . down_proj.bias + merge bias),
        cached until one of the four parameters changes (in-place updates bump torch's version counters)."""
        ps = (self.down_proj.weight, self.down_proj.bias, self.merge_feat.weight, self.merge_feat.bias)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if getattr(self, '_merge_key', None) != key:
            cf = self.d_model_f
            w_c = self.merge_feat.weight[:, cf:].float()
            self._merge_cache = (ops.pack_merge_weights(self.merge_feat.weight.detach()),
                                 (w_c @ self.down_proj.weight.float()).detach().contiguous(),
                                 (w_c @ self.down_proj.bias.float() + self.merge_feat.bias.float()).detach().contiguous())
            self._merge_key = key
        return self._merge_cache

    def prepare(self, feat_c0, feat_c1):
        """Optional: enqueue the part of forward() that does not depend on the matches - the per-cell context tables
        W_c.(down_proj(feat_c)) + bias, two plain GEMMs - ahead of time.  A caller that runs this BEFORE
        CoarseMatching.forward (whose match count is a host sync) leaves only the crop launch behind the sync
        (matcher.Matcher.forward_features does).  forward() uses the tables when it is handed the same tensors."""
        self._ctx_ready = None
        if not (self.cat_c_feat and self.fused_merge and not self.training and feat_c0.is_cuda):
            return
        if _wants_grad(feat_c0, feat_c1):
            return
        with torch.no_grad():
            _, e_w, e_b = self._merge_constants()
            self._ctx_ready = ((feat_c0.data_ptr(), feat_c0._version, feat_c1.data_ptr(), feat_c1._version),
                               F.linear(feat_c0.float(), e_w, e_b), F.linear(feat_c1.float(), e_w, e_b))

    def forward(self, feat_f0, feat_f1, feat_c0, feat_c1, data):
        W = self.W
        stride = data['hw0_f'][0] // data['hw0_c'][0]
        data.update({'W': W})
        b_ids, i_ids, j_ids = data['b_ids'], data['i_ids'], data['j_ids']
        if b_ids.shape[0] == 0:
            feat0 = torch.empty(0, W ** 2, self.d_model_f, device=feat_f0.device)
            feat1 = torch.empty(0, W ** 2, self.d_model_f, device=feat_f0.device)
            return feat0, feat1
        # windows of the matched cells only (the reference unfolds all L cells, then selects)
        # Cell-ordered crop when the ids are this coarse call's own (its cell -> match maps are still in the
        # workspace): every XCD then reads one band of the map.
        cells0 = cells1 = None
        buf = data.get('_fm_coarse') if self.cell_ordered else None
        if buf is not None and buf.b_ids.data_ptr() == b_ids.data_ptr():     # ids are this coarse call's
            cells0, cells1 = buf.cell_maps()
        hw0_c, hw1_c = data['hw0_c'], data['hw1_c']
        if self.cat_c_feat and self._fused_ok(feat_f0, feat_f1, feat_c0, feat_c1, W):
            # inference: crop + merge in one HIP kernel (fm_gather_merge_windows); the un-merged windows never
            # reach memory.  The position-independent half of merge_feat becomes a per-cell table (plain GEMMs).
            with torch.no_grad():
                packed, e_w, e_b = self._merge_constants()
                ready = getattr(self, '_ctx_ready', None)
                self._ctx_ready = None
                if ready is not None and ready[0] == (feat_c0.data_ptr(), feat_c0._version, feat_c1.data_ptr(), feat_c1._version):
                    ctx0, ctx1 = ready[1], ready[2]                 # prepare() ran on these very tensors
                else:
                    ctx0 = F.linear(feat_c0.float(), e_w, e_b)      # [N, L, 64] = W_c.(down_proj(feat_c)) + bias
                    ctx1 = F.linear(feat_c1.float(), e_w, e_b)
                # one launch for both images: cell order on NCHW maps (needs this coarse call's cell maps), list order on
                # channels-last maps (fm_gather_merge_windows_nhwc reads them in place and needs no cell map)
                nhwc = ops.maps_read_in_place(feat_f0, feat_f1)
                if (cells0 is not None or nhwc) and feat_f1.shape[1] == 64:
                    win0, win1 = ops.gather_windows_pair(feat_f0, feat_f1, b_ids, i_ids, j_ids, W, stride, hw0_c, hw1_c,
                                                         None if nhwc else (cells0, cells1), packed_w=packed, ctx0=ctx0,
                                                         ctx1=ctx1)
                else:
                    win0 = ops.gather_merge_windows(feat_f0, packed, ctx0, b_ids, i_ids, W, stride, hw0_c[0], hw0_c[1])
                    win1 = ops.gather_merge_windows(feat_f1, packed, ctx1, b_ids, j_ids, W, stride, hw1_c[0], hw1_c[1])
            return win0, win1
        if self._hip_merge_ok(feat_f0, feat_f1, feat_c0, feat_c1, W):
            half = self.d_model_f
            w_win = self.merge_feat.weight[:, :half]
            rows = []
            for feat_c, ids in ((feat_c0, i_ids), (feat_c1, j_ids)):     # the position-independent half, a row per match
                rows.append(F.linear(self.down_proj(feat_c[b_ids, ids]), self.merge_feat.weight[:, half:], self.merge_feat.bias))
            win0 = ops.window_merge(feat_f0, w_win, rows[0], b_ids, i_ids, W, stride, hw0_c[0], hw0_c[1])
            win1 = ops.window_merge(feat_f1, w_win, rows[1], b_ids, j_ids, W, stride, hw1_c[0], hw1_c[1])
            return win0, win1
        if _wants_grad(feat_f0, feat_f1, training=self.training):
            # the crop with its HIP backward (fm_gather_windows_backward): the fine loss reaches the fine maps
            win0 = ops.gather_windows_grad(feat_f0, b_ids, i_ids, W, stride, hw0_c[1], hw0_c[0], cells=cells0)
            win1 = ops.gather_windows_grad(feat_f1, b_ids, j_ids, W, stride, hw1_c[1], hw1_c[0], cells=cells1)
        else:
            with torch.no_grad():
                win0 = ops.gather_windows(feat_f0, b_ids, i_ids, W, stride, hw0_c[1], cells=cells0, h_c=hw0_c[0])
                win1 = ops.gather_windows(feat_f1, b_ids, j_ids, W, stride, hw1_c[1], cells=cells1, h_c=hw1_c[0])
        if self.cat_c_feat:      # training (autograd through the two Linear layers) or shapes outside the fused kernel
            feat_c_win = self.down_proj(torch.cat([feat_c0[b_ids, i_ids], feat_c1[b_ids, j_ids]], 0))
            feat_cf_win = self.merge_feat(torch.cat([
                torch.cat([win0, win1], 0),
                feat_c_win[:, None, :].expand(-1, W ** 2, -1)], -1))
            win0, win1 = torch.chunk(feat_cf_win, 2, dim=0)
        return win0, win1


class FineMatching(nn.Module):
    """FineMatching with s2d paradigm; ``window`` fixes the length of the position-mix weights
    (the reference hard-codes Linear(49, 1), i.e. window 7)."""

    def __init__(self, config=None, window: int = 7):
        super().__init__()
        ww = window * window
        self.mix_feat_0 = nn.Linear(ww, 1, bias=True)
        self.mix_feat_1 = nn.Linear(ww, 1, bias=True)

    def _mix(self, lin):
        """[WW + 1] = weights then bias, cached until the layer changes (in-place updates bump the version counters)"""
        key = (lin.weight.data_ptr(), lin.weight._version, lin.bias.data_ptr(), lin.bias._version)
        cache = self.__dict__.setdefault('_mix_cache', {})
        hit = cache.get(id(lin))
        if hit is None or hit[0] != key:
            hit = (key, torch.cat([lin.weight.detach().reshape(-1), lin.bias.detach().reshape(-1)]).float().contiguous())
            cache[id(lin)] = hit
        return hit[1]

    def forward(self, feat_f0, feat_f1, data):
        """In training mode, or when feat_f0 / feat_f1 require grad (under grad mode), the outputs carry the HIP
        backward (ops.fine_match_grad): the gradient of mkpts*_f reaches the windows and mix_feat_0 / mix_feat_1.
        Otherwise the plain kernel call, as under no_grad."""
        M, WW, C = feat_f0.shape
        W = int(math.sqrt(WW))
        scale = data['hw0_i'][0] / data['hw0_f'][0]
        self.M, self.W, self.WW, self.C, self.scale = M, W, WW, C, scale
        if M == 0:
            assert self.training is False, "M is always >0, when training, see coarse_matching.py"
            logger.warning('No matches found in coarse-level.')
            data.update({'expec_f': torch.empty(0, 3, device=feat_f0.device),
                         'mkpts0_f': data['mkpts0_c'], 'mkpts1_f': data['mkpts1_c']})
            return
        if _wants_grad(feat_f0, feat_f1, training=self.training):
            mix = [torch.cat([lin.weight.view(-1), lin.bias]) for lin in (self.mix_feat_0, self.mix_feat_1)]
            k0, k1 = ops.fine_match_grad(feat_f0, feat_f1, mix[0], mix[1], data['mkpts0_c'], data['mkpts1_c'], scale)
        else:
            with torch.no_grad():
                k0, k1 = ops.fine_match(feat_f0, feat_f1, self._mix(self.mix_feat_0), self._mix(self.mix_feat_1),
                                        data['mkpts0_c'], data['mkpts1_c'], scale)
        data.update({"mkpts0_f": k0, "mkpts1_f": k1})
