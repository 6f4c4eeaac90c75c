"""The step after the matching path: per-match epipolar errors, per-pair inlier scores (HIP kernel
`k_epipolar`, csrc/post.hip), the relative pose of every pair by five-point RANSAC on the device (csrc/pose.hip), the
reference's validation metrics and the wire / on-disk format of match lists.

`compute_symmetrical_epipolar_errors(data)` has the reference's name, reads the reference's keys
(utils/metrics.py:60-81: T_0to1 [N,4,4], K0/K1 [N,3,3], m_bids, mkpts0_f, mkpts1_f) and writes data['epi_errs'];
the reference loops over the batch on the host and builds E with kornia, here one launch does the whole list.

Wire format (little-endian): a 16-byte header {magic "FMT1", uint32 version = 1,
uint32 record_bytes = 24, uint32 count} followed by `count` records {int32 pair_id, float32 x0, y0, x1, y1, conf} -
the records `dist.pack_records` produces and `dist.gather_match_lists` exchanges between ranks.
"""
from __future__ import annotations

import struct
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _lib
from .dist import RECORD, pack_records, unpack_records
from .ops import _call, _ptr

MAGIC = b"FMT1"
VERSION = 1


def epipolar_errors(mkpts0: torch.Tensor, mkpts1: torch.Tensor, m_bids: torch.Tensor, T_0to1: torch.Tensor,
                    K0: torch.Tensor, K1: torch.Tensor, inlier_thr: float = 1e-4, count: Optional[torch.Tensor] = None):
    """-> (epi_errs float32 [M], inlier bool [M], per_pair int32 [N,2] = matches / inliers per pair).
    `count`: a tensor holding the number of rows, on any device and of any integer type (converted as estimate_poses
    converts it; a negative count is none).  A row behind the count, like a row whose id lies outside [0, N) - tested in
    64 bits, as estimate_poses tests it - reads NaN and not-inlier and is counted in no pair."""
    if not mkpts0.is_cuda:
        raise RuntimeError("mkpts0 must live on the GPU: the HIP path has no CPU fallback")
    dev = mkpts0.device
    k0, k1 = mkpts0.float().contiguous(), mkpts1.float().contiguous()
    m, stride = k0.shape
    n = T_0to1.shape[0]
    f = lambda t: t.to(dev).float().contiguous()
    T, a0, a1 = f(T_0to1), f(K0), f(K1)
    if count is not None:                                 # the C call reads one int32 on the device
        count = count.to(dev, torch.int32).reshape(-1)[:1].contiguous()
    epi = torch.full((m,), float("nan"), dtype=torch.float32, device=dev)   # the kernel writes the rows that exist
    inl = torch.zeros(m, dtype=torch.uint8, device=dev)
    per = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    if m:
        _call("fm_epipolar_errors", _ptr(k0), _ptr(k1), stride, _ptr(m_bids.to(dev).long().contiguous()), _ptr(count), m, n,
              _ptr(T), _ptr(a0), _ptr(a1), float(inlier_thr), _ptr(epi), _ptr(inl), _ptr(per), dev=dev)
    return epi, inl.bool(), per


def compute_symmetrical_epipolar_errors(data: dict) -> None:
    """Drop-in for utils/metrics.py:60-81: data['epi_errs'] [M] from data['T_0to1'], 'K0', 'K1', 'm_bids',
    'mkpts0_f', 'mkpts1_f'."""
    epi, _, _ = epipolar_errors(data['mkpts0_f'], data['mkpts1_f'], data['m_bids'], data['T_0to1'], data['K0'], data['K1'])
    data.update({'epi_errs': epi})


Poses = namedtuple("Poses", "R t E inliers per_pair ok")


def estimate_poses(mkpts0: torch.Tensor, mkpts1: torch.Tensor, m_bids: torch.Tensor, K0: torch.Tensor, K1: torch.Tensor, *,
                   pixel_thr: float = 1.0, samples: int = 2048, seed: int = 0, count: Optional[torch.Tensor] = None,
                   sorted_bids: bool = True) -> Poses:
    """Relative pose of every pair from its matches: five-point RANSAC over `samples` hypotheses per pair on the device
    (fm_estimate_pose), no host synchronisation.  mkpts* [M, 2] or [M, 3] pixels, m_bids [M], K0 / K1 [N, 3, 3].
    -> Poses(R float64 [N, 3, 3], t float64 [N, 3] of unit length, E float64 [N, 3, 3], inliers bool [M], per_pair int32
    [N, 4] = matches / inliers / inliers in front of both cameras / ok, ok bool [N]).  m_bids must be non-decreasing, as the
    matcher writes it; with sorted_bids=False the list (its first `count` rows, if a count is given) is sorted
    stably first and `inliers` comes back in the caller's order.  `count`: a tensor holding the number of rows.  Where ok is False R is the identity and t is zero."""
    lib = _lib.load()
    if not mkpts0.is_cuda:
        raise RuntimeError("mkpts0 must live on the GPU: the HIP path has no CPU fallback")
    dev = mkpts0.device
    k0, k1 = mkpts0.float().contiguous(), mkpts1.float().contiguous()
    bids = m_bids.to(dev).long().contiguous()
    if count is not None:                                 # the C call reads one int32 on the device
        count = count.to(dev, torch.int32).reshape(-1)[:1].contiguous()
    order = None
    if not sorted_bids:
        if count is not None:                             # rows behind the count do not exist: they sort to the end
            beyond = torch.arange(bids.shape[0], device=dev) >= count
            bids = torch.where(beyond, torch.full_like(bids, torch.iinfo(torch.int64).max), bids)
        bids, order = torch.sort(bids, stable=True)
        k0, k1 = k0[order].contiguous(), k1[order].contiguous()
    m, stride = k0.shape
    f = lambda t: t.to(dev).float().contiguous()
    a0, a1 = f(K0), f(K1)
    n = a0.shape[0]
    need = lib.fm_pose_workspace_bytes(n, m, int(samples))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).repeat(n, 1, 1)
    t = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    E = torch.zeros(n, 3, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(m, dtype=torch.uint8, device=dev)
    per = torch.zeros(n, 4, dtype=torch.int32, device=dev)
    if m == 0:                                            # nothing to estimate from (and an empty tensor has no address)
        return Poses(R, t, E, inl.bool(), per, per[:, 3] != 0)
    _call("fm_estimate_pose", _ptr(k0), _ptr(k1), stride, _ptr(bids), _ptr(count), m, n, _ptr(a0), _ptr(a1),
          float(pixel_thr), int(samples), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ws), need, _ptr(R), _ptr(t), _ptr(E),
          _ptr(inl), _ptr(per), dev=dev)
    if order is not None:
        inl = torch.zeros_like(inl).index_copy_(0, order, inl)
    return Poses(R, t, E, inl.bool(), per, per[:, 3] != 0)


def estimate_pose(kpts0, kpts1, K0, K1, thresh=None, conf=None, **kw):
    """utils/metrics.py:79-109 for one pair, on the device: NumPy arrays or tensors in, None or (R [3, 3], t [3], mask
    [M]) as NumPy arrays out.  `thresh` and `conf` are accepted and unused, as in the reference (:89 hard-codes 1.0 px
    and 0.999); the keyword pixel_thr (and samples, seed) is what counts."""
    if len(kpts0) < 5:
        return None
    dev = kpts0.device if isinstance(kpts0, torch.Tensor) and kpts0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    g = lambda x: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(dev)
    k0 = g(kpts0)
    out = estimate_poses(k0, g(kpts1), torch.zeros(k0.shape[0], dtype=torch.long, device=dev), g(K0)[None], g(K1)[None], **kw)
    if not bool(out.ok[0]):
        return None
    return out.R[0].cpu().numpy(), out.t[0].cpu().numpy(), out.inliers.cpu().numpy()


def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0):
    """utils/metrics.py:12-29 -> (t_err, R_err): t_err is the Euclidean distance of the translations (the reference's
    quirk: not an angle), R_err the rotation angle in degrees"""
    T_0to1 = np.asarray(T_0to1)
    t_err = np.linalg.norm(T_0to1[:3, 3] - t, ord=2)
    cos = np.clip((np.trace(np.asarray(R).T @ T_0to1[:3, :3]) - 1) / 2, -1.0, 1.0)
    return t_err, np.rad2deg(np.abs(np.arccos(cos)))


def compute_pose_errors(data: dict, **kw) -> None:
    """Drop-in for utils/metrics.py:124-159: reads m_bids, mkpts0_f, mkpts1_f, K0, K1, T_0to1 and writes the lists
    data['R_errs'], data['t_errs'] (inf where a pair has no pose) and data['inliers'] (the pair's inlier mask; empty where
    it has no pose) - one device call for the batch."""
    poses = estimate_poses(data['mkpts0_f'], data['mkpts1_f'], data['m_bids'], data['K0'], data['K1'], **kw)
    truth = data['T_0to1'].cpu().numpy()
    rot, trans, has_pose = poses.R.cpu().numpy(), poses.t.cpu().numpy(), poses.ok.cpu().numpy()
    flags, owner = poses.inliers.cpu().numpy(), data['m_bids'].cpu().numpy()
    pairs = truth.shape[0]
    r_errs, t_errs = np.full(pairs, np.inf), np.full(pairs, np.inf)
    for b in np.flatnonzero(has_pose):
        t_errs[b], r_errs[b] = relative_pose_error(truth[b], rot[b], trans[b])
    data['R_errs'], data['t_errs'] = list(r_errs), list(t_errs)
    data['inliers'] = [flags[owner == b] if has_pose[b] else np.zeros(0, dtype=bool) for b in range(pairs)]


AUC_LIMITS = (5, 10, 20)


def error_auc(errors, thresholds=None, ret_dict=True):
    """utils/metrics.py:162-182: area under the recall curve up to 5, 10 and 20, each divided by its limit (`thresholds`
    is ignored, as there).  The curve rises by 1 / n at every error and is joined by straight lines from (0, 0); behind the
    last error below a limit it runs level to the limit."""
    e = np.sort(np.asarray(list(errors), dtype=np.float64))
    n = max(e.size, 1)
    areas = []
    for limit in AUC_LIMITS:
        k = int(np.count_nonzero(e < limit))
        knots = np.concatenate(([0.0], e[:k], [float(limit)]))
        height = np.concatenate((np.arange(k + 1), [k])) / n
        areas.append(float(0.5 * np.dot(np.diff(knots), height[1:] + height[:-1])) / limit)
    return dict(zip((f'auc@{limit}' for limit in AUC_LIMITS), areas)) if ret_dict else areas


def epidist_prec(errors, thresholds, ret_dict=True):
    """utils/metrics.py:185-196: per threshold, the mean over pairs of the share of a pair's matches whose epipolar error
    lies below it (a pair without matches counts as 0, no pair at all gives 0)"""
    lists = [np.asarray(e, dtype=np.float64).ravel() for e in errors]
    means = []
    for bound in thresholds:
        shares = [np.count_nonzero(e < bound) / e.size if e.size else 0.0 for e in lists]
        means.append(sum(shares) / len(shares) if shares else 0)
    return dict(zip((f'prec@{bound:.0e}' for bound in thresholds), means)) if ret_dict else means


def aggregate_metrics(metrics: dict, epi_err_thr: float = 5e-4) -> dict:
    """utils/metrics.py:199-219: pose AUC@5/10/20 of max(R_err, t_err) and the epipolar precision over the unique
    identifiers (of a repeated identifier the LAST index is kept, as there)"""
    names = list(metrics['identifiers'])
    seen, keep = set(), []
    for pos in range(len(names) - 1, -1, -1):            # from the back: the first sight of a name is its last index
        if names[pos] not in seen:
            seen.add(names[pos])
            keep.append(pos)
    keep.reverse()
    worse = np.maximum(np.asarray(metrics['R_errs'], dtype=np.float64), np.asarray(metrics['t_errs'], dtype=np.float64))
    result = error_auc(worse[keep])
    result.update(epidist_prec([metrics['epi_errs'][pos] for pos in keep], [epi_err_thr]))
    return result


def dumps(records: torch.Tensor) -> bytes:
    """int32 [M,6] records (dist.pack_records) -> bytes in the wire format."""
    rec = records.detach().to("cpu", torch.int32).contiguous().numpy().astype("<i4", copy=False)
    if rec.ndim != 2 or rec.shape[1] != RECORD:
        raise ValueError(f"records must be [M, {RECORD}] int32")
    return MAGIC + struct.pack("<III", VERSION, RECORD * 4, rec.shape[0]) + rec.tobytes()


def loads(buf: bytes) -> torch.Tensor:
    if len(buf) < 16 or buf[:4] != MAGIC:
        raise ValueError("not a match-list stream (bad magic)")
    version, rbytes, count = struct.unpack("<III", buf[4:16])
    if version != VERSION or rbytes != RECORD * 4:
        raise ValueError(f"unsupported match-list stream: version {version}, {rbytes}-byte records")
    if len(buf) != 16 + count * rbytes:
        raise ValueError(f"truncated match-list stream: {len(buf)} bytes for {count} records")
    rec = np.frombuffer(buf, dtype="<i4", offset=16).reshape(count, RECORD)
    return torch.from_numpy(rec.astype(np.int32))


def save_matches(path: str, m_bids, kpts0, kpts1, conf, pair_offset: int = 0) -> int:
    rec = pack_records(m_bids, kpts0, kpts1, conf, pair_offset)
    with open(path, "wb") as f:
        f.write(dumps(rec))
    return int(rec.shape[0])


def load_matches(path: str):
    """-> (pair_ids int64 [M], kpts0 [M,2], kpts1 [M,2], conf [M])"""
    with open(path, "rb") as f:
        return unpack_records(loads(f.read()))
