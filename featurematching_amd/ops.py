"""Functional wrappers over the C ABI: torch tensors in, torch tensors out.

torch is used for device memory and streams only; every computation below happens in
the hand-written HIP kernels of libfmatch_hip.so.  All functions enqueue on the current
torch stream of the inputs' device.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib


_P = C.c_void_p


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else _P(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_DTYPES = {torch.float32: _lib.FM_F32, torch.float16: _lib.FM_F16, torch.bfloat16: _lib.FM_BF16}


def _on_gpu(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the HIP path has no CPU fallback")
    return t


def _desc(t: torch.Tensor, name: str) -> torch.Tensor:
    """Coarse descriptors go to the kernels in the type they come in (float32, float16 or bfloat16: no up-cast
    pass); anything else is converted to float32."""
    if _on_gpu(t, name).dtype not in _DTYPES:
        t = t.float()
    return t.contiguous()


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if _on_gpu(t, name).dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _aligned(ws: torch.Tensor) -> C.c_void_p:
    """the first 256-byte aligned address inside a byte buffer"""
    return C.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)


def _aligned_workspace(nbytes: int, device):
    """(buffer, 256-byte aligned address) of at least nbytes of device memory"""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return ws, _aligned(ws)


def _workspace(query: str, device, *dims, empty_ok: bool = False):
    """(buffer, 256-byte aligned address, bytes) of the workspace the size query `query` asks for at `dims`; with
    empty_ok a query that answers 0 gives (None, None, 0) - the call is then handed NULL"""
    need = int(getattr(_lib.load(), query)(*dims))
    if empty_ok and not need:
        return None, None, 0
    return (*_aligned_workspace(need, device), need)


def _call(name: str, *args, dev, head=()) -> None:
    """the C call `name`(*head, *args, the current stream of `dev`); a status raises under that name"""
    _lib.check(getattr(_lib.load(), name)(*head, *args, _stream(dev)), name)


def _rows64(t: torch.Tensor) -> torch.Tensor:
    """[..., 64] as the token-wise kernels read it: [T, 64], contiguous (the results are viewed back to the shape)"""
    return t.reshape(-1, 64).contiguous()


def _param_grads(params, wanted):
    """Parameter gradients are computed all or none: (what the backward call is handed - an uninitialised tensor per
    parameter when any is wanted, else None for each and the kernels skip that work; what autograd gets back - those
    tensors where wanted, None elsewhere)"""
    full = [torch.empty_like(p) for p in params] if any(wanted) else [None] * len(params)
    return full, [d if want else None for d, want in zip(full, wanted)]


@functools.lru_cache(maxsize=256)
def _workspace_bytes(query: str, *args) -> int:
    """fm_coarse_workspace_bytes_mode / _auto: a pure function of its arguments, asked once per distinct call"""
    nb = C.c_size_t(0)
    _lib.check(getattr(_lib.load(), query)(*args, C.byref(nb)), query)
    return int(nb.value)


@dataclass
class CoarseBuffers:
    """Capacity-sized device outputs of the coarse stage plus the device-side count, and what the call that filled
    them ran with (coarse_match_async / coarse_match write every field below `conf_matrix`)."""
    b_ids: torch.Tensor
    i_ids: torch.Tensor
    j_ids: torch.Tensor
    mkpts0_c: torch.Tensor
    mkpts1_c: torch.Tensor
    mconf: torch.Tensor
    count: torch.Tensor       # int32[2] on device: {M, status bits}
    cap: int
    workspace: torch.Tensor   # kept alive until the stream has consumed it
    conf_matrix: Optional[torch.Tensor] = None   # dense [N,L,S] when requested
    _shape: tuple = ()                 # (N, L, S, C, candidate slots) the workspace is laid out for
    _has_cell_maps: bool = False       # the call did not run with FM_MODE_NO_CELL_MAPS
    _has_stats: bool = False           # the call ran with stats=True or conf_matrix=True
    _temperature: float = 0.1
    info: int = 0                      # raw FM_DEV_* bits (read_count, coarse_match)
    hint: int = 0                      # coarse_match: mode bits + slots of the attempt that served the call
    attempts: int = 0                  # coarse_match: attempts fm_coarse_match_auto made
    side_scratch: Optional[torch.Tensor] = None   # coarse_match_async(side_map=...): image 1's channels-last copy
    _side_map: Optional[torch.Tensor] = None
    _keep: tuple = ()                  # inputs must outlive the enqueued kernels

    def read_count(self) -> int:
        """The single host sync of the path: returns M (raises on a device-side status)."""
        lib = _lib.load()
        m, info = C.c_int32(0), C.c_int32(0)
        st = lib.fm_read_count_info(_ptr(self.count), self.cap, C.byref(m), C.byref(info), _stream(self.count.device))
        self.info = int(info.value)          # raw FM_DEV_* bits, the informational ones included (FM_DEV_ALL_DENSE)
        if st != _lib.FM_OK:
            err = _lib.FMatchError(st, "fm_coarse_match")
            err.required = int(m.value)
            raise err
        return int(m.value)

    def _workspace_query(self, query: str, *kinds):
        """the six values (addresses, and pitches where `kinds` says c_int) a layout query of the workspace returns"""
        outs = [kind() for kind in kinds]
        _lib.check(getattr(_lib.load(), query)(_aligned(self.workspace), *self._shape, *map(C.byref, outs)), query)
        return [o.value for o in outs]

    def cell_maps(self):
        """((map0, pitch0, ties0), (map1, pitch1, ties1)): device addresses of the cell -> match-index+1
        maps and tie lists of image 0 and image 1 inside the workspace (valid while this object is alive);
        feed them to gather_windows(cells=...) for the cell-ordered crops."""
        if not self._has_cell_maps:
            raise RuntimeError("this coarse call ran with cell_maps=False (FM_MODE_NO_CELL_MAPS)")
        v = self._workspace_query("fm_coarse_cell_maps", _P, C.c_int, _P, _P, C.c_int, _P)
        return tuple(v[:3]), tuple(v[3:])

    def softmax_stats(self):
        """(nm_r, sum_r, pitch_r, nm_c, sum_c, pitch_c): device addresses of the stabilisers and denominators of every
        row / column inside the workspace (fm_coarse_softmax_stats; valid while this object is alive).  Needs
        stats=True or conf_matrix=True."""
        if not self._has_stats:
            raise RuntimeError("this coarse call ran without stats=True / conf_matrix=True: no softmax statistics")
        nr, sr, qr, nc, sc, qc = self._workspace_query("fm_coarse_softmax_stats", _P, _P, C.c_int, _P, _P, C.c_int)
        return _P(nr), _P(sr), qr, _P(nc), _P(sc), qc

    def sliced(self, m: int) -> dict:
        return dict(b_ids=self.b_ids[:m], i_ids=self.i_ids[:m], j_ids=self.j_ids[:m],
                    mkpts0_c=self.mkpts0_c[:m], mkpts1_c=self.mkpts1_c[:m], mconf=self.mconf[:m])


def _mode_word(exact_screening=None, dense=None, exact_step=None, flat=None, stats=None, alone=None,
               cell_maps=True) -> int:
    """the `mode` argument of the coarse calls: None and False both leave a bit off; cell_maps=False sets its bit"""
    flags = ((exact_screening, _lib.FM_MODE_EXACT_SCREENING), (dense, _lib.FM_MODE_DENSE),
             (exact_step, _lib.FM_MODE_EXACT_STEP), (flat, _lib.FM_MODE_FLAT), (stats, _lib.FM_MODE_STATS),
             (alone, _lib.FM_MODE_ALONE), (not cell_maps, _lib.FM_MODE_NO_CELL_MAPS))
    return sum(bit for on, bit in flags if on)


def _coarse_inputs(feat_c0, feat_c1, scale0, scale1):
    """(f0, f1, scale0, scale1, (N, L, S, C)) as the coarse calls read them: descriptors of one element type,
    contiguous, float32 scales on the descriptors' device"""
    f0 = _desc(feat_c0, "feat_c0")
    f1 = _desc(feat_c1, "feat_c1")
    if f1.dtype != f0.dtype:
        f1 = f1.to(f0.dtype)
    n, l, c = f0.shape
    if f1.shape[0] != n or f1.shape[2] != c:
        raise ValueError(f"feat_c0 {tuple(f0.shape)} and feat_c1 {tuple(f1.shape)} disagree")
    sc0 = None if scale0 is None else _f32c(scale0.to(f0.device), "scale0")
    sc1 = None if scale1 is None else _f32c(scale1.to(f0.device), "scale1")
    return f0, f1, sc0, sc1, (n, l, f1.shape[1], c)


def _coarse_call(inputs, hw0_c, hw1_c, scale_px, thr, border_rm, temperature, ws_bytes, slots, mode, cap, conf):
    """(CoarseBuffers for `cap` matches on a fresh workspace of ws_bytes, the leading arguments fm_coarse_match_dtype,
    fm_coarse_match_maps and fm_coarse_match_auto share)"""
    f0, f1, sc0, sc1, (n, l, s, c) = inputs
    dev = f0.device
    # (one block for the workspace and the outputs, carved into typed views, was tried: the slicing costs a module
    # caller more than the nine allocations it replaces - 5.1 k against 6.4 k pairs/s)
    ws, ws_ptr = _aligned_workspace(ws_bytes, dev)
    i64 = dict(dtype=torch.int64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = CoarseBuffers(torch.empty(cap, **i64), torch.empty(cap, **i64), torch.empty(cap, **i64),
                        torch.empty(cap, 2, **f32), torch.empty(cap, 2, **f32), torch.empty(cap, **f32),
                        torch.empty(2, dtype=torch.int32, device=dev), cap, ws, conf,
                        _shape=(n, l, s, c, slots), _has_cell_maps=not mode & _lib.FM_MODE_NO_CELL_MAPS,
                        _has_stats=bool(mode & _lib.FM_MODE_STATS or conf is not None),
                        _temperature=float(temperature),
                        _keep=(f0, f1, sc0, sc1))
    args = (_ptr(f0), _ptr(f1), _DTYPES[f0.dtype], n, l, s, c, int(hw0_c[0]), int(hw0_c[1]), int(hw1_c[0]),
            int(hw1_c[1]), float(temperature), float(thr), int(border_rm), float(scale_px),
            _ptr(sc0), _ptr(sc1), ws_ptr, ws_bytes, slots, mode,
            _ptr(out.b_ids), _ptr(out.i_ids), _ptr(out.j_ids), _ptr(out.mkpts0_c),
            _ptr(out.mkpts1_c), _ptr(out.mconf), cap, _ptr(out.count), _ptr(conf))
    return out, args


def coarse_match_async(feat_c0: torch.Tensor, feat_c1: torch.Tensor, hw0_c, hw1_c, scale_px: float,
                       thr: float = 0.2, border_rm: int = 2, temperature: float = 0.1,
                       scale0: Optional[torch.Tensor] = None, scale1: Optional[torch.Tensor] = None,
                       cap: Optional[int] = None, cand_slots: Optional[int] = None,
                       conf_matrix: bool = False, exact_screening: bool = False, dense: bool = False,
                       cell_maps: bool = True, exact_step: bool = False, stats: bool = False,
                       flat: bool = False, side_map: Optional[torch.Tensor] = None,
                       side_scratch: Optional[torch.Tensor] = None, alone: bool = False) -> CoarseBuffers:
    """Enqueue the coarse stage (coarse_matching_new.py:43-143, eval) and return the
    capacity-sized device buffers without synchronising.  feat_c0 / feat_c1 may be float32, float16 or bfloat16
    (fm_coarse_match_dtype: half-precision values are exact in float32, so the result equals the float32 call on
    the up-cast tensors).  The common path is four launches (prep, int8 max pass, screening kernel, assignment);
    `dense` (FM_MODE_DENSE) adds the float16 planes and the dense sum kernel for samples with flat similarity (without
    it such samples report FM_E_DENSE through read_count), `exact_screening` (FM_MODE_EXACT_SCREENING) the two kernels
    that re-screen the candidates with exact softmax denominators (without it rows / columns that overflow their
    candidate slots report FM_E_CANDIDATES).  cell_maps=False (FM_MODE_NO_CELL_MAPS) skips the cell -> match maps the
    cell-ordered window crops read (CoarseBuffers.cell_maps() is then meaningless).  `exact_step`
    (FM_MODE_EXACT_STEP) derives the int8 screening step from the images' true maxima (one more small kernel) instead
    of from a sample of rows: the answer to FM_E_STEP (an outlier descriptor outside the sample).  `stats`
    (FM_MODE_STATS) leaves the log-softmax offsets of every row and column in the workspace
    (CoarseBuffers.softmax_stats(): what dual_softmax_at and its backward read).  `flat` (FM_MODE_FLAT, implies
    dense) is the hint that every sample has flat similarity: the screening sweep is skipped, the planes come out of the
    prep kernel and all samples go to the dense sum kernel (two launches fewer); the result does not depend on it.
    `side_map` (fm_coarse_match_maps): image 1's NCHW float32 fine map [N, 64, Hf, Wf] - its channels-last copy, which
    fine_match_maps would make as its first launch, rides in the assignment kernel's launch instead and lands in
    `side_scratch` (allocated when not given; CoarseBuffers.side_scratch) - pass that to fine_match_maps(prepared=...).
    `alone` (FM_MODE_ALONE): this call has the GPU to itself - launches that cannot fill the chip take the grid that is
    fastest for the kernel alone instead of the small footprint that leaves room for other streams' kernels."""
    lib = _lib.load()
    inputs = _coarse_inputs(feat_c0, feat_c1, scale0, scale1)
    n, l, s, c = inputs[4]
    dev = inputs[0].device
    if cap is None:
        cap = n * min(l, s)
    if cand_slots is None:
        cand_slots = lib.fm_default_cand_slots(float(thr))
    mode = _mode_word(exact_screening, dense, exact_step, flat, stats, alone, cell_maps)
    ws_bytes = _workspace_bytes("fm_coarse_workspace_bytes_mode", n, l, s, c, cand_slots, mode, int(bool(conf_matrix)))
    # data['conf_matrix'] (coarse_matching_new.py:70): one more sweep + N*L*S*4 bytes
    conf = torch.empty(n, l, s, dtype=torch.float32, device=dev) if conf_matrix else None
    out, args = _coarse_call(inputs, hw0_c, hw1_c, scale_px, thr, border_rm, temperature, ws_bytes, cand_slots, mode,
                             cap, conf)
    if side_map is not None:
        if not (side_map.is_cuda and side_map.dtype == torch.float32 and side_map.dim() == 4 and side_map.shape[1] == 64
                and side_map.is_contiguous()):
            raise ValueError("side_map: a contiguous NCHW float32 GPU map with 64 channels")
        need = side_map.numel() * 4
        if side_scratch is None or side_scratch.numel() * side_scratch.element_size() < need:
            side_scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        st = lib.fm_coarse_match_maps(*args, _ptr(side_map), int(side_map.shape[0]), 64, int(side_map.shape[2]),
                                      int(side_map.shape[3]), _ptr(side_scratch), _stream(dev))
        out.side_scratch, out._side_map = side_scratch, side_map
    else:
        st = lib.fm_coarse_match_dtype(*args, _stream(dev))
    _lib.check(st, "fm_coarse_match_dtype")
    return out


class HintMemory:
    """The `hint_io` word of fm_coarse_match_auto, kept per problem kind.

    fm_coarse_match_auto (C) answers what the data asks for by itself - flat similarity, candidate overflow, a clipped
    int8 step - and leaves the mode that served the call in a hint word; a call that starts from that word does not
    repeat the failing attempts (flat data runs FM_MODE_FLAT from its second call on).  This class only stores the word:
      * keyed by (shapes, thr, temperature); at most `capacity` keys, least recently used dropped first;
      * it DECAYS: every `reprobe`-th call of a remembered key passes no hint; when the common path then serves the
        call the key is forgotten, otherwise the new word replaces the old one;
      * guarded by a lock (module callers may run on several threads / streams);
      * visible: `snapshot()` decodes what is remembered, `clear()` forgets it.
    A hint is never wrong, only possibly slower than the common path.  Callers that pass modes themselves bypass it."""

    def __init__(self, capacity: int = 64, reprobe: int = 64):
        import threading
        from collections import OrderedDict
        self._lock = threading.Lock()
        self._d = OrderedDict()          # key -> [hint word, calls]
        self.capacity, self.reprobe = capacity, reprobe

    def start(self, key):
        """(hint word to begin the call with, probing?)"""
        with self._lock:
            e = self._d.get(key)
            if e is None:
                return 0, False
            self._d.move_to_end(key)
            e[1] += 1
            if e[1] % self.reprobe == 0:
                return 0, True
            return e[0], False

    def finish(self, key, hint: int):
        """store what fm_coarse_match_auto left in hint_io (0 = the common path served the call: forget the key)"""
        hint &= 0xffff                   # (mode bits + slots; the attempts byte is per call)
        with self._lock:
            if hint == 0:
                self._d.pop(key, None)
                return
            e = self._d.get(key)
            if e is None:
                self._d[key] = [hint, 0]
            else:
                e[0] = hint
            self._d.move_to_end(key)
            while len(self._d) > self.capacity:
                self._d.popitem(last=False)

    def clear(self):
        with self._lock:
            self._d.clear()

    @staticmethod
    def decode(hint: int) -> dict:
        return {'dense': bool(hint & (_lib.FM_MODE_DENSE | _lib.FM_MODE_FLAT)), 'exact': bool(hint & _lib.FM_MODE_EXACT_SCREENING),
                'step': bool(hint & _lib.FM_MODE_EXACT_STEP), 'flat': bool(hint & _lib.FM_MODE_FLAT),
                'slots': (hint >> 8) & 0xff, 'wide': ((hint >> 8) & 0xff) >= 16, 'attempts': (hint >> 24) & 0xff}

    def snapshot(self):
        with self._lock:
            return {k: dict(self.decode(v[0]), calls=v[1], hint=v[0]) for k, v in self._d.items()}


def hint_key(shape0, shape1, thr=0.2, temperature=0.1, dtype=torch.float32, conf_matrix=False, stats=False):
    """The problem kind MODE_MEMORY keys a hint word by: shapes, thr, temperature, descriptor dtype, and whether the call
    asks for the conf_matrix / the softmax statistics (such a call starts at 16 slots and runs the denominator
    reduction whatever the data: its word must not follow plain inference calls of the same shape, nor the reverse)."""
    return (tuple(shape0), tuple(shape1), float(thr), float(temperature), dtype, bool(conf_matrix), bool(stats))


MODE_MEMORY = HintMemory()
# how often a correct-but-slow route served a call in this process (bench.py prints them in `extra.slow_paths`, so a
# silent detour shows in the record): the torch formula of the conf_matrix backward (three [N,L,S] temporaries)
SLOW_PATHS = {"conf_matrix_grad_torch_formula": 0}


def coarse_match(feat_c0, feat_c1, hw0_c, hw1_c, scale_px, thr=0.2, border_rm=2, temperature=0.1,
                 scale0=None, scale1=None, conf_matrix: bool = False, exact_screening: Optional[bool] = None,
                 dense: Optional[bool] = None, exact_step: Optional[bool] = None, stats: bool = False,
                 flat: Optional[bool] = None, cell_maps: bool = True, alone: bool = True) -> dict:
    """Synchronous form: sliced outputs.  A thin caller of fm_coarse_match_auto - the ONE C entry point that serves any
    data (flat similarity, candidate overflow, a clipped int8 step and the assignment's bounded wait are answered inside
    it, behind the host sync the reference's torch.where has at coarse_matching_new.py:109).  What is left here: the
    allocations, FM_E_CAPACITY (exact ties can exceed N*min(L,S): larger output buffers, once more) and the optional
    hint word per problem kind (MODE_MEMORY: flat data starts its second call where the first ended).
    exact_screening / dense / exact_step / flat: None = left to the library (and the hint); True = the mode to START
    with (a caller that knows its data).  conf_matrix / stats as in coarse_match_async.  `alone` (FM_MODE_ALONE, default
    on HERE): the synchronous form waits for its result on the host - the reference's single-pair caller,
    demo/demo.py:95-116 - so its launches take the grids that are fastest for a kernel alone on the device; a process
    that runs several such calls side by side (threads, streams) passes alone=False."""
    lib = _lib.load()
    inputs = _coarse_inputs(feat_c0, feat_c1, scale0, scale1)
    n, l, s, c = inputs[4]
    dev = inputs[0].device
    key = hint_key(feat_c0.shape, feat_c1.shape, thr, temperature, inputs[0].dtype, conf_matrix, stats)
    managed = exact_screening is None and dense is None and exact_step is None and flat is None
    mode = _mode_word(exact_screening, dense, exact_step, flat, stats, alone, cell_maps)
    hint0, probing = MODE_MEMORY.start(key) if managed else (0, False)
    cap = n * min(l, s)
    max_slots = 16                      # (64 only when 16 slots and the exact re-screening still overflow: thr < 1/16)
    conf = torch.empty(n, l, s, dtype=torch.float32, device=dev) if conf_matrix else None
    for _ in range(4):
        ws_bytes = _workspace_bytes("fm_coarse_workspace_bytes_auto", n, l, s, c, max_slots)
        out, args = _coarse_call(inputs, hw0_c, hw1_c, scale_px, thr, border_rm, temperature, ws_bytes, max_slots, mode,
                                 cap, conf)
        hint, m, info = C.c_int32(hint0), C.c_int32(0), C.c_int32(0)
        st = lib.fm_coarse_match_auto(*args, C.byref(hint), C.byref(m), C.byref(info), _stream(dev))
        if st == _lib.FM_E_CAPACITY:
            cap, hint0 = int(m.value), int(hint.value) & 0xffff
            continue
        if st == _lib.FM_E_CANDIDATES and max_slots < 64:
            max_slots, hint0 = 64, int(hint.value) & 0xffff
            continue
        _lib.check(st, "fm_coarse_match_auto")
        if managed:
            MODE_MEMORY.finish(key, int(hint.value))
        h = int(hint.value)
        out._shape = (n, l, s, c, (h >> 16) & 0xff)  # the slot count the serving attempt ran with (always written)
        out.info, out.hint, out.attempts = int(info.value), h & 0xffff, (h >> 24) & 0xff
        res = out.sliced(int(m.value))
        if conf_matrix:
            res['conf_matrix'] = conf
        res['_coarse_buffers'] = out          # keeps the workspace (and its cell maps) alive
        return res
    raise RuntimeError("coarse_match: overflow persisted after retries")


def _i64c(t: torch.Tensor) -> torch.Tensor:
    """an id list as the library reads it: int64, contiguous"""
    return t.to(torch.int64).contiguous()


def _d_loss(grad: torch.Tensor) -> torch.Tensor:
    """the upstream gradient of a loss's scalar as its backward call reads it on the device: float32 [1]"""
    return grad.detach().to(torch.float32).reshape(1).contiguous()


class _DualSoftmax:
    """One dual-softmax / coarse-loss call prepared: the descriptors as the kernels read them (float32, contiguous), the
    callers' element types, shape = (N, L, S, C), the device, and `head`: the 13 leading arguments every entry point of
    the family takes - descriptors, sizes, temperature, the softmax statistics of `buffers` (asked for on first use)."""

    def __init__(self, feat_c0, feat_c1, temperature, buffers):
        self.x0, self.x1 = _f32c(feat_c0, "feat_c0"), _f32c(feat_c1, "feat_c1")
        self.dtypes, self.dev = (feat_c0.dtype, feat_c1.dtype), self.x0.device
        self.shape = (*self.x0.shape[:2], self.x1.shape[1], self.x0.shape[2])
        self.temperature, self.buffers = float(temperature), buffers

    @functools.cached_property
    def head(self):
        return (_ptr(self.x0), _ptr(self.x1), *self.shape, self.temperature, *self.buffers.softmax_stats())

    ids = staticmethod(lambda *lists: [_i64c(t) for t in lists])        # the id lists as the library reads them

    def grads(self):                                                     # (d_feat0, d_feat1), uninitialised
        return torch.empty_like(self.x0), torch.empty_like(self.x1)

    @functools.cached_property
    def run(self):                                                       # run(name, *args): `name`(*head, *args, current stream)
        return functools.partial(_call, dev=self.dev, head=self.head)

    def finish(self, d0, d1, *keep):
        """The gradients in the callers' element types.  The kernels run on the current stream and torch's caching
        allocator is stream-ordered: a block freed here is reused only by later work on that stream.  d0 still keeps
        alive what the enqueued kernels read and ANOTHER stream's work could otherwise take over: the float32 descriptors,
        `buffers` (its workspace holds the statistics) and `keep` - the call's workspace, id lists, gradient inputs."""
        d0._keep = (self.x0, self.x1, self.buffers, *keep)
        return d0.to(self.dtypes[0]), d1.to(self.dtypes[1])


def _dsm_backward(f0, f1, temperature, buffers, b_ids, i_ids, j_ids, gc):
    """(dL/df0, dL/df1) of sum_e g_e conf_e from gc = g * conf at the entries (fm_dual_softmax_backward): two launches of
    one tiled kernel that recomputes the similarities tile by tile - no [N, L, S] array."""
    p = _DualSoftmax(f0, f1, temperature, buffers)
    p.head                                                               # (statistics first, as ever)
    ws, wsp, need = _workspace("fm_dual_softmax_backward_workspace_bytes", p.dev, *p.shape)
    d0, d1 = p.grads()
    bb, ii, jj = p.ids(b_ids, i_ids, j_ids)
    g = _f32c(gc, "gc")
    p.run("fm_dual_softmax_backward", _ptr(bb), _ptr(ii), _ptr(jj), _ptr(g), int(bb.shape[0]), wsp, need, _ptr(d0), _ptr(d1))
    return p.finish(d0, d1, ws, bb, ii, jj, g)


class _DualSoftmaxAt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_c0, feat_c1, b_ids, i_ids, j_ids, temperature, buffers):
        p = _DualSoftmax(feat_c0, feat_c1, temperature, buffers)
        bb, ii, jj = p.ids(b_ids, i_ids, j_ids)
        k = int(bb.shape[0])
        conf = torch.empty(k, dtype=torch.float32, device=p.dev)
        p.run("fm_dual_softmax_conf_at", _ptr(bb), _ptr(ii), _ptr(jj), k, _ptr(conf))
        ctx.save_for_backward(feat_c0, feat_c1, bb, ii, jj, conf)
        ctx.temperature, ctx.buffers = p.temperature, buffers
        return conf

    @staticmethod
    def backward(ctx, grad):
        f0, f1, bb, ii, jj, conf = ctx.saved_tensors
        d0, d1 = _dsm_backward(f0, f1, ctx.temperature, ctx.buffers, bb, ii, jj, grad.float() * conf)
        return d0, d1, None, None, None, None, None


def dual_softmax_at(feat_c0: torch.Tensor, feat_c1: torch.Tensor, b_ids, i_ids, j_ids, buffers: CoarseBuffers) -> torch.Tensor:
    """conf_matrix[b_ids, i_ids, j_ids] (coarse_matching_new.py:64-68) as a differentiable function of the descriptors,
    without the matrix: `buffers` = the CoarseBuffers of a coarse call on the same descriptors that ran with stats=True
    (out['_coarse_buffers'] of ops.coarse_match(..., stats=True)).  What the reference's coarse loss with sparse
    supervision reads (losses/loss.py:57-61: conf[pos_mask]); forward and backward allocate O(N (L + S) C)."""
    return _DualSoftmaxAt.apply(feat_c0, feat_c1, b_ids, i_ids, j_ids, buffers._temperature, buffers)


def _dsm_backward_dense(f0, f1, temperature, buffers, grad):
    """(dL/df0, dL/df1) for a DENSE dL/dconf (fm_dual_softmax_backward_dense): three tiled sweeps that recompute conf from
    exact float32 dot products and the forward call's softmax statistics - no [N, L, S] temporary."""
    p = _DualSoftmax(f0, f1, temperature, buffers)
    g = _f32c(grad, "grad")
    p.head                                                               # (statistics first, as ever)
    ws, wsp, need = _workspace("fm_dual_softmax_backward_workspace_bytes", p.dev, *p.shape)
    d0, d1 = p.grads()
    p.run("fm_dual_softmax_backward_dense", _ptr(g), wsp, need, _ptr(d0), _ptr(d1))
    return p.finish(d0, d1, ws, g)


def _count_nonzero_bounded(t: torch.Tensor, chunk_elems: int = 1 << 20) -> int:
    """number of non-zero entries of a large tensor with temporaries of at most `chunk_elems` bytes (torch.count_nonzero
    materialises a boolean mask of the whole tensor) and one host sync"""
    flat = t.reshape(-1)
    tot = torch.zeros((), dtype=torch.int64, device=t.device)
    for o in range(0, flat.numel(), chunk_elems):
        tot += torch.count_nonzero(flat[o:o + chunk_elems])
    return int(tot)


class _ConfMatrixGrad(torch.autograd.Function):
    """Attaches the gradient of the dual softmax to the conf_matrix the HIP forward produced, so that the
    reference's coarse loss (losses/loss.py:27-67 reads data['conf_matrix']) trains the descriptors.

    conf = A * B with A = softmax(sim, dim 1), B = softmax(sim, dim 2), sim = f0 . f1^T / (C T)
    (coarse_matching_new.py:64-68).  With G = dL/dconf and c = conf:
        dL/dsim = 2 G c - A u - B v,   u_j = sum_i (G c)_ij,   v_i = sum_j (G c)_ij
        dL/df0  = dL/dsim . f1 / (C T),   dL/df1 = dL/dsim^T . f0 / (C T)
    Both forms of G are served by HIP kernels that recompute A and B tile by tile from the softmax statistics of the
    forward call - no [N, L, S] temporary:
      * the reference's default loss reads conf at the supervised entries only (sparse_spvs: loss.py:57-61), so G is zero
        almost everywhere: its non-zero entries go to fm_dual_softmax_backward;
      * a G that is dense (the focal / cross-entropy terms over ALL negatives, loss.py:44-50, 62-65: more than 16 entries
        per row on average) goes to fm_dual_softmax_backward_dense, which streams G through the same tiled sweep.
    Without the forward call's buffers (no statistics) the plain torch formula is all that is left."""

    @staticmethod
    def forward(ctx, feat_c0, feat_c1, conf, temperature, buffers):
        ctx.save_for_backward(feat_c0, feat_c1, conf)
        ctx.temperature, ctx.buffers = float(temperature), buffers
        return conf.view_as(conf)

    @staticmethod
    def backward(ctx, grad):
        f0, f1, conf = ctx.saved_tensors
        n, l, s = conf.shape
        if ctx.buffers is not None:
            if _count_nonzero_bounded(grad) <= 16 * n * max(l, s):
                nz = torch.nonzero(grad, as_tuple=True)
                gc = grad[nz] * conf[nz]
                d0, d1 = _dsm_backward(f0, f1, ctx.temperature, ctx.buffers, nz[0], nz[1], nz[2], gc)
            else:
                d0, d1 = _dsm_backward_dense(f0, f1, ctx.temperature, ctx.buffers, grad)
            return d0, d1, None, None, None
        import warnings
        SLOW_PATHS["conf_matrix_grad_torch_formula"] += 1
        warnings.warn("attach_conf_matrix_grad without the forward call's buffers: the torch formula (three [N,L,S] temporaries)")
        k = 1.0 / (f0.shape[-1] * ctx.temperature)
        sim = torch.bmm(f0.float(), f1.float().transpose(1, 2)) * k
        gc = grad * conf
        a = torch.softmax(sim, dim=1)
        dsim = 2.0 * gc - a * gc.sum(dim=1, keepdim=True)
        del a
        dsim -= torch.softmax(sim, dim=2) * gc.sum(dim=2, keepdim=True)
        del sim, gc
        g0 = torch.bmm(dsim, f1.float()) * k
        g1 = torch.bmm(dsim.transpose(1, 2), f0.float()) * k
        return g0.to(f0.dtype), g1.to(f1.dtype), None, None, None


def attach_conf_matrix_grad(feat_c0: torch.Tensor, feat_c1: torch.Tensor, conf_matrix: torch.Tensor,
                            temperature: float, buffers: Optional[CoarseBuffers] = None) -> torch.Tensor:
    """conf_matrix (from coarse_match(..., conf_matrix=True)) as a differentiable function of the descriptors;
    `buffers` = out['_coarse_buffers'] of that call (its softmax statistics serve the HIP backward)."""
    return _ConfMatrixGrad.apply(feat_c0, feat_c1, conf_matrix, temperature, buffers)


_LOSS_KINDS = {'cross_entropy': _lib.FM_LOSS_CROSS_ENTROPY, 'focal': _lib.FM_LOSS_FOCAL}


def _distinct_entries(b_ids, i_ids, j_ids, l: int, s: int, device):
    """the distinct (b, i, j) triples, as conf_matrix_gt[b, i, j] = 1 collapses repeated ones: one torch.unique over a
    linearised int64 key (its data-dependent output size is a host sync)"""
    b, i, j = (torch.as_tensor(t).to(device=device, dtype=torch.int64) for t in (b_ids, i_ids, j_ids))
    key = torch.unique((b * l + i) * s + j)
    rows = torch.div(key, s, rounding_mode='floor')
    return torch.div(rows, l, rounding_mode='floor'), rows % l, key % s


class _CoarseLoss(torch.autograd.Function):
    """fm_coarse_loss_forward / fm_coarse_loss_backward: the workspace of the forward call (row / column sums of
    dloss/dconf * conf, the entries' terms) stays on ctx for the backward call."""

    @staticmethod
    def forward(ctx, feat_c0, feat_c1, bb, ii, jj, buffers, kind, alpha, gamma, pos_weight, neg_weight):
        p = _DualSoftmax(feat_c0, feat_c1, buffers._temperature, buffers)
        k = int(bb.shape[0])
        ws, wsp, need = _workspace("fm_coarse_loss_workspace_bytes", p.dev, *p.shape, k)
        out = torch.empty(3, dtype=torch.float32, device=p.dev)
        ids = (_ptr(bb), _ptr(ii), _ptr(jj)) if k else (None, None, None)
        ctx.problem = (kind, float(alpha), float(gamma), float(pos_weight), float(neg_weight), *ids, k, wsp, need)
        p.run("fm_coarse_loss_forward", *ctx.problem, _ptr(out))
        ctx.call, ctx.keep = p, (bb, ii, jj, ws)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad, _):
        p, d_loss = ctx.call, _d_loss(grad)
        d0, d1 = p.grads()
        p.run("fm_coarse_loss_backward", *ctx.problem, _ptr(d_loss), _ptr(d0), _ptr(d1))
        return p.finish(d0, d1, ctx.keep, d_loss) + (None,) * 9


def coarse_loss(feat_c0: torch.Tensor, feat_c1: torch.Tensor, b_ids, i_ids, j_ids, buffers: CoarseBuffers,
                coarse_type: str = 'focal', alpha: float = 0.25, gamma: float = 2.0, pos_weight: float = 1.0,
                neg_weight: float = 1.0, sparse_spvs: bool = False) -> torch.Tensor:
    """What the reference's Loss.compute_coarse_loss(conf_matrix, conf_matrix_gt) returns (losses/loss.py:27-67), as a
    differentiable function of the descriptors, without conf_matrix and without conf_matrix_gt: the supervision is the
    id lists compute_supervision_coarse writes (spv_b_ids, spv_i_ids, spv_j_ids; any integer type, repeated triples
    count once) and `buffers` the CoarseBuffers of a coarse call on the same descriptors that ran with stats=True or
    conf_matrix=True, as for dual_softmax_at.  'cross_entropy' and 'focal' over all negatives are one tiled HIP sweep
    forward and two backward (fm_coarse_loss_forward / _backward), O(N (L + S) C) bytes; 'focal' with sparse_spvs reads
    the supervised entries only and goes through dual_softmax_at.  One host sync: the number of distinct triples
    (torch.unique).  An empty supervision and the upstream gradient are handled on the device.  The returned scalar
    carries `.means` = (mean positive term, mean negative term) for logging (dense forms only)."""
    if coarse_type not in _LOSS_KINDS:
        raise ValueError(f"coarse_type {coarse_type!r}: 'focal' or 'cross_entropy'")
    if not gamma > 0:
        raise ValueError("gamma must be positive")
    l, s = feat_c0.shape[1], feat_c1.shape[1]
    bb, ii, jj = _distinct_entries(b_ids, i_ids, j_ids, l, s, feat_c0.device)
    if coarse_type == 'focal' and sparse_spvs:                   # loss.py:57-61
        if bb.shape[0] == 0:                                       # :37-39: entry (0, 0, 0) with weight 0
            bb = ii = jj = torch.zeros(1, dtype=torch.int64, device=feat_c0.device)
            pos_weight = 0.0
        p = torch.clamp(dual_softmax_at(feat_c0, feat_c1, bb, ii, jj, buffers), 1e-6, 1 - 1e-6)
        return pos_weight * (-alpha * torch.pow(1 - p, gamma) * p.log()).mean()
    loss, out = _CoarseLoss.apply(feat_c0, feat_c1, bb, ii, jj, buffers, _LOSS_KINDS[coarse_type], alpha, gamma, pos_weight,
                                  neg_weight)
    loss.means = out[1:]
    return loss


def supervise_matches(kp0: torch.Tensor, kp1: torch.Tensor, hw0_c, hw1_c, cell: float = 8) -> dict:
    """Ground-truth supervision of one image pair from K correspondences kp0 / kp1 [K, 2] = (x, y) in pixels: what the
    reference's data_preprocess computes on the host with two np.unique calls (datasets/data_preprocessing.py:9-64), in
    five small HIP launches (fm_supervise_matches).  Per image-1 cell the correspondence with the smallest index
    survives; the K' survivors come sorted by (cx1, cy1).  Returns i_ids, j_ids (int64 [K']), coarse_kp0/1, fine_kp0/1
    (float32 [K', 2]), lists_f0/1 (float32 [K']: the ids as the reference keeps them) and the per-cell tables fine_mtx_0
    [L, 2] / fine_mtx_1 [S, 2] (zero where no survivor lands; of several survivors in one image-0 cell the last wins).
    One host read: K'.  A point outside its grid (negative, too large, NaN) raises FMatchError (FM_E_RANGE)."""
    lib = _lib.load()
    kp0, kp1 = _f32c(kp0, "kp0"), _f32c(kp1, "kp1")
    if kp0.dim() != 2 or kp0.shape[1] != 2 or kp0.shape != kp1.shape:
        raise ValueError(f"kp0 / kp1 must both be [K, 2], got {tuple(kp0.shape)} and {tuple(kp1.shape)}")
    (h0c, w0c), (h1c, w1c) = (int(v) for v in hw0_c), (int(v) for v in hw1_c)
    dev = kp0.device
    k = int(kp0.shape[0])
    cap = max(0, min(k, h1c * w1c))
    ws, wsp, need = _workspace("fm_supervise_workspace_bytes", dev, h0c, w0c, h1c, w1c, empty_ok=True)
    if need == 0:
        raise ValueError(f"coarse grids {hw0_c} / {hw1_c}: positive, at most 2^24 cells each")
    ids = torch.empty(2, cap, dtype=torch.int64, device=dev)
    pts = torch.empty(4, cap, 2, dtype=torch.float32, device=dev)
    lists = torch.empty(2, cap, dtype=torch.float32, device=dev)
    mtx0 = torch.empty(h0c * w0c, 2, dtype=torch.float32, device=dev)
    mtx1 = torch.empty(h1c * w1c, 2, dtype=torch.float32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    _call("fm_supervise_matches", _ptr(kp0), _ptr(kp1), k, h0c, w0c, h1c, w1c, float(cell), wsp, need, _ptr(ids[0]),
          _ptr(ids[1]), _ptr(pts[0]), _ptr(pts[1]), _ptr(pts[2]), _ptr(pts[3]), _ptr(lists[0]), _ptr(lists[1]), _ptr(mtx0),
          _ptr(mtx1), cap, _ptr(count), dev=dev)
    m = C.c_int32(0)
    _lib.check(lib.fm_read_count(_ptr(count), cap, C.byref(m), _stream(dev)), "fm_supervise_matches")
    n = m.value
    return {'i_ids': ids[0, :n], 'j_ids': ids[1, :n], 'coarse_kp0': pts[0, :n], 'coarse_kp1': pts[1, :n],
            'fine_kp0': pts[2, :n], 'fine_kp1': pts[3, :n], 'lists_f0': lists[0, :n], 'lists_f1': lists[1, :n],
            'fine_mtx_0': mtx0, 'fine_mtx_1': mtx1}


class _FineLoss(torch.autograd.Function):
    """fm_fine_loss_forward / fm_fine_loss_backward: the forward call's workspace (the reduced scalars) stays on ctx for
    the backward call."""

    @staticmethod
    def forward(ctx, expec0, expec1, gt0, gt1, count):
        e0, e1 = _f32c(expec0, "expec0"), _f32c(expec1, "expec1")
        g0, g1 = _f32c(gt0, "gt0"), _f32c(gt1, "gt1")
        m_max, dev = int(e0.shape[0]), e0.device
        ws, wsp, need = _workspace("fm_fine_loss_workspace_bytes", dev, m_max)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        _call("fm_fine_loss_forward", _ptr(e0), _ptr(e1), 3, _ptr(g0), _ptr(g1), m_max, _ptr(count), wsp, need, _ptr(out),
              dev=dev)
        ctx.problem, ctx.keep = (_ptr(e0), _ptr(e1), 3, _ptr(g0), _ptr(g1), m_max, wsp, need), (e0, e1, g0, g1, ws, count)
        ctx.dtypes = (expec0.dtype, expec1.dtype)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad, _):
        e0 = ctx.keep[0]
        d_loss = _d_loss(grad)
        d0, d1 = torch.empty_like(e0), torch.empty_like(e0)
        _call("fm_fine_loss_backward", *ctx.problem, _ptr(d_loss), _ptr(d0), _ptr(d1), dev=e0.device)
        d0._keep = (ctx.keep, d_loss)
        return d0.to(ctx.dtypes[0]), d1.to(ctx.dtypes[1]), None, None, None


def fine_loss(expec0: torch.Tensor, expec1: torch.Tensor, gt0: torch.Tensor, gt1: torch.Tensor,
              count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What the reference's Loss.compute_fine_loss(expec_f_0, expec_f_1, expec_f_gt_0, expec_f_gt_1) returns in training
    mode (losses/loss.py:70-98), as a differentiable function of expec0 / expec1 [M, 3] = (x, y, std); gt0 / gt1 [M, 2].
    No host sync: whether expec0 sums to exactly 0 (then the loss is 0 with zero gradients) and which rows have gt x != 0
    are decided on the device; when no row has, the loss is NaN as in the reference.  The std column gets zero gradient
    (the weights are detached).  M = 0 returns 0 without a HIP launch (a zero that still has both inputs' graph).  `count`: optional device int32 row count (rows at or
    beyond min(count, M) are ignored and get zero gradients).  The returned scalar carries `.terms` = (loss_0, loss_1)."""
    if expec0.dim() != 2 or expec0.shape[1] != 3 or expec1.shape != expec0.shape:
        raise ValueError(f"expec0 / expec1 must both be [M, 3], got {tuple(expec0.shape)} and {tuple(expec1.shape)}")
    m = expec0.shape[0]
    if tuple(gt0.shape) != (m, 2) or tuple(gt1.shape) != (m, 2):
        raise ValueError(f"gt0 / gt1 must be [{m}, 2], got {tuple(gt0.shape)} and {tuple(gt1.shape)}")
    if m == 0:
        _on_gpu(expec0, "expec0")
        return (expec0.sum() + expec1.sum()).float() * 0         # 0, attached to the graph of both inputs; no HIP launch
    loss, out = _FineLoss.apply(expec0, expec1, gt0, gt1, count)
    loss.terms = out[1:]
    return loss


def _stored_layout(t: torch.Tensor) -> Optional[int]:
    """0 = NCHW-contiguous, 1 = channels-last storage (and not also NCHW-contiguous), None = any other strides"""
    if t.is_contiguous():
        return 0
    return 1 if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) else None


def _map_layout(t: torch.Tensor):
    """(tensor, layout) of a logical [N,Cf,Hf,Wf] fine map as the crop and fine kernels read it: 0 = NCHW-contiguous
    (any other strides are copied to it), 1 = channels-last storage.  float32, float16 and bfloat16 maps are taken as
    they are (no up-cast pass)."""
    if t.dtype not in _DTYPES:
        t = t.float()
    layout = _stored_layout(t)
    return (t.contiguous(), 0) if layout is None else (t, layout)


def merge_reads_in_place(feat_f: torch.Tensor) -> bool:
    """A channels-last float32 / float16 / bfloat16 map goes to fm_gather_merge_windows_nhwc as it is (no layout
    copy, no up-cast pass); every other map takes the NCHW float32 kernels."""
    return feat_f.dim() == 4 and feat_f.dtype in _DTYPES and _stored_layout(feat_f) == 1


def maps_read_in_place(feat_f0: torch.Tensor, feat_f1: torch.Tensor) -> bool:
    """... both maps, in one element type (what gather_windows_pair and modules.FinePreprocess both ask)"""
    return feat_f0.is_cuda and feat_f0.dtype == feat_f1.dtype and merge_reads_in_place(feat_f0) \
        and merge_reads_in_place(feat_f1)


def _fast_nchw64(cf: int, hf: int, wf: int, w: int) -> bool:
    """what the 64-channel NCHW float32 kernels serve (csrc/fine.hip, window_route): sizes and 31-bit byte offsets"""
    return cf == 64 and w in (5, 7) and hf * wf * 64 * 4 < 1 << 31


class _Windows:
    """One window call prepared: the map(s) as the kernels read them (one layout and element type per call: image 1
    follows image 0), the outputs [M, *out_tail], m_max, each image's coarse grid, its cell map (cells[i] = one entry of
    CoarseBuffers.cell_maps(), or None: list order) as ctypes values and its checked context table.  nchw_f32: the
    call's kernels read NCHW float32 only (anything else is copied to it); otherwise _map_layout decides."""

    def __init__(self, feats, b_ids, out_tail, outs, hw_c, nchw_f32=False, cells=None, ctx=None):
        names = ("feat_f",) if len(feats) == 1 else ("feat_f0", "feat_f1")
        _on_gpu(feats[0], names[0])
        if nchw_f32:
            self.maps, self.layout = [_f32c(f, nm) for f, nm in zip(feats, names)], 0
        else:
            f0, self.layout = _map_layout(feats[0])
            mf = torch.channels_last if self.layout else torch.contiguous_format
            self.maps = [f0] + [_map_layout(f)[0].to(f0.dtype).contiguous(memory_format=mf) for f in feats[1:]]
        self.n, self.cf = self.maps[0].shape[:2]
        self.sizes = [tuple(f.shape[2:]) for f in self.maps]
        self.dev, self.dt = self.maps[0].device, _DTYPES[self.maps[0].dtype]
        self.m_max = int(b_ids.shape[0])
        self.outs = [torch.empty(self.m_max, *out_tail, dtype=torch.float32, device=self.dev) if o is None else o
                     for o in outs]
        self.hw_c = [(int(h or 0), int(w)) for h, w in hw_c]
        self.cells = [(None, 0, None) if c is None else (C.c_void_p(c[0]), int(c[1]), C.c_void_p(c[2]))
                      for c in cells or [None] * len(feats)]
        self.ctx = []
        for i, t in enumerate(ctx or ()):
            t, want = _f32c(t, f"ctx{i}"), (self.n, self.hw_c[i][0] * self.hw_c[i][1], 64)
            if tuple(t.shape) != want:
                raise ValueError(f"ctx{i} must be {list(want)}, got {tuple(t.shape)}")
            self.ctx.append(t)
        self.run = functools.partial(_call, dev=self.dev)     # run(name, *args): the C call on the maps' stream

    def merge_nhwc(self, w, stride, pad, packed_w, b_ids, ids, count) -> None:
        """fm_gather_merge_windows_nhwc on the call's one or two channels-last maps (list order; image 1 absent: NULL / 0)"""
        def of(xs, k, absent=None):
            return xs[k] if k < len(self.maps) else absent
        f, c, i, o = ([_ptr(of(xs, k)) for k in (0, 1)] for xs in (self.maps, self.ctx, ids, self.outs))
        self.run("fm_gather_merge_windows_nhwc", f[0], f[1], self.dt, self.n, self.cf, *self.sizes[0], *of(self.sizes, 1, (0, 0)),
                 w, stride, pad, *self.hw_c[0], *of(self.hw_c, 1, (0, 0)), _ptr(packed_w), c[0], c[1], _ptr(b_ids), i[0], i[1],
                 _ptr(count), self.m_max, o[0], o[1])


def gather_windows(feat_f: torch.Tensor, b_ids: torch.Tensor, ids: torch.Tensor, w: int, stride: int,
                   w_c: int, pad: int = 2, count: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, cells=None, h_c: Optional[int] = None) -> torch.Tensor:
    """Window crop (fine_preprocess.py:43-50) of the selected coarse cells only.
    feat_f is the logical [N,Cf,Hf,Wf] tensor, stored NCHW-contiguous or channels_last.
    cells = (map address, pitch, tie-list address) of this image (CoarseBuffers.cell_maps())
    selects the cell-ordered kernel when the shape allows it (NCHW float32, Cf 64, W 5/7, h_c given): the windows are
    visited in raster order of THIS image's cells, which keeps each XCD's reads inside a band of the map.  Any other
    shape takes the per-window kernels, silently."""
    p = _Windows([feat_f], b_ids, (w * w, feat_f.shape[1]), [out], [(h_c, w_c)], cells=[cells])
    if p.m_max == 0:
        return p.outs[0]
    (hf, wf), (h_c, w_c) = p.sizes[0], p.hw_c[0]
    head = (_ptr(p.maps[0]), p.n, p.cf, hf, wf)
    tail = (_ptr(b_ids), _ptr(ids), _ptr(count), p.m_max, _ptr(p.outs[0]))
    if p.dt != _lib.FM_F32:
        p.run("fm_gather_windows_dtype", head[0], p.dt, *head[1:], p.layout, w, stride, pad, w_c, *tail)
    elif cells is not None and h_c and p.layout == 0 and _fast_nchw64(p.cf, hf, wf, w):
        p.run("fm_gather_windows_cells", *head, w, stride, pad, h_c, w_c, *p.cells[0], *tail)
    else:
        p.run("fm_gather_windows", *head, p.layout, w, stride, pad, w_c, *tail)
    return p.outs[0]


def pack_merge_weights(merge_w: torch.Tensor) -> torch.Tensor:
    """merge_feat.weight [64, 128] -> the 16 KiB MFMA fragment buffer fm_gather_merge_windows reads."""
    w = _f32c(merge_w, "merge_w")
    if tuple(w.shape) != (64, 128):
        raise ValueError(f"merge_feat.weight must be [64, 128], got {tuple(w.shape)}")
    packed = torch.empty(16384, dtype=torch.uint8, device=w.device)
    _call("fm_merge_pack_weights", _ptr(w), 64, _ptr(packed), dev=w.device)
    return packed


def gather_merge_windows(feat_f: torch.Tensor, packed_w: torch.Tensor, ctx_bias: torch.Tensor, b_ids: torch.Tensor,
                         ids: torch.Tensor, w: int, stride: int, h_c: int, w_c: int, pad: int = 2,
                         count: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         cells=None) -> torch.Tensor:
    """Window crop fused with FinePreprocess's context merge (fine_preprocess.py:43-60): returns
    merge_feat(cat[window, down_proj(feat_c)]) for the selected cells, [M, WW, 64].  ctx_bias [N, h_c*w_c, 64]
    is the position-independent half (W_c . down_proj(feat_c) + bias) per coarse cell.
    A channels-last map (float32, float16 or bfloat16) is read in place, in list order (`cells` is ignored: such a
    window is W contiguous runs wherever it lies); the result is bit-identical to the call on the same float32 values
    stored NCHW."""
    nhwc = merge_reads_in_place(_on_gpu(feat_f, "feat_f"))
    p = _Windows([feat_f], b_ids, (w * w, feat_f.shape[1]), [out], [(h_c, w_c)], nchw_f32=not nhwc,
                 cells=[None if nhwc else cells], ctx=[ctx_bias])
    if p.m_max and nhwc:
        p.merge_nhwc(w, stride, pad, packed_w, b_ids, [ids], count)
    elif p.m_max:
        p.run("fm_gather_merge_windows", _ptr(p.maps[0]), p.n, p.cf, *p.sizes[0], w, stride, pad, *p.hw_c[0], *p.cells[0],
              _ptr(packed_w), _ptr(p.ctx[0]), _ptr(b_ids), _ptr(ids), _ptr(count), p.m_max, _ptr(p.outs[0]))
    return p.outs[0]


def gather_windows_pair(feat_f0: torch.Tensor, feat_f1: torch.Tensor, b_ids, i_ids, j_ids, w: int, stride: int,
                        hw0_c, hw1_c, cells, pad: int = 2, count: Optional[torch.Tensor] = None, out0=None, out1=None,
                        packed_w: Optional[torch.Tensor] = None, ctx0=None, ctx1=None):
    """Both images' window crops in one launch (cell order; cells = CoarseBuffers.cell_maps()); with
    packed_w / ctx0 / ctx1 the crop is fused with the context merge.  NCHW maps, Cf = 64, W in {5,7}.
    The fused form also reads two channels-last maps of one element type (float32, float16, bfloat16) in place, in
    list order (`cells` is ignored, may be None): same outputs, bit for bit."""
    merge = packed_w is not None
    nhwc = merge and maps_read_in_place(feat_f0, feat_f1)
    p = _Windows([feat_f0, feat_f1], b_ids, (w * w, feat_f0.shape[1]), [out0, out1], [hw0_c, hw1_c], nchw_f32=not nhwc,
                 cells=None if nhwc else cells, ctx=[ctx0, ctx1] if merge else None)
    if p.m_max and nhwc:
        p.merge_nhwc(w, stride, pad, packed_w, b_ids, [i_ids, j_ids], count)
    elif p.m_max:
        c0, c1 = p.ctx or (None, None)
        p.run("fm_gather_windows_pair", _ptr(p.maps[0]), _ptr(p.maps[1]), p.n, p.cf, *p.sizes[0], *p.sizes[1], w, stride, pad,
              *p.hw_c[0], *p.hw_c[1], *p.cells[0], *p.cells[1], _ptr(packed_w), _ptr(c0), _ptr(c1), _ptr(b_ids),
              _ptr(i_ids), _ptr(j_ids), _ptr(count), p.m_max, _ptr(p.outs[0]), _ptr(p.outs[1]))
    return p.outs[0], p.outs[1]


def fine_match(win0: torch.Tensor, win1: torch.Tensor, mix0: torch.Tensor, mix1: torch.Tensor,
               mkpts0_c: torch.Tensor, mkpts1_c: torch.Tensor, scale_f: float,
               count: Optional[torch.Tensor] = None):
    """Fine stage (fine_matching_new.py:50-79).  mix0/mix1 = float32 [WW+1] (weight, bias).
    Returns (mkpts0_f, mkpts1_f), each [M,3] = (x, y, std)."""
    win0 = _f32c(win0, "win0")
    win1 = _f32c(win1, "win1")
    m_max, ww, cf = win0.shape
    dev = win0.device
    out0 = torch.empty(m_max, 3, dtype=torch.float32, device=dev)
    out1 = torch.empty(m_max, 3, dtype=torch.float32, device=dev)
    if m_max == 0:
        return out0, out1
    k0 = _f32c(mkpts0_c, "mkpts0_c")
    k1 = _f32c(mkpts1_c, "mkpts1_c")
    _call("fm_fine_match", _ptr(win0), _ptr(win1), m_max, _ptr(count), ww, cf, _ptr(_f32c(mix0, "mix0")),
          _ptr(_f32c(mix1, "mix1")), _ptr(k0), _ptr(k1), float(scale_f), _ptr(out0), _ptr(out1), dev=dev)
    return out0, out1


class _FineMatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, win0, win1, mix0, mix1, mkpts0_c, mkpts1_c, scale_f):
        w0, w1 = _f32c(win0, "win0"), _f32c(win1, "win1")
        m0, m1 = _f32c(mix0, "mix0"), _f32c(mix1, "mix1")
        k0, k1 = fine_match(w0, w1, m0, m1, mkpts0_c, mkpts1_c, scale_f)
        ctx.save_for_backward(w0, w1, m0, m1)
        ctx.scale_f = float(scale_f)
        ctx.dtypes = (win0.dtype, win1.dtype, mix0.dtype, mix1.dtype)
        return k0, k1

    @staticmethod
    def backward(ctx, g0, g1):
        w0, w1, m0, m1 = ctx.saved_tensors
        m_max, ww, cf = w0.shape
        dev = w0.device
        g0 = torch.zeros(m_max, 3, dtype=torch.float32, device=dev) if g0 is None else _f32c(g0, "grad")
        g1 = torch.zeros(m_max, 3, dtype=torch.float32, device=dev) if g1 is None else _f32c(g1, "grad")
        d_w0, d_w1 = torch.zeros_like(w0), torch.zeros_like(w1)
        d_m0, d_m1 = torch.zeros_like(m0), torch.zeros_like(m1)
        if m_max > 0:
            ws, wsp, need = _workspace("fm_fine_match_backward_workspace_bytes", dev, m_max, ww)
            _call("fm_fine_match_backward", _ptr(w0), _ptr(w1), m_max, None, ww, cf, _ptr(m0), _ptr(m1), ctx.scale_f,
                  _ptr(g0), _ptr(g1), wsp, need, _ptr(d_w0), _ptr(d_w1), _ptr(d_m0), _ptr(d_m1), dev=dev)
            d_w0._keep = (ws, g0, g1)
        t0, t1, t2, t3 = ctx.dtypes
        return d_w0.to(t0), d_w1.to(t1), d_m0.to(t2), d_m1.to(t3), g0[:, :2], g1[:, :2], None


def fine_match_grad(win0: torch.Tensor, win1: torch.Tensor, mix0: torch.Tensor, mix1: torch.Tensor,
                    mkpts0_c: torch.Tensor, mkpts1_c: torch.Tensor, scale_f: float):
    """fine_match as a differentiable function of the windows, the position-mix parameters mix0 / mix1 ([WW+1] =
    weight, bias) and the coarse keypoints: the forward is fine_match itself, the backward fm_fine_match_backward
    (HIP, deterministic).  Cf = 64, WW in {25, 49}."""
    return _FineMatch.apply(win0, win1, mix0, mix1, mkpts0_c, mkpts1_c, scale_f)


def gather_windows_backward(d_win: torch.Tensor, b_ids: torch.Tensor, ids: torch.Tensor, shape, w: int, stride: int,
                            w_c: int, h_c: int, pad: int = 2, layout: int = 0,
                            count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adjoint of gather_windows (fm_gather_windows_backward): d_feat float32 of the logical shape [N, Cf, Hf, Wf]
    (stored channels-last for layout 1), the sum of d_win over every (match, window position) that read each pixel, in
    a fixed order (bitwise reproducible).  count = the coarse stage's device-side int32 count: rows at or beyond
    min(count[0], M) contribute nothing (no host sync)."""
    n, cf, hf, wf = shape
    dev = d_win.device
    mf = torch.channels_last if layout == 1 else torch.contiguous_format
    d_feat = torch.empty(n, cf, hf, wf, dtype=torch.float32, device=dev, memory_format=mf)
    m_max = int(b_ids.shape[0])
    if m_max == 0:
        return d_feat.zero_()
    g = _f32c(d_win, "d_win")
    bb, ii = _i64c(b_ids), _i64c(ids)
    ws, wsp, need = _workspace("fm_gather_windows_backward_workspace_bytes", dev, n, int(h_c), int(w_c), m_max)
    _call("fm_gather_windows_backward", _ptr(g), _ptr(bb), _ptr(ii), _ptr(count), m_max, n, cf, hf, wf, layout, w, stride,
          pad, int(h_c), int(w_c), wsp, need, _ptr(d_feat), dev=dev)
    d_feat._keep = (ws, g, bb, ii, count)
    return d_feat


class _GatherWindows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_f, b_ids, ids, w, stride, w_c, h_c, pad, cells):
        feat, layout = _map_layout(_on_gpu(feat_f, "feat_f"))
        out = gather_windows(feat, b_ids, ids, w, stride, w_c, pad=pad, cells=cells, h_c=h_c)
        ctx.save_for_backward(b_ids, ids)
        ctx.args = (tuple(feat_f.shape), w, stride, w_c, h_c, pad, layout, feat_f.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        b_ids, ids = ctx.saved_tensors
        shape, w, stride, w_c, h_c, pad, layout, dtype = ctx.args
        d = gather_windows_backward(grad, b_ids, ids, shape, w, stride, w_c, h_c, pad, layout)
        return d.to(dtype), None, None, None, None, None, None, None, None


def gather_windows_grad(feat_f: torch.Tensor, b_ids: torch.Tensor, ids: torch.Tensor, w: int, stride: int, w_c: int,
                        h_c: int, pad: int = 2, cells=None) -> torch.Tensor:
    """gather_windows as a differentiable function of the fine map: the forward is gather_windows itself, the backward
    fm_gather_windows_backward (HIP; the gradient is cast to the map's dtype, in the map's layout).  h_c = rows of the
    coarse grid (the backward's CSR of matches per cell)."""
    return _GatherWindows.apply(feat_f, b_ids, ids, w, stride, w_c, h_c, pad, cells)


def linear_attention_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """Whether linear_attention serves q [N,L,H,D] / k [N,S,H,D]: float32 GPU tensors of 8 heads, D = 8 with L, S <= 64
    (the window route) or D = 32 with any L, S (the long route) - la_route of csrc/linear_attn.hip."""
    if not (q.is_cuda and k.is_cuda and q.dtype == torch.float32 and k.dtype == torch.float32 and q.dim() == 4
            and k.dim() == 4):
        return False
    n, l, h, d = q.shape
    s = k.shape[1]
    if k.shape[0] != n or tuple(k.shape[2:]) != (h, d) or min(n, l, s) < 1 or h != 8:
        return False
    return (d == 8 and l <= 64 and s <= 64) or (d == 32 and n <= 65535)


def _mask_bytes(mask: Optional[torch.Tensor], rows: int, cols: int, name: str) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if tuple(mask.shape) != (rows, cols):
        raise ValueError(f"{name} must be [{rows}, {cols}], got {tuple(mask.shape)}")
    return (_on_gpu(mask, name) != 0).to(torch.uint8).contiguous()


class _LinearAttention(torch.autograd.Function):
    """fm_linear_attention_forward / fm_linear_attention_backward: q, k, v, the masks and the forward call's state stay
    on ctx; each call has a workspace of its own."""

    @staticmethod
    def forward(ctx, q, k, v, q_mask, kv_mask, eps):
        qc, kc, vc = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
        n, l, h, d = qc.shape
        s, dev = kc.shape[1], qc.device
        qm, km = _mask_bytes(q_mask, n, l, "q_mask"), _mask_bytes(kv_mask, n, s, "kv_mask")
        dims = (n, l, s, h, d)
        state_bytes = int(_lib.load().fm_linear_attention_state_bytes(*dims))
        state = torch.empty(state_bytes // 4, dtype=torch.float32, device=dev) if state_bytes else None
        ws, wsp, need = _workspace("fm_linear_attention_workspace_bytes", dev, *dims, empty_ok=True)
        out = torch.empty_like(qc)
        _call("fm_linear_attention_forward", _ptr(qc), _ptr(kc), _ptr(vc), _ptr(qm), _ptr(km), *dims, float(eps), wsp, need,
              _ptr(state), _ptr(out), dev=dev)
        ctx.save_for_backward(qc, kc, vc, qm, km, state)
        ctx.call = (dims, float(eps), need, (q.dtype, k.dtype, v.dtype))
        return out.to(q.dtype)

    @staticmethod
    def backward(ctx, grad):
        qc, kc, vc, qm, km, state = ctx.saved_tensors
        dims, eps, need, dtypes = ctx.call
        dev = qc.device
        g = _f32c(grad, "grad")
        ws, wsp = _aligned_workspace(need, dev) if need else (None, None)
        d_q, d_k, d_v = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
        _call("fm_linear_attention_backward", _ptr(qc), _ptr(kc), _ptr(vc), _ptr(qm), _ptr(km), _ptr(g), _ptr(state), *dims,
              eps, wsp, need, _ptr(d_q), _ptr(d_k), _ptr(d_v), dev=dev)
        return d_q.to(dtypes[0]), d_k.to(dtypes[1]), d_v.to(dtypes[2]), None, None, None


def linear_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_mask: Optional[torch.Tensor] = None,
                     kv_mask: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """transformer.linear_attention (the reference's LinearAttention, attentions.py:19-46) as a differentiable HIP op:
    q [N,L,H,D], k / v [N,S,H,D] -> [N,L,H,D]; q_mask [N,L] / kv_mask [N,S] (any dtype, 0 = padded) get no gradient.
    Forward fm_linear_attention_forward, backward fm_linear_attention_backward, both deterministic.  Shapes that
    linear_attention_supported refuses raise (FM_E_UNSUPPORTED); so do CPU tensors."""
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2:] != q.shape[2:]:
        raise ValueError(f"q [N,L,H,D] and k, v [N,S,H,D] expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    return _LinearAttention.apply(q, k, v, q_mask, kv_mask, eps)


def full_attention_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """Whether full_attention serves q [N,L,H,D] / k [N,S,H,D]: float32 GPU tensors of 8 heads of 8 or 32 channels, any
    L, S >= 1, N * max(L, S) * H * D < 2^31 - fa_supported of csrc/full_attn.hip."""
    if not (q.is_cuda and k.is_cuda and q.dtype == torch.float32 and k.dtype == torch.float32 and q.dim() == 4
            and k.dim() == 4):
        return False
    n, l, h, d = q.shape
    s = k.shape[1]
    if k.shape[0] != n or tuple(k.shape[2:]) != (h, d) or min(n, l, s) < 1 or h != 8 or d not in (8, 32):
        return False
    return n * max(l, s) * h * d < 1 << 31


class _FullAttention(torch.autograd.Function):
    """fm_full_attention_forward / fm_full_attention_backward: q, k, v, out and the forward call's state (one
    log-sum-exp per query and head) stay on ctx; each call has a workspace of its own.  A call that nothing will
    differentiate hands a NULL state and saves nothing."""

    @staticmethod
    def forward(ctx, q, k, v):
        qc, kc, vc = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
        n, l, h, d = qc.shape
        s, dev = kc.shape[1], qc.device
        dims = (n, l, s, h, d)
        wants = any(ctx.needs_input_grad)
        state_bytes = int(_lib.load().fm_full_attention_state_bytes(*dims)) if wants else 0
        state = torch.empty(state_bytes // 4, dtype=torch.float32, device=dev) if state_bytes else None
        ws, wsp, need = _workspace("fm_full_attention_workspace_bytes", dev, *dims, empty_ok=True)
        out = torch.empty_like(qc)
        _call("fm_full_attention_forward", _ptr(qc), _ptr(kc), _ptr(vc), *dims, wsp, need, _ptr(state), _ptr(out), dev=dev)
        if wants:
            ctx.save_for_backward(qc, kc, vc, out, state)
            ctx.call = (dims, need, (q.dtype, k.dtype, v.dtype))
        return out.to(q.dtype)

    @staticmethod
    def backward(ctx, grad):
        qc, kc, vc, out, state = ctx.saved_tensors
        dims, need, dtypes = ctx.call
        dev = qc.device
        g = _f32c(grad, "grad")
        ws, wsp = _aligned_workspace(need, dev)
        d_q, d_k, d_v = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
        _call("fm_full_attention_backward", _ptr(qc), _ptr(kc), _ptr(vc), _ptr(out), _ptr(g), _ptr(state), *dims, wsp, need,
              _ptr(d_q), _ptr(d_k), _ptr(d_v), dev=dev)
        return d_q.to(dtypes[0]), d_k.to(dtypes[1]), d_v.to(dtypes[2])


def full_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_mask: Optional[torch.Tensor] = None,
                   kv_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformer.full_attention (the reference's FullAttention, attentions.py:48-79, no dropout) as a differentiable
    HIP op that never stores the [L, S] scores: q [N,L,H,D], k / v [N,S,H,D] -> [N,L,H,D].  Forward
    fm_full_attention_forward, backward fm_full_attention_backward, both deterministic.  Padding masks are not served
    (ValueError: masked calls keep the torch function); shapes that full_attention_supported refuses raise
    (FM_E_UNSUPPORTED); so do CPU tensors."""
    if q_mask is not None or kv_mask is not None:
        raise ValueError("ops.full_attention takes no padding masks: use transformer.full_attention")
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2:] != q.shape[2:]:
        raise ValueError(f"q [N,L,H,D] and k, v [N,S,H,D] expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    return _FullAttention.apply(q, k, v)


def encoder_tail_supported(x: torch.Tensor, a: torch.Tensor) -> bool:
    """Whether encoder_tail serves x, a [..., 64]: float32 GPU tensors of equal shape, 64 channels, at least one token (and
    at most 2^24) - et_route of csrc/encoder_tail.hip."""
    if not (x.is_cuda and a.is_cuda and x.dtype == torch.float32 and a.dtype == torch.float32 and x.dim() >= 1):
        return False
    return x.shape == a.shape and x.shape[-1] == 64 and 1 <= x.numel() // 64 <= 1 << 24


class _EncoderTail(torch.autograd.Function):
    """fm_encoder_tail_forward / fm_encoder_tail_backward: x, a, the seven parameters and the forward call's state (none
    on the present route) stay on ctx; each call has a workspace of its own."""

    @staticmethod
    def forward(ctx, x, a, eps1, eps2, *params):
        xc, ac = _rows64(x), _rows64(a)
        pc = [_f32c(p.detach(), "parameter") for p in params]
        t, dev = xc.shape[0], xc.device
        state_bytes = int(_lib.load().fm_encoder_tail_state_bytes(t, 64))
        state = torch.empty(state_bytes // 4, dtype=torch.float32, device=dev) if state_bytes else None
        ws, wsp, need = _workspace("fm_encoder_tail_workspace_bytes", dev, t, 64)
        y = torch.empty_like(xc)
        _call("fm_encoder_tail_forward", _ptr(xc), _ptr(ac), *map(_ptr, pc), t, 64, float(eps1), float(eps2), wsp, need,
              _ptr(state), _ptr(y), dev=dev)
        ctx.save_for_backward(xc, ac, state, *pc)
        ctx.call = (t, float(eps1), float(eps2), need, x.shape)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, grad):
        xc, ac, state, *pc = ctx.saved_tensors
        t, eps1, eps2, need, shape = ctx.call
        dev = xc.device
        g = _rows64(_f32c(grad, "grad"))
        ws, wsp = _aligned_workspace(need, dev)
        d_x, d_a = torch.empty_like(xc), torch.empty_like(ac)
        d_p, d_p_back = _param_grads(pc, ctx.needs_input_grad[4:])       # all seven or none
        _call("fm_encoder_tail_backward", _ptr(xc), _ptr(ac), *map(_ptr, pc), _ptr(g), _ptr(state), t, 64, eps1, eps2, wsp,
              need, _ptr(d_x), _ptr(d_a), *map(_ptr, d_p), dev=dev)
        return (d_x.view(shape), d_a.view(shape), None, None, *d_p_back)


def encoder_tail(x: torch.Tensor, a: torch.Tensor, merge_w: torch.Tensor, ln1_w: torch.Tensor, ln1_b: torch.Tensor,
                 mlp0_w: torch.Tensor, mlp2_w: torch.Tensor, ln2_w: torch.Tensor, ln2_b: torch.Tensor, eps1: float = 1e-5,
                 eps2: float = 1e-5) -> torch.Tensor:
    """The tail of transformer.EncoderLayer.forward as a differentiable HIP op (float32 on the exact-float32 matrix
    instructions, forward and backward, both deterministic):
        n1 = LayerNorm1(a merge_w^T);  y = x + LayerNorm2(relu([x, n1] mlp0_w^T) mlp2_w^T)
    x (the layer's input), a (the attention's output) [..., 64] -> [..., 64].  The backward recomputes the chain from x and
    a: only they and the parameters are kept.  Inputs that encoder_tail_supported refuses raise; so do CPU tensors."""
    _on_gpu(x, "x"), _on_gpu(a, "a")
    if not encoder_tail_supported(x, a):
        raise ValueError(f"encoder_tail serves float32 x, a of one shape [..., 64] with at least one token, got "
                         f"{tuple(x.shape)} {x.dtype}, {tuple(a.shape)} {a.dtype}")
    params = (merge_w, ln1_w, ln1_b, mlp0_w, mlp2_w, ln2_w, ln2_b)
    want = ((64, 64), (64,), (64,), (128, 128), (64, 128), (64,), (64,))
    for p, shape in zip(params, want):
        if tuple(p.shape) != shape or p.dtype != torch.float32 or not p.is_cuda:
            raise ValueError(f"encoder_tail parameters are float32 GPU tensors of shapes {want}, got {tuple(p.shape)} {p.dtype}")
    return _EncoderTail.apply(x, a, eps1, eps2, *params)


def coarse_tail_supported(x: torch.Tensor, a: torch.Tensor) -> bool:
    """Whether coarse_tail serves x, a [..., 256]: float32 GPU tensors of equal shape, 256 channels, at least one token
    (and at most 2^24) - ct_route of csrc/coarse_tail.hip."""
    if not (x.is_cuda and a.is_cuda and x.dtype == torch.float32 and a.dtype == torch.float32 and x.dim() >= 1):
        return False
    return x.shape == a.shape and x.shape[-1] == 256 and 1 <= x.numel() // 256 <= 1 << 24


def _rows256(t: torch.Tensor) -> torch.Tensor:
    """[..., 256] as the coarse tail reads it: [T, 256], contiguous (the results are viewed back to the shape)"""
    return t.reshape(-1, 256).contiguous()


class _CoarseTail(torch.autograd.Function):
    """fm_coarse_tail_forward / fm_coarse_tail_backward: x, a, the seven parameters and the forward call's state (none:
    the backward recomputes) stay on ctx; each call has a workspace of its own, freed when the call has been enqueued."""

    @staticmethod
    def forward(ctx, x, a, eps1, eps2, *params):
        xc, ac = _rows256(x), _rows256(a)
        pc = [_f32c(p.detach(), "parameter") for p in params]
        t, dev = xc.shape[0], xc.device
        state_bytes = int(_lib.load().fm_coarse_tail_state_bytes(t, 256))
        state = torch.empty(state_bytes // 4, dtype=torch.float32, device=dev) if state_bytes else None
        ws, wsp, need = _workspace("fm_coarse_tail_workspace_bytes", dev, t, 256)
        y = torch.empty_like(xc)
        _call("fm_coarse_tail_forward", _ptr(xc), _ptr(ac), *map(_ptr, pc), t, 256, float(eps1), float(eps2), wsp, need,
              _ptr(state), _ptr(y), dev=dev)
        ctx.save_for_backward(xc, ac, state, *pc)
        ctx.call = (t, float(eps1), float(eps2), need, x.shape)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, grad):
        xc, ac, state, *pc = ctx.saved_tensors
        t, eps1, eps2, need, shape = ctx.call
        dev = xc.device
        g = _rows256(_f32c(grad, "grad"))
        ws, wsp = _aligned_workspace(need, dev)
        d_x, d_a = torch.empty_like(xc), torch.empty_like(ac)
        d_p, d_p_back = _param_grads(pc, ctx.needs_input_grad[4:])       # all seven or none
        _call("fm_coarse_tail_backward", _ptr(xc), _ptr(ac), *map(_ptr, pc), _ptr(g), _ptr(state), t, 256, eps1, eps2, wsp,
              need, _ptr(d_x), _ptr(d_a), *map(_ptr, d_p), dev=dev)
        return (d_x.view(shape), d_a.view(shape), None, None, *d_p_back)


def coarse_tail(x: torch.Tensor, a: torch.Tensor, merge_w: torch.Tensor, ln1_w: torch.Tensor, ln1_b: torch.Tensor,
                mlp0_w: torch.Tensor, mlp2_w: torch.Tensor, ln2_w: torch.Tensor, ln2_b: torch.Tensor, eps1: float = 1e-5,
                eps2: float = 1e-5) -> torch.Tensor:
    """encoder_tail at d_model 256, the coarse context layers' width (float32 on the exact-float32 matrix instructions,
    forward and backward, both deterministic):
        n1 = LayerNorm1(a merge_w^T);  y = x + LayerNorm2(relu([x, n1] mlp0_w^T) mlp2_w^T)
    x (the layer's input), a (the attention's output) [..., 256] -> [..., 256].  The backward recomputes the chain from x
    and a, chunk by chunk in a workspace whose size does not grow with the token count: only x, a and the parameters are
    kept.  Inputs that coarse_tail_supported refuses raise; so do CPU tensors."""
    _on_gpu(x, "x"), _on_gpu(a, "a")
    if not coarse_tail_supported(x, a):
        raise ValueError(f"coarse_tail serves float32 x, a of one shape [..., 256] with at least one token, got "
                         f"{tuple(x.shape)} {x.dtype}, {tuple(a.shape)} {a.dtype}")
    params = (merge_w, ln1_w, ln1_b, mlp0_w, mlp2_w, ln2_w, ln2_b)
    want = ((256, 256), (256,), (256,), (512, 512), (256, 512), (256,), (256,))
    for p, shape in zip(params, want):
        if tuple(p.shape) != shape or p.dtype != torch.float32 or not p.is_cuda:
            raise ValueError(f"coarse_tail parameters are float32 GPU tensors of shapes {want}, got {tuple(p.shape)} {p.dtype}")
    return _CoarseTail.apply(x, a, eps1, eps2, *params)


def qkv_projection_supported(x: torch.Tensor, source: torch.Tensor) -> bool:
    """Whether qkv_projection serves x, source: float32 GPU tensors [T, 64] (Tx, Ts independent) or [N, L, 64], [N, S, 64]
    with the same leading batch dimension, at least one token each (and at most 2^24) - qp_route of csrc/qkv_proj.hip."""
    for t in (x, source):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.shape[-1] == 64):
            return False
        if not 1 <= t.numel() // 64 <= 1 << 24:
            return False
    return x.dim() == source.dim() and (x.dim() == 2 or x.shape[0] == source.shape[0])


def _same_memory(x: torch.Tensor, source: torch.Tensor) -> bool:
    """source is x, or a view of the same storage with x's offset, shape and strides"""
    return source is x or (source.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
                           and source.storage_offset() == x.storage_offset() and source.shape == x.shape
                           and source.stride() == x.stride())


class _QkvProjection(torch.autograd.Function):
    """fm_qkv_projection_forward / fm_qkv_projection_backward: x, source (self mode: x alone) and the three weights stay on
    ctx; each call has a workspace of its own."""

    @staticmethod
    def forward(ctx, x, source, wq, wk, wv):
        self_mode = source is None
        xc = _rows64(x)
        sc = xc if self_mode else _rows64(source)
        wc = [_f32c(w.detach(), "weight") for w in (wq, wk, wv)]
        tx, ts, dev = xc.shape[0], sc.shape[0], xc.device
        ws, wsp, need = _workspace("fm_qkv_projection_workspace_bytes", dev, tx, ts, 64)
        q, k, v = torch.empty_like(xc), torch.empty_like(sc), torch.empty_like(sc)
        _call("fm_qkv_projection_forward", _ptr(xc), _ptr(sc), *map(_ptr, wc), tx, ts, 64, wsp, need, _ptr(q), _ptr(k),
              _ptr(v), dev=dev)
        if self_mode:
            ctx.save_for_backward(xc, *wc)
        else:
            ctx.save_for_backward(xc, sc, *wc)
        s_shape = x.shape if self_mode else source.shape
        ctx.call = (self_mode, need, x.shape, s_shape)
        return q.view(x.shape), k.view(s_shape), v.view(s_shape)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        self_mode, need, x_shape, s_shape = ctx.call
        if self_mode:
            xc, *wc = ctx.saved_tensors
            sc = xc
        else:
            xc, sc, *wc = ctx.saved_tensors
        tx, ts, dev = xc.shape[0], sc.shape[0], xc.device
        g = [_rows64(_f32c(t, "grad")) for t in (gq, gk, gv)]
        ws, wsp = _aligned_workspace(need, dev)
        d_x = torch.empty_like(xc)
        d_src = None if self_mode else torch.empty_like(sc)
        d_w, d_w_back = _param_grads(wc, ctx.needs_input_grad[2:])         # all three or none
        _call("fm_qkv_projection_backward", _ptr(xc), _ptr(sc), *map(_ptr, wc), *map(_ptr, g), tx, ts, 64, wsp, need,
              _ptr(d_x), _ptr(d_src), *map(_ptr, d_w), dev=dev)
        return (d_x.view(x_shape), None if self_mode else d_src.view(s_shape), *d_w_back)


def qkv_projection(x: torch.Tensor, source: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor):
    """The three projections at the top of transformer.EncoderLayer.forward as one differentiable HIP op (float32 on the
    exact-float32 matrix instructions, forward and backward, both deterministic):
        q = x wq^T,  k = source wk^T,  v = source wv^T
    x, source [T, 64] or [N, L, 64], [N, S, 64] -> (q shaped as x, k and v shaped as source).  Self mode - `source` is x, or the
    same storage, offset, shape and strides - reads x once per pass, and the whole gradient comes back in x's slot (None in
    source's).  Only x, source and the weights are kept for the backward.  Inputs that qkv_projection_supported refuses
    raise; so do CPU tensors."""
    _on_gpu(x, "x"), _on_gpu(source, "source")
    if not qkv_projection_supported(x, source):
        raise ValueError(f"qkv_projection serves float32 x, source [..., 64] of one batch size with at least one token each, "
                         f"got {tuple(x.shape)} {x.dtype}, {tuple(source.shape)} {source.dtype}")
    for w in (wq, wk, wv):
        if tuple(w.shape) != (64, 64) or w.dtype != torch.float32 or not w.is_cuda:
            raise ValueError(f"qkv_projection weights are float32 GPU tensors [64, 64], got {tuple(w.shape)} {w.dtype}")
    return _QkvProjection.apply(x, None if _same_memory(x, source) else source, wq, wk, wv)


def window_merge_supported(feat_f: torch.Tensor, w: int) -> bool:
    """Whether window_merge serves the fine map feat_f at window size w: a float32 GPU map [N, 64, Hf, Wf] stored
    NCHW-contiguous or channels-last, w in (5, 7) - wm_status of csrc/window_merge.hip."""
    return feat_f.is_cuda and feat_f.dtype == torch.float32 and feat_f.dim() == 4 and feat_f.shape[1] == 64 \
        and w in (5, 7) and _stored_layout(feat_f) is not None


class _WindowMerge(torch.autograd.Function):
    """fm_window_merge_forward / fm_window_merge_backward: the map, the ids, w_win and ctx_rows stay on ctx (no window,
    no concatenation); each call has a workspace of its own."""

    @staticmethod
    def forward(ctx, feat_f, w_win, ctx_rows, b_ids, ids, w, stride, h_c, w_c, pad):
        layout = _stored_layout(feat_f)
        n, _, hf, wf = feat_f.shape
        dev, m_max = feat_f.device, int(b_ids.shape[0])
        wc, cc = _f32c(w_win.detach(), "w_win"), _f32c(ctx_rows.detach(), "ctx_rows")
        bb, ii = _i64c(b_ids), _i64c(ids)
        geom = (n, 64, hf, wf, layout, w, stride, pad, int(h_c), int(w_c))
        ws, wsp, need = _workspace("fm_window_merge_workspace_bytes", dev, n, int(h_c), int(w_c), m_max, w)
        out = torch.empty(m_max, w * w, 64, dtype=torch.float32, device=dev)
        _call("fm_window_merge_forward", _ptr(feat_f), *geom, _ptr(wc), _ptr(cc), _ptr(bb), _ptr(ii), m_max, wsp, need,
              _ptr(out), dev=dev)
        ctx.save_for_backward(feat_f, wc, cc, bb, ii)
        ctx.call = (geom, need, m_max)
        return out

    @staticmethod
    def backward(ctx, grad):
        feat_f, wc, cc, bb, ii = ctx.saved_tensors
        geom, need, m_max = ctx.call
        dev = feat_f.device
        g = _f32c(grad, "grad")
        ws, wsp = _aligned_workspace(need, dev)
        d_feat = torch.empty_like(feat_f) if ctx.needs_input_grad[0] else None     # (preserve_format: the map's own layout)
        d_w = torch.empty_like(wc) if ctx.needs_input_grad[1] else None
        d_ctx = torch.empty_like(cc)
        if m_max == 0:
            d_feat = None if d_feat is None else d_feat.zero_()
            d_w = None if d_w is None else d_w.zero_()
        _call("fm_window_merge_backward", _ptr(feat_f), *geom, _ptr(wc), _ptr(cc), _ptr(bb), _ptr(ii), m_max, _ptr(g), wsp,
              need, _ptr(d_feat), _ptr(d_w), _ptr(d_ctx), dev=dev)
        return (d_feat, d_w, d_ctx if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None)


def window_merge(feat_f: torch.Tensor, w_win: torch.Tensor, ctx_rows: torch.Tensor, b_ids: torch.Tensor, ids: torch.Tensor,
                 w: int, stride: int, h_c: int, w_c: int, pad: int = 2) -> torch.Tensor:
    """Window crop + context merge of one image as one differentiable HIP op (float32 on the exact-float32 matrix
    instructions, forward and backward, both deterministic):
        out[m, r, :] = w_win win[m, r, :] + ctx_rows[m, :]          [M, w w, 64]
    win = the w x w window of feat_f [N, 64, Hf, Wf] at cell ids[m] of sample b_ids[m] on the h_c x w_c grid (gather_windows'
    crop: zero padding), w_win [64, 64] = the window half of merge_feat.weight, ctx_rows [M, 64] = its other half applied to
    the projected coarse descriptors, plus the bias.  The windows are never written to memory.  The map's gradient comes
    back in the map's layout; the map's and w_win's are computed only where they are asked for.  Inputs that window_merge_supported refuses
    raise; so do CPU tensors."""
    _on_gpu(feat_f, "feat_f")
    if not window_merge_supported(feat_f, w):
        raise ValueError(f"window_merge serves float32 maps [N, 64, Hf, Wf] (NCHW-contiguous or channels-last) at w in (5, 7), "
                         f"got {tuple(feat_f.shape)} {feat_f.dtype}, w = {w}")
    m = int(b_ids.shape[0])
    if tuple(w_win.shape) != (64, 64) or w_win.dtype != torch.float32 or not w_win.is_cuda:
        raise ValueError(f"window_merge: w_win is a float32 GPU tensor [64, 64], got {tuple(w_win.shape)} {w_win.dtype}")
    if tuple(ctx_rows.shape) != (m, 64) or ctx_rows.dtype != torch.float32 or not ctx_rows.is_cuda:
        raise ValueError(f"window_merge: ctx_rows is a float32 GPU tensor [{m}, 64], got {tuple(ctx_rows.shape)} {ctx_rows.dtype}")
    if int(ids.shape[0]) != m:
        raise ValueError("window_merge: b_ids and ids differ in length")
    return _WindowMerge.apply(feat_f, w_win, ctx_rows, b_ids, ids, int(w), int(stride), int(h_c), int(w_c), int(pad))


def fine_match_maps(feat_f0: torch.Tensor, feat_f1: torch.Tensor, b_ids, i_ids, j_ids, w: int, stride: int, w0c: int,
                    w1c: int, mix0: torch.Tensor, mix1: torch.Tensor, mkpts0_c: torch.Tensor, mkpts1_c: torch.Tensor,
                    scale_f: float, pad: int = 2, count: Optional[torch.Tensor] = None,
                    scratch: Optional[torch.Tensor] = None, prepared: Optional[torch.Tensor] = None):
    """Window crop + fine stage from the maps in one call (fm_fine_match_maps_dtype; fine_preprocess.py:43-50 with plain
    windows + fine_matching_new.py:50-79): no window tensors.  Channels-last maps are read in place; of NCHW float32
    maps image 1 is first copied to channels-last storage in `scratch` (allocated when not given), of NCHW float16 /
    bfloat16 maps (an autocast backbone, network/net.py:56-57) both images are, in their own element type.
    `prepared`: the scratch buffer a coarse_match_async(side_map=feat_f1) call filled (FM_LAYOUT_NCHW_PREPARED: NCHW
    float32 maps, image 1's copy exists already - no transpose launch here).
    Returns (mkpts0_f, mkpts1_f), float32."""
    p = _Windows([feat_f0, feat_f1], b_ids, (3,), [None, None], [(0, w0c), (0, w1c)])
    out0, out1 = p.outs
    if p.m_max == 0:
        return out0, out1
    layout = p.layout
    need = int(_lib.load().fm_fine_maps_scratch_bytes_dtype(p.n, p.cf, *p.sizes[0], *p.sizes[1], layout, p.dt))
    if prepared is not None:
        if layout != 0 or p.dt != _lib.FM_F32 or prepared.numel() * prepared.element_size() < need:
            raise ValueError("prepared: NCHW float32 maps and the scratch a coarse_match_async(side_map=...) call filled")
        scratch, layout = prepared, _lib.FM_LAYOUT_NCHW_PREPARED
    if need and (scratch is None or scratch.numel() * scratch.element_size() < need):
        scratch = torch.empty(need, dtype=torch.uint8, device=p.dev)
    p.run("fm_fine_match_maps_dtype", _ptr(p.maps[0]), _ptr(p.maps[1]), p.dt, layout, p.n, p.cf, *p.sizes[0], *p.sizes[1], w,
          stride, pad, p.hw_c[0][1], p.hw_c[1][1], _ptr(b_ids), _ptr(i_ids), _ptr(j_ids), _ptr(count), p.m_max,
          _ptr(_f32c(mix0, "mix0")), _ptr(_f32c(mix1, "mix1")), _ptr(_f32c(mkpts0_c, "mkpts0_c")),
          _ptr(_f32c(mkpts1_c, "mkpts1_c")), float(scale_f), _ptr(scratch) if need else None, _ptr(out0), _ptr(out1))
    out0._keep = (*p.maps, scratch)
    return out0, out1


_TF_NAMES = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight",
             "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def _tf_pointer_tables(state_dict: dict, n_layers: int, device, kind: str, d: int):
    """(tensors to keep alive, per layer the (void* x 10) table of its _TF_NAMES tensors as float32 on `device`) of a
    LocalFeatureTransformer with d_model `d`"""
    keep, tables = [], []
    want = [(d, d)] * 4 + [(2 * d, 2 * d), (d, 2 * d)] + [(d,)] * 4
    for l in range(n_layers):
        ts = [state_dict[f"layers.{l}.{name}"].detach().to(device=device, dtype=torch.float32).contiguous()
              for name in _TF_NAMES]
        if [tuple(t.shape) for t in ts] != want:
            raise ValueError(f"fm_{kind}_transformer serves d_model {d} only, got {[tuple(t.shape) for t in ts]}")
        keep.extend(ts)
        tables.append((C.c_void_p * 10)(*[t.data_ptr() for t in ts]))
    return keep, tables


def pack_coarse_transformer(state_dict: dict, n_layers: int, device) -> torch.Tensor:
    """state dict of a coarse LocalFeatureTransformer (d_model 256, 8 heads, `n_layers` encoder layers) -> the
    A-operand fragments fm_coarse_transformer reads (fm_coarse_tf_pack_weights)."""
    lib = _lib.load()
    keep, arrs = _tf_pointer_tables(state_dict, n_layers, device, "coarse", 256)
    table = (C.POINTER(C.c_void_p) * n_layers)(*[C.cast(a, C.POINTER(C.c_void_p)) for a in arrs])
    nbytes = int(lib.fm_coarse_tf_packed_bytes(n_layers))
    if nbytes == 0:
        raise ValueError(f"fm_coarse_transformer: unsupported layer count {n_layers}")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _call("fm_coarse_tf_pack_weights", C.cast(table, C.c_void_p), n_layers, _ptr(packed), dev=packed.device)
    torch.cuda.current_stream(packed.device).synchronize()       # the sources in `keep` may be freed after this
    return packed


def coarse_transformer(feat0: torch.Tensor, feat1: torch.Tensor, packed: torch.Tensor, layer_names, nhead: int = 8,
                       workspace: Optional[torch.Tensor] = None, mask0: Optional[torch.Tensor] = None,
                       mask1: Optional[torch.Tensor] = None):
    """The coarse context layers (network/net.py:74) on feat0 [N,L,256], feat1 [N,S,256]; layer_names as in the
    reference's config (['self', 'cross', ...]).  mask0 [N,L] / mask1 [N,S]: the reference's optional padding masks
    (transformer.py:78-96; True = a real token), served by the same kernels (fm_coarse_transformer_masked)."""
    lib = _lib.load()
    feat0, feat1 = _f32c(feat0, "feat0"), _f32c(feat1, "feat1")
    n, l, c = feat0.shape
    s = feat1.shape[1]
    if feat1.shape[0] != n or feat1.shape[2] != c:
        raise ValueError(f"feat0 {tuple(feat0.shape)} and feat1 {tuple(feat1.shape)} do not belong together")
    kinds = (C.c_int * len(layer_names))(*[{'self': 0, 'cross': 1}[k] for k in layer_names])
    nbytes = C.c_size_t()
    _lib.check(lib.fm_coarse_tf_workspace_bytes(n, l, s, C.byref(nbytes)), "fm_coarse_tf_workspace_bytes")
    if workspace is None or workspace.numel() < nbytes.value:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=feat0.device)
    out0, out1 = torch.empty_like(feat0), torch.empty_like(feat1)

    def as_bytes(m, length, name):
        if m is None:
            return None
        if tuple(m.shape) != (n, length):
            raise ValueError(f"{name} must be [{n}, {length}], got {tuple(m.shape)}")
        return (m != 0).to(device=feat0.device, dtype=torch.uint8).contiguous()
    m0, m1 = as_bytes(mask0, l, "mask0"), as_bytes(mask1, s, "mask1")
    _call("fm_coarse_transformer_masked", _ptr(feat0), _ptr(feat1), _ptr(m0), _ptr(m1), n, l, s, c, nhead, kinds,
          len(layer_names), _ptr(packed), _ptr(workspace), workspace.numel(), _ptr(out0), _ptr(out1), dev=feat0.device)
    out0._keep = (m0, m1)
    return out0, out1


def pack_fine_transformer(state_dict: dict, device) -> torch.Tensor:
    """state dict of a fine LocalFeatureTransformer (layers.0 = 'self', layers.1 = 'cross'; d_model 64, 8 heads) ->
    the packed operand fragments fm_fine_transformer reads (fm_fine_tf_pack_weights)."""
    lib = _lib.load()
    keep, arrs = _tf_pointer_tables(state_dict, 2, device, "fine", 64)
    packed = torch.empty(int(lib.fm_fine_tf_packed_bytes()), dtype=torch.uint8, device=device)
    _call("fm_fine_tf_pack_weights", arrs[0], arrs[1], _ptr(packed), dev=packed.device)
    torch.cuda.current_stream(packed.device).synchronize()       # the sources in `keep` may be freed after this
    return packed


def fine_transformer(win0: torch.Tensor, win1: torch.Tensor, packed: torch.Tensor, count: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None, start_scale: int = 8):
    """The fine context layers (network/net.py:79-80) on the windows [M, WW, 64] of both images, WW in {25, 49}.
    `status` = a zeroed int32 device tensor: the kernel ORs FM_DEV_RANGE into element 0 when a value did not fit its
    float16 operand halves at any of its activation scales (see fmatch.h) - the outputs must then be discarded; with two
    elements, element 1 receives by how much the matches went below `start_scale` (log2 of the first attempt's activation
    scale: 8, 4, 0 or -4; fm_fine_transformer_start)."""
    lib = _lib.load()
    win0, win1 = _f32c(win0, "win0"), _f32c(win1, "win1")
    m, ww, cf = win0.shape
    out0, out1 = torch.empty_like(win0), torch.empty_like(win1)
    if m:
        lowered = None
        if status is not None and status.numel() > 1:
            lowered = C.c_void_p(status.data_ptr() + 4)
        _lib.check(lib.fm_fine_transformer_start(_ptr(win0), _ptr(win1), m, _ptr(count), ww, cf, _ptr(packed), _ptr(out0),
                                                 _ptr(out1), _ptr(status), int(start_scale), lowered, _stream(win0.device)),
                   "fm_fine_transformer")
    return out0, out1
