// Host side of the C ABI (include/fmatch.h): argument checks, workspace layout, launch order.
#include <math.h>
#include <stdlib.h>

#include "fm_debug.h"
#include "fm_internal.h"

namespace fm {

int g_unit_cert = 0;
int g_defer_exact = 0;

int choose_splits(int N, int panels, int tiles, int target) {
  // One workgroup per (sample, panel, split); aim at one full round of the 256 CUs when the
  // batch alone cannot fill them (a split shorter than 2 tiles is not worth its prologue).
  const int wg = N * panels;
#ifdef FM_TUNE_ENV
  if (const char* e = getenv("FM_TARGET_WGS")) target = atoi(e) > 0 ? atoi(e) : 256;
#endif
  int s = target / (wg > 0 ? wg : 1);
  if (s < 1) s = 1;
  const int smax = tiles / 2 > 0 ? tiles / 2 : 1;
  if (s > smax) s = smax;
  if (s > 32) s = 32;
  return s;
}

// Items of the screening kernel k_screen_rows: one wave per (32-row block, chunk of <= 64 column units).  64 units when the
// launch holds thousands of items anyway (a batch, a 1024x1024 pair); 32 - shorter waves, more of them - for a pair or two
// (one 640x480 pair on 4 streams: 27.0 / 28.0 / 27.3 / 26.1 k pairs/s at 64 / 32 / 16 / 8 units; 64 pairs: 286 / 309 /
// 375 us at 64 / 32 / 16)
static int choose_screen_chunks(int N, int Lp, int nunits, int* units_per_chunk, bool alone) {
  const long nrb = (long)N * (Lp / 32);
  // (FM_MODE_ALONE, a pair or two: 8-unit chunks - 3.5 us faster alone at one 640x480 pair, 7 % slower on four streams)
  // (round 6: 64-unit chunks from 1024 items on - a 640x960 pair, 1520 items: 13 624 against 13 306 pairs/s at 32 units)
  const int cu = nrb * ((nunits + 63) / 64) >= 1024 ? 64 : (alone && nrb * ((nunits + 7) / 8) <= 8192 ? 8 : 32);
  *units_per_chunk = cu;
  return (nunits + cu - 1) / cu;
}

// k_max_i8's workgroups are 4 waves (256 rows x a range of tiles) and two of them fit a CU.  When the batch alone cannot
// fill the chip the grid aims at ONE workgroup per compute unit, not two: alone the kernel is 2.8 us slower at one
// 640x480 pair (15.4 against 12.7 us), but on the bench's four streams the other half of every compute unit's registers and
// LDS is what the other pairs' kernels run in - 128 / 192 / 256 / 384 / 512 workgroups: 28.4 / 28.9 / 28.7 / 28.3 / 27.9 k
// pairs/s (round 5, with k_screen_rows; round 4's measurement with the 128-KiB-of-LDS screening kernel beside it saw no
// difference).  A batch that fills the resident slots by itself gets ~10 rounds of 512.
constexpr int kMaxPassTarget = 256;
constexpr int kMaxPassSlots = 512;

CoarseWs coarse_layout(int N, int L, int S, int C, int slots, bool alone) {
  CoarseWs w{};
  C = padded_channels(C);
  w.N = N; w.L = L; w.S = S; w.C = C; w.slots = slots;
  w.Lp = round_up(L, kPanelRows);
  w.Sp = round_up(S, kTileCols);
  w.panels = w.Lp / kPanelRows;
  w.tiles = w.Sp / kTileCols;
  w.splits = choose_splits(N, w.panels, w.tiles);
  // (a batch that fills the resident slots by itself gets ~10 rounds of workgroups, so that the last round's tail is a
  // small share of the launch: 1216 workgroups on 512 slots were "2.4 of 3 rounds"; 64 pairs of 640x480: 351 -> 333 us
  // with 4 splits; 2 / 3 / 4 / 5 / 8 splits: 335 / 340 / 333 / 348 / 363 us)
  {
    int target = N * w.panels >= kMaxPassSlots ? 10 * kMaxPassSlots : (alone ? kMaxPassSlots : kMaxPassTarget);
    // (round 6: a launch whose workgroups would each sweep >= 32 tiles at one workgroup per CU - a 1024x1024 pair: 64 -
    // is long enough for the matrix cores to decide, and one wave per SIMD runs them at 40 %: two workgroups per CU there.
    // 1024x1024 on four streams, 256 / 384 / 512 / 768 workgroups: 6228 / 6307 / 6364 / 6207 pairs/s, max pass alone 100 /
    // 91 / 77 / 88 us; 640x960 (25 tiles per workgroup) keeps 256: 12 949 against 12 792 pairs/s)
    if (target == kMaxPassTarget && w.tiles / choose_splits(N, w.panels, w.tiles, kMaxPassTarget) >= 32) target = kMaxPassSlots;
    w.splits0 = choose_splits(N, w.panels, w.tiles, target);
    // The top-2 epilogue of the max pass (and the screening that reads it) where a launch cannot fill the chip and its
    // workgroups are short: the rule that picks kMaxPassTarget above, and FM_MODE_ALONE launches of the same shapes (the
    // answer must not depend on `alone`: the diagnostic entry points lay a workspace out without it).  A batch is bound
    // by the max pass's epilogue and a 1024x1024 pair by its matrix cores: they keep the plain epilogue.
    w.top2 = N * w.panels < kMaxPassSlots && w.tiles / choose_splits(N, w.panels, w.tiles, kMaxPassTarget) < 32;
  }
#ifdef FM_TUNE_ENV
  if (const char* e = getenv("FM_TARGET_WGS0")) w.splits0 = choose_splits(N, w.panels, w.tiles, atoi(e) > 0 ? atoi(e) : kMaxPassTarget);
#endif
  w.splits_s = choose_screen_chunks(N, w.Lp, w.Sp / 32, &w.units_s, alone);
  const size_t rows = (size_t)N * w.Lp, cols = (size_t)N * w.Sp;
  const size_t nblk = (rows * slots + 255) / 256;
  Carver c;      // (every region starts on a 256-byte boundary, and the spans and totals run on to the next one)
  // ---- the common path ----
  c.take(w.cand.count, rows);
  c.take(w.ccand.count, cols);
  c.take(w.cand_b.count, rows);
  c.take(w.ccand_b.count, cols);
  c.take(w.dense_cnt, N);
  w.counters[0] = c.since(w.cand.count.at, 256);
  c.take(w.cell0, rows);
  c.take(w.cell1, cols);
  c.take(w.ties0, kTieCap + 1);
  c.take(w.ties1, kTieCap + 1);
  w.reassign[0] = c.since(w.cell0.at, 256);
  c.take(w.rowmax_u, rows);
  c.take(w.colmax_u, cols);
  c.take(w.blocktot, nblk);
  w.reassign[1] = c.since(w.blocktot.at, 256);
  c.take(w.scalars, 1);
  w.reassign[2] = Span{w.scalars.at, sizeof(Scalars::flags)};     // (dense_units stays: the dense kernels read it)
  w.counters[1] = Span{w.scalars.at, sizeof(Scalars)};
  w.prep_zero = c.since(w.cand.count.at, 256);
  c.take(w.q0, rows * C); c.take(w.q1, cols * C);
  c.take(w.sigimg, (size_t)N * 2);
  c.take(w.imgstat, (size_t)N * 8);
  c.take(w.l1_0, rows); c.take(w.l1_1, cols);
  c.take(w.bstat0, rows / 32); c.take(w.bstat1, cols / 32);
  c.take(w.emarg, N);
  c.take(w.nmr, rows); c.take(w.nmc, cols);
  c.take(w.umax, rows / 32 * (cols / N / 32));
  c.take(w.cand.idx, rows * slots); c.take(w.cand.x, rows * slots);
  c.take(w.ccand.idx, cols * slots); c.take(w.ccand.x, cols * slots);
  c.take(w.thr_r, rows); c.take(w.thr_c, cols);
  c.take(w.wmaxb, rows / 32); c.take(w.cmaxu, cols / 32);
  c.take(w.tmin_r, rows / 32); c.take(w.tmin_c, cols / 32);
  c.take(w.umax2, rows / 32 * (cols / N / 32));
  c.take(w.upos, rows / 32 * (cols / N / 32));
  w.common_total = c.pad();
  // ---- FM_MODE_DENSE / FM_MODE_EXACT_SCREENING / conf_matrix ----
  c.take(w.hi0, rows * C); c.take(w.lo0, rows * C);
  c.take(w.hi1, cols * C); c.take(w.lo1, cols * C);
  c.take(w.f16inv, N);
  c.take(w.rowB, rows * w.splits); c.take(w.colB, cols * w.panels);
  c.take(w.rsum, rows); c.take(w.csum, cols);
  c.take(w.nmr2, rows); c.take(w.nmc2, cols);
  c.take(w.cand_b.idx, rows * slots); c.take(w.cand_b.x, rows * slots);
  c.take(w.ccand_b.idx, cols * slots); c.take(w.ccand_b.x, cols * slots);
  w.total = c.pad();
  return w;
}

}  // namespace fm

using namespace fm;

extern "C" int fm_version(void) { return FM_VERSION; }

extern "C" const char* fm_strerror(int s) {
  switch (s) {
    case FM_OK: return "ok";
    case FM_E_NULL: return "required pointer is NULL";
    case FM_E_SHAPE: return "inconsistent or non-positive shape";
    case FM_E_UNSUPPORTED: return "unsupported configuration (C % 4 == 0 and C <= 256, Cf = 64, W in {5,7}, thr in (0,1))";
    case FM_E_WORKSPACE: return "workspace too small or not 256-byte aligned";
    case FM_E_CAPACITY: return "more matches than the output capacity";
    case FM_E_CANDIDATES: return "a coarse row or column exceeded its candidate slots (FM_MODE_EXACT_SCREENING, then more cand_slots)";
    case FM_E_RANGE: return "descriptor not finite or |x| >= 32768, or similarities of several thousand (screening margin >= 2^60)";
    case FM_E_DENSE: return "flat similarity in a sample: call again with FM_MODE_DENSE";
    case FM_E_INTERNAL: return "assignment kernel: bounded wait for predecessor workgroups ran out; call again";
    case FM_E_STEP: return "int8 screening step too small for a descriptor outside the sampled rows: call again with FM_MODE_EXACT_STEP";
    default: return s > 0 ? hipGetErrorString((hipError_t)s) : "unknown fmatch status";
  }
}

extern "C" int fm_default_cand_slots(float thr) {
  if (!(thr > 0.f)) return 64;
  int need = (int)ceilf(1.0f / thr) + 3;
  int s = 8;
  while (s < need && s < 64) s <<= 1;
  return s;
}

// a power of two in [4, 64]: a row's slots are adjacent lanes of one wave and k_keep_emit keeps 256/slots <= 64 rows
static bool valid_slots(int s) { return s >= 4 && s <= 64 && (s & (s - 1)) == 0; }

constexpr int kKnownModes = FM_MODE_DENSE | FM_MODE_EXACT_SCREENING | FM_MODE_NO_CELL_MAPS | FM_MODE_EXACT_STEP | FM_MODE_STATS |
                            FM_MODE_FLAT | FM_MODE_ALONE;

static int check_coarse_shape(int N, int L, int S, int C, int cand_slots) {
  if (N <= 0 || L <= 0 || S <= 0) return FM_E_SHAPE;
  if (!valid_channels(C) || !valid_slots(cand_slots)) return FM_E_UNSUPPORTED;
  return FM_OK;
}

// The checks of an entry point that works on a coarse workspace (its pointers, then the shape), then the layout.
static int checked_layout(bool have_ptrs, int N, int L, int S, int C, int cand_slots, CoarseWs* w) {
  if (!have_ptrs) return FM_E_NULL;
  if (const int bad = check_coarse_shape(N, L, S, C, cand_slots)) return bad;
  *w = coarse_layout(N, L, S, C, cand_slots);
  return FM_OK;
}

// Everything a coarse call decides from its mode bits, from whether the dense conf_matrix is wanted and from its
// candidate slots: which launches coarse_match_impl enqueues, with which switches, and how much workspace they need.
struct CoarsePlan {
  bool alone;          // FM_MODE_ALONE: launch geometry only
  bool exact_step;     // prep finds the images' largest |x| first (one small kernel) and the int8 step from them
  bool flat;           // prep writes every sample's float16 planes and k_stab stands in for the screening kernel
  bool allow_dead;     // dead-row certificates: only when nobody reads every row's denominator
  bool prep_f16;       // the float16 planes of the flagged samples; f16_force 1: of every sample, 2: hi planes of the
  int f16_force;       // other samples too (the conf sweep alone wants them)
  bool dense;          // the dense sum kernel redoes the flagged samples; the workspace's dense region
  float list_cap;      // the dense kernels list candidates down to min(thr, list_cap)
  bool reduce;         // k_reduce_sums: the softmax denominators of EVERY row and column
  bool rescreen;       // the exact re-screening sweep
  bool exact_lists;    // k_exact_lists: the dense kernel's lists and their denominators made exact together
  bool conf;           // the dense conf_matrix sweep and its patch
  bool cell_maps;      // the assignment writes the cell -> match maps
  SelectFlags select(bool deferred) const { return {rescreen, dense, cell_maps, reduce, deferred}; }
  size_t workspace_bytes(const CoarseWs& w) const { return dense ? w.total : w.common_total; }
};

static CoarsePlan plan_coarse(int mode, bool conf, int cand_slots) {
  const bool all_rows = conf || (mode & FM_MODE_STATS) != 0;    // the statistics of EVERY row and column are read
  CoarsePlan p;
  p.alone = (mode & FM_MODE_ALONE) != 0;
  p.exact_step = (mode & FM_MODE_EXACT_STEP) != 0;
  // (the FM_MODE_FLAT hint is not taken when every row is read: their exact rewrite reads the screening kernel's lists)
  p.flat = (mode & FM_MODE_FLAT) != 0 && !all_rows;
  p.allow_dead = !all_rows;
  // (the exact screening and the conf_matrix sweep read the float16 planes too)
  p.dense = all_rows || (mode & (FM_MODE_DENSE | FM_MODE_EXACT_SCREENING | FM_MODE_FLAT)) != 0;
  p.prep_f16 = p.dense && !p.flat;
  p.f16_force = (mode & FM_MODE_EXACT_SCREENING) ? 1 : (conf ? 2 : 0);
  // (a conf_matrix request: candidates down to min(thr, 0.1) - the lists then name every entry of a dense sample with
  // conf > 0.1, which k_exact_lists resolves from exact dot products; the assignment applies thr itself.  thr < 1)
  p.list_cap = conf ? 0.1f : 1.f;
  p.rescreen = (mode & FM_MODE_EXACT_SCREENING) != 0;
  // The assignment folds the softmax denominators of its candidates from the partial sums itself.  FM_MODE_FLAT with
  // more than the default 8 slots (rows without a peak next to peaked ones): every sample's denominators are folds of
  // the dense kernel's 13 + 19 partials, and the assignment would redo them for every candidate and every competing row
  // - 35 us at 16 slots against 21 us with one reduction launch (5 us) in front; at 8 slots the rows hold one or two
  // candidates and the launch costs more than it saves
  p.reduce = p.rescreen || all_rows || (p.flat && cand_slots > 8);
  p.exact_lists = all_rows;
  p.conf = conf;
  p.cell_maps = (mode & FM_MODE_NO_CELL_MAPS) == 0;
  return p;
}

extern "C" int fm_coarse_workspace_bytes_mode(int N, int L, int S, int C, int cand_slots, int mode, int want_conf_matrix,
                                              size_t* bytes) {
  CoarseWs w;
  if (const int bad = checked_layout(bytes != nullptr, N, L, S, C, cand_slots, &w)) return bad;
  if (mode & ~kKnownModes) return FM_E_UNSUPPORTED;
  *bytes = plan_coarse(mode, want_conf_matrix != 0, cand_slots).workspace_bytes(w);
  return FM_OK;
}

extern "C" int fm_coarse_workspace_bytes(int N, int L, int S, int C, int cand_slots, size_t* bytes) {
  return fm_coarse_workspace_bytes_mode(N, L, S, C, cand_slots, FM_MODE_DENSE | FM_MODE_EXACT_SCREENING, 1, bytes);
}

// Diagnostic: the workspace layout (ints then byte offsets), so that tests can inspect the
// intermediate statistics of a run.  out[0..9] = N,L,S,C,Lp,Sp,panels,tiles,splits,slots;
// out[10..] = cand_count, ccand_count, scalars, blocktot, hi0, lo0, hi1, lo1, q0, q1, sigimg, l1_0,
// nmr, nmr (22, 23: the slots of two zero-length regions that lay in front of nmr, so its offset is what they always
// held), rowB, colB, nmr, nmc, rsum, csum, cand_j, cand_x, ccand_i, umax, dense_cnt, rowmax_u,
// colmax_u, splits_s, units_s, total; out[40] = common_total (when n_out > 40)  (40 or 41 values).
extern "C" int fm_debug_coarse_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out) {
  if (!out) return FM_E_NULL;
  if (n_out < 40) return FM_E_SHAPE;
  CoarseWs w;
  if (const int bad = checked_layout(true, N, L, S, C, cand_slots, &w)) return bad;
  const auto at = [](const auto& r) { return (int64_t)r.at; };
  const int64_t v[41] = {w.N, w.L, w.S, w.C, w.Lp, w.Sp, w.panels, w.tiles, w.splits, w.slots,
                         at(w.cand.count), at(w.ccand.count), at(w.scalars), at(w.blocktot), at(w.hi0), at(w.lo0),
                         at(w.hi1), at(w.lo1), at(w.q0), at(w.q1), at(w.sigimg), at(w.l1_0), at(w.nmr), at(w.nmr),
                         at(w.rowB), at(w.colB), at(w.nmr), at(w.nmc), at(w.rsum), at(w.csum), at(w.cand.idx),
                         at(w.cand.x), at(w.ccand.idx), at(w.umax), at(w.dense_cnt), at(w.rowmax_u), at(w.colmax_u),
                         w.splits_s, w.units_s, (int64_t)w.total, (int64_t)w.common_total};
  for (int i = 0; i < 40; ++i) out[i] = v[i];
  if (n_out > 40) out[40] = v[40];
  return FM_OK;
}

template <int K>
static hipError_t clear_spans(char* base, const Span (&spans)[K], hipStream_t st) {
  for (const Span& s : spans) {
    const hipError_t e = hipMemsetAsync(base + s.at, 0, s.bytes, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Enqueues the plan of (mode, conf_matrix, cand_slots) top to bottom.  resume (fm_coarse_match_auto): a call with the
// same arguments on the common path - mode without FM_MODE_DENSE, the only plan whose screening reports flat similarity -
// reported just that; its prep, max pass and screening results are in the workspace, so what its assignment left is
// cleared and the plan of mode | FM_MODE_DENSE continues from the float16 planes.
static int coarse_match_impl(const CoarseCall& c, const MapCopyJob* job, bool resume) {
  if (!c.feat0 || !c.feat1 || !c.workspace || !c.d_count) return FM_E_NULL;
  if (c.in_dtype != FM_F32 && c.in_dtype != FM_F16 && c.in_dtype != FM_BF16) return FM_E_UNSUPPORTED;
  if (c.cap > 0 && (!c.b_ids || !c.i_ids || !c.j_ids || !c.mkpts0_c || !c.mkpts1_c || !c.mconf)) return FM_E_NULL;
  if (c.cap < 0 || c.L != c.h0c * c.w0c || c.S != c.h1c * c.w1c) return FM_E_SHAPE;
  if (const int bad = check_coarse_shape(c.N, c.L, c.S, c.C, c.cand_slots)) return bad;
  if (!(c.thr > 0.f) || !(c.thr < 1.f) || !(c.temperature > 0.f)) return FM_E_UNSUPPORTED;
  if (c.mode & ~kKnownModes) return FM_E_UNSUPPORTED;
  const CoarsePlan p = plan_coarse(c.mode, c.conf_matrix != nullptr, c.cand_slots);
  const CoarseWs w = coarse_layout(c.N, c.L, c.S, c.C, c.cand_slots, p.alone);
  if (!workspace_ok(c.workspace, c.workspace_bytes, p.workspace_bytes(w))) return FM_E_WORKSPACE;
  char* base = (char*)c.workspace;
  hipStream_t st = (hipStream_t)c.stream;
  const float inv_ct = inv_ct_of(c.C, c.temperature);
  const float thr_list = fminf(c.thr, p.list_cap);     // candidate threshold of the dense kernels' LISTS
#define FM_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)
  if (!resume) {
    // The common path is four launches: prep -> max pass -> sparse sum kernel -> assignment.
    // prep: clear the per-call counters, quantise both images (one int8 step per image), L1 norms
    FM_TRY(launch_prep(c.feat0, c.feat1, c.in_dtype, c.C, w, base, p.exact_step, p.flat, st));
    // max pass: row / column / unit maxima of the integer screening product (atomicMax: no partials, no reduction kernel)
    FM_TRY(launch_max_i8(w, base, unit_cert_on(w, !p.dense), st));
    // sparse sum kernel: stabilisers, live units, exact terms of the few significant entries, candidates (listed per row
    // and per column); flags the samples with too many significant entries per unit (flat similarity).  FM_MODE_FLAT:
    // the sweep would only find that out again - a small kernel forms the stabilisers and flags every sample
    if (p.flat) FM_TRY(launch_stab(w, base, inv_ct, c.thr, p.allow_dead, st));
    // (sure entries without their exact dot product only where the assignment is the lists' sole reader: fm_internal.h)
    else FM_TRY(launch_screen(c.feat0, c.feat1, c.in_dtype, c.C, w, base, inv_ct, c.thr, p.dense, p.allow_dead,
                              defer_exact_on(w, !p.dense), st));
  } else {
    FM_TRY(clear_spans(base, w.reassign, st));
  }
  if (p.prep_f16) FM_TRY(launch_prep_f16(c.feat0, c.feat1, c.in_dtype, c.C, w, base, p.f16_force, st));
  // (the dense sum kernel redoes the flagged samples - one arithmetic per sample keeps exact conf ties exact - and exits
  // at once when there are none)
  if (p.dense) FM_TRY(launch_dense(w, base, inv_ct, thr_list, st));
  if (p.reduce) FM_TRY(launch_reduce(w, base, inv_ct, st));
  // (exits immediately unless the sum kernels' screening overflowed a row's slots)
  if (p.rescreen) FM_TRY(launch_dense(w, base, inv_ct, thr_list, st, nullptr, 1));
  if (p.exact_lists) FM_TRY(launch_exact_lists(w, base, inv_ct, c.feat0, c.feat1, c.in_dtype, c.C, st));
  if (p.conf) {
    // dense data['conf_matrix'] (one more sweep), whose hi/lo-split products carry 22 bits: the entries that matter are
    // rewritten from their exact float32 dot products (the rows' lists of significant entries)
    FM_TRY(launch_dense(w, base, inv_ct, c.thr, st, c.conf_matrix));
    FM_TRY(launch_conf_patch(w, base, inv_ct, c.conf_matrix, st));
  }
#undef FM_TRY
  // (the lists hold tagged entries when this call's screening deferred, or - resume - when the common-path call did
  // whose results this one continues)
  return (int)launch_select(w, base, c, inv_ct, p.select(defer_exact_on(w, resume || !p.dense)), job);
}

extern "C" int fm_coarse_match(const float* feat0, const float* feat1, int N, int L, int S, int C, int h0c, int w0c,
                               int h1c, int w1c, float temperature, float thr, int border_rm, float scale_px,
                               const float* scale0, const float* scale1, void* workspace, size_t workspace_bytes,
                               int cand_slots, int mode, int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                               float* mkpts0_c, float* mkpts1_c, float* mconf, int cap, int32_t* d_count,
                               float* conf_matrix, void* stream) {
  const CoarseCall c{feat0, feat1, FM_F32, N, L, S, C, h0c, w0c, h1c, w1c, temperature, thr, border_rm, scale_px, scale0, scale1,
                     workspace, workspace_bytes, cand_slots, mode, b_ids, i_ids, j_ids, mkpts0_c, mkpts1_c, mconf, cap,
                     d_count, conf_matrix, stream};
  return coarse_match_impl(c, nullptr, false);
}

extern "C" int fm_coarse_match_dtype(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                                     int h0c, int w0c, int h1c, int w1c, float temperature, float thr, int border_rm,
                                     float scale_px, const float* scale0, const float* scale1, void* workspace,
                                     size_t workspace_bytes, int cand_slots, int mode, int64_t* b_ids,
                                     int64_t* i_ids, int64_t* j_ids, float* mkpts0_c, float* mkpts1_c, float* mconf,
                                     int cap, int32_t* d_count, float* conf_matrix, void* stream) {
  const CoarseCall c{feat0, feat1, in_dtype, N, L, S, C, h0c, w0c, h1c, w1c, temperature, thr, border_rm, scale_px, scale0,
                     scale1, workspace, workspace_bytes, cand_slots, mode, b_ids, i_ids, j_ids, mkpts0_c, mkpts1_c, mconf, cap,
                     d_count, conf_matrix, stream};
  return coarse_match_impl(c, nullptr, false);
}

// fm_coarse_match_dtype + the channels-last copy of image 1's fine map as a side job of the assignment launch
extern "C" int fm_coarse_match_maps(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                                    int h0c, int w0c, int h1c, int w1c, float temperature, float thr, int border_rm,
                                    float scale_px, const float* scale0, const float* scale1, void* workspace,
                                    size_t workspace_bytes, int cand_slots, int mode, int64_t* b_ids,
                                    int64_t* i_ids, int64_t* j_ids, float* mkpts0_c, float* mkpts1_c, float* mconf,
                                    int cap, int32_t* d_count, float* conf_matrix, const float* feat_f1, int Nf, int Cf,
                                    int Hf1, int Wf1, void* scratch1, void* stream) {
  if (!feat_f1 || !scratch1) return FM_E_NULL;
  if (Nf <= 0 || Hf1 <= 0 || Wf1 <= 0) return FM_E_SHAPE;
  if (Cf != 64) return FM_E_UNSUPPORTED;
  if (((uintptr_t)scratch1 & 15) || ((uintptr_t)feat_f1 & 15)) return FM_E_WORKSPACE;
  const MapCopyJob job{feat_f1, (float*)scratch1, Nf, Hf1, Wf1};
  const CoarseCall c{feat0, feat1, in_dtype, N, L, S, C, h0c, w0c, h1c, w1c, temperature, thr, border_rm, scale_px, scale0,
                     scale1, workspace, workspace_bytes, cand_slots, mode, b_ids, i_ids, j_ids, mkpts0_c, mkpts1_c, mconf, cap,
                     d_count, conf_matrix, stream};
  return coarse_match_impl(c, &job, false);
}

// ---------------------------------------------------------------------------------------------------------------------
// fm_coarse_match_auto: ONE call for any data (the reference's CoarseMatching.forward is one call,
// network/utils/coarse_matching_new.py:43-73).  The data-dependent conditions the device reports - flat similarity,
// candidate-slot overflow, a clipped int8 step, the assignment's bounded wait - are answered here, on the host, behind
// the host sync the reference has too (torch.where, :109); what is left for the caller is FM_E_CAPACITY (its output
// buffers are too small: *m_out = the capacity needed), FM_E_RANGE (bad input) and argument errors.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kAutoDataModes = FM_MODE_DENSE | FM_MODE_EXACT_SCREENING | FM_MODE_EXACT_STEP | FM_MODE_FLAT;

extern "C" int fm_coarse_workspace_bytes_auto(int N, int L, int S, int C, int max_cand_slots, size_t* bytes) {
  if (max_cand_slots == 0) max_cand_slots = 64;
  return fm_coarse_workspace_bytes(N, L, S, C, max_cand_slots, bytes);
}

extern "C" int fm_coarse_match_auto(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                                    int h0c, int w0c, int h1c, int w1c, float temperature, float thr, int border_rm,
                                    float scale_px, const float* scale0, const float* scale1, void* workspace,
                                    size_t workspace_bytes, int max_cand_slots, int mode, int64_t* b_ids, int64_t* i_ids,
                                    int64_t* j_ids, float* mkpts0_c, float* mkpts1_c, float* mconf, int cap,
                                    int32_t* d_count, float* conf_matrix, int32_t* hint_io, int32_t* m_out,
                                    int32_t* info_out, void* stream) {
  if (!m_out) return FM_E_NULL;
  if (max_cand_slots == 0) max_cand_slots = 64;
  if (!valid_slots(max_cand_slots)) return FM_E_UNSUPPORTED;
  if (mode & ~kKnownModes) return FM_E_UNSUPPORTED;
  if (!(thr > 0.f) || !(thr < 1.f)) return FM_E_UNSUPPORTED;
  const int slots0 = fm_default_cand_slots(thr) < max_cand_slots ? fm_default_cand_slots(thr) : max_cand_slots;
  // the caller's fixed options (cell maps, statistics) stay; the data-dependent bits it passes are a starting point
  const int fixed = mode & ~kAutoDataModes;
  const bool full_stats = conf_matrix != nullptr || (mode & FM_MODE_STATS) != 0;
  int cur = mode & kAutoDataModes;
  if (full_stats) cur |= FM_MODE_EXACT_SCREENING;        // (that path runs the denominator reduction the re-screening needs anyway)
  int slots = slots0;
  if (conf_matrix && slots < 16 && max_cand_slots >= 16) slots = 16;     // (its dense lists go down to conf 0.1: <= 10 + band per row)
  const int slots_start = slots;                         // what this REQUEST starts with: not something the data taught
  if (hint_io && *hint_io) {                             // what served the previous call of this kind
    cur |= *hint_io & kAutoDataModes;
    const int hs = (*hint_io >> 8) & 0xff;
    if (valid_slots(hs) && hs <= max_cand_slots && hs > slots) slots = hs;
  }
  bool tried_wide = slots > slots0, retried_internal = false;
  int st = FM_OK;
  int32_t m = 0, info = 0;
  int attempts = 0;
  // one call for every attempt: only its slots and its mode change
  CoarseCall c{feat0, feat1, in_dtype, N, L, S, C, h0c, w0c, h1c, w1c, temperature, thr, border_rm, scale_px, scale0, scale1,
               workspace, workspace_bytes, slots, mode, b_ids, i_ids, j_ids, mkpts0_c, mkpts1_c, mconf, cap, d_count,
               conf_matrix, stream};
  for (int attempt = 0; attempt < 10; ++attempt) {
    ++attempts;
    const int call_mode = fixed | cur | ((cur & FM_MODE_FLAT) ? FM_MODE_DENSE : 0);
    // every attempt must fit the caller's workspace (sized by fm_coarse_workspace_bytes_auto for max_cand_slots)
    c.cand_slots = slots; c.mode = call_mode;
    st = coarse_match_impl(c, nullptr, false);
    if (st != FM_OK) return st;
    st = fm_read_count_info(d_count, cap, &m, &info, stream);
    if (st == FM_E_DENSE && !(cur & FM_MODE_DENSE) && !conf_matrix && !(mode & FM_MODE_STATS)) {
      // the common path's own results are still in the workspace: add the dense kernels' part and assign again
      cur |= FM_MODE_DENSE;
      // (the resume clears the WHOLE status word: only when "flat similarity" is all it holds - anything else the device
      // reported with it would be dropped, so such a call is repeated from the start instead)
      if ((info & ~FM_DEV_ALL_DENSE) != FM_DEV_DENSE) continue;
      c.mode = fixed | cur;
      st = coarse_match_impl(c, nullptr, true);
      if (st != FM_OK) return st;
      st = fm_read_count_info(d_count, cap, &m, &info, stream);
    }
    if (st == FM_OK) break;
    if (st == FM_E_STEP && !(cur & FM_MODE_EXACT_STEP)) { cur |= FM_MODE_EXACT_STEP; continue; }
    if (st == FM_E_DENSE && !(cur & FM_MODE_DENSE)) { cur |= FM_MODE_DENSE; continue; }
    if (st == FM_E_CANDIDATES && (cur & FM_MODE_DENSE) && !tried_wide && slots < 16 && max_cand_slots >= 16 &&
        !(cur & FM_MODE_EXACT_SCREENING)) {
      // rows without a peak next to peaked ones hold more near-candidates than the default slots: twice the slots and
      // the int8 step from the images' true maxima (margins 1.5x narrower) before the exact re-screening sweep
      slots = 16; cur |= FM_MODE_EXACT_STEP; tried_wide = true;
      continue;
    }
    if (st == FM_E_CANDIDATES && !(cur & FM_MODE_EXACT_SCREENING)) {
      if (tried_wide) slots = slots0;                    // the wider lists did not hold them either
      cur |= FM_MODE_EXACT_SCREENING | FM_MODE_DENSE;
      continue;
    }
    if (st == FM_E_CANDIDATES && slots < max_cand_slots) { slots *= 2; continue; }
    if (st == FM_E_INTERNAL && !retried_internal) { retried_internal = true; continue; }
    break;                                               // FM_E_CAPACITY, FM_E_RANGE, what persists: the caller's
  }
  *m_out = m;
  if (info_out) *info_out = info;
  if (hint_io && (st == FM_OK || st == FM_E_CAPACITY)) {
    int learnt = cur & kAutoDataModes;
    if (full_stats) learnt &= ~FM_MODE_EXACT_SCREENING | (mode & FM_MODE_EXACT_SCREENING);   // (implied by the request, not learnt)
    // every sample went to the dense sum kernel: the next call of this kind skips the screening sweep (FM_MODE_FLAT)
    if ((learnt & FM_MODE_DENSE) && !full_stats) {
      if (info & FM_DEV_ALL_DENSE) learnt |= FM_MODE_FLAT; else learnt &= ~FM_MODE_FLAT;
    }
    // second byte: the slots the DATA asked for beyond this request's own starting point (0 = none: a conf_matrix
    // call's 16 are implied by the request and must not follow plain calls of the shape); third byte: the slot count
    // the serving attempt ran with - ALWAYS written (the workspace layout fm_coarse_cell_maps / fm_coarse_softmax_stats
    // must be asked for), ignored on input
    *hint_io = learnt | (slots != slots_start ? slots << 8 : 0) | (slots << 16) | (attempts << 24);
  }
  return st;
}

// Device pointers of the cell -> (match index + 1) maps the coarse stage leaves in its workspace
// (0 = cell unmatched; pitch = padded cells per sample).  fm_gather_windows_cells consumes them.
extern "C" int fm_coarse_cell_maps(void* workspace, int N, int L, int S, int C, int cand_slots, int32_t** cell0,
                                   int* pitch0, int32_t** ties0, int32_t** cell1, int* pitch1, int32_t** ties1) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && cell0 && cell1 && pitch0 && pitch1 && ties0 && ties1, N, L, S, C,
                                     cand_slots, &w))
    return bad;
  *cell0 = w.cell0.in(workspace); *pitch0 = w.Lp; *ties0 = w.ties0.in(workspace);
  *cell1 = w.cell1.in(workspace); *pitch1 = w.Sp; *ties1 = w.ties1.in(workspace);
  return FM_OK;
}

// Device pointers of the softmax statistics the coarse stage leaves in its workspace when it ran with FM_MODE_STATS or a
// conf_matrix request: softmax(sim, dim 2)[b,i,j] = exp2(k2 x + nm_r[b * pitch_r + i]) / sum_r[b * pitch_r + i] and
// softmax(sim, dim 1)[b,i,j] = exp2(k2 x + nm_c[b * pitch_c + j]) / sum_c[b * pitch_c + j] with x = feat0[b,i] . feat1[b,j]
// and k2 = log2(e) / (C temperature).
extern "C" int fm_coarse_softmax_stats(void* workspace, int N, int L, int S, int C, int cand_slots, const float** nm_r,
                                       const float** sum_r, int* pitch_r, const float** nm_c, const float** sum_c,
                                       int* pitch_c) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && nm_r && sum_r && pitch_r && nm_c && sum_c && pitch_c, N, L, S, C,
                                     cand_slots, &w))
    return bad;
  *nm_r = w.nmr.in(workspace); *sum_r = w.rsum.in(workspace); *pitch_r = w.Lp;
  *nm_c = w.nmc.in(workspace); *sum_c = w.csum.in(workspace); *pitch_c = w.Sp;
  return FM_OK;
}

// Diagnostic: launch ONE correlation sweep (mode 0 = pass A, 1 = pass B) on a workspace that a
// previous fm_coarse_match call with the same shapes has filled, so that a benchmark can bracket
// exactly that kernel with events.  Pass B's candidate counters are zeroed first (outside any
// bracket the caller places after this function's memset is enqueued... the memset precedes the kernel).
extern "C" int fm_debug_launch_corr(void* workspace, int N, int L, int S, int C, int cand_slots, float temperature,
                                    float thr, int mode, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace, N, L, S, C, cand_slots, &w)) return bad;
  if (mode < 0 || mode > 2) return FM_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) return (int)launch_max_i8(w, (char*)workspace, unit_cert_on(w), st);
  if (mode == 1) return (int)launch_dense(w, (char*)workspace, inv_ct_of(C, temperature), thr, st);
  return (int)launch_dense(w, (char*)workspace, inv_ct_of(C, temperature), thr, st, nullptr, 1);      // mode 2: the re-screening
}

// Diagnostic: launch the sparse sum kernel alone on a workspace a previous fm_coarse_match filled.
extern "C" int fm_debug_launch_screen(void* workspace, const float* feat0, const float* feat1, int N, int L, int S,
                                          int C, int cand_slots, float temperature, float thr, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && feat0 && feat1, N, L, S, C, cand_slots, &w)) return bad;
  return (int)launch_screen(feat0, feat1, FM_F32, C, w, (char*)workspace, inv_ct_of(C, temperature), thr, 1, 1,
                            defer_exact_on(w), (hipStream_t)stream);
}

// Diagnostic: launch k_prep_split alone (it clears the per-call counters: run a complete fm_coarse_match afterwards
// before anything reads the workspace's candidate lists again).
extern "C" int fm_debug_launch_prep(void* workspace, const float* feat0, const float* feat1, int N, int L, int S, int C,
                                    int cand_slots, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && feat0 && feat1, N, L, S, C, cand_slots, &w)) return bad;
  return (int)launch_prep(feat0, feat1, FM_F32, C, w, (char*)workspace, 0, 0, (hipStream_t)stream);
}

// Diagnostic: launch the float16 plane kernel alone (force = 1: every sample; 0: the samples flagged for the dense
// kernel) on a workspace a previous fm_coarse_match filled.
extern "C" int fm_debug_launch_prep_f16(void* workspace, const float* feat0, const float* feat1, int N, int L, int S,
                                        int C, int cand_slots, int force, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && feat0 && feat1, N, L, S, C, cand_slots, &w)) return bad;
  return (int)launch_prep_f16(feat0, feat1, FM_F32, C, w, (char*)workspace, force, (hipStream_t)stream);
}

// Diagnostic: the two launches FM_MODE_FLAT has of its own (which = 0: k_prep_split writing the float16 planes too,
// 1: k_stab) on a workspace a previous FM_MODE_FLAT call filled.
extern "C" int fm_debug_launch_flat(void* workspace, const float* feat0, const float* feat1, int N, int L, int S, int C,
                                    int cand_slots, float temperature, float thr, int which, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace && feat0 && feat1, N, L, S, C, cand_slots, &w)) return bad;
  if (which < 0 || which > 1) return FM_E_UNSUPPORTED;
  if (which == 0) return (int)launch_prep(feat0, feat1, FM_F32, C, w, (char*)workspace, 0, 1, (hipStream_t)stream);
  return (int)launch_stab(w, (char*)workspace, inv_ct_of(C, temperature), thr, 1, (hipStream_t)stream);
}

// Diagnostic: zero the candidate counters and the scalars, so that the sum kernels can be launched again on a
// workspace whose max-pass results are kept.
extern "C" int fm_debug_reset_counters(void* workspace, int N, int L, int S, int C, int cand_slots, void* stream) {
  CoarseWs w;
  if (const int bad = checked_layout(workspace, N, L, S, C, cand_slots, &w)) return bad;
  return (int)clear_spans((char*)workspace, w.counters, (hipStream_t)stream);
}

// Test-only switch of the unit certificate (process-global; returns the previous value, mode outside 0..2 only reads).
extern "C" int fm_debug_unit_cert(int mode) {
  const int prev = g_unit_cert;
  if (mode >= 0 && mode <= 2) g_unit_cert = mode;
  return prev;
}

// Diagnostic: where the certificate's arrays live (byte offsets: umax, umax2, upos, thr_r, thr_c, tmin_r, tmin_c, the
// counter of certified units) and whether the launch plan of this shape uses them (out[8]).
extern "C" int fm_debug_unit_cert_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out) {
  if (!out) return FM_E_NULL;
  if (n_out < 9) return FM_E_SHAPE;
  CoarseWs w;
  if (const int bad = checked_layout(true, N, L, S, C, cand_slots, &w)) return bad;
  const int64_t v[9] = {(int64_t)w.umax.at, (int64_t)w.umax2.at, (int64_t)w.upos.at, (int64_t)w.thr_r.at, (int64_t)w.thr_c.at,
                        (int64_t)w.tmin_r.at, (int64_t)w.tmin_c.at, (int64_t)(w.scalars.at + offsetof(Scalars, cert_units)), w.top2};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return FM_OK;
}

// Test-only switch of the deferred exact dot products (process-global; returns the previous value, mode outside 0..2
// only reads).
extern "C" int fm_debug_defer_exact(int mode) {
  const int prev = g_defer_exact;
  if (mode >= 0 && mode <= 2) g_defer_exact = mode;
  return prev;
}

// Diagnostic: byte offset of the per-call counter of deferred entries, the tag bit of a list index, and whether the
// common path of this shape defers under the present switch (3 values).
extern "C" int fm_debug_defer_exact_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out) {
  if (!out) return FM_E_NULL;
  if (n_out < 3) return FM_E_SHAPE;
  CoarseWs w;
  if (const int bad = checked_layout(true, N, L, S, C, cand_slots, &w)) return bad;
  out[0] = (int64_t)(w.scalars.at + offsetof(Scalars, defer_entries));
  out[1] = 0x40000000;
  out[2] = defer_exact_on(w) ? 1 : 0;
  return FM_OK;
}

extern "C" int fm_read_count(const int32_t* d_count, int cap, int32_t* m_out, void* stream) {
  return fm_read_count_info(d_count, cap, m_out, nullptr, stream);
}

extern "C" int fm_read_count_info(const int32_t* d_count, int cap, int32_t* m_out, int32_t* info_out, void* stream) {
  if (!d_count || !m_out) return FM_E_NULL;
  int32_t h[2] = {0, 0};
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(h, d_count, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return (int)e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  *m_out = h[0];
  if (info_out) *info_out = h[1];
  if (h[1] & FM_DEV_INTERNAL) return FM_E_INTERNAL;
  if (h[1] & FM_DEV_RANGE) return FM_E_RANGE;
  if (h[1] & FM_DEV_STEP) return FM_E_STEP;
  if (h[1] & FM_DEV_DENSE) return FM_E_DENSE;
  if (h[1] & FM_DEV_CANDIDATES) return FM_E_CANDIDATES;
  if (h[1] & FM_DEV_CAPACITY) return FM_E_CAPACITY;
  if (h[0] > cap) return FM_E_CAPACITY;
  return FM_OK;
}
