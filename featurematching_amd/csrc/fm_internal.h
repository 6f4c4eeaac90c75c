// Internal declarations shared by the translation units of libfmatch_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "fmatch.h"

namespace fm {

constexpr int kPanelRows = 256;   // coarse rows (image-0 cells) one workgroup owns
constexpr int kTieCap = 1023;        // listed tie losers per image; beyond it the gathers scan the match list
constexpr int kTileCols = 64;     // coarse columns (image-1 cells) per streamed tile
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kSkipLog2 = 32.f;    // terms more than 2^32 below every stabiliser are negligible (see sig_threshold in coarse_screen.hip)
// internal status bit (not reported): pass B's max-based screening overflowed a row's slots
constexpr unsigned FM_INT_SCREEN_OVERFLOW = 16u;
constexpr unsigned FM_INT_LOOKBACK_TIMEOUT = 64u;   // k_select: a predecessor's total never showed up (reported as FM_DEV_INTERNAL)
constexpr int kPrepSampleRows = 32;  // rows of an image every k_prep_split workgroup samples for the image's int8 step
constexpr float kPrepHeadroom = 1.5f; // step = headroom * (largest |x| of the sample) / 127: what lies beyond is clipped
                                      // and accounted for in the screening margins (fm_device.h)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// descriptor channels the kernels are instantiated for; smaller C is zero-padded by k_prep_split
inline int padded_channels(int c) { return c <= 64 ? 64 : (c <= 128 ? 128 : 256); }
inline bool valid_channels(int c) { return c >= 4 && c <= 256 && c % 4 == 0; }
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// bytes [at, at + bytes) of a workspace: a range that is set as a whole (hipMemsetAsync), whatever arrays lie in it
struct Span {
  size_t at, bytes;
  char* in(void* base) const { return static_cast<char*>(base) + at; }
};
// Where a workspace's array of T starts.  in(base) is its pointer: the element type is stated once, where the region is
// declared, and a launcher that hands it to a kernel argument of another type does not compile.
template <typename T>
struct Region {
  size_t at;
  T* in(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + at); }
  static size_t bytes(size_t count) { return count * sizeof(T); }
};
// Lays a workspace out front to back; `o` is the bytes taken so far.
struct Carver {
  size_t o = 0;
  size_t pad(size_t align = 256) { return o = (o + align - 1) / align * align; }     // on to the next boundary
  // r = the next `count` elements of r's type, from an `align`-byte boundary on (sizeof(T): packed behind the last one)
  template <typename T>
  void take(Region<T>& r, size_t count, size_t align = 256) { r.at = pad(align); o += r.bytes(count); }
  // what was taken from `at` on; align: through the padding behind the last region
  Span since(size_t at, size_t align = 1) { return Span{at, pad(align) - at}; }
};
// the caller's workspace holds `need` bytes and is aligned (else FM_E_WORKSPACE)
inline bool workspace_ok(const void* workspace, size_t have, size_t need, size_t align = 256) {
  return have >= need && ((uintptr_t)workspace & (align - 1)) == 0;
}
// one listing of the candidates, per row or per column: how many each holds, then `slots` entries each - the index on
// the other side and the exact dot product
struct CandList { Region<int> count, idx; Region<float> x; };

// A runtime choice as a compile-time constant, so that a launch's argument list is written once: with_window calls
// f(int_c<W>) for the window sizes the fine kernels are instantiated for and returns false (f not called) for any other
// size; which status that is stays with the entry point's own checks.
template <int V> using int_c = std::integral_constant<int, V>;
template <typename F>
inline bool with_window(int W, F&& f) {
  if (W == 5) f(int_c<5>{});
  else if (W == 7) f(int_c<7>{});
  else return false;
  return true;
}

// what every window-crop entry point asks of the batch, a fine map, the stride and the list capacity (else FM_E_SHAPE)
inline bool crop_shape_ok(int N, int Hf, int Wf, int stride, int m_max) {
  return N > 0 && Hf > 0 && Wf > 0 && stride > 0 && m_max >= 0;
}

// the generic crop kernels and the crop's backward take any window up to 15 x 15 of up to 512 channels
inline bool generic_window_shape_ok(int Cf, int W) { return Cf > 0 && W > 0; }
inline bool generic_window_supported(int Cf, int W, int layout) {
  return W <= 15 && Cf <= 512 && (layout == 0 || layout == 1);
}
inline bool map_dtype_ok(int dt) { return dt == FM_F32 || dt == FM_F16 || dt == FM_BF16; }
// f(int_c<dt>) for a fine map's element type (map_dtype_ok(dt) is the caller's to have checked: anything else is float32)
template <typename F>
inline void with_map_dtype(int dt, F&& f) {
  if (dt == FM_F16) f(int_c<FM_F16>{});
  else if (dt == FM_BF16) f(int_c<FM_BF16>{});
  else f(int_c<FM_F32>{});
}

// One window call as the crop ABI takes it: which W x W windows of which one or two fine maps, named by a match list.
// Every forward entry point of fine.hip fills one and hands it on (window_status, window_route); what an entry point
// does not have stays NULL / 0.
struct WindowImage {
  const void* feat; int Hf, Wf, h_c, w_c;
  const int64_t* ids;
  const int32_t* cell_map; int cell_pitch; const int32_t* ties;     // cell order: this image's cell -> match map, tie list
  float* out; const float* ctx;                                     // ctx: the merge's per-cell context table
};
struct WindowCall {
  int images; WindowImage im[2];                                    // im[1] is not looked at when images == 1
  int N, Cf, W, stride, pad, layout, dtype;
  const int64_t* b_ids; const int32_t* d_count; int m_max;
  const void* wpack;                                                // packed merge weights
  void* stream;
  bool cells, merge;    // cell order (else list order); crop + context merge.  h_c is looked at only where one is set
  bool free_size;       // fm_gather_windows*: Cf and W are the caller's (not positive: FM_E_SHAPE, where every other
                        // entry point answers FM_E_UNSUPPORTED), and the element type is looked at before the shape
  bool fine;            // fm_fine_match_maps*: crop + fine stage; layout may be FM_LAYOUT_NCHW_PREPARED, NCHW needs `scratch`
  bool missing;         // ... one of the pointers only that entry point has (mix0 .. mkpts1_c) is NULL
  void* scratch;
};

struct Scalars {          // lives at ws.scalars (zeroed per call)
  unsigned flags;         // FM_DEV_* bits
  int dense_units;        // 32x32 units the sparse sum kernel left to the dense one (0: that kernel exits at once)
  int cert_units;         // live units k_screen_rows resolved from the max pass's certificate (counted only while
                          // fm_debug_unit_cert forces the certificate on)
  int defer_entries;      // entries k_screen_rows listed without their exact dot product (counted only while
                          // fm_debug_defer_exact forces the deferral on)
};

// Device workspace of the coarse stage; all offsets in bytes from the base.  The regions the common path uses come
// first (`common_total` bytes); the float16 planes, the dense sum kernel's partials and candidate set and the
// softmax denominators of every row / column follow and are needed only with FM_MODE_DENSE / FM_MODE_EXACT_SCREENING /
// a conf_matrix request.
struct CoarseWs {
  int N, L, S, C, Lp, Sp, panels, tiles, splits, slots;
  int splits0;                                // column splits of the max pass (its own grid size)
  int splits_s, units_s;                      // screening kernel: column chunks per row block and 32-column units per chunk (<= 64)
  int top2;                                   // the launch plan's choice: the max pass also publishes every unit's runner-up and
                                              // the place of its maximum (k_max_i8<C, true>), and the screening resolves the
                                              // units they certify without sweeping them (a function of the shape alone)
  Span prep_zero;                             // zeroed by k_prep_split on every call: the (zeroed) fields below
  Span reassign[3];                           // zeroed before the assignment runs again on a call's results: its cell
                                              // maps and tie lists, its look-back totals, the status word
  Span counters[2];                           // zeroed by fm_debug_reset_counters: the candidate counters, the scalars
  // zeroed on every call (contiguous, starts at the base)
  CandList cand, ccand;                       // every significant entry the sparse sum kernel found, listed per row
                                              // (column, exact dot product) and per column (row, ...): the same entries
  CandList cand_b, ccand_b;                   // ... the dense kernel's candidate set (samples it redid); its lists lie in
                                              // the dense region below, the four counts here (zeroed on every call)
  Region<int> dense_cnt;                      // [N]: units of a sample the sparse kernel left to the dense one (> 0: the
                                              // dense kernel redoes the sample)
  Region<Scalars> scalars;
  Region<int> cell0, cell1;                   // (zeroed) match index + 1 of every image-0 / image-1 cell
  Region<int> ties0, ties1;                   // (zeroed) [0] = count, [1..kTieCap] = matches that lost their cell to an
                                              // exactly tied match (the cell-ordered gathers pick them up)
  Region<unsigned> rowmax_u, colmax_u;        // (zeroed) q_encode'd row / column maxima of the integer screening
                                              // product (max pass: atomicMax, exact and order independent)
  Region<int> blocktot;                       // (zeroed) k_select: matches per workgroup | published flag
  // per-row / per-column statistics
  Region<signed char> q0, q1;                 // int8 screening planes
  Region<float> sigimg;                       // [N][2] the int8 step of image 0 / image 1 of every sample
  Region<float> imgstat;                      // [N][8] per sample {largest L1 norm, largest clipped mass, largest |x|} of
                                              // image 0, then of image 1 (max pass: the block statistics folded once);
                                              // [6]: 1 when that max pass wrote umax2 / upos, else 0
  Region<float> l1_0, l1_1;                   // L1 norm per descriptor
  Region<float4> bstat0, bstat1;              // per 32-row block: {largest L1 norm (+inf: a bad value), largest
                                              // clipped L1 mass sum_k max(|x_k| - 127 sigma, 0), largest |x|, 0}
  Region<float> emarg;                        // [N] log2-domain bound of k * |screening product - exact product|
  Region<float> nmr, nmc;                     // -stabiliser*log2e per row / column
  Region<float> umax;                         // unit maxima [N][Lp/32][Sp/32] of the integer screening product (as float)
  Region<int> thr_r, thr_c;                   // k_thresh (batched screening): integer significance threshold per row / column
  Region<float> wmaxb, cmaxu;                 // ... largest -stabiliser*log2e of every 32-row block / 32-column unit
  Region<int> tmin_r, tmin_c;                 // ... smallest integer threshold of every 32-row block / 32-column unit
  Region<int> umax2, upos;                    // k_max_i8<C, true>, [N][Lp/32][Sp/32]: the unit's second-largest valid entry
                                              // (with multiplicity; kQMasked: none) and where one entry equal to its maximum
                                              // sits: (lane of the accumulator << 4) | register, lane = 32 (row bit 2) + column
  size_t common_total;
  // ---- dense / exact-screening / conf_matrix only ----
  Region<_Float16> hi0, lo0, hi1, lo1;        // float16 planes
  Region<float> f16inv;                       // [N] 1 / (power-of-two scales of the two images' float16 planes)
  Region<float> rowB, colB;                   // partial sum-exp of the dense sum kernel: rows [N][splits][Lp],
                                              // columns [N][panels][Sp] (one partial per workgroup)
  Region<float> rsum, csum;                   // softmax denominators per row / column
  Region<float> nmr2, nmc2;                   // nmr - log2(rsum), nmc - log2(csum): log-softmax offsets
  size_t total;
};

// splits of the column sweep so that panels*splits*N fills the chip once
int choose_splits(int N, int panels, int tiles, int target = 256);
// (alone: FM_MODE_ALONE - launch geometry only, the offsets and sizes do not depend on it)
CoarseWs coarse_layout(int N, int L, int S, int C, int slots, bool alone = false);

// fm_debug_unit_cert: 0 = the launch plan decides, 1 = never, 2 = always.  The plan takes the top-2 epilogue where the
// shape allows it (CoarseWs::top2) and the call runs the common path: with FM_MODE_DENSE / FM_MODE_FLAT / every row's
// statistics the caller expects flat similarity, where the screening stops at its first dense unit or does not run at
// all and the epilogue would only cost ('mixed' / 'borderline' pairs: -1.4 % / -2.6 %).  Every max pass records in
// imgstat[b][6] whether it wrote umax2 / upos, and the screening looks only then - whatever ran on the workspace last.
extern int g_unit_cert;
inline bool unit_cert_on(const CoarseWs& w, bool common_path = true) {
  return g_unit_cert == 2 || (g_unit_cert == 0 && w.top2 != 0 && common_path);
}

// fm_debug_defer_exact: 0 = the launch plan decides, 1 = never, 2 = always where the plan allows it (and count).  The
// screening may list a sure entry with a stand-in for its exact dot product (coarse_screen.hip: sure_slack) only where
// k_select - which resolves a stand-in before any expression but e / e reads it - is the ONLY reader of the screening
// kernel's lists: the common path.  Every other reader runs in a plan with `dense` set:
//   k_reduce_sums (rescreen / every row's statistics / FM_MODE_FLAT), k_exact_lists + k_fix_sums and k_conf_patch (every
//   row's statistics, conf_matrix) - and tools/gpu_bringup.py reads the lists of an FM_MODE_DENSE call.
// The dense resume of fm_coarse_match_auto continues a common-path call: its plan is mode | FM_MODE_DENSE alone (a call
// with FM_MODE_EXACT_SCREENING, statistics or a conf_matrix never reported FM_E_DENSE from the common path), so reduce,
// exact_lists and conf are off and k_select alone reads the unflagged samples' lists, stand-ins included; the dense
// kernels write and read the other set of lists (cand_b).  The tag needs bit 30 of an index to be free.
extern int g_defer_exact;
inline bool defer_exact_on(const CoarseWs& w, bool common_path = true) {
  return g_defer_exact != 1 && common_path && w.Lp < 0x40000000 && w.Sp < 0x40000000;
}

// One coarse call as the C ABI takes it (fmatch.h: fm_coarse_match_dtype's arguments, in their order)
struct CoarseCall {
  const void *feat0, *feat1; int in_dtype;
  int N, L, S, C, h0c, w0c, h1c, w1c;
  float temperature, thr; int border_rm; float scale_px; const float *scale0, *scale1;
  void* workspace; size_t workspace_bytes;
  int cand_slots, mode;
  int64_t *b_ids, *i_ids, *j_ids; float *mkpts0_c, *mkpts1_c, *mconf; int cap; int32_t* d_count; float* conf_matrix;
  void* stream;
};

// ---- launchers (each enqueues on `st`, returns hipGetLastError()) ----
hipError_t launch_prep(const void* feat0, const void* feat1, int in_dtype, int c_in, const CoarseWs& w, char* base,
                       int exact_step, int planes, hipStream_t st);
// FM_MODE_FLAT: stabilisers of every row / column, the pair margin, the float16 planes' scale; flags every sample for
// the dense sum kernel (what the screening kernel does besides screening)
hipError_t launch_stab(const CoarseWs& w, char* base, float inv_ct, float thr, int allow_dead, hipStream_t st);
hipError_t launch_prep_f16(const void* feat0, const void* feat1, int in_dtype, int c_in, const CoarseWs& w, char* base,
                           int force, hipStream_t st);
hipError_t launch_max_i8(const CoarseWs& w, char* base, bool top2, hipStream_t st);
// (conf != NULL: the CONF variant - writes the dense conf_matrix of every sample from the log-softmax offsets;
// rescreen: the exact re-screening of FM_MODE_EXACT_SCREENING with the same offsets)
hipError_t launch_dense(const CoarseWs& w, char* base, float inv_ct, float thr, hipStream_t st, float* conf = nullptr,
                        int rescreen = 0);
hipError_t launch_reduce(const CoarseWs& w, char* base, float inv_ct, hipStream_t st);
// side job of the assignment launch (fm_coarse_match_maps): channels-last copy of a float32 NCHW map, or src == NULL
struct MapCopyJob {
  const float* src; float* dst; int N, Hf, Wf;
};
// what the assignment launch is told about the launches before it (SelArgs: exact, dense_enabled, cell_maps, sums_ready;
// deferred: the screening kernel's lists may hold tagged entries - k_select<true>)
struct SelectFlags { bool exact, dense, cell_maps, sums_ready, deferred; };
// (reads c.feat0 / c.feat1: the exact dot products of the entries the screening listed with a stand-in)
hipError_t launch_select(const CoarseWs& w, char* base, const CoarseCall& c, float inv_ct, SelectFlags flags,
                         const MapCopyJob* job = nullptr);
hipError_t launch_conf_patch(const CoarseWs& w, char* base, float inv_ct, float* conf, hipStream_t st);
hipError_t launch_exact_lists(const CoarseWs& w, char* base, float inv_ct, const void* feat0, const void* feat1, int in_dtype,
                              int c_in, hipStream_t st);
// (the batched form of the screening - k_thresh + k_screen_rows, one wave per (row block, 64 units) - is chosen inside
// launch_screen when the batch alone fills the chip with waves)
hipError_t launch_screen(const void* feat0, const void* feat1, int in_dtype, int c_in, const CoarseWs& w, char* base,
                             float inv_ct, float thr, int dense_enabled, int allow_dead, bool defer, hipStream_t st);

// 1 / (C temperature) scales a dot product into a similarity, k2 = log2(e) / (C temperature) into an exponent of 2.  The
// ONE definition of both: every launch of the coarse stage and of its training calls must hold the SAME two roundings -
// the stabilisers are -k2 x_max, and a k2 one ulp away leaves (k2 - k2') x in both exponents: 4.5e-5 of a conf near 1 at
// |sim| ~ 160 and C = 36 or 100, where kLog2e / (C T) and kLog2e * (1 / (C T)) round differently.
inline float inv_ct_of(int C, float temperature) { return 1.0f / ((float)C * temperature); }
inline float k2_of(float inv_ct) { return inv_ct * kLog2e; }

// ---- the coarse training entry points: the dual softmax at entries, its two backwards (dsm_grad.hip), the coarse loss (coarse_loss.hip)
// the softmax statistics the forward pass kept: -stabiliser*log2e and denominator of every row / column
struct DsmStats { const float *ofs_r, *sum_r; int pitch_r; const float *ofs_c, *sum_c; int pitch_c; };
// K listed entries (b, i, j) and, where the call has one, gc[e] = g_e conf_e
struct DsmEntries { const int64_t *b_ids, *i_ids, *j_ids; const float* gc; int K; };
struct LossSpec { int kind; float alpha, gamma, pos_weight, neg_weight; };
// One call of the five entry points as the C ABI takes it (fmatch.h, in its order).  Each of them fills one and hands
// it on (dsm_status, then dsm_carve / dsm_begin); what an entry point does not have stays NULL / 0.
struct DsmCall {
  const float *feat0, *feat1; int N, L, S, C; float temperature;
  DsmStats s; DsmEntries e;
  const float* G;                    // the dense dL/dconf [N, L, S]
  void* workspace; size_t workspace_bytes; void* stream;
  float *conf, *loss_out; const float* d_loss; float *d_feat0, *d_feat1;
  // where the entry points differ
  bool listed, with_gc;              // there is an entry list; it carries gc
  bool empty_ok;                     // K == 0 is FM_OK before anything is looked at (and the lists before K's sign)
  bool needs_ws, is_loss; LossSpec loss;     // every call but conf_at has a workspace; the two loss calls
  bool missing;                      // one of the pointers only this entry point has (its outputs, d_loss) is NULL
  hipStream_t st() const { return (hipStream_t)stream; }
};

// Workspace of the backward entry points: v [N][L] row sums and u [N][S] column sums of g conf, one behind the other
// (sums: the two, zeroed per call) | part, 256-byte aligned: up to 4 (dsm_zsplit) partial gradients [N][max(L, S)][C].
// A statistics sweep (side 0) has no gradient and borrows `part` for the partial sums that k_sweep_fold_sums adds up in
// index order, every element written by exactly one workgroup: vpart [4 (z)][N][L], then upart [ceil(L / 32) (row tile of
// image 0)][N][S] from the next 256-byte boundary; `part` is as large as the larger of its two uses (the sums' only for
// fewer channels than about a 128th of the grid).
struct DsmBwdWs { Region<float> v, u, part, vpart, upart; Span sums; size_t total; };
inline DsmBwdWs dsm_bwd_layout(int N, int L, int S, int C) {
  DsmBwdWs w;
  Carver c;
  c.take(w.v, (size_t)N * L);
  c.take(w.u, (size_t)N * S, sizeof(float));
  w.sums = c.since(w.v.at);                   // v and u
  const size_t grads = (size_t)4 * N * (size_t)(L > S ? L : S) * C;
  const size_t vpart = align256((size_t)4 * N * L * sizeof(float)) / sizeof(float);
  const size_t upart = (size_t)((L + 31) / 32) * N * S;
  c.take(w.part, grads > vpart + upart ? grads : vpart + upart);
  w.vpart.at = w.part.at;
  w.upart.at = w.part.at + vpart * sizeof(float);
  w.total = c.o;
  return w;
}
// Workspace of the coarse loss: the dual softmax backward's | one loss partial (double) per workgroup of the kSums sweep |
// the id 0 of the stand-in entry (0, 0, 0) of an empty supervision (zeros: its 256 bytes, zeroed when it stands in) |
// per entry l_pos, l_neg, gc and gc * d_loss
struct ClossWs {
  DsmBwdWs dsm; Region<double> loss_part; Region<int64_t> zero_ids; Span zeros; Region<float> l_pos, l_neg, gc, gcs;
  int Ke; size_t total;
};
inline ClossWs closs_layout(int N, int L, int S, int C, int K) {
  ClossWs w;
  w.dsm = dsm_bwd_layout(N, L, S, C);
  w.Ke = K > 0 ? K : 1;
  Carver c{w.dsm.total};
  c.take(w.loss_part, (size_t)4 * N * ((L + 31) / 32));
  c.take(w.zero_ids, 1);
  w.zeros = c.since(w.zero_ids.at, 256);
  c.take(w.l_pos, w.Ke);
  c.take(w.l_neg, w.Ke);
  c.take(w.gc, w.Ke);
  c.take(w.gcs, w.Ke);
  w.total = c.pad();
  return w;
}

int dsm_status(const DsmCall& c);   // the ONLY copy of the five entry points' argument checks (the table: DESIGN.md 6g)
// one call past its status: the descriptors, the shape, the temperature terms and the carved workspace
struct DsmProblem { const float *feat0, *feat1; int N, L, S, C; float k2, inv_ct; float *v, *u, *part, *vpart, *upart; };
// dsm_carve: a pure function of a call (with a workspace) that passed dsm_status; dsm_begin: the same, and v and u zeroed
// on the call's stream (the coarse loss's backward takes v and u from its forward call).  Neither checks anything.
DsmProblem dsm_carve(const DsmCall& c);
int dsm_begin(const DsmCall& c, DsmProblem* p);
int dsm_zsplit(int N, int R);      // z slices of a sweep's column range, so that N * ceil(R / 32) * z fills the chip
// the problem as the owner image of side `side` sees it (0: image 0, 1: image 1): its own descriptors, length, statistics
// and sums come first; part is shared
struct DsmSide { DsmProblem p; DsmStats s; };
inline DsmSide dsm_side(const DsmProblem& p, const DsmStats& s, int side) {
  if (!side) return {p, s};
  return {{p.feat1, p.feat0, p.N, p.S, p.L, p.C, p.k2, p.inv_ct, p.u, p.v, p.part},
          {s.ofs_c, s.sum_c, s.pitch_c, s.ofs_r, s.sum_r, s.pitch_r}};
}
inline dim3 dsm_sweep_grid(const DsmSide& o) { return dim3((o.p.L + 31) / 32, o.p.N, dsm_zsplit(o.p.N, o.p.L)); }
// f(int_c<padded C>): the channel counts the sweeps are instantiated for
template <typename F>
inline hipError_t with_padded_channels(int C, F&& f) {
  const int Cp = padded_channels(C);
  return Cp == 64 ? f(int_c<64>{}) : Cp == 128 ? f(int_c<128>{}) : f(int_c<256>{});
}
// d_out [N][o.p.L][C] = inv_ct (* d_loss[0], if given: on the device) * sum over the Z partials of a gradient sweep
// (add: + what d_out holds)
hipError_t launch_sweep_combine(const DsmSide& o, int Z, const float* d_loss, float* d_out, bool add, hipStream_t st);
// behind a statistics sweep of side 0: v += the z slices' row sums, u += the row tiles' column sums, each in index order
hipError_t launch_sweep_fold_sums(const DsmProblem& p, hipStream_t st);
// v / u contributions and own term 2 g c of the listed entries (k_dsm_uv, k_dsm_entries; the latter clears d_feat0 /
// d_feat1 first and goes BEFORE the gradient sweeps, whose combine adds to it)
hipError_t launch_dsm_uv(const DsmEntries& e, int L, int S, float* v, float* u, hipStream_t st);
hipError_t launch_dsm_entries(const DsmProblem& p, const DsmEntries& e, float* d_feat0, float* d_feat1, hipStream_t st);

// Raises a kernel's dynamic-LDS limit once per (kernel, device) instead of on every launch: the
// attribute call costs tens of host microseconds, which an eager (non-graph) caller would pay per step.
template <typename K>
inline hipError_t ensure_dynamic_lds(K kernel, int bytes, unsigned long long* done_mask) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (__atomic_load_n(done_mask, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) __atomic_fetch_or(done_mask, bit, __ATOMIC_RELEASE);
  return e;
}

// The launch site of a tiled sweep (fm_sweep_device.h) of one side, for both of its kernels: KERNEL = an instantiation of
// k_dsm_bwd or k_closs_sweep, smem = its dynamic LDS, tail = the kernel's arguments behind the 14 the two share.
template <auto KERNEL, typename... Tail>
inline hipError_t launch_sweep(const DsmSide& o, int smem, hipStream_t st, Tail... tail) {
  static unsigned long long lds_set = 0;        // (one per instantiation, that is, per kernel)
  const hipError_t e = ensure_dynamic_lds(KERNEL, smem, &lds_set);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(KERNEL, dsm_sweep_grid(o), dim3(256), smem, st, o.p.feat0, o.p.feat1, o.p.L, o.p.S, o.p.C, o.s.ofs_r,
                     o.s.sum_r, o.s.pitch_r, o.s.ofs_c, o.s.sum_c, o.s.pitch_c, o.p.v, o.p.u, o.p.k2, tail...);
  return hipSuccess;
}

}  // namespace fm
