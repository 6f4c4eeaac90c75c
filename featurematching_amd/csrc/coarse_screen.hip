// Coarse stage, the SCREENING kernels: which entries of the L x S product matter, and their exact values.
//
// Reproduces network/utils/coarse_matching_new.py:64-68 (correlation + dual softmax) for every entry whose
// term is not negligible.  After the max pass (k_max_i8: row / column maxima and the maximum of every
// 32 x 32 unit of the int8 screening product x~, error bounded by fm_device.h) each entry s_ij falls in one of
// three classes:
//   * negligible : k x~_ij + margin lies more than 2^32 below BOTH its row's and its column's stabiliser: it adds
//                  < 2^-32 to sums that are >= e^-2E ~ 1 (<= S 2^-32 ~ 1e-6 relative in total, inside the 1e-5
//                  parity bar) and cannot be a candidate.  Never touched again.  With dual-softmax-trained
//                  (peaked) descriptors that is all but ~1 entry per row.
//   * significant, few per row / column : the exact float32 dot product of the two descriptors is recomputed from the
//                  caller's rows (16 lanes per entry, 16 channels per lane, fixed order) and the entry (index, x) is
//                  appended to its ROW's list when exp2(k x - m^_i) > 2^-32 and to its COLUMN's list when
//                  exp2(k x - c^_j) > 2^-32.  k_select forms sum_j exp2(k x - m^_i), sum_i exp2(k x - c^_j) and conf
//                  from these lists (in index order: deterministic) - the same number in numerator and denominator of
//                  conf, as in the reference's softmax.
//   * significant, many (flat similarity: untrained network, repetitive texture, a partner that is missing) : a unit with
//                  more than kMaxExact significant entries, or a row / column with more than cand_slots, flags its
//                  SAMPLE for the dense sum kernel (k_dense: float32-equivalent hi/lo product on the matrix cores
//                  for all 1024 entries of every live unit), which redoes that sample when the call runs with
//                  FM_MODE_DENSE; without it the call reports FM_E_DENSE (fm_coarse_match_auto then adds the dense part).
//                  A sample is handled by ONE of the two kernels: their float32 products agree to ~1e-7 but not bit
//                  for bit, and coarse_matching_new.py:105-106 keeps exactly tied entries (conf == row max == column
//                  max), so identical descriptors must see one arithmetic.
//
// Kernels (round 5): k_thresh (one thread per row / column: stabilisers, integer thresholds, per-block maxima of them)
// and k_screen_rows (ONE independent wave per (32-row block, <= 64 column units): live units only, B fragments straight
// from global memory into registers, no barrier, 12 KiB of LDS per workgroup) - see the block comment in front of them
// for the one-round-trip, 128-KiB-of-LDS workgroup kernel of round 4 they replace and why.  k_stab serves FM_MODE_FLAT.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "fm_device.h"
#include "fm_exact_device.h"
#include "fm_wave_device.h"

namespace fm {

constexpr int kMaxExact = 24;         // significant entries of a unit resolved by exact dot products; more -> dense kernel

struct ScreenArgs {
  const signed char* q0; const signed char* q1;       // int8 screening planes (k_prep_split)
  DescRows desc;                                       // the caller's descriptors [N,L,c_in] / [N,S,c_in]
  const unsigned* rowmax_u; const unsigned* colmax_u;  // max pass: q_encode'd maxima of the integer screening product
  const float* sigimg;                                 // [N][2] quantisation step of image 0 / image 1
  const float* imgstat;                                // [N][8] {largest L1 norm, clipped mass, |x|} of image 0, of image 1 (max pass)
  const float* l1_0; const float* l1_1;                // L1 norms
  const float4* bstat0; const float4* bstat1;          // per 32-row block: {largest L1 norm, largest clipped L1 mass, ..}
  const float* umax;                                   // unit maxima of the integer screening product
  float* nmr; float* nmc; float* emarg;                // written here: stabilisers, pair margin
  int* dense_cnt; Scalars* scal;                       // [N] units per sample left to the dense kernel
  int* rcount; int* rlist_j; float* rlist_x;           // significant entries per row: columns, exact dot products
  int* ccount; int* clist_i; float* clist_x;           // ... per column: rows, exact dot products
  int L, S, Lp, Sp, slots, dense_enabled;
  int allow_dead;                                      // 0: every row / column keeps its stabiliser and its full sum (conf_matrix)
  float k, lt, inv_ct, cpad;
};

// Integer significance threshold: an entry with integer screening product q can matter for a row / column whose
// -stabiliser*log2e is nm iff  kss q + emu + nm > -kSkipLog2  <=>  q > (-kSkipLog2 - emu - nm) / kss.
// floor() - 1 absorbs the float roundings of the quotient (a lower threshold only lets more entries through).
__device__ __forceinline__ int sig_threshold(float nm, float emu, float inv_kss) {
  const float t = floorf((-kSkipLog2 - emu - nm) * inv_kss) - 1.f;
  return (int)fminf(fmaxf(t, -1.0e9f), 1.0e9f);       // (NaN -> -1e9: everything significant)
}

// Sure entries (deferred exact dot products).  The exact phase lists a parked entry (i, j) with its float32 dot product x
// in row i's list iff fma(x, k, nmr_i) > -kSkipLog2 and in column j's iff fma(x, k, nmc_j) > -kSkipLog2.  An entry whose
// INTEGER product q already proves both is listed without the two 1-KiB gathers (k_select forms x if it ever needs it):
//     q > max(thr_r[i], thr_c[j]) + D        (and both thresholds are real ones, > -1e9: see sig_threshold's NaN case)
// with one slack D per sample.  Proof for the row (the column is the same with nmc, thr_c):
//   * thr_r = floor(t) - 1, t = fl((-kSkipLog2 - emu - nmr) / kss), emu the margin of the row's block (k_thresh).  q and
//     thr_r + D are integers, so q >= floor(t) + D > t - 1 + D:   kss q > (-kSkipLog2 - emu - nmr) + kss (D - 1) - r1,
//     r1 = the roundings of t (four operations on a quantity <= kSkipLog2 + emu + |nmr|).
//   * the int8 product is within the pair margin of the real dot product x* (fm_device.h; its factor 1.0001 covers the
//     roundings of kss and of the scaled product):   k x* >= kss q - emarg,   and emu <= emarg (the same monotone float
//     expression on a block's largest L1 norm instead of the image's).
//   * float32 x against x*: 16 fmas and 4 additions per lane, |x - x*| <= 20 u sum|a_k b_k| <= 20 u l1A_max infB
//     (u = 2^-24; float16 / bfloat16 rows convert exactly); the filter's own fma rounds once more: u |k x + nmr|.
//   Together:  fma(x, k, nmr) > -kSkipLog2 + kss (D - 1) - 2 emarg - r,   r <= 30 u P + 10 u (kSkipLog2 + 2 emarg + 1),
//   P = k l1A_max infB  (|nmr| <= P + emarg + 1: the stabiliser is a screening product less a margin).  With emarg < 60
//   (k_thresh reports FM_DEV_RANGE / FM_DEV_STEP otherwise, and then nothing is sure) r < 2^-19 P + 1e-4, and
//       D = ceil((2 emarg + 2^-17 P + 0.01) / kss * 1.0001) + 2
//   makes kss (D - 1) >= 2 emarg + 4 r with a whole integer step to spare for the roundings of D itself.
// The stand-in x~ = fl(sigma_0 sigma_1 q) passes the same two tests with more room (k x~ = kss q up to roundings), and
// k x~ + nm <= emarg + 1 < 61 (q <= the row's / column's maximum, the stabiliser is that maximum less a margin); the exact
// term's exponent is below 2 emarg + 1 < 121.  Both exponentials are finite, non-zero normals, and e / e = 1.0f for
// either (k_select's one-entry lists: the only expression that reads a stand-in).
// tests/test_defer_model.py replays this rule in float32 against the exact filters.
__device__ __forceinline__ int sure_slack(float emarg, float kss, float k, float l1A_max, float infB) {
#pragma clang fp contract(off)
  const float P = k * l1A_max * infB;
  const float dq = ceilf((2.0f * emarg + 7.62939453125e-6f * P + 0.01f) * (1.0f / kss) * 1.0001f);
  return (emarg < 60.f && dq < 1.0e9f) ? (int)dq + 2 : 0x3fffffff;        // (NaN -> never sure)
}

// FM_MODE_FLAT: what the screening kernel does besides screening, for a call whose samples all go to the dense sum
// kernel - the stabilisers of every row and column (the SAME expressions as in k_screen: lower bounds from the int8 max
// pass, dead rows / columns at -inf), the pair margin and the range checks, the inverse scale of the float16 planes
// k_prep_split<C, true> wrote, and the dense flags.  grid (chunks of 256 lines, N, 2): z = 0 rows, 1 columns.
__global__ __launch_bounds__(256) void k_stab(ScreenArgs a, float* f16inv) {
  const int side = blockIdx.z, b = blockIdx.y;
  const int len = side ? a.S : a.L, lenp = side ? a.Sp : a.Lp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float sig0 = a.sigimg[b * 2], sig1 = a.sigimg[b * 2 + 1];
  const float* ist = a.imgstat + (long)b * 8;
  const float l1A_max = ist[0], clipA = ist[1], infA = ist[2], l1B_max = ist[3], clipB = ist[4], infB = ist[5];
  const float ss = sig0 * sig1;
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {
    const float emarg = margin_log2(q8_margin_raw(sig0, l1A_max, clipA, sig1, l1B_max, clipB, a.cpad), a.inv_ct);
    a.emarg[b] = emarg;
    const bool clipped = clipA > 0.f || clipB > 0.f;
    // float16 planes: scale from the int8 step (k_prep_split<C, true>); the image's true maximum must fit
    const float sc0 = f16_plane_scale(127.f * sig0), sc1 = f16_plane_scale(127.f * sig1);
    f16inv[b] = (1.0f / sc0) * (1.0f / sc1);
    if (!(l1A_max < INFINITY) || !(l1B_max < INFINITY)) atomicOr(&a.scal->flags, (unsigned)FM_DEV_RANGE);
    else if (!(emarg < 60.f)) atomicOr(&a.scal->flags, (unsigned)(clipped ? FM_DEV_STEP : FM_DEV_RANGE));
    else if (!(infA * sc0 < 65504.f) || !(infB * sc1 < 65504.f)) atomicOr(&a.scal->flags, (unsigned)FM_DEV_STEP);
    a.dense_cnt[b] = 1;
    a.scal->dense_units = 1;
  }
  if (idx >= lenp) return;
  const long g = (long)b * lenp + idx;
  float nm = -INFINITY;                      // padded lines
  if (idx < len) {
    const float ln2 = 0.69314718f;
    const float l1 = (side ? a.l1_1 : a.l1_0)[g];
    const unsigned mx = (side ? a.colmax_u : a.rowmax_u)[g];
    const bool dead = a.allow_dead && 2.002f * l1 * (side ? infA : infB) * a.inv_ct + 1e-3f <
                                          (a.lt + __builtin_log2f((float)(side ? a.L : a.S))) * ln2;
    const float mraw = side ? q8_margin_raw(sig0, l1A_max, clipA, sig1, l1, clipB, a.cpad)
                            : q8_margin_raw(sig0, l1, clipA, sig1, l1B_max, clipB, a.cpad);
    nm = dead ? -INFINITY : neg_stabiliser_log2(ss * q_decode(mx), mraw, a.inv_ct);
  }
  (side ? a.nmc : a.nmr)[g] = nm;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_thresh + k_screen_rows (round 5).
//
// Round 4's k_screen was built for ONE pair per launch and one stream: a workgroup = 8 row blocks x <= 16 units, everything
// in one memory round trip, the int8 B fragments of ALL units of the range by LDS-DMA whether alive or not (64-128 KiB of
// LDS per workgroup), one barrier - 361 workgroups that each live ~7 us: 13 us per 640x480 pair.  Two things were wrong
// with that shape, both measured in round 5:
//   * at a batch of 64 pairs it is 23 104 workgroups in 45 rounds of two per compute unit (LDS), every one the same
//     latency chain: 523 us against ~90 us of bytes;
//   * on the bench's FOUR streams a workgroup that parks 128 KiB of LDS and 8 waves for 7 us keeps the other pairs' max
//     pass (64 KiB of LDS per workgroup) off its compute unit: with the kernels below - 5 us SLOWER alone at one pair -
//     the four-stream rate went from 25.4 k to 28.0 k pairs/s.
// What matters is that nothing couples waves to each other and that a wave holds few resources:
//   * k_thresh (one thread per row / column): stabilisers, integer significance thresholds, the largest stabiliser of
//     every 32-row block and 32-column unit, the pair margin and the range checks - what every k_screen workgroup
//     derived for its panel and range, computed once.  (Folding it into every wave of k_screen_rows - no launch, a
//     bound per unit from the unit's smallest column maximum - was tried: 25.3 us against 23.6 us alone, 26.9 k against
//     27.5 k pairs/s: the redundant column work is on every wave's critical path.)
//   * k_screen_rows: ONE WAVE per (row block, <= 64 units) item, no barrier, no LDS-DMA: the wave loads its A fragments
//     and thresholds, derives its live mask from the unit maxima, and walks the LIVE units only - B fragments straight
//     from global memory into registers (8 KiB per unit, the next unit's in flight while this one is screened: 16 KiB
//     per wave, 12 waves per compute unit keep its 64 B/clk busy), 8 MFMAs, the integer screening, the exact float32 dot
//     products and list reservations.  Items are ordered so that an XCD works on one or two samples at a time (their
//     int8 planes, 2.4 MiB, stay in its L2).  64 pairs: 530 -> 270 us (sweep 110 us, exact phase 150 us: 630 MB of
//     descriptor rows from HBM through the compute units' ~23 GB/s each); one 1024x1024 pair 75 -> 32 us.
// ---------------------------------------------------------------------------------------------------------------------
struct RowsExtra {
  int* thr_r; int* thr_c; float* wmaxb; float* cmaxu;
  int* tmin_r; int* tmin_c;              // k_thresh: smallest integer threshold of every 32-row block / 32-column unit
  const int* umax2; const int* upos;     // max pass with the top-2 epilogue (valid when imgstat[b][6] != 0; fm_internal.h)
  int look;                              // 0: fm_debug_unit_cert(1), never look
  int count_cert;                        // fm_debug_unit_cert(2): count the certified live units
  int defer;                             // list sure entries without their exact dot product (k_select is the lists' only reader)
  int count_defer;                       // fm_debug_defer_exact(2): count them
  int nchunks, chunk_units, items;       // chunk_units <= 64 units per item (one ballot covers a chunk)
};

// grid (chunks of 256 lines, N, 2): z = 0 rows, 1 columns; a 256-thread block = 8 row blocks / units of 32 lines
__global__ __launch_bounds__(256) void k_thresh(ScreenArgs a, RowsExtra x) {
  const int side = blockIdx.z, b = blockIdx.y;
  const int len = side ? a.S : a.L, lenp = side ? a.Sp : a.Lp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const float sig0 = a.sigimg[b * 2], sig1 = a.sigimg[b * 2 + 1];
  const float* ist = a.imgstat + (long)b * 8;
  const float l1A_max = ist[0], clipA = ist[1], infA = ist[2], l1B_max = ist[3], clipB = ist[4], infB = ist[5];
  const float ss = sig0 * sig1;
  const float kss = a.k * ss;
  const bool screen_ok = kss > 1e-30f && kss < 1e30f;
  const float inv_kss = screen_ok ? 1.0f / kss : 0.f;
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {      // (the same checks as k_screen's first workgroup)
    const float emarg = margin_log2(q8_margin_raw(sig0, l1A_max, clipA, sig1, l1B_max, clipB, a.cpad), a.inv_ct);
    a.emarg[b] = emarg;
    const bool clipped = clipA > 0.f || clipB > 0.f;
    const float emarg0 = margin_log2(q8_margin_raw(sig0, l1A_max, 0.f, sig1, l1B_max, 0.f, a.cpad), a.inv_ct);
    if (!(l1A_max < INFINITY) || !(l1B_max < INFINITY)) atomicOr(&a.scal->flags, (unsigned)FM_DEV_RANGE);
    else if (!(emarg < 60.f)) atomicOr(&a.scal->flags, (unsigned)(clipped ? FM_DEV_STEP : FM_DEV_RANGE));
    else if (clipped && emarg > 2.0f * emarg0 + 1.0f) atomicOr(&a.scal->flags, (unsigned)FM_DEV_STEP);
  }
  if (idx >= lenp) return;                 // (lenp is a multiple of 64: whole waves leave)
  const long g = (long)b * lenp + idx;
  const int blk = idx >> 5;                // row block / unit of this line
  const int nblk = lenp / 32;
  float nm = -INFINITY;                    // padded lines: no stabiliser, nothing significant on their account
  float emu = 0.f;
  if (idx < len) {
    const float ln2 = 0.69314718f;
    const float l1 = (side ? a.l1_1 : a.l1_0)[g];
    const unsigned mx = (side ? a.colmax_u : a.rowmax_u)[g];
    const float bl1 = (side ? a.bstat1 : a.bstat0)[(long)b * nblk + blk].x;       // largest L1 norm of the line's block
    const bool dead = a.allow_dead && 2.002f * l1 * (side ? infA : infB) * a.inv_ct + 1e-3f <
                                          (a.lt + __builtin_log2f((float)(side ? a.L : a.S))) * ln2;
    const float mraw = side ? q8_margin_raw(sig0, l1A_max, clipA, sig1, l1, clipB, a.cpad)
                            : q8_margin_raw(sig0, l1, clipA, sig1, l1B_max, clipB, a.cpad);
    nm = dead ? -INFINITY : neg_stabiliser_log2(ss * q_decode(mx), mraw, a.inv_ct);
    // margin of any entry of this line's block against the other image's largest L1 norm
    emu = margin_log2(side ? q8_margin_raw(sig0, l1A_max, clipA, sig1, bl1, clipB, a.cpad)
                           : q8_margin_raw(sig0, bl1, clipA, sig1, l1B_max, clipB, a.cpad), a.inv_ct);
  }
  (side ? a.nmc : a.nmr)[g] = nm;
  const int thr = idx < len ? sig_threshold(nm, emu, inv_kss) : 0x3fffffff;
  (side ? x.thr_c : x.thr_r)[g] = thr;
  const float bm = half_all<OpMax>(nm);
  const int tm = half_all<OpMin>(thr);
  if ((lane & 31) == 0) {
    (side ? x.cmaxu : x.wmaxb)[(long)b * nblk + blk] = bm;
    (side ? x.tmin_c : x.tmin_r)[(long)b * nblk + blk] = tm;
  }
}

template <int C>
__global__ __launch_bounds__(256, 3) void k_screen_rows(ScreenArgs a, RowsExtra x) {
  constexpr int KS8 = C / 32;
  constexpr int LIST = 256;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  __shared__ int s_list[4][LIST];          // parked entries that take the exact phase: (unit << 10) | (row << 5) | column
  __shared__ int s_sure[4][LIST];          // ... that are sure: the same key
  __shared__ int s_sq[4][LIST];            // ... and their integer product

  // item = (sample, chunk, group of 4 row blocks) -> the 4 waves of a workgroup take 4 consecutive row blocks of one
  // chunk: their live units overlap (L1 / L2 hits on the B fragments); through the bijective XCD remap one XCD's share
  // is a contiguous range of items, i.e. one or two samples at a time
  const int nrb = a.Lp / 32, nunits = a.Sp / 32;
  const int item = xcd_contiguous(blockIdx.x, gridDim.x) * 4 + wv;
  if (item >= x.items) return;                      // (wave-uniform; the kernel has no barrier)
  const int per_sample = nrb * x.nchunks;
  const int b = item / per_sample;
  int kk = item - b * per_sample;
  const int chunk = kk / nrb;
  const int rb = kk - chunk * nrb;
  const int wrow0 = rb * 32;
  if (wrow0 >= a.L) return;                         // nothing but padding rows
  const int u0 = chunk * x.chunk_units;
  const int U = min(x.chunk_units, nunits - u0);

  // ---- one round trip: steps and statistics, thresholds of this lane's 16 rows, unit maxima / largest column
  // stabilisers / largest L1 norms of the chunk's units (lane = unit), the A fragments ----
  const float sig0 = a.sigimg[b * 2], sig1 = a.sigimg[b * 2 + 1];
  const float* ist = a.imgstat + (long)b * 8;
  const float clipA = ist[1], clipB = ist[4];
  const float l1A_max = ist[0], infB = ist[5];
  const float emarg_b = a.emarg[b];                 // (k_thresh wrote it)
  const float bl1A = a.bstat0[(long)b * nrb + rb].x;
  const float wmax = x.wmaxb[(long)b * nrb + rb];
  const int ul_c = min(lane, U - 1);
  const float um = a.umax[((long)b * nrb + rb) * nunits + u0 + ul_c];
  const float cm = x.cmaxu[(long)b * nunits + u0 + ul_c];
  const float bl1B = a.bstat1[(long)b * nunits + u0 + ul_c].x;
  // the unit certificate (lane = unit): the unit's runner-up against the smallest threshold any of its entries can meet
  // (loaded in the same round trip whether or not the max pass wrote them - ist[6] says so: the values are used only then)
  const bool look = x.look && ist[6] != 0.f;
  const int um2 = x.umax2[((long)b * nrb + rb) * nunits + u0 + ul_c];
  const int upos = x.upos[((long)b * nrb + rb) * nunits + u0 + ul_c];
  const int tmin = min(x.tmin_r[(long)b * nrb + rb], x.tmin_c[(long)b * nunits + u0 + ul_c]);
  v16i trr;                                 // (a vector, not an array: the hit walk picks one by a uniform index, and an array would go to scratch for that)
  {
    const int* tp = x.thr_r + (long)b * a.Lp + wrow0 + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 t4 = *reinterpret_cast<const int4*>(tp + 8 * q);
      trr[4 * q] = t4.x; trr[4 * q + 1] = t4.y; trr[4 * q + 2] = t4.z; trr[4 * q + 3] = t4.w;
    }
  }
  v4i aq[KS8];
  {
    const signed char* src = a.q0 + (((long)b * a.Lp + wrow0) / 32 * KS8 * 64 + lane) * 16;
#pragma unroll
    for (int ks = 0; ks < KS8; ++ks) aq[ks] = *reinterpret_cast<const v4i*>(src + ks * 1024);
  }
  const float ss = sig0 * sig1;
  const float kss = a.k * ss;
  const bool screen_ok = kss > 1e-30f && kss < 1e30f;
  const int D = (x.defer && screen_ok) ? sure_slack(emarg_b, kss, a.k, l1A_max, infB) : 0x3fffffff;

  // ---- live units of this row block (the same bound as k_screen) ----
  unsigned long long live;
  {
    const float emu = margin_log2(q8_margin_raw(sig0, bl1A, clipA, sig1, bl1B, clipB, a.cpad), a.inv_ct);
    const float top = __builtin_fmaf(um, kss, emu);
    const bool hot = lane < U && (!screen_ok || !((top + wmax < -kSkipLog2) && (top + cm < -kSkipLog2)));
    live = __ballot(hot);
  }
  // Certified units: every entry but the one at upos is <= um2 <= tmin <= min(thr_r[i], thr_c[j]), so the unit parks
  // exactly that entry if the unit's maximum passes ITS two thresholds, and nothing otherwise - the same integers on
  // both sides as in screen_unit below, without the unit's B fragments and MFMAs.  A tie (um2 == the maximum) passes only
  // when nothing of the unit is significant.
  const unsigned long long cert = look ? (live & __ballot(um2 <= tmin)) : 0ull;
  live &= ~cert;
  // A unit with more significant entries than the exact phase resolves (flat similarity) sends its whole SAMPLE to the
  // dense sum kernel, and from then on every list of the sample is dead weight: a wave stops at its first such unit, and
  // does not start when the sample is flagged already (a plain, possibly stale load: only an optimisation).
  const bool flat = !screen_ok || a.dense_cnt[b] != 0;
  int nd_units = flat ? 1 : 0;
  int nlist = 0, nsure = 0;
#ifdef FM_ABL_ROWS          // ablation builds (tools/): 1 = no sweep, 2 = no exact phase
  if (FM_ABL_ROWS & 1) live = 0;
#endif
  int cert_thr = 0x3fffffff, cert_tmx = 0x3fffffff, cert_key = 0;
  if (!flat && ((cert >> lane) & 1)) {
    const int g = upos & 15, lw = (upos >> 4) & 63;
    const int rl = (g & 3) + 8 * (g >> 2) + 4 * (lw >> 5), cl = lw & 31;
    const int tr = x.thr_r[(long)b * a.Lp + wrow0 + rl], tc = x.thr_c[(long)b * a.Sp + (u0 + lane) * 32 + cl];
    cert_thr = min(tr, tc);
    cert_tmx = max(tr, tc);
    cert_key = (lane << 10) | (rl << 5) | cl;
  }
  if (x.count_cert && cert && lane == 0) atomicAdd(&a.scal->cert_units, __builtin_popcountll(cert));
  if (!flat && live) {
    const bool row_edge = (wrow0 + 32 > a.L);
    const signed char* q1b = a.q1 + ((long)b * nunits + u0) * KS8 * 1024 + lane * 16;
    const int* tcb = x.thr_c + (long)b * a.Sp + u0 * 32 + r;
    auto load_unit = [&](int ul, v4i (&bq)[KS8], int& tcl) {
      const signed char* src = q1b + (long)ul * KS8 * 1024;
#pragma unroll
      for (int ks = 0; ks < KS8; ++ks) bq[ks] = *reinterpret_cast<const v4i*>(src + ks * 1024);
      tcl = tcb[ul * 32];
    };
    auto screen_unit = [&](int ul, const v4i (&bq)[KS8], int tcl) {
      const int ucol0 = (u0 + ul) * 32;
      v16i acc;
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[g] = 0;
#pragma unroll
      for (int ks = 0; ks < KS8; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[ks], bq[ks], acc, 0, 0, 0);
      if (row_edge || ucol0 + 32 > a.S) {
        const bool cok = ucol0 + r < a.S;
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if (!cok || wrow0 + (g & 3) + 8 * (g >> 2) + 4 * h >= a.L) acc[g] = kQMasked;
      }
      unsigned bm = 0;
#pragma unroll
      for (int g = 0; g < 16; ++g) bm |= (acc[g] > min(trr[g], tcl)) ? (1u << g) : 0u;
      unsigned long long hitl = __ballot(bm != 0);
      if (!hitl) return;
      // (count first: a flat unit has hundreds of hits, and walking them one by one is a scalar loop)
      int cnt = 0;
#pragma unroll
      for (int g = 0; g < 16; ++g) cnt += __builtin_popcountll(__ballot((bm >> g) & 1u));
      if (cnt > kMaxExact || nlist + nsure + cnt > LIST) { ++nd_units; return; }
      while (hitl) {
        const int l = __builtin_ctzll(hitl);
        hitl &= hitl - 1;
        unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)bm, l);
        while (bits) {
          const int g = __builtin_ctz(bits);
          bits &= bits - 1;
          const int rl = (g & 3) + 8 * (g >> 2) + 4 * (l >> 5);
          const int key = (ul << 10) | (rl << 5) | (l & 31);
          int sure_e = 0, q_e = 0;             // (uniform)
          if (D != 0x3fffffff) {               // (uniform: a call that does not defer pays nothing per hit - flat units hold dozens)
            // this entry's product and row threshold out of the 16 registers (g is uniform: a chain of selects, no indexing)
            int qv = acc[0], tv = trr[0];
#pragma unroll
            for (int g2 = 1; g2 < 16; ++g2) { qv = (g == g2) ? acc[g2] : qv; tv = (g == g2) ? trr[g2] : tv; }
            const bool sure_l = min(tv, tcl) > -1000000000 && qv > max(tv, tcl) + D;
            q_e = __builtin_amdgcn_readlane(qv, l);
            sure_e = __builtin_amdgcn_readlane((int)sure_l, l);
          }
          if (lane == 0) {
            if (sure_e) { s_sure[wv][nsure] = key; s_sq[wv][nsure] = q_e; }
            else s_list[wv][nlist] = key;
          }
          nsure += sure_e;                     // (plain sums: two counters picked by a branch end up in scratch)
          nlist += 1 - sure_e;
        }
      }
    };
    // the live units two at a time: the next unit's fragments are in flight while this one is screened
    v4i bA[KS8], bB[KS8];
    int tcA = 0, tcB = 0;
    unsigned long long mask = live;
    int ulA = __builtin_ctzll(mask), ulB = -1;
    mask &= mask - 1;
    load_unit(ulA, bA, tcA);
    while (true) {
      ulB = -1;
      if (mask) { ulB = __builtin_ctzll(mask); mask &= mask - 1; load_unit(ulB, bB, tcB); }
      screen_unit(ulA, bA, tcA);
      if (ulB < 0 || nd_units) break;
      ulA = -1;
      if (mask) { ulA = __builtin_ctzll(mask); mask &= mask - 1; load_unit(ulA, bA, tcA); }
      screen_unit(ulB, bB, tcB);
      if (ulA < 0 || nd_units) break;
    }
  }
  if (!flat && cert && !nd_units) {
    // (the lists are unordered: k_select sorts by key.  Certified units hold <= 1 entry each, so the only limit they can
    // meet is LIST, and the wave's total decides that in either order)
    const unsigned long long hits = __ballot((int)um > cert_thr);
    const int nh = __builtin_popcountll(hits);
    if (nlist + nsure + nh > LIST) ++nd_units;
    else {
      const unsigned long long sure = hits & __ballot(cert_thr > -1000000000 && (int)um > cert_tmx + D);
      const unsigned long long rest = hits & ~sure, below = (1ull << lane) - 1ull;
      if ((rest >> lane) & 1) s_list[wv][nlist + __builtin_popcountll(rest & below)] = cert_key;
      if ((sure >> lane) & 1) {
        s_sure[wv][nsure + __builtin_popcountll(sure & below)] = cert_key;
        s_sq[wv][nsure + __builtin_popcountll(sure & below)] = (int)um;
      }
      nlist += __builtin_popcountll(rest);
      nsure += __builtin_popcountll(sure);
    }
  }
  if (nd_units) nlist = nsure = 0;     // the sample goes to the dense kernel: its lists are not read

  // ---- the sure entries: a place in the row's and in the column's list (the same two returning atomics as the exact
  // phase), the tagged index and the stand-in sigma_0 sigma_1 q - one lane per entry, no descriptor, no stabiliser ----
  int overflow = 0;
#ifdef FM_ABL_ROWS
  if (FM_ABL_ROWS & 2) nsure = 0;
#endif
  for (int e0 = 0; e0 < nsure; e0 += 64) {
    if (e0 + lane < nsure) {
      const int ky = s_sure[wv][e0 + lane];
      const float xq = ss * (float)s_sq[wv][e0 + lane];
      const int row = wrow0 + ((ky >> 5) & 31), col = (u0 + ((ky >> 10) & 63)) * 32 + (ky & 31);
      const long grow = (long)b * a.Lp + row, gcol = (long)b * a.Sp + col;
      const int pr = atomicAdd(&a.rcount[grow], 1);
      const int pc = atomicAdd(&a.ccount[gcol], 1);
      if (pr < a.slots) { a.rlist_j[grow * a.slots + pr] = col | kDeferTag; a.rlist_x[grow * a.slots + pr] = xq; }
      else overflow = 1;
      if (pc < a.slots) { a.clist_i[gcol * a.slots + pc] = row | kDeferTag; a.clist_x[gcol * a.slots + pc] = xq; }
      else overflow = 1;
    }
  }
  if (x.count_defer && nsure && lane == 0) atomicAdd(&a.scal->defer_entries, nsure);

  // ---- the parked entries: exact float32 dot products (as in k_screen; stabilisers from k_thresh's arrays) ----
#ifdef FM_ABL_ROWS
  if (FM_ABL_ROWS & 2) nlist = 0;
#endif
  {
    constexpr int NPASS = 4;
    const int sub = lane >> 4, l16 = lane & 15;
    for (int e0 = 0; e0 < nlist; e0 += 4 * NPASS) {
      int myres = 0;
      float my_nmr = 0.f, my_nmc = 0.f;
      if (lane < 4 * NPASS && e0 + lane < nlist) {
        const int ky = s_list[wv][e0 + lane];
        const int row = wrow0 + ((ky >> 5) & 31), col = (u0 + ((ky >> 10) & 63)) * 32 + (ky & 31);
        const int pr = atomicAdd(&a.rcount[(long)b * a.Lp + row], 1);
        const int pc = atomicAdd(&a.ccount[(long)b * a.Sp + col], 1);
        my_nmr = a.nmr[(long)b * a.Lp + row];
        my_nmc = a.nmc[(long)b * a.Sp + col];
        myres = min(pr, 0xffff) | (min(pc, 0xffff) << 16);
      }
      int key[NPASS];
      float xs[NPASS];
#pragma unroll
      for (int h2 = 0; h2 < NPASS; h2 += 2) {
        float4 av[2][4], bv[2][4];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const int p = h2 + pp;
          const int idx = e0 + 4 * p + sub;
          key[p] = s_list[wv][min(idx, nlist - 1)];
          const int row = wrow0 + ((key[p] >> 5) & 31), col = (u0 + ((key[p] >> 10) & 63)) * 32 + (key[p] & 31);
          exact_dot16_load(a.desc, b, row, col, l16, av[pp], bv[pp]);
        }
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) xs[h2 + pp] = exact_dot16_sum(av[pp], bv[pp]);
        if (e0 + 4 * (h2 + 2) >= nlist) break;
      }
#pragma unroll
      for (int p = 0; p < NPASS; ++p) {
        const int idx = e0 + 4 * p + sub;
        if (e0 + 4 * p >= nlist) break;
        const int pos = __shfl(myres, 4 * p + sub);
        const float nmr_e = __shfl(my_nmr, 4 * p + sub), nmc_e = __shfl(my_nmc, 4 * p + sub);
        if (l16 == 0 && idx < nlist) {
          const int row = wrow0 + ((key[p] >> 5) & 31), col = (u0 + ((key[p] >> 10) & 63)) * 32 + (key[p] & 31);
          const float rr = __builtin_fmaf(xs[p], a.k, nmr_e);
          const float cc = __builtin_fmaf(xs[p], a.k, nmc_e);
          const int pr = pos & 0xffff, pc = (pos >> 16) & 0xffff;
          const long grow = (long)b * a.Lp + row, gcol = (long)b * a.Sp + col;
          if (pr < a.slots) { a.rlist_j[grow * a.slots + pr] = col; a.rlist_x[grow * a.slots + pr] = rr > -kSkipLog2 ? xs[p] : -INFINITY; }
          else overflow = 1;
          if (pc < a.slots) { a.clist_i[gcol * a.slots + pc] = row; a.clist_x[gcol * a.slots + pc] = cc > -kSkipLog2 ? xs[p] : -INFINITY; }
          else overflow = 1;
        }
      }
    }
  }
  nd_units += __builtin_popcountll(__ballot(overflow != 0));
  if (nd_units && lane == 0) {
    a.dense_cnt[b] = 1;
    a.scal->dense_units = 1;
    if (!a.dense_enabled) atomicOr(&a.scal->flags, (unsigned)FM_DEV_DENSE);
  }
}

static void fill_screen_stats(ScreenArgs& a, const CoarseWs& w, char* base, float inv_ct, float thr, int allow_dead) {
  a.rowmax_u = w.rowmax_u.in(base); a.colmax_u = w.colmax_u.in(base);
  a.sigimg = w.sigimg.in(base); a.imgstat = w.imgstat.in(base);
  a.l1_0 = w.l1_0.in(base); a.l1_1 = w.l1_1.in(base);
  a.bstat0 = w.bstat0.in(base); a.bstat1 = w.bstat1.in(base);
  a.umax = w.umax.in(base);
  a.nmr = w.nmr.in(base); a.nmc = w.nmc.in(base); a.emarg = w.emarg.in(base);
  a.dense_cnt = w.dense_cnt.in(base); a.scal = w.scalars.in(base);
  a.L = w.L; a.S = w.S; a.Lp = w.Lp; a.Sp = w.Sp;
  a.slots = w.slots; a.allow_dead = allow_dead;
  a.k = k2_of(inv_ct); a.lt = log2f(thr); a.inv_ct = inv_ct; a.cpad = (float)w.C;
}

hipError_t launch_stab(const CoarseWs& w, char* base, float inv_ct, float thr, int allow_dead, hipStream_t st) {
  ScreenArgs a;
  memset(&a, 0, sizeof(a));
  fill_screen_stats(a, w, base, inv_ct, thr, allow_dead);
  const int lenp = w.Lp > w.Sp ? w.Lp : w.Sp;
  hipLaunchKernelGGL(k_stab, dim3((lenp + 255) / 256, w.N, 2), dim3(256), 0, st, a, w.f16inv.in(base));
  return hipGetLastError();
}

hipError_t launch_screen(const void* feat0, const void* feat1, int in_dtype, int c_in, const CoarseWs& w, char* base,
                         float inv_ct, float thr, int dense_enabled, int allow_dead, bool defer, hipStream_t st) {
  ScreenArgs a;
  memset(&a, 0, sizeof(a));
  fill_screen_stats(a, w, base, inv_ct, thr, allow_dead);
  a.q0 = w.q0.in(base); a.q1 = w.q1.in(base);
  a.desc = DescRows{feat0, feat1, c_in, in_dtype, w.L, w.S};
  a.rcount = w.cand.count.in(base); a.rlist_j = w.cand.idx.in(base); a.rlist_x = w.cand.x.in(base);
  a.ccount = w.ccand.count.in(base); a.clist_i = w.ccand.idx.in(base); a.clist_x = w.ccand.x.in(base);
  a.dense_enabled = dense_enabled;
  RowsExtra x;
  x.thr_r = w.thr_r.in(base); x.thr_c = w.thr_c.in(base);
  x.wmaxb = w.wmaxb.in(base); x.cmaxu = w.cmaxu.in(base);
  x.tmin_r = w.tmin_r.in(base); x.tmin_c = w.tmin_c.in(base);
  x.umax2 = w.umax2.in(base); x.upos = w.upos.in(base);
  x.look = g_unit_cert != 1;
  x.count_cert = g_unit_cert == 2;
  x.defer = defer ? 1 : 0;
  x.count_defer = defer && g_defer_exact == 2;
  x.chunk_units = w.units_s;
  x.nchunks = w.splits_s;
#ifdef FM_TUNE_ENV
  if (const char* ev = getenv("FM_ROWS_CHUNK")) { x.chunk_units = atoi(ev); x.nchunks = (w.Sp / 32 + x.chunk_units - 1) / x.chunk_units; }
#endif
  x.items = (int)((long)w.N * (w.Lp / 32) * x.nchunks);
  const int lenp = w.Lp > w.Sp ? w.Lp : w.Sp;
  hipLaunchKernelGGL(k_thresh, dim3((lenp + 255) / 256, w.N, 2), dim3(256), 0, st, a, x);
  const int blocks_r = (x.items + 3) / 4;
  return with_padded_channels(w.C, [&](auto cc) {
    hipLaunchKernelGGL(k_screen_rows<cc.value>, dim3(blocks_r), dim3(256), 0, st, a, x);
    return hipGetLastError();
  });
}

}  // namespace fm
