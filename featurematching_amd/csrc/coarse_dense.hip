// Coarse stage, the DENSE sum kernel (round 4): dual-softmax denominators and candidates of the samples whose similarity
// is flat - every entry matters - from a float32-equivalent product on the f16 matrix cores.
//
// Reproduces network/utils/coarse_matching_new.py:64-68 for the samples the screening kernel flagged (dense_cnt[b] > 0):
//   raw = hi0.hi1 + lo0.hi1 + hi0.lo1   (float16 hi / lo planes of k_prep_f16: 22 significant bits)
//   row sums  sum_j exp2(k raw - m^_i), column sums  sum_i exp2(k raw - c^_j)  with the stabilisers of the screening
//   kernel, and the candidate list {(i,j): both terms > thr} - a superset of every entry with conf > thr (:99).
// It replaces k_corr<C,1> of rounds 1-3, whose in-kernel stamps at 640x480 read: 85k cycles per wave for 12 units of
// 1.5k cycles of matrix work each - 10k of prologue, 2.1k + 1.1k per unit for the MFMA chain and the epilogue one after
// the other, 9k in barriers of a two-deep tile ring, 2k per unit of bookkeeping (unit maxima, skip tests, wave-wide
// maxima).  What is different here:
//   * NO block-sparse skipping: a sample comes here because its similarity is flat; the unit maxima, their margins and
//     the per-unit wave-wide reductions are gone;
//   * the ring holds four UNITS (32 columns, hi + lo = 32 KiB at C = 256) instead of two 64-column tiles: three units
//     of LDS-DMA in flight, handed over by counted vmcnt + one raw s_barrier per unit;
//   * the epilogue of unit u-1 (exp2 of the row and of the column term of 16 accumulator registers, the running sums,
//     the candidate test) is sliced over the 16 k-steps of unit u's MFMA chain: a wave issues in order, so the vector
//     work only runs under the matrix cores' 96 cycles per k-step if it sits between the MFMAs in program order;
//   * the rows' stabilisers come from one register by v_readlane (no LDS reads between the counted B-fragment waits).
// Structure otherwise as before: one workgroup = 8 waves = a 256-row panel x a range of columns; each wave keeps its 32
// rows' hi and lo A fragments (128 VGPRs at C = 256) for the whole sweep; the 8 waves' column sums of a unit meet in
// LDS and one wave folds them in a fixed order (deterministic) into the panel's partial.
//
// At the end of this file: what makes the dense kernel's lists exact and patches its conf_matrix when a forward call
// reads every entry (conf_matrix requests, FM_MODE_STATS) - k_exact_lists, k_fix_sums, k_conf_patch, their two launchers.
#include <type_traits>

#include "fm_exact_device.h"

namespace fm {

constexpr int kDenseQueue = 64;       // candidates a wave parks in LDS (one per lane at the hand-over)
constexpr int kDenseRing = 4;         // units of the LDS ring

struct DenseArgs {
  const _Float16* hi0; const _Float16* lo0; const _Float16* hi1; const _Float16* lo1;
  const float* nmr; const float* nmc;
  float* rowpart; float* colpart;       // [N][splits][Lp], [N][panels][Sp]
  const int* dense_cnt; const int* dense_units; const float* f16inv;
  int* cand_count; int* cand_j; float* cand_x; int* ccand_count; int* ccand_i; float* ccand_x;   // the dense kernel's lists
  unsigned* flags;
  float* diag;                          // diagnostic build: stamp buffer (the screening kernel's cand_x region)
  float* conf;                          // CONF variant: the dense [N, L, S] conf_matrix (nmr / nmc then hold the log-softmax offsets)
  int L, S, Lp, Sp, panels, units, splits, units_per_split, slots, pgroup;
  float k, lt;
};

// CONF (round 4): the same sweep writes data['conf_matrix'] (coarse_matching_new.py:68,70) for EVERY sample instead of
// forming sums and candidates - conf = exp2(k x + nmr2_i) * exp2(k x + nmc2_j) with the log-softmax offsets of
// k_reduce_sums, the arithmetic of k_corr<C,3>, which it replaces (2.50 ms for the 5.9 GB of a 64-pair batch: a two-deep
// tile ring whose epilogue - and with it every store - ran behind the MFMA chain).  The epilogue slice of a register is
// two fused multiply-adds, two exp2, one multiply and ONE store (a scalar row base + a per-lane offset: 32 consecutive
// floats of two rows per instruction), spread over the next unit's k-steps like the sums' slices.
// RESCREEN (round 4; replaces k_corr<C,2>, the last user of the tile-based sweep of rounds 1-3): the exact re-screening
// of FM_MODE_EXACT_SCREENING - only when the sum sweep overflowed a row's or a column's candidate slots: the same
// product again, the candidate test with the now-known softmax denominators (log2 P_row > log2 thr and log2 P_col >
// log2 thr: at most 1/thr entries of a row can pass), no sums; the lists of the samples the sum sweep served are
// refilled from scratch (k_reduce_sums cleared their counters).  Enqueued always, exits at once when not needed.
// CONF_LITE (round 5): the conf sweep of the samples the SCREENING kernel served.  There every entry that is not on its
// row's list of significant entries has exp2(k x + nm) < 2^-32 of its row's largest term - conf < 2.4e-10 whatever a few
// per cent of relative error do to it - and every entry that is on a list is rewritten from its exact float32 dot product
// by k_conf_patch: ONE float16 product (hi x hi, 11 bits) is enough.  A third of the MFMAs and, more to the point, half
// of the plane bytes per unit: the sweep is bound by its memory stream (tools/microbench_store_pattern.hip: the same
// stores with 32 KiB of plane reads per unit and NO arithmetic take 1.6-1.9 ms at cfg#3, with reads that always hit 0.93).
// The samples the dense kernel served (flat similarity: entries of every size) keep the hi/lo-split product (CONF).
enum { kDenseSums = 0, kDenseConf = 1, kDenseRescreen = 2, kDenseConfLite = 3 };
template <int C, int VAR = kDenseSums>
__global__ __launch_bounds__(512) void k_dense(DenseArgs a) {
  constexpr bool LITE = VAR == kDenseConfLite;
  constexpr bool CONF = VAR == kDenseConf || LITE, RESCREEN = VAR == kDenseRescreen, SUMS = VAR == kDenseSums;
  constexpr int KSTEPS = C / 16;
  constexpr int PLANE = KSTEPS * 1024;              // bytes of one plane (hi or lo) of a unit
  constexpr int UNIT_BYTES = 2 * PLANE;             // hi then lo
  constexpr int NPIECE = LITE ? KSTEPS : 2 * KSTEPS;      // LDS-DMA pieces (1 KiB) per unit: (plane, k-step)
  constexpr int PW = (NPIECE + 7) / 8;              // ... per wave (LITE at C = 64: 4 pieces - waves 4 .. 7 bring none)
  constexpr int SPK = 16 / KSTEPS;                  // epilogue slices (accumulator registers) per k-step
  extern __shared__ __attribute__((aligned(16))) char smem[];      // the unit ring
  __shared__ float s_meta[kDenseRing * 64];         // per ring slot: the unit's 32 column stabilisers (twice)
  __shared__ float s_colred[3 * 8 * 32];            // per unit (mod 3): the 8 waves' column sums of 32 columns
  __shared__ int s_qkey[8 * kDenseQueue];           // wave-private candidate queue: (col << 5) | local row
  __shared__ float s_qx[8 * kDenseQueue];

  if (SUMS && *a.dense_units == 0) return;          // uniform: the screening kernel handled every sample
  if (RESCREEN && !(*a.flags & FM_INT_SCREEN_OVERFLOW)) return;     // uniform: the sum sweep's screening sufficed
#ifdef FM_DIAG_CLOCK       // diagnostic build only: shader-clock stamps per phase of every wave (tools/diag_clock.py)
  const unsigned long long dg0 = __builtin_amdgcn_s_memtime(), dgr0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long dg_chain = 0, dg_bar = 0, dg_pro = 0, dg_loop_end = 0;
#define DG_T0 const unsigned long long dg_t = __builtin_amdgcn_s_memtime();
#define DG_ADD(x) x += __builtin_amdgcn_s_memtime() - dg_t;
#else
#define DG_T0
#define DG_ADD(x)
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  int kk = xcd_contiguous(blockIdx.x, gridDim.x);
  const int per_sample = a.panels * a.splits;
  const int b = kk / per_sample;
  kk -= b * per_sample;
  const int gsz = a.pgroup * a.splits;
  const int pg = kk / gsz;
  kk -= pg * gsz;
  const int pcount = min(a.pgroup, a.panels - pg * a.pgroup);
  const int split = kk / pcount;
  const int panel = pg * a.pgroup + (kk - split * pcount);
  const int u0 = split * a.units_per_split, u1 = min(u0 + a.units_per_split, a.units);
  if (!CONF && a.dense_cnt[b] == 0) return;         // uniform: this sample was served by the screening kernel
  if (CONF && LITE != (a.dense_cnt[b] == 0)) return;        // uniform: the conf sweep of this sample is the other variant's
  const float inv_sc = a.f16inv[b];                 // the planes carry exact power-of-two scales (k_prep_f16)
  const float kq = a.k * inv_sc;                    // accumulator -> log2-domain similarity
  const char* plane_hi = reinterpret_cast<const char*>(a.hi1 + (long)b * a.Sp * C);
  const char* plane_lo = reinterpret_cast<const char*>(a.lo1 + (long)b * a.Sp * C);
  const unsigned ring_a = lds_addr(smem), meta_a = lds_addr(s_meta), colred_a = lds_addr(s_colred);
  const unsigned qkey_a = lds_addr(s_qkey + wv * kDenseQueue), qx_a = lds_addr(s_qx + wv * kDenseQueue);

  // one unit = 2 * KSTEPS pieces of 1 KiB ((plane, k-step): the 64 lanes of an MFMA operand fragment), contiguous in
  // the fragment-major planes; the waves take the pieces round robin; wave 0 also brings the unit's 32 column stabilisers
  auto stage = [&](int u) {
    const int slot = (u - u0) % kDenseRing;
#pragma unroll
    for (int n = 0; n < PW; ++n) {
      const int p = wv * PW + n;                    // 0 .. 2 KSTEPS - 1: hi pieces first, then lo
      if (NPIECE < 8 * PW && p >= NPIECE) break;
      const char* src = (p < KSTEPS ? plane_hi : plane_lo) + ((long)u * KSTEPS + (p < KSTEPS ? p : p - KSTEPS)) * 1024 + lane * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(smem + slot * UNIT_BYTES + p * 1024), 16, 0, 0);
    }
    if (wv == 0)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.nmc + (long)b * a.Sp + u * 32 + r),
                                       (__attribute__((address_space(3))) void*)(s_meta + slot * 64), 4, 0, 0);
  };
#pragma unroll
  for (int d = 0; d < kDenseRing - 1; ++d)
    if (u0 + d < u1) stage(u0 + d);

  // ---- this wave's 32 rows as A fragments (lane (r,h): row r, k = h*C/2 + 8*ks + 0..7), hi and lo ----
  const int wrow0 = panel * kPanelRows + wv * 32;
  // -stabiliser*log2e of row wrow0 + (lane & 31) (both halves hold it), requested AHEAD of the A fragments: older in the
  // vmcnt order, so picking the rows' values out of it below does not wait for them
  const float nv = a.nmr[(long)b * a.Lp + wrow0 + r];
  half8 ahi[KSTEPS], alo[KSTEPS];
  {
    const long off = (((long)b * a.Lp + wrow0) / 32 * KSTEPS * 64 + lane) * 8;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      ahi[ks] = *reinterpret_cast<const half8*>(a.hi0 + off + ks * 512);
      if constexpr (!LITE) alo[ks] = *reinterpret_cast<const half8*>(a.lo0 + off + ks * 512);
    }
  }
  float nmsel[16];                                  // ... of this lane's 16 rows (accumulator register g: row (g&3) + 8 (g>>2) + 4 h)
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row0 = (g & 3) + 8 * (g >> 2);
    const float n0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nv), row0));
    const float n1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nv), row0 + 4));
    nmsel[g] = h ? n1 : n0;
  }
  const bool row_edge = (wrow0 + 32 > a.L);
  int qn = 0;                                       // parked candidates (per lane: the wave's count is kept in lane 0's view)
  float rstat[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) rstat[g] = 0.f;

  auto unit_barrier = [&](int units_after) {        // the next unit has landed; later ones stay in flight
    if (units_after <= 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else if (units_after == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(PW) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(2 * PW) : "memory");
    __builtin_amdgcn_s_barrier();
  };
  // The first unit has landed once its pieces - the OLDEST vector-memory operations of this wave - are done: everything
  // younger (the next units' pieces, the 2 KSTEPS A-fragment loads, the stabilisers) may stay in flight across the
  // barrier; the first chain then takes each A fragment as it arrives (the compiler's own counted waits), instead of
  // the whole prologue - ~350 KB per workgroup through one CU's 64 B/clk - in front of the first MFMA (12k cycles).
  {
    constexpr int YOUNGER = LITE ? KSTEPS : 2 * KSTEPS;      // the A fragments (the other units' pieces only make it safer)
    static_assert(YOUNGER <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(YOUNGER) : "memory");
    __builtin_amdgcn_s_barrier();
  }
  float* colout = a.colpart + ((long)b * a.panels + panel) * a.Sp;
  auto fold_columns = [&](int u) {                  // the 8 waves' sums of unit u's 32 columns, in wave order
    if (!SUMS || wv != (u & 7) || lane >= 32) return;
    const unsigned ad = colred_a + (((u - u0) % 3) * 8 * 32 + lane) * 4;
    float pv[8];
#pragma unroll
    for (int w8 = 0; w8 < 8; ++w8) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(pv[w8]) : "v"(ad), "i"(w8 * 128));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]), "+v"(pv[4]), "+v"(pv[5]),
                 "+v"(pv[6]), "+v"(pv[7]));
    float cv = pv[0];
#pragma unroll
    for (int w8 = 1; w8 < 8; ++w8) cv += pv[w8];
    colout[u * 32 + lane] = cv;
  };

  f32x16 accC;                                      // the accumulators of the unit whose epilogue is due
  float nmc_c = 0.f;                                // its column stabiliser (this lane's column)
#pragma unroll
  for (int g = 0; g < 16; ++g) accC[g] = 0.f;

  // one pass: the MFMA chain of unit `un` (when DN) with the epilogue of unit `uc` (when DC) sliced between its k-steps
  auto pass = [&](auto dn, auto dc, int un, int uc) {
    constexpr bool DN = decltype(dn)::value, DC = decltype(dc)::value;
    f32x16 accN;
    float nmc_n = 0.f;
    float cstat = 0.f;
    unsigned bm = 0;                                  // this lane's candidate registers of unit uc: bit 15 - g
    const float kqv = kq, ltv = a.lt;
    // CONF: unit uc's tile of the matrix - a scalar base (row wrow0, column 32 uc), the lane's own offset (row 4 h, column
    // r), the row pitch in bytes; a (wave, unit) that touches the matrix's edge stores behind the chain, predicated
    const char* conf_base = nullptr;
    long conf_pitch = 0;
    unsigned conf_voff = 0;
    bool conf_full = false;
    if constexpr (CONF) {
      if (DC) {
        conf_pitch = (long)a.S * 4;
        conf_base = reinterpret_cast<const char*>(a.conf + ((long)b * a.L + wrow0) * a.S + (long)uc * 32);
        conf_voff = (unsigned)((4 * h * a.S + r) * 4);
        conf_full = !row_edge && uc * 32 + 32 <= a.S;
#ifdef FM_ABL_CONF_SMALLDST     // timing-only ablation (results are wrong): every store lands in the same 64 KiB
        conf_pitch = 0;
        conf_base = reinterpret_cast<const char*>(a.conf) + wv * 8192;
        conf_voff = (unsigned)(lane * 4);
#endif
      }
    }
    const unsigned base = ring_a + ((un - u0) % kDenseRing) * UNIT_BYTES + lane * 16;
    constexpr int PF = KSTEPS < 3 ? KSTEPS - 1 : 2;      // B-fragment read-ahead (k-steps): LDS latency under 8 waves' reads
    constexpr int RING = PF + 1;                         // is ~300 cycles, a k-step of this wave ~150
    half8 bh[RING], bl[RING];
    // (a capture-less lambda with explicit operands: hipcc does not let a generic lambda nested in a generic lambda
    // capture the enclosing one's arrays)
    auto issue_ = [](auto ksc, half8 (&bh_)[RING], half8 (&bl_)[RING], unsigned base_) {
      constexpr int ks = decltype(ksc)::value;
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bh_[ks % RING]) : "v"(base_), "i"(ks * 1024));
      if constexpr (!LITE) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bl_[ks % RING]) : "v"(base_), "i"(PLANE + ks * 1024));
    };
#define issue(...) issue_(__VA_ARGS__, bh, bl, base)
    if (DN) {
      asm volatile("ds_read_b32 %0, %1" : "=v"(nmc_n) : "v"(meta_a + (((un - u0) % kDenseRing) * 64 + r) * 4));
      issue(std::integral_constant<int, 0>{});
      if constexpr (PF > 1) issue(std::integral_constant<int, 1>{});
    }
    auto kstep = [&](auto self, auto ksc) {
      constexpr int ks = decltype(ksc)::value;
      if (DN) {
        if constexpr (ks + PF < KSTEPS) issue(std::integral_constant<int, ks + PF>{});
        constexpr int ahead = (KSTEPS - 1 - ks) < PF ? (KSTEPS - 1 - ks) : PF;     // k-steps issued beyond ks
        if constexpr (LITE) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(bh[ks % RING]), "+v"(nmc_n) : "n"(ahead));
        else asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(bh[ks % RING]), "+v"(bl[ks % RING]), "+v"(nmc_n) : "n"(2 * ahead));
        if (ks == 0) {
          // The accumulator starts at 0, or at -inf for padded rows (>= L) / padded columns (>= S): such entries stay
          // -inf through the whole chain, so the epilogue needs no masks (exp2 gives 0, the candidate test fails)
          f32x16 z;
#pragma unroll
          for (int g = 0; g < 16; ++g) z[g] = 0.f;
          if (row_edge || un * 32 + 32 > a.S) {
            const float cb = (un * 32 + r < a.S) ? 0.f : -INFINITY;
#pragma unroll
            for (int g = 0; g < 16; ++g) z[g] = (wrow0 + (g & 3) + 8 * (g >> 2) + 4 * h < a.L) ? cb : -INFINITY;
          }
          accN = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ks], bh[ks % RING], z, 0, 0, 0);
        } else {
          accN = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ks], bh[ks % RING], accN, 0, 0, 0);
        }
#ifndef FM_ABL_DENSE_ONEMFMA    // timing-only ablation: one product instead of three
        if constexpr (!LITE) {
          accN = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[ks], bh[ks % RING], accN, 0, 0, 0);
          accN = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ks], bl[ks % RING], accN, 0, 0, 0);
        }
#endif
      }
#ifndef FM_ABL_DENSE_NOEPI      // timing-only ablation (results are wrong): never defined in the shipped build
      if (DC) {
#pragma unroll
        for (int sg = 0; sg < SPK; ++sg) {
          const int g = ks * SPK + sg;
          // One slice = one accumulator register (x = -inf for padded rows / columns), as volatile asm: hipcc moved the
          // row half of a C++ version behind the whole MFMA chain, where nothing hides it.  Seven vector instructions:
          // the SIMD's instruction issue is what two waves' epilogues and MFMAs compete for (a 15-instruction slice
          // - stabiliser by v_readlane + per-half exec masks, min / max candidate filter - cost 35k of 94k cycles).
          // Candidates (both terms > thr) are marked on the spot: v_cmp + v_addc shift the hit into a per-lane bit mask
          // (bit 15 - g).  A filter + rescan of the 16 registers took ~1k cycles whenever ANY of the workgroup's 8 waves
          // entered it - nearly every unit - and the per-unit barrier made all of them wait: 13k of 82k cycles.
          if constexpr (CONF) {
            // (round 5, in-kernel clock at cfg#3, tools/diag_conf_clock.py: 6140 cycles per unit and workgroup; the same
            // kernel with the store removed 3160 at one product (FM_ABL_CONF_NOSTORE), with every store aimed at the same
            // 64 KiB 3350 (FM_ABL_CONF_SMALLDST): what the stores cost is the write path behind the L2, ~160 cycles of
            // wave time each, while the whole sweep writes at 2.5 TB/s - a store-only kernel of the same shape and
            // occupancy reaches 5.5 (tools/microbench_store_pattern.hip).  Tried without effect: counting the stores in
            // the per-unit vmcnt wait instead of draining them, the SIMD's two waves storing in alternate halves of the
            // k-steps, the conf value formed in the accumulator register (no write-after-read on the store's data),
            // nontemporal stores (slower there: 7070).)
            // conf of register g's entry and its store: rows (g & 3) + 8 (g >> 2) [+ 4 for the upper half], column r
            float t1, t2;
            const char* rowbase = conf_base + (long)((g & 3) + 8 * (g >> 2)) * conf_pitch;      // (wave-uniform: scalar)
            if (conf_full) {
              // (nontemporal stores in the one-product sweep, whose limit is the memory stream: 3.05 -> 2.84 ms for the whole
              // conf stage at cfg#3; in the hi/lo-split sweep, which the matrix cores' power budget clocks down, they cost time:
              // 7070 against 6410 cycles per unit)
#if defined(FM_ABL_CONF_NOEXP)           // timing-only ablations (results are wrong): never defined in the shipped build
#define FM_CONF_EXP ""
#else
#define FM_CONF_EXP "v_exp_f32 %[t1], %[t1]\n\tv_exp_f32 %[t2], %[t2]\n\ts_nop 0\n\t"
#endif
#if defined(FM_ABL_CONF_NOSTORE)
#define FM_CONF_STORE(POLICY) ""
#else
#define FM_CONF_STORE(POLICY) "global_store_dword %[vo], %[t1], %[sb]" POLICY
#endif
#define FM_CONF_SLICE(POLICY)                                                                                              \
  asm volatile("v_fma_f32 %[t1], %[x], %[kq], %[nm]\n\t"                                                                   \
               "v_fma_f32 %[t2], %[x], %[kq], %[nmc]\n\t" FM_CONF_EXP "v_mul_f32 %[t1], %[t1], %[t2]\n\t" FM_CONF_STORE(POLICY) \
               : [t1] "=&v"(t1), [t2] "=&v"(t2)                                                                            \
               : [x] "v"(accC[g]), [kq] "v"(kqv), [nm] "v"(nmsel[g]), [nmc] "v"(nmc_c), [vo] "v"(conf_voff), [sb] "s"(rowbase) \
               : "memory")
              if constexpr (LITE) FM_CONF_SLICE(" nt");
              else FM_CONF_SLICE("");
#undef FM_CONF_SLICE
#undef FM_CONF_STORE
#undef FM_CONF_EXP
            }
          } else if constexpr (RESCREEN) {
            // log2 P_row and log2 P_col of register g's entry against log2 thr: the hit goes into the lane's bit mask
            float t1, t2;
            asm volatile(
                "v_fma_f32 %[t1], %[x], %[kq], %[nm]\n\t"
                "v_fma_f32 %[t2], %[x], %[kq], %[nmc]\n\t"
                "v_min_f32 %[t1], %[t1], %[t2]\n\t"
                "v_cmp_lt_f32 vcc, %[lt], %[t1]\n\t"
                "v_addc_co_u32 %[bm], vcc, %[bm], %[bm], vcc"
                : [t1] "=&v"(t1), [t2] "=&v"(t2), [bm] "+v"(bm)
                : [x] "v"(accC[g]), [kq] "v"(kqv), [nm] "v"(nmsel[g]), [nmc] "v"(nmc_c), [lt] "v"(ltv)
                : "vcc");
          } else {
          float t1, t2, t3;
          asm volatile(
              "v_fma_f32 %[t1], %[x], %[kq], %[nm]\n\t"
              "v_fma_f32 %[t2], %[x], %[kq], %[nmc]\n\t"
              "v_min_f32 %[t3], %[t1], %[t2]\n\t"
#ifndef FM_ABL_DENSE_NOEXP       // timing-only ablation
              "v_exp_f32 %[t1], %[t1]\n\t"
              "v_exp_f32 %[t2], %[t2]\n\t"
#endif
              "v_cmp_lt_f32 vcc, %[lt], %[t3]\n\t"
              "v_addc_co_u32 %[bm], vcc, %[bm], %[bm], vcc\n\t"
              "v_add_f32 %[rs], %[rs], %[t1]\n\t"
              "v_add_f32 %[cs], %[cs], %[t2]"
              : [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [bm] "+v"(bm), [rs] "+v"(rstat[g]), [cs] "+v"(cstat)
              : [x] "v"(accC[g]), [kq] "v"(kqv), [nm] "v"(nmsel[g]), [nmc] "v"(nmc_c), [lt] "v"(ltv)
              : "vcc");
          }
        }
      }
#endif
      if (DN && DC) __builtin_amdgcn_sched_barrier(0);
      if constexpr (ks + 1 < KSTEPS) self(self, std::integral_constant<int, ks + 1>{});
    };
    kstep(kstep, std::integral_constant<int, 0>{});
#undef issue
    if constexpr (CONF) {
      if (DC && !conf_full && wrow0 < a.L) {        // the matrix's edge: predicated stores (x = -inf beyond it)
        const int col = uc * 32 + r;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = wrow0 + (g & 3) + 8 * (g >> 2) + 4 * h;
          const float cf = __builtin_amdgcn_exp2f(__builtin_fmaf(accC[g], kqv, nmsel[g])) *
                           __builtin_amdgcn_exp2f(__builtin_fmaf(accC[g], kqv, nmc_c));
          if (row < a.L && col < a.S) a.conf[((long)b * a.L + row) * a.S + col] = cf;
        }
      }
    }
    if (DC && !CONF) {
      if constexpr (SUMS) {
        cstat = pair_op<32, OpAdd>(cstat);          // lane l + lane l ^ 32: this wave's 32 rows of column r
        if (h == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(colred_a + ((((uc - u0) % 3) * 8 + wv) * 32 + r) * 4), "v"(cstat) : "memory");
      }
      {
        // (padded rows / columns carry x = -inf: never marked)
        unsigned long long hitl = __ballot(bm != 0);
        while (hitl) {                              // wave-uniform, usually one lane
          const int l = __builtin_ctzll(hitl);
          hitl &= hitl - 1;
          unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)bm, l);
          while (bits) {
            const int g = 15 - __builtin_ctz(bits);
            bits &= bits - 1;
            const int key = ((uc * 32 + (l & 31)) << 5) | ((g & 3) + 8 * (g >> 2) + 4 * (l >> 5));
            // (accumulator register g of lane l: a dynamic register index - sixteen selects, on this rare path)
            float xg = accC[0];
#pragma unroll
            for (int q = 1; q < 16; ++q) xg = g == q ? accC[q] : xg;
            const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xg), l)) * inv_sc;
            if (qn < kDenseQueue) {
              if (lane == 0) {
                asm volatile("ds_write_b32 %0, %1" ::"v"(qkey_a + qn * 4), "v"(key) : "memory");
                asm volatile("ds_write_b32 %0, %1" ::"v"(qx_a + qn * 4), "v"(xv) : "memory");
              }
            } else if (lane == 0) {                 // queue full: straight to the lists
              const long grow = (long)b * a.Lp + wrow0 + (key & 31), gcol = (long)b * a.Sp + (key >> 5);
              const int pos = atomicAdd(&a.cand_count[grow], 1), cpos = atomicAdd(&a.ccand_count[gcol], 1);
              if (pos < a.slots) { a.cand_j[grow * a.slots + pos] = key >> 5; a.cand_x[grow * a.slots + pos] = xv; }
              if (cpos < a.slots) { a.ccand_i[gcol * a.slots + cpos] = wrow0 + (key & 31); a.ccand_x[gcol * a.slots + cpos] = xv; }
              if (pos >= a.slots || cpos >= a.slots) atomicOr(a.flags, RESCREEN ? (unsigned)FM_DEV_CANDIDATES : (unsigned)FM_INT_SCREEN_OVERFLOW);
            }
            ++qn;
          }
        }
      }
    }
    if (DN) {
#pragma unroll
      for (int g = 0; g < 16; ++g) accC[g] = accN[g];
      nmc_c = nmc_n;
    }
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;

  // Per unit u: refill the ring slot of unit u-1 (every wave left it at the previous barrier) | MFMAs(u) with the
  // epilogue of u-1 between them | barrier: every wave has read unit u, unit u+1 has landed | fold unit u-1's columns
#ifdef FM_DIAG_CLOCK
  dg_pro = __builtin_amdgcn_s_memtime() - dg0;
#endif
#ifdef FM_DENSE_PRIO      // experiment: static priority for the later-dispatched half (MI355X_MICROARCH.md, two waves per SIMD, item 4)
  if (wv >= 4) __builtin_amdgcn_s_setprio(1);
#endif
  if (u0 < u1) {
    if (u0 + kDenseRing - 1 < u1) stage(u0 + kDenseRing - 1);
    { DG_T0 pass(T_{}, F_{}, u0, 0); asm volatile("" ::"v"(accC)); DG_ADD(dg_chain) }
    { DG_T0 unit_barrier(min(u0 + kDenseRing - 1, u1 - 1) - (u0 + 1)); DG_ADD(dg_bar) }
    for (int u = u0 + 1; u < u1; ++u) {
      if (u + kDenseRing - 1 < u1) stage(u + kDenseRing - 1);
      { DG_T0 pass(T_{}, T_{}, u, u - 1); asm volatile("" ::"v"(accC)); DG_ADD(dg_chain) }
      { DG_T0 unit_barrier(min(u + kDenseRing - 1, u1 - 1) - (u + 1)); DG_ADD(dg_bar) }
      fold_columns(u - 1);
    }
    { DG_T0 pass(F_{}, T_{}, 0, u1 - 1); DG_ADD(dg_chain) }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    fold_columns(u1 - 1);
  }

#ifdef FM_DIAG_CLOCK
  dg_loop_end = __builtin_amdgcn_s_memtime();
#endif
#ifdef FM_DIAG_CLOCK       // the screening kernel's row-list slots of the padded rows (>= L, never used) carry 64 waves' stamps
  auto diag_stamp = [&]() {
  if (split == 0 && panel < 8 && (a.Lp - a.L) * a.slots >= 512 && lane < 8) {
    const float vals[8] = {(float)(__builtin_amdgcn_s_memtime() - dg0), (float)(__builtin_amdgcn_s_memrealtime() - dgr0),
                           (float)(u1 - u0), (float)dg_chain, 0.f, (float)dg_bar, (float)dg_pro,
                           (float)(__builtin_amdgcn_s_memtime() - dg_loop_end)};
    float vv = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) vv = lane == q ? vals[q] : vv;
    a.diag[((long)b * a.Lp + a.L) * a.slots + (panel * 8 + wv) * 8 + lane] = vv;
  }
  };
  if constexpr (CONF) diag_stamp();
#endif
  if constexpr (CONF) return;
  // ---- the parked candidates -> the per-row / per-column slot lists: one entry per lane; the slot reservation (a
  // returning atomic: one memory round trip) is issued here and consumed behind the row reduction below ----
  int q_pos = -1, q_cpos = -1, q_key = 0;
  float q_x = 0.f;
  long q_row = 0, q_col = 0;
  {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int nq = min(qn, kDenseQueue);
    if (lane < nq) {
      asm volatile("ds_read_b32 %0, %1" : "=v"(q_key) : "v"(qkey_a + lane * 4));
      asm volatile("ds_read_b32 %0, %1" : "=v"(q_x) : "v"(qx_a + lane * 4));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q_key), "+v"(q_x));
      q_row = (long)b * a.Lp + wrow0 + (q_key & 31);
      q_col = (long)b * a.Sp + (q_key >> 5);
      q_pos = atomicAdd(&a.cand_count[q_row], 1);
      q_cpos = atomicAdd(&a.ccand_count[q_col], 1);
    }
  }
  // ---- row sums of this workgroup's column range: reduce over the 32 lanes of each half ----
  if constexpr (SUMS) {
#pragma unroll
    for (int g = 0; g < 16; ++g) rstat[g] = half_all<OpAdd>(rstat[g]);
    if (r == 0) {
      float* out = a.rowpart + ((long)b * a.splits + split) * a.Lp + wrow0 + 4 * h;
#pragma unroll
      for (int g = 0; g < 16; ++g) out[(g & 3) + 8 * (g >> 2)] = rstat[g];
    }
  }
  if (q_pos >= 0) {
    if (q_pos < a.slots) { a.cand_j[q_row * a.slots + q_pos] = q_key >> 5; a.cand_x[q_row * a.slots + q_pos] = q_x; }
    if (q_cpos < a.slots) { a.ccand_i[q_col * a.slots + q_cpos] = wrow0 + (q_key & 31); a.ccand_x[q_col * a.slots + q_cpos] = q_x; }
    if (q_pos >= a.slots || q_cpos >= a.slots) atomicOr(a.flags, RESCREEN ? (unsigned)FM_DEV_CANDIDATES : (unsigned)FM_INT_SCREEN_OVERFLOW);
  }
#ifdef FM_DIAG_CLOCK
  diag_stamp();
#endif
}

hipError_t launch_dense(const CoarseWs& w, char* base, float inv_ct, float thr, hipStream_t st, float* conf, int rescreen) {
  DenseArgs a;
  a.conf = conf;
  const bool offsets = conf != nullptr || rescreen;      // both read the log-softmax offsets of k_reduce_sums
  a.hi0 = w.hi0.in(base); a.lo0 = w.lo0.in(base);
  a.hi1 = w.hi1.in(base); a.lo1 = w.lo1.in(base);
  a.nmr = (offsets ? w.nmr2 : w.nmr).in(base); a.nmc = (offsets ? w.nmc2 : w.nmc).in(base);
  a.rowpart = w.rowB.in(base); a.colpart = w.colB.in(base);
  a.dense_cnt = w.dense_cnt.in(base);
  a.dense_units = &w.scalars.in(base)->dense_units;
  a.f16inv = w.f16inv.in(base);
  a.cand_count = w.cand_b.count.in(base); a.cand_j = w.cand_b.idx.in(base); a.cand_x = w.cand_b.x.in(base);
  a.ccand_count = w.ccand_b.count.in(base); a.ccand_i = w.ccand_b.idx.in(base); a.ccand_x = w.ccand_b.x.in(base);
  a.flags = &w.scalars.in(base)->flags;
  a.diag = w.cand.x.in(base);
  a.L = w.L; a.S = w.S; a.Lp = w.Lp; a.Sp = w.Sp; a.panels = w.panels; a.units = w.Sp / 32;
  // the row partials are [N][w.splits][Lp] (k_select / k_reduce_sums fold w.splits of them): the same number of splits
  // as the tile-based kernel it replaces, in units of 32 columns
  a.splits = w.splits;
  a.units_per_split = 2 * ((w.tiles + w.splits - 1) / w.splits);
  a.slots = w.slots;
  {
    const int blocks_all = w.N * a.splits * w.panels;
    const float share = fmaxf(1.f, (float)blocks_all / 8.f);
    int pgr = (int)lroundf(sqrtf(share * (float)(a.units_per_split * 32) / (float)kPanelRows));
    a.pgroup = pgr < 1 ? 1 : (pgr > w.panels ? w.panels : pgr);
    if (a.splits == 1) a.pgroup = w.panels;
  }
  a.k = k2_of(inv_ct);
  a.lt = log2f(thr) - (rescreen ? 2e-4f : 0.f);      // the re-screening compares rounded log-softmax values: small guard
  const int blocks = w.N * a.splits * w.panels;
  return with_padded_channels(w.C, [&](auto cc) {
    constexpr int CC = cc.value;
    hipError_t e = hipSuccess;
    constexpr int lds = kDenseRing * 2 * (CC / 16) * 1024;
    static unsigned long long lds_set = 0, lds_set_c = 0, lds_set_r = 0;
    if (conf) {      // the samples the screening kernel served, then (exits at once without any) the dense kernel's
      static unsigned long long lds_set_l = 0;
      e = ensure_dynamic_lds(&k_dense<CC, kDenseConfLite>, lds, &lds_set_l);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((k_dense<CC, kDenseConfLite>), dim3(blocks), dim3(512), lds, st, a);
      e = ensure_dynamic_lds(&k_dense<CC, kDenseConf>, lds, &lds_set_c);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((k_dense<CC, kDenseConf>), dim3(blocks), dim3(512), lds, st, a);
    } else if (rescreen) {
      e = ensure_dynamic_lds(&k_dense<CC, kDenseRescreen>, lds, &lds_set_r);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((k_dense<CC, kDenseRescreen>), dim3(blocks), dim3(512), lds, st, a);
    } else {
      e = ensure_dynamic_lds(&k_dense<CC, kDenseSums>, lds, &lds_set);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((k_dense<CC, kDenseSums>), dim3(blocks), dim3(512), lds, st, a);
    }
    return hipGetLastError();
  });
}

// Dense data['conf_matrix'] (k_dense<C, CONF>: hi/lo-split float16 products, 22 significant bits - 2e-4 in a conf near 1 at
// |sim| ~ 200): every entry that matters takes the exact float32 route.  For the samples the screening kernel served,
// the rows' lists hold every entry with a row term above 2^-32 (all entries with conf > 2.4e-10 are among them) together
// with its exact dot product; their conf is rewritten from that number and the same log-softmax offsets.
// One thread per (row, slot).
__global__ __launch_bounds__(256) void k_conf_patch(const int* __restrict__ rcount, const int* __restrict__ rlist_j,
                                                    const float* __restrict__ rlist_x, const int* __restrict__ rcount_d,
                                                    const int* __restrict__ rlist_j_d, const float* __restrict__ rlist_x_d,
                                                    const float* __restrict__ nm_r,
                                                    const float* __restrict__ sum_r, const float* __restrict__ nm_c,
                                                    const float* __restrict__ sum_c, const int* __restrict__ dense_cnt, int N,
                                                    int L, int S, int Lp, int Sp, int slots, float k2, float* __restrict__ conf) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long grow = gid / slots;
  const int slot = (int)(gid - grow * slots);
  if (grow >= (long)N * Lp) return;
  const int b = (int)(grow / Lp), i = (int)(grow - (long)b * Lp);
  if (i >= L) return;
  const bool dense = dense_cnt[b] > 0;         // the dense kernel's lists, made exact by k_exact_lists
  if (slot >= min((dense ? rcount_d : rcount)[grow], slots)) return;
  const float x = (dense ? rlist_x_d : rlist_x)[grow * slots + slot];
  if (!(x > -INFINITY)) return;                    // a reserved but empty place
  const int j = (dense ? rlist_j_d : rlist_j)[grow * slots + slot];
  const long gcol = (long)b * Sp + j;
  conf[((long)b * L + i) * S + j] = (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_r[grow])) / sum_r[grow]) *
                                    (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_c[gcol])) / sum_c[gcol]);
}

// The samples the DENSE kernel served (flat similarity somewhere in the sample), when every entry is read (conf_matrix,
// softmax statistics): the hi/lo-split float16 products carry 22 bits, 2^-22 |sim| ~ 4e-5 at similarities of ~170 - and
// a peaked row of such a sample (conf ~ 1: the entry IS its row's and its column's denominator) is only right when the
// entry and the two denominators hold the SAME x.  So the lists of such a sample - with a conf_matrix request they are
// formed with min(thr, 0.1): every entry whose two softmax factors both exceed 0.1, i.e. every entry with conf > 0.1 -
// are resolved exactly, entries and denominators together:
//   k_exact_lists : 16 lanes per row list and per column list, its entries in turn: the exact float32 dot product of the caller's
//                   descriptors (fm_exact_device.h: the screening's, and k_conf_at's) replaces the list's x; the term's change
//                   exp2(k x + nm) - exp2(k x22 + nm) goes to the screening kernel's list region of the sample (idle)
//   k_fix_sums    : one thread per row / column: adds the changes in index order (same bits every run) to the
//                   denominator, refreshes the log-softmax offset
// The assignment then reads exact x and matching denominators (mconf = the conf_matrix entry), k_conf_patch rewrites the
// listed entries of the dense matrix.  What stays 22-bit has conf <= 0.1: 2 * 2^-22 |sim| conf <= 8e-6 at |sim| ~ 170.
__global__ __launch_bounds__(256) void k_exact_lists(const void* __restrict__ f0, const void* __restrict__ f1, int in_dtype, int c_in,
                                                     const int* __restrict__ rcount, const int* __restrict__ rkey, float* __restrict__ rx,
                                                     float* __restrict__ rdelta, const int* __restrict__ ccount,
                                                     const int* __restrict__ ckey, float* __restrict__ cx, float* __restrict__ cdelta,
                                                     const float* __restrict__ nm_r, const float* __restrict__ nm_c,
                                                     const int* __restrict__ dense_cnt, int N, int L, int S, int Lp, int Sp,
                                                     int slots, float k2) {
  const int side = blockIdx.z;
  const int len = side ? Sp : Lp;
  const long gl = (long)blockIdx.x * 16 + (threadIdx.x >> 4);           // one 16-lane group per list, its slots in turn
  const int l16 = threadIdx.x & 15;
  if (gl >= (long)N * len) return;
  const int b = (int)(gl / len), own = (int)(gl - (long)b * len);
  if (own >= (side ? S : L) || dense_cnt[b] == 0) return;              // (uniform over the group)
  const int n = min((side ? ccount : rcount)[gl], slots);
  const DescRows d = {f0, f1, c_in, in_dtype, L, S};
  for (int slot = 0; slot < n; ++slot) {
    const long at = gl * slots + slot;
    const int other = (side ? ckey : rkey)[at];
    const long ro = desc_row0(d, b, side ? other : own), co = desc_row1(d, b, side ? own : other);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 va, vb;
      exact_dot16_load1(d, ro, co, l16, q, va, vb);
      s = exact_dot16_link(s, va, vb);
    }
    const float x = row_sum16(s);
    if (l16 == 0) {
      float* xs = side ? cx : rx;
      const float nm = (side ? nm_c : nm_r)[gl];
      (side ? cdelta : rdelta)[at] = __builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm)) - __builtin_amdgcn_exp2f(__builtin_fmaf(xs[at], k2, nm));
      xs[at] = x;
    }
  }
}

__global__ __launch_bounds__(256) void k_fix_sums(const int* __restrict__ rcount, const int* __restrict__ rkey,
                                                  const float* __restrict__ rdelta, const int* __restrict__ ccount,
                                                  const int* __restrict__ ckey, const float* __restrict__ cdelta,
                                                  const float* __restrict__ nm_r, const float* __restrict__ nm_c,
                                                  float* __restrict__ sum_r, float* __restrict__ sum_c, float* __restrict__ nm2_r,
                                                  float* __restrict__ nm2_c, const int* __restrict__ dense_cnt, int Lp, int Sp,
                                                  int slots) {
  const int side = blockIdx.z, b = blockIdx.y;
  const int len = side ? Sp : Lp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= len || dense_cnt[b] == 0) return;
  const long gl = (long)b * len + idx;
  const int n = min((side ? ccount : rcount)[gl], slots);
  if (n == 0) return;
  const int* key = (side ? ckey : rkey) + gl * slots;
  const float* d = (side ? cdelta : rdelta) + gl * slots;
  float acc = 0.f;
  int last = -1;
  for (int t = 0; t < n; ++t) {           // in index order (the lists are filled in the order the waves arrive)
    int best = 0x7fffffff, at = 0;
    for (int q = 0; q < n; ++q) { const int kq = key[q]; if (kq > last && kq < best) { best = kq; at = q; } }
    acc += d[at];
    last = best;
  }
  float* sum = side ? sum_c : sum_r;
  const float v = sum[gl] + acc;
  sum[gl] = v;
  (side ? nm2_c : nm2_r)[gl] = (side ? nm_c : nm_r)[gl] - __log2f(v);
}

hipError_t launch_exact_lists(const CoarseWs& w, char* base, float inv_ct, const void* feat0, const void* feat1, int in_dtype,
                              int c_in, hipStream_t st) {
  // the dense kernel's lists; every term's change goes to the same slot of the sparse kernel's x arrays (idle for the
  // samples the dense kernel redid), where k_fix_sums reads it
  const CandList &rows = w.cand_b, &cols = w.ccand_b;
  float *rdelta = w.cand.x.in(base), *cdelta = w.ccand.x.in(base);
  const long groups = (long)w.N * max(w.Lp, w.Sp);
  hipLaunchKernelGGL(k_exact_lists, dim3((unsigned)((groups + 15) / 16), 1, 2), dim3(256), 0, st, feat0, feat1, in_dtype, c_in,
                     rows.count.in(base), rows.idx.in(base), rows.x.in(base), rdelta, cols.count.in(base), cols.idx.in(base),
                     cols.x.in(base), cdelta, w.nmr.in(base), w.nmc.in(base), w.dense_cnt.in(base), w.N, w.L, w.S, w.Lp, w.Sp,
                     w.slots, k2_of(inv_ct));
  hipLaunchKernelGGL(k_fix_sums, dim3((max(w.Lp, w.Sp) + 255) / 256, w.N, 2), dim3(256), 0, st, rows.count.in(base),
                     rows.idx.in(base), rdelta, cols.count.in(base), cols.idx.in(base), cdelta, w.nmr.in(base), w.nmc.in(base),
                     w.rsum.in(base), w.csum.in(base), w.nmr2.in(base), w.nmc2.in(base), w.dense_cnt.in(base), w.Lp, w.Sp, w.slots);
  return hipGetLastError();
}

hipError_t launch_conf_patch(const CoarseWs& w, char* base, float inv_ct, float* conf, hipStream_t st) {
  const long total = (long)w.N * w.Lp * w.slots;
  hipLaunchKernelGGL(k_conf_patch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w.cand.count.in(base),
                     w.cand.idx.in(base), w.cand.x.in(base), w.cand_b.count.in(base), w.cand_b.idx.in(base), w.cand_b.x.in(base),
                     w.nmr.in(base), w.rsum.in(base), w.nmc.in(base), w.csum.in(base), w.dense_cnt.in(base), w.N, w.L, w.S, w.Lp,
                     w.Sp, w.slots, k2_of(inv_ct), conf);
  return hipGetLastError();
}

}  // namespace fm
