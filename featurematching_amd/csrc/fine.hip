// Fine stage: window crop (network/module/fine_preprocess.py:43-50) and the dual-direction
// local-window correlation + soft-argmax (network/utils/fine_matching_new.py:50-79).
#include "fm_device.h"
#include "fm_fine_device.h"
#include "fm_maps_device.h"

namespace fm {

// ----------------------------------------------------------------------------------------
// Window crop for NCHW maps with Cf = 64 (W compile-time): ONE WAVE PER WINDOW, four windows per
// workgroup, no workgroup barrier.
// The reference unfolds EVERY coarse cell's window (60 MB per image at 640x480) and then selects M
// of them; here only the M selected windows are read, straight from the NCHW map.  Lanes run along
// (channel, window row, x) with x fastest, so one wave-load touches ~64/W short runs in 2-3 channel
// planes.  (Lane = channel would put the 64 lanes of a load one plane stride apart - 307200 B at
// 240x320 - which lands on a handful of L2/HBM channels; measured 2x slower.)  All loads of the window
// are issued before the first use (25 / 49 in flight per lane).  The [c][r] -> [r][c] transpose goes
// through a wave-private LDS tile (pitch 68 floats: 16-byte aligned rows) and the window leaves as one
// contiguous record in 16-byte stores.  Window origin = stride*cell - pad with the reference's literal
// pad = 2, zero outside the map.
// (One workgroup per window, 3776 four-wave workgroups at 640x480, was bound by workgroup launch
// rate: its time followed the number of workgroups, not the bytes.)
// ----------------------------------------------------------------------------------------
// In-place context merge of one window tile in LDS (fine_preprocess.py:56-59, the window half of
// merge_feat): tile[r][n] <- sum_k W_w[n][k] * tile[r][k] + ctx[n], r = window position, k/n = channels.
// (The context half W_c . down_proj(feat_c) + bias does not depend on the position: it arrives as ctx, one
// row of a per-cell table the caller computes with a plain library GEMM.)  f32-equivalent product on the f16
// matrix cores, as in the coarse stage: window values and weights are split x = hi + lo (f16 each) and
// hi*hi + lo*hi + hi*lo is accumulated in f32 (~2^-22 relative).  wpack = the weights pre-split into MFMA B
// fragments by fm_merge_pack_weights: [n-tile 2][k-step 4][hi|lo][lane 64] x 8 halfs.
// Both operands carry exact power-of-two scales, undone on the accumulator: the matrix cores flush float16 SUBNORMAL
// inputs, and the lo half of anything below 2^-3 - every weight of a 128-wide Linear layer - would be one (see
// fine_tf.hip).  Weights x kMergeWgtScale (fixed: |w| < 16, merge_feat is a 128-wide Linear layer).  Window values x a
// scale that FOLLOWS THE WINDOW (round 4): the power of two that brings the window's largest magnitude into
// [2^13, 2^14) - a fixed 2^8 turned every window value beyond 255.9 into inf without a word (un-normalised backbone
// features; found by a matcher test on maps of magnitude 3e5).
constexpr float kMergeWgtScale = 4096.f;
// exact power of two s with amax * s in [2^13, 2^14), clamped to [2^-100, 2^40] (a window of zeros / denormals: the
// context term alone decides, and c * s * 2^12 must stay inside float32)
__device__ __forceinline__ float merge_act_scale(float amax) {
  const unsigned bits = __float_as_uint(amax);
  const int e = (int)((bits >> 23) & 0xffu);           // amax in [2^(e-127), 2^(e-126))
  int k = 140 - e;                                     // 13 - (e - 127)
  if (e == 255) k = 0;                                 // (Inf / NaN window: the result is NaN either way)
  k = k > 40 ? 40 : (k < -100 ? -100 : k);
  return __uint_as_float((unsigned)(127 + k) << 23);
}
template <int W>
__device__ __forceinline__ void wave_merge_tile(float* tile, int lane, const half8* __restrict__ wpack,
                                                const float* __restrict__ ctx_row) {
  constexpr int WW = W * W, PITCH = 68, MT = (WW + 31) / 32;
  const int r = lane & 31, h = lane >> 5;
  const float c0 = ctx_row[r], c1 = ctx_row[32 + r];
  half8 bhi[2][4], blo[2][4];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bhi[nt][ks] = wpack[((nt * 4 + ks) * 2 + 0) * 64 + lane];
      blo[nt][ks] = wpack[((nt * 4 + ks) * 2 + 1) * 64 + lane];
    }
  // the window's largest magnitude (every lane reads the values it will split below: the 64 lanes cover the tile)
  float amax = 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = min(32 * mt + r, WW - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 p = *reinterpret_cast<const float4*>(tile + row * PITCH + ks * 16 + 8 * h);
      const float4 q = *reinterpret_cast<const float4*>(tile + row * PITCH + ks * 16 + 8 * h + 4);
      amax = fmaxf(amax, fmaxf(fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fmaxf(fabsf(p.z), fabsf(p.w))),
                               fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w)))));
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
  const float act_scale = merge_act_scale(amax);
  // A fragments of all window rows first (the tile is overwritten below): lane (r, h) holds row r,
  // channels 16*ks + 8*h .. +7; rows beyond the window re-read its last row (their outputs are dropped)
  half8 ahi[MT][4], alo[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = min(32 * mt + r, WW - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 p = *reinterpret_cast<const float4*>(tile + row * PITCH + ks * 16 + 8 * h);
      const float4 q = *reinterpret_cast<const float4*>(tile + row * PITCH + ks * 16 + 8 * h + 4);
      const float x[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) split_f16(x[e] * act_scale, ahi[mt][ks], alo[mt][ks], e);
    }
  }
  __builtin_amdgcn_wave_barrier();
  const float inv_scale = (1.0f / act_scale) * (1.0f / kMergeWgtScale);      // (both exact powers of two)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[g] = (nt ? c1 : c0) * (act_scale * kMergeWgtScale);   // column n = 32*nt + r
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {      // mma3, written out: called, k_gather_merge_nhwc64<5>'s registers come out renamed
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[mt][ks], bhi[nt][ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[mt][ks], bhi[nt][ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[mt][ks], blo[nt][ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = 32 * mt + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (row < WW) tile[row * PITCH + 32 * nt + r] = acc[g] * inv_scale;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// One W x W window of a 64-channel NCHW map into a wave-private LDS tile [position][channel] (pitch 68 floats).
// lane -> (channel within the instruction, window position) is the same for every load: W = 5 puts two channels x 32
// position slots (25 used) in one wave-load, W = 7 one channel x 64 slots (49 used).  Only the channel advances from
// load to load, by a SCALAR offset, so the address math is done once.  Buffer loads through a descriptor of this
// sample's map (src is wave-uniform): positions outside the map (the zero padding of the unfold) get an out-of-range
// offset, which the hardware range check answers with 0 - no branch, no 64-bit address per load.
template <int W>
__device__ __forceinline__ void wave_load_window64(const float* src, int Hf, int Wf, int oy, int ox, float* tile, int lane) {
  constexpr int CF = 64, WW = W * W, PITCH = CF + 4;
  constexpr int SLOTS = W == 5 ? 32 : 64, CPI = 64 / SLOTS, NLOAD = CF / CPI;
  static_assert(W == 5 || W == 7, "position decode below is for W in {5,7}");
  const int rem = lane & (SLOTS - 1), hi = lane / SLOTS;
  const int wy = W == 5 ? (rem * 13) >> 6 : (rem * 37) >> 8;       // rem / W for rem < W*W
  const int wx = rem - wy * W;
  const int y = oy + wy, x = ox + wx;
  const bool ok = rem < WW && y >= 0 && y < Hf && x >= 0 && x < Wf;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, CF * Hf * Wf * 4, 0x00020000);
  const unsigned voff = ok ? (unsigned)((hi * Hf + y) * Wf + x) * 4u : 0x80000000u;
  const int step = Hf * Wf * 4 * CPI;                               // bytes from one load to the next
  float v[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) {
#ifndef FM_ABL_G_NOLOAD      // timing-only ablations (wrong results): never defined in the shipped build
    v[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, it * step, 0));
#else
    v[it] = 0.f;
#endif
  }
  float* slot = tile + rem * PITCH + hi;
#pragma unroll
  for (int it = 0; it < NLOAD; ++it)
    if (rem < WW) slot[it * CPI] = v[it];
  __builtin_amdgcn_wave_barrier();       // same-wave LDS accesses are processed in order: no s_barrier needed
}

// the tile [position][channel] leaves as one contiguous window record [WW][64] in 16-byte stores
template <int W>
__device__ __forceinline__ void wave_store_tile64(const float* tile, float* __restrict__ dst, int lane) {
  constexpr int CF = 64, WW = W * W, TOTAL = CF * WW, PITCH = CF + 4;
  float4* dst4 = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int it = 0; it < (TOTAL / 4 + 63) / 64; ++it) {
    const int idx = it * 64 + lane;          // float4 index: position idx / 16, channels 4*(idx % 16) ..
    if (idx < TOTAL / 4) {
      const float4 q = *reinterpret_cast<const float4*>(tile + (idx >> 4) * PITCH + (idx & 15) * 4);
#ifdef FM_ABL_G_NOSTORE
      if (q.x == 1.2345e-30f) dst4[idx] = q;
#else
      dst4[idx] = q;
#endif
    }
  }
  __builtin_amdgcn_wave_barrier();       // the tile may be refilled by this wave right away
}

template <int W, bool MERGE = false>
__device__ __forceinline__ void wave_copy_window64(const float* src, int Hf, int Wf, int oy, int ox,
                                                   float* __restrict__ dst, float* tile, int lane,
                                                   const half8* __restrict__ wpack = nullptr,
                                                   const float* __restrict__ ctx_row = nullptr) {
  wave_load_window64<W>(src, Hf, Wf, oy, ox, tile, lane);
  if (MERGE) wave_merge_tile<W>(tile, lane, wpack, ctx_row);
  wave_store_tile64<W>(tile, dst, lane);
}

constexpr int kGatherTileFloats(int W) { return W * W * 68; }

// List order: the M = min(*d_count, m_max) live windows of the match list (not the m_max launched ones) are spread
// contiguously over the XCDs - 8 ranges of ceil(M / 8) windows, four windows (waves) per workgroup.  m = the window of
// wave wv of this workgroup; false = it has none.
__device__ __forceinline__ bool list_window(const int32_t* d_count, int m_max, int wv, int& m) {
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  const int per = (M + 7) >> 3;
  const int slot = (int)(blockIdx.x >> 3) * 4 + wv;
  m = (blockIdx.x & 7) * per + slot;
  return slot < per && m < M;
}

// list order: window m of the match list (any ids; the generic entry point)
template <int W, bool MERGE>
__global__ __launch_bounds__(256) void k_gather_nchw64(const float* __restrict__ feat, int Hf, int Wf, int stride,
                                                       int pad, int w_c, const int64_t* __restrict__ b_ids,
                                                       const int64_t* __restrict__ ids,
                                                       const int32_t* __restrict__ d_count, int m_max,
                                                       float* __restrict__ out, const half8* __restrict__ wpack,
                                                       const float* __restrict__ ctx, int ctx_cells) {
  constexpr int CF = 64, TOTAL = CF * W * W;
  __shared__ __attribute__((aligned(16))) float tile[4 * kGatherTileFloats(W)];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int m;
  if (!list_window(d_count, m_max, wv, m)) return;
  const int b = __builtin_amdgcn_readfirstlane((int)b_ids[m]);       // wave-uniform values into scalars
  const int id = __builtin_amdgcn_readfirstlane((int)ids[m]);
  const int cy = id / w_c;
  wave_copy_window64<W, MERGE>(feat + (long)b * CF * Hf * Wf, Hf, Wf, cy * stride - pad, (id - cy * w_c) * stride - pad,
                               out + (long)m * TOTAL, tile + wv * kGatherTileFloats(W), lane, wpack,
                               MERGE ? ctx + ((long)b * ctx_cells + id) * CF : nullptr);
}

// ----------------------------------------------------------------------------------------
// k_gather_cellorder64<W>: the same per-window copy, but the waves run over the CELLS of this image
// in raster order (cell -> match map from the coarse stage, 0 = unmatched) and each XCD takes a
// contiguous band of cells.  For image 1 the match list is sorted by the image-0 cell, so in list
// order the windows of one XCD are scattered over the whole map (20 MB at 640x480 against a 4 MB L2:
// every 20-byte run misses to the fabric); in cell order one XCD touches only its band (2.5 MB).
// Matches that lost their cell to an exactly tied match (listed by k_emit) are copied by the first
// waves of the grid, one each; if that list overflowed (> kTieCap) every wave scans its slice of the
// match list instead.
// ----------------------------------------------------------------------------------------
// One launch can serve BOTH images of the pairs (blockIdx.y = image): the two crops are independent and each
// is bound by one round of memory latency at 640x480, so a second launch only adds its ramp and tail.
struct CellImage {
  const float* feat; int Hf, Wf, w_c, cells, total_cells;
  const int32_t* cell_to_match; int cell_pitch; const int32_t* ties;
  const int64_t* ids; float* out; const float* ctx;
};
struct CellArgs {
  CellImage im[2];
  int stride, pad, m_max;
  const int64_t* b_ids; const int32_t* d_count; const half8* wpack;
};

template <int W, bool MERGE>
__global__ __launch_bounds__(256) void k_gather_cellorder64(CellArgs a) {
  constexpr int CF = 64, TOTAL = CF * W * W;
  __shared__ __attribute__((aligned(16))) float tile_all[4 * kGatherTileFloats(W)];
  const CellImage& I = a.im[blockIdx.y];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* tile = tile_all + wv * kGatherTileFloats(W);
  const int M = a.d_count ? min(a.d_count[0], a.m_max) : a.m_max;
  const int nties = I.ties[0];
  const int lid = xcd_contiguous(blockIdx.x, gridDim.x) * 4 + wv;      // grid.x is a multiple of 8
  // job = (match, sample, cell) this wave copies next; first its own cell, then tie losers (rare)
  int jm = -1, jb = 0, jcell = 0;
  if (lid < I.total_cells) {
    const int b = lid / I.cells, cell = lid - b * I.cells;
    const int m = I.cell_to_match[(long)b * I.cell_pitch + cell] - 1;
    if (m >= 0 && m < M) { jm = m; jb = b; jcell = cell; }
  }
  const int gwave = blockIdx.x * 4 + wv, nwaves = gridDim.x * 4;
  const int mode = nties == 0 ? 0 : (nties <= kTieCap ? 1 : 2);          // 2: list overflowed, scan the matches
  int q = gwave;
  const int chunk = (M + nwaves - 1) / nwaves;
  int scan = gwave * chunk;
  const int scan_end = min(M, scan + chunk);
  for (;;) {
    if (jm >= 0) {
      jm = __builtin_amdgcn_readfirstlane(jm); jb = __builtin_amdgcn_readfirstlane(jb);
      jcell = __builtin_amdgcn_readfirstlane(jcell);
      const int cy = jcell / I.w_c;
      wave_copy_window64<W, MERGE>(I.feat + (long)jb * CF * I.Hf * I.Wf, I.Hf, I.Wf, cy * a.stride - a.pad,
                                   (jcell - cy * I.w_c) * a.stride - a.pad, I.out + (long)jm * TOTAL, tile, lane,
                                   a.wpack, MERGE ? I.ctx + ((long)jb * I.cells + jcell) * CF : nullptr);
    }
    jm = -1;
    if (mode == 0) break;                                                // the common case: no exact ties
    if (mode == 1) {
      if (q >= nties) break;
      const int m = I.ties[1 + q];
      q += nwaves;
      if (m >= 0 && m < M) { jm = m; jb = (int)a.b_ids[m]; jcell = (int)I.ids[m]; }
    } else {
      if (scan >= scan_end) break;
      const int m = scan++;
      const int mb = (int)a.b_ids[m], id = (int)I.ids[m];
      if (I.cell_to_match[(long)mb * I.cell_pitch + id] != m + 1) { jm = m; jb = mb; jcell = id; }
    }
  }
}

// element of a float32 / float16 / bfloat16 map as float32 (exact)
template <int DT> struct MapElem { using type = float; };
template <> struct MapElem<FM_F16> { using type = unsigned short; };
template <> struct MapElem<FM_BF16> { using type = unsigned short; };
template <int DT>
__device__ __forceinline__ float map_value(const typename MapElem<DT>::type* p, long i) {
  if constexpr (DT == FM_F32) return p[i];
  else return half_bits_to_float(p[i], DT);
}

// generic fallback (any Cf / W, any element type): one workgroup per window, transposed through LDS
template <int DT>
__global__ __launch_bounds__(256) void k_gather_nchw(const typename MapElem<DT>::type* __restrict__ feat, int Cf, int Hf, int Wf, int W,
                                                     int stride, int pad, int w_c, const int64_t* __restrict__ b_ids,
                                                     const int64_t* __restrict__ ids, const int32_t* __restrict__ d_count,
                                                     int m_max, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [WW][Cf+1]
  const int m = blockIdx.x;
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  if (m >= M) return;
  const int WW = W * W;
  const int b = (int)b_ids[m];
  const int id = (int)ids[m];
  const int oy = (id / w_c) * stride - pad;
  const int ox = (id % w_c) * stride - pad;
  const typename MapElem<DT>::type* src = feat + (long)b * Cf * Hf * Wf;
  const int total = Cf * WW;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int c = idx / WW;
    const int rem = idx - c * WW;
    const int wy = rem / W, wx = rem - wy * W;
    const int y = oy + wy, x = ox + wx;
    float v = 0.f;
    if (y >= 0 && y < Hf && x >= 0 && x < Wf) v = map_value<DT>(src, ((long)c * Hf + y) * Wf + x);
    tile[rem * (Cf + 1) + c] = v;
  }
  __syncthreads();
  float* dst = out + (long)m * total;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int rpos = idx / Cf;
    const int c = idx - rpos * Cf;
    dst[idx] = tile[rpos * (Cf + 1) + c];
  }
}

// NHWC storage: every window row is W*Cf contiguous elements - a straight copy, four channels per thread and step.
template <int DT>
__global__ __launch_bounds__(256) void k_gather_nhwc(const typename MapElem<DT>::type* __restrict__ feat, int Cf, int Hf, int Wf, int W,
                                                     int stride, int pad, int w_c, const int64_t* __restrict__ b_ids,
                                                     const int64_t* __restrict__ ids, const int32_t* __restrict__ d_count,
                                                     int m_max, float* __restrict__ out) {
  const int m = blockIdx.x;
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  if (m >= M) return;
  const int WW = W * W;
  const int b = (int)b_ids[m];
  const int id = (int)ids[m];
  const int oy = (id / w_c) * stride - pad;
  const int ox = (id % w_c) * stride - pad;
  const int c4 = Cf / 4;
  const typename MapElem<DT>::type* src = feat + (long)b * Hf * Wf * Cf;
  float4* dst = reinterpret_cast<float4*>(out + (long)m * WW * Cf);
  for (int idx = threadIdx.x; idx < WW * c4; idx += 256) {
    const int rpos = idx / c4;
    const int c = idx - rpos * c4;
    const int wy = rpos / W, wx = rpos - wy * W;
    const int y = oy + wy, x = ox + wx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < Hf && x >= 0 && x < Wf) {
      const long e = ((long)y * Wf + x) * c4 + c;          // in units of four elements
      if constexpr (DT == FM_F32) v = reinterpret_cast<const float4*>(src)[e];
      else v = half4_to_float4(reinterpret_cast<const uint2*>(src)[e], DT);
    }
    dst[idx] = v;
  }
}

// ----------------------------------------------------------------------------------------
// k_fine: one wave per match, lane = channel (Cf = 64).
//   q0[c]   = b0 + sum_r w0[r] F0[r][c]            (Linear over the POSITION axis, :50,53)
//   sim0[r] = sum_c q0[c] F1[r][c]                 (:56)   -> refines keypoint 0
//   q1 / sim1 symmetrically (:51,54,57)            -> refines keypoint 1
//   heat = softmax(sim / sqrt(C)); coords = E[grid]; std = sum sqrt(clamp(var, 1e-10))  (:58-73)
//   out  = mkpts_c + (coords * (W//2) * scale + W//2), std                              (:75-79)
// The WW cross-lane sums of sim are done with one butterfly "transpose-reduce" built from DPP and
// permlane swaps (no LDS): after the exchange steps every lane holds one sim[pos], so the softmax
// runs with lane = window position.
// ----------------------------------------------------------------------------------------

// Soft-argmax of BOTH directions at once from the heat-map sums of heat_sums2 (fm_fine_device.h): lane 0 writes
// out = mkpts_c + (coords * (W//2) * scale + W//2), std.
template <int W>
__device__ __forceinline__ void soft_argmax2(float sim0, float sim1, int pos, bool on, int lane, float inv_sqrt_c,
                                             float scale_f, float k0x, float k0y, float k1x, float k1y, float* out0,
                                             float* out1) {
  const Heat2 e = heat_exp2(sim0, sim1, on, inv_sqrt_c);
  const float t = heat_sums2<W>(e.e0, e.e1, pos);
  auto sum_k = [&](int k) { return heat_sum(t, k); };
  if (lane == 0) {
    float* const outs[2] = {out0, out1};
    const float kx[2] = {k0x, k1x}, ky[2] = {k0y, k1y};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const float inv = 1.0f / sum_k(5 * d);
      const float cx = sum_k(5 * d + 1) * inv, cy = sum_k(5 * d + 2) * inv;
      const float vx = sum_k(5 * d + 3) * inv - cx * cx, vy = sum_k(5 * d + 4) * inv - cy * cy;
      outs[d][0] = kx[d] + (cx * (float)(W / 2) * scale_f + (float)(W / 2));
      outs[d][1] = ky[d] + (cy * (float)(W / 2) * scale_f + (float)(W / 2));
      outs[d][2] = sqrtf(fmaxf(vx, 1e-10f)) + sqrtf(fmaxf(vy, 1e-10f));
    }
  }
}

// the arithmetic of one match once both windows sit in registers (lane = channel, f[r] = window position r)
template <int W>
__device__ __forceinline__ void fine_core(const float (&f0)[W * W], const float (&f1)[W * W], int lane,
                                          const float* __restrict__ mix0, const float* __restrict__ mix1, float k0x,
                                          float k0y, float k1x, float k1y, float scale_f, float* __restrict__ out0,
                                          float* __restrict__ out1) {
  constexpr int WW = W * W;
  constexpr int CF = 64;
  const Mix2 q = fine_mix<W>(f0, f1, mix0, mix1);
  const float q0 = q.q0, q1 = q.q1;

#ifdef FM_ABL_F_NOCOMPUTE     // timing-only: loads and one store, no correlation / soft-argmax
  if (q0 + q1 == 1.2345e-30f) out0[0] = q0;
  return;
#endif
  const float inv_sqrt_c = 1.0f / sqrtf((float)CF);
  // (fine_sims in fm_fine_device.h is this arithmetic for the backward; kept inline here: moved into a helper it
  // changes the register allocation of k_fine and k_fine_maps)
  constexpr int NP = WW > 32 ? 64 : 32;      // butterfly width
  float p[NP];
#pragma unroll
  for (int r = 0; r < NP; ++r) p[r] = r < WW ? q0 * f1[r] : 0.f;
  const float sim0 = transpose_reduce<NP>(p, lane);
#pragma unroll
  for (int r = 0; r < NP; ++r) p[r] = r < WW ? q1 * f0[r] : 0.f;
  const float sim1 = transpose_reduce<NP>(p, lane);

  const int pos = tr_index<NP>(lane);
  const bool on = pos < WW && (NP == 64 || !(lane & 1));      // NP = 32: the even lane of the pair that holds a sum
  soft_argmax2<W>(sim0, sim1, pos, on, lane, inv_sqrt_c, scale_f, k0x, k0y, k1x, k1y, out0, out1);
}

template <int W>
__global__ __launch_bounds__(256) void k_fine(const float* __restrict__ win0, const float* __restrict__ win1, int m_max,
                                              const int32_t* __restrict__ d_count, const float* __restrict__ mix0,
                                              const float* __restrict__ mix1, const float* __restrict__ kc0,
                                              const float* __restrict__ kc1, float scale_f, float* __restrict__ out0,
                                              float* __restrict__ out1) {
  constexpr int WW = W * W;
  constexpr int CF = 64;
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  if (m >= M) return;
  const float* p0 = win0 + (long)m * WW * CF + lane;
  const float* p1 = win1 + (long)m * WW * CF + lane;
  float f0[WW], f1[WW];
  // read-once data: non-temporal loads keep the windows from displacing the fine maps in L2 (-2 us per pair)
#pragma unroll
  for (int r = 0; r < WW; ++r) { f0[r] = __builtin_nontemporal_load(p0 + r * CF); f1[r] = __builtin_nontemporal_load(p1 + r * CF); }
  fine_core<W>(f0, f1, lane, mix0, mix1, kc0[m * 2], kc0[m * 2 + 1], kc1[m * 2], kc1[m * 2 + 1], scale_f,
               out0 + (long)m * 3, out1 + (long)m * 3);
}

// ----------------------------------------------------------------------------------------
// Channels-last maps: storage [N, Hf, Wf, 64] of the logical [N, 64, Hf, Wf] tensor (layout 1).  A window row is
// W x 256 contiguous bytes there - ten cache lines at W = 5 instead of the 64 x 20-byte runs of the NCHW layout - so
//   * the crop is a plain copy in 16-byte chunks (the output window [WW][64] is the W row segments one after the
//     other), one wave per window, every load of the window in flight before the first store;
//   * the fine stage can take its windows straight from the maps: k_fine_maps reads position r of both windows as one
//     coalesced 256-byte wave load each (exactly the loads k_fine issues on a window tensor) and the window tensors
//     (48 MB written and read back per 640x480 pair) never exist.  Matches are visited in list order, an XCD a
//     contiguous range: image-0 windows then walk the map in raster order, image-1 windows land wherever their partner
//     is - at ten full lines per window that costs nothing extra.
//   * NCHW maps get there through k_nchw_to_nhwc64 (a tiled transpose through LDS, both sides coalesced) into a
//     caller-provided scratch buffer.
// ----------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_gather_nhwc64(const float* __restrict__ feat, int Hf, int Wf, int stride, int pad,
                                                       int w_c, const int64_t* __restrict__ b_ids,
                                                       const int64_t* __restrict__ ids, const int32_t* __restrict__ d_count,
                                                       int m_max, float* __restrict__ out) {
  constexpr int ROW16 = W * 16;              // 16-byte chunks per window row (64 channels x 4 bytes = 16 chunks per pixel)
  constexpr int TOTAL16 = W * ROW16;         // ... per window: 400 / 784
  constexpr int NIT = (TOTAL16 + 63) / 64;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int m;
  if (!list_window(d_count, m_max, wv, m)) return;
  const int b = __builtin_amdgcn_readfirstlane((int)b_ids[m]);
  const int id = __builtin_amdgcn_readfirstlane((int)ids[m]);
  const int cy = id / w_c;
  const int oy = cy * stride - pad, ox = (id - cy * w_c) * stride - pad;
  const float4* src = reinterpret_cast<const float4*>(feat + (long)b * Hf * Wf * 64);
  float4* dst = reinterpret_cast<float4*>(out + (long)m * W * W * 64);
  float4 v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int k = it * 64 + lane;
    const int wy = k / ROW16, within = k - wy * ROW16;
    const int y = oy + wy, x = ox + (within >> 4);
    const bool ok = k < TOTAL16 && y >= 0 && y < Hf && x >= 0 && x < Wf;
    // (clamped address + select: no load behind a branch)
    const float4 t = src[ok ? ((long)y * Wf + x) * 16 + (within & 15) : 0];
    v[it] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int k = it * 64 + lane;
    if (k < TOTAL16) dst[k] = v[it];
  }
}

// k_gather_merge_nhwc64<W, DT>: the crop fused with the context merge (wave_merge_tile) for channels-last maps of
// float32 / float16 / bfloat16 elements.  One wave per window, four per workgroup, no workgroup barrier (the shape of
// k_gather_nchw64<W, true>); list order, an XCD a contiguous range of the live windows (a window is W rows of W x 256
// contiguous bytes, see above: no cell-ordered walk needed); blockIdx.y = image, as in k_gather_cellorder64.  The loader
// is k_gather_nhwc64's - one chunk of four channels per lane and step (16 bytes, or 8 bytes of a half-precision map,
// widened exactly), every load of the window in flight before the first use, clamped address + select for the zero
// padding - and fills the wave-private tile [position][channel] (chunk k belongs to position k / 16, channels
// 4 * (k % 16) ..).  From there on the window takes the NCHW kernel's path instruction for instruction, so the
// outputs are bit-identical to k_gather_nchw64<W, true> / k_gather_cellorder64<W, true> on the same logical tensor.
struct MergeNhwcImage {
  const void* feat; int Hf, Wf, w_c, cells;
  const int64_t* ids; float* out; const float* ctx;
};
struct MergeNhwcArgs {
  MergeNhwcImage im[2];
  int stride, pad, m_max;
  const int64_t* b_ids; const int32_t* d_count; const half8* wpack;
};

template <int W, int DT>
__global__ __launch_bounds__(256) void k_gather_merge_nhwc64(MergeNhwcArgs a) {
  constexpr int WW = W * W, PITCH = 68;
  constexpr int TOTAL16 = WW * 16;           // chunks of four channels per window: 400 / 784
  constexpr int NIT = (TOTAL16 + 63) / 64;
  using Chunk = typename std::conditional<DT == FM_F32, float4, uint2>::type;
  __shared__ __attribute__((aligned(16))) float tile_all[4 * kGatherTileFloats(W)];
  const MergeNhwcImage& I = a.im[blockIdx.y];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* tile = tile_all + wv * kGatherTileFloats(W);
  // list_window, written out: a.m_max is then loaded only on the side of the branch that needs it
  const int M = a.d_count ? min(a.d_count[0], a.m_max) : a.m_max;
  const int per = (M + 7) >> 3;
  const int slot = (int)(blockIdx.x >> 3) * 4 + wv;
  const int m = (blockIdx.x & 7) * per + slot;
  if (slot >= per || m >= M) return;
  const int b = __builtin_amdgcn_readfirstlane((int)a.b_ids[m]);
  const int id = __builtin_amdgcn_readfirstlane((int)I.ids[m]);
  const int cy = id / I.w_c;
  const int oy = cy * a.stride - a.pad, ox = (id - cy * I.w_c) * a.stride - a.pad;
  const Chunk* src = reinterpret_cast<const Chunk*>(I.feat) + (long)b * I.Hf * I.Wf * 16;
  Chunk v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int k = it * 64 + lane;
    const int pos = k >> 4, wy = pos / W;
    const int y = oy + wy, x = ox + (pos - wy * W);
    const bool ok = k < TOTAL16 && y >= 0 && y < I.Hf && x >= 0 && x < I.Wf;
    // (clamped address + select: no load behind a branch)
    const Chunk t = src[ok ? ((long)y * I.Wf + x) * 16 + (k & 15) : 0];
    if constexpr (DT == FM_F32) v[it] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
    else v[it] = ok ? t : make_uint2(0u, 0u);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int k = it * 64 + lane;
    if (k < TOTAL16) {
      float4* slot4 = reinterpret_cast<float4*>(tile + (k >> 4) * PITCH + (k & 15) * 4);
      if constexpr (DT == FM_F32) *slot4 = v[it];
      else *slot4 = half4_to_float4(v[it], DT);
    }
  }
  __builtin_amdgcn_wave_barrier();       // same-wave LDS accesses are processed in order: no s_barrier needed
  wave_merge_tile<W>(tile, lane, a.wpack, I.ctx + ((long)b * I.cells + id) * 64);
  wave_store_tile64<W>(tile, I.out + (long)m * WW * 64, lane);
}

// NCHW0: image 0 is still in the reference's NCHW layout - its windows are visited in raster order here (the match list
// is sorted by the image-0 cell), which is the access pattern the NCHW loader of the cell-ordered crop copes with, so only
// image 1 (whose windows land wherever the partners are) needs the channels-last copy.
// DT = element type of the maps (FM_F32; FM_F16 / FM_BF16: channels-last maps of 2-byte elements, every value exact in
// float32, so the arithmetic - and the result - equals the float32 call on the up-cast maps).
template <int W, bool NCHW0, int DT = FM_F32>
__global__ __launch_bounds__(256) void k_fine_maps(const float* __restrict__ map0, const float* __restrict__ map1, int Hf0,
                                                   int Wf0, int Hf1, int Wf1, int stride, int pad, int w0c, int w1c,
                                                   const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                   const int64_t* __restrict__ j_ids, const int32_t* __restrict__ d_count,
                                                   int m_max, const float* __restrict__ mix0, const float* __restrict__ mix1,
                                                   const float* __restrict__ kc0, const float* __restrict__ kc1, float scale_f,
                                                   float* __restrict__ out0, float* __restrict__ out1) {
  constexpr int WW = W * W;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  const int per = (M + 7) >> 3;      // list_window's order, written out: M and per stay outside the loop over slots
  __shared__ __attribute__((aligned(16))) float tile_all[NCHW0 ? 4 * kGatherTileFloats(W) : 4];
  // (a grid smaller than the match list walks it in strides: fm_fine_match_maps may cap the grid so that the kernel's
  // workgroups do not fill every wave slot of the chip while another pair's coarse kernels wait for theirs)
  for (int slot = (int)(blockIdx.x >> 3) * 4 + wv; slot < per; slot += (int)(gridDim.x >> 3) * 4) {
  const int m = (blockIdx.x & 7) * per + slot;
  if (m >= M) break;
  const int b = __builtin_amdgcn_readfirstlane((int)b_ids[m]);
  const int i = __builtin_amdgcn_readfirstlane((int)i_ids[m]);
  const int j = __builtin_amdgcn_readfirstlane((int)j_ids[m]);
  const int cy0 = i / w0c, cy1 = j / w1c;
  const int oy0 = cy0 * stride - pad, ox0 = (i - cy0 * w0c) * stride - pad;
  const int oy1 = cy1 * stride - pad, ox1 = (j - cy1 * w1c) * stride - pad;
  // One buffer descriptor per window ROW (base = that row of the map, size = one map row, or 0 bytes for a row above /
  // below the map), one vector offset per window COLUMN (pixel x, this lane's channel; a negative x gets an offset
  // beyond any row): the unfold's zero padding on all four sides then comes from the hardware's range check - no
  // per-position conditions, ~10 scalar instructions per window row instead of ~12 per window position.
  constexpr int EB = DT == FM_F32 ? 4 : 2;          // bytes per element
  constexpr int PXB = 64 * EB;                      // bytes per pixel (64 channels)
  static_assert(!(NCHW0 && DT != FM_F32), "half-precision maps are read channels-last");
  const char* base0 = reinterpret_cast<const char*>(map0) + (long)b * Hf0 * Wf0 * PXB;
  const char* base1 = reinterpret_cast<const char*>(map1) + (long)b * Hf1 * Wf1 * PXB;
  unsigned vo0[W], vo1[W];
#pragma unroll
  for (int wx = 0; wx < W; ++wx) {
    const int x0 = ox0 + wx, x1 = ox1 + wx;
    vo0[wx] = x0 >= 0 ? (unsigned)(x0 * PXB + lane * EB) : 0x80000000u;
    vo1[wx] = x1 >= 0 ? (unsigned)(x1 * PXB + lane * EB) : 0x80000000u;
  }
  auto load_elem = [](const __amdgpu_buffer_rsrc_t r, unsigned vo) -> float {
    if constexpr (DT == FM_F32) return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, 0, 0));
    else return half_bits_to_float((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, vo, 0, 0), DT);
  };
  float f0[WW], f1[WW];
#pragma unroll
  for (int wy = 0; wy < W; ++wy) {
    const int y0 = oy0 + wy, y1 = oy1 + wy;
    const bool ok0 = y0 >= 0 && y0 < Hf0, ok1 = y1 >= 0 && y1 < Hf1;          // wave-uniform
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(base1 + (long)(ok1 ? y1 : 0) * Wf1 * PXB), 0, ok1 ? Wf1 * PXB : 0, 0x00020000);
    if (!NCHW0) {
      const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(base0 + (long)(ok0 ? y0 : 0) * Wf0 * PXB), 0, ok0 ? Wf0 * PXB : 0, 0x00020000);
#pragma unroll
      for (int wx = 0; wx < W; ++wx) f0[wy * W + wx] = load_elem(r0, vo0[wx]);
    }
#pragma unroll
    for (int wx = 0; wx < W; ++wx) f1[wy * W + wx] = load_elem(r1, vo1[wx]);
  }
  if (NCHW0) {      // image 0 straight from the NCHW map: the crop's loader into a wave-private tile, read back by channel
    float* tile = tile_all + wv * kGatherTileFloats(W);
    wave_load_window64<W>(reinterpret_cast<const float*>(base0), Hf0, Wf0, oy0, ox0, tile, lane);
#pragma unroll
    for (int r = 0; r < WW; ++r) f0[r] = tile[r * 68 + lane];
  }
  fine_core<W>(f0, f1, lane, mix0, mix1, kc0[m * 2], kc0[m * 2 + 1], kc1[m * 2], kc1[m * 2 + 1], scale_f,
               out0 + (long)m * 3, out1 + (long)m * 3);
  }
}


// [N, 64, Hf, Wf] -> [N, Hf, Wf, 64]: one workgroup per (sample, row y, 64 pixels of the row); reads 64 channel
// segments of 256 bytes (16-byte loads along x), writes one contiguous 16 KiB block; the transpose goes through an
// LDS tile with an odd pitch.  grid (ceil(Wf / 64), Hf, N).
// T = float, or unsigned short for float16 / bfloat16 maps (2-byte elements moved as they are: half the bytes).
template <typename T>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc64(const T* __restrict__ src, T* __restrict__ dst, int Hf, int Wf,
                                                        int N) {
  __shared__ T tile[64 * 65];                  // [x][c], pitch 65
  nchw_to_nhwc64_units<T>(src, dst, Hf, Wf, N, tile, blockIdx.x, gridDim.x);     // (fm_maps_device.h)
}

}  // namespace fm

using namespace fm;

// ---- the window calls: every entry point fills a WindowCall (fm_internal.h); one status, one route, one launch site per
// ---- kernel.  None: FM_E_UNSUPPORTED (a plain two-image crop in list order, say, is a hole in the table)
enum class WindowRoute { None, Cells64, List64, List64Merge, Nhwc64Copy, Nhwc64Merge, Generic, FineMaps };

static WindowRoute window_route(const WindowCall& c) {
  using R = WindowRoute;
  // the 64-channel kernels: the sizes they are instantiated for; the NCHW ones and the fine kernel address one sample's
  // map with 31-bit byte offsets (buffer descriptor), counted in float32 whatever the element type
  bool k64 = c.Cf == 64 && (c.W == 5 || c.W == 7), fits31 = true;
  for (int i = 0; i < c.images; ++i) fits31 = fits31 && (long)c.im[i].Hf * c.im[i].Wf * 64 * 4 < (1L << 31);
  const bool f32 = c.dtype == FM_F32, fast = f32 && k64 && fits31, one = c.images == 1, nchw = c.layout == 0;
  if (!map_dtype_ok(c.dtype)) return R::None;
  if (c.fine)      // (FM_LAYOUT_NCHW_PREPARED: image 1's channels-last copy was made by the coarse call - float32 maps only)
    return (nchw || c.layout == 1 || (c.layout == FM_LAYOUT_NCHW_PREPARED && f32)) && k64 && fits31 ? R::FineMaps : R::None;
  if (nchw && c.cells) return fast ? R::Cells64 : R::None;                            // one or two images, plain or merge
  if (nchw && one && c.merge) return fast ? R::List64Merge : R::None;
  if (nchw && one && fast) return R::List64;
  if (c.layout == 1 && !c.cells && c.merge) return k64 ? R::Nhwc64Merge : R::None;    // one or two images, any element type
  if (c.layout == 1 && !c.cells && one && f32 && k64) return R::Nhwc64Copy;           // one wave per window, 16-byte chunks
  // the generic kernels: the NCHW one stages a window of every channel in LDS, the channels-last one loads 4 channels at once
  const bool fits = nchw ? (size_t)c.W * c.W * (c.Cf + 1) * sizeof(float) <= 64 * 1024 : c.Cf % 4 == 0;
  return !c.cells && !c.merge && one && generic_window_supported(c.Cf, c.W, c.layout) && fits ? R::Generic : R::None;
}

// m_max == 0 is FM_OK before anything is looked at; then NULL, shape, unsupported
static int window_status(const WindowCall& c) {
  if (c.m_max == 0) return FM_OK;
  if (c.missing || !c.b_ids || (c.merge && !c.wpack)) return FM_E_NULL;
  for (int i = 0; i < c.images; ++i) {
    const WindowImage& im = c.im[i];
    if (!im.feat || !im.ids || !im.out || (c.cells && (!im.cell_map || !im.ties)) || (c.merge && !im.ctx)) return FM_E_NULL;
  }
  if (c.free_size && !map_dtype_ok(c.dtype)) return FM_E_UNSUPPORTED;
  if (c.free_size && !generic_window_shape_ok(c.Cf, c.W)) return FM_E_SHAPE;
  for (int i = 0; i < c.images; ++i) {
    const WindowImage& im = c.im[i];
    if (!crop_shape_ok(c.N, im.Hf, im.Wf, c.stride, c.m_max) || im.w_c <= 0 || ((c.cells || c.merge) && im.h_c <= 0) ||
        (c.cells && im.cell_pitch < im.h_c * im.w_c))
      return FM_E_SHAPE;
  }
  if (window_route(c) == WindowRoute::None) return FM_E_UNSUPPORTED;
  return c.fine && c.layout != 1 && !c.scratch ? FM_E_NULL : FM_OK;      // (the channels-last copies of NCHW maps)
}

// 8 XCD ranges of ceil(M/8) windows, four windows (waves) per workgroup
static int list_blocks(int m_max) { return 8 * (((m_max + 7) / 8 + 3) / 4); }
// largest grid of the kernels of fm_fine_match_maps (a multiple of 8; they walk longer lists in grid strides)
constexpr int kFineGridCap = 1 << 20;
// one wave per cell, four per workgroup, grid a multiple of 8
static int cell_blocks(long total) { return (int)(((total + 3) / 4 + 7) / 8 * 8); }

// the kernels' argument structs from the record (a one-image call names image 0 twice)
static CellArgs cell_args(const WindowCall& c) {
  auto image = [&](const WindowImage& s) {
    return CellImage{(const float*)s.feat, s.Hf, s.Wf, s.w_c, s.h_c * s.w_c, c.N * s.h_c * s.w_c, s.cell_map, s.cell_pitch,
                     s.ties, s.ids, s.out, s.ctx};
  };
  return {{image(c.im[0]), image(c.im[c.images - 1])}, c.stride, c.pad, c.m_max, c.b_ids, c.d_count, (const half8*)c.wpack};
}
static MergeNhwcArgs merge_nhwc_args(const WindowCall& c) {
  auto image = [](const WindowImage& s) {
    return MergeNhwcImage{s.feat, s.Hf, s.Wf, s.w_c, s.h_c * s.w_c, s.ids, s.out, s.ctx};
  };
  return {{image(c.im[0]), image(c.im[c.images - 1])}, c.stride, c.pad, c.m_max, c.b_ids, c.d_count, (const half8*)c.wpack};
}

// the cell-ordered crop of every image of the call in one launch (grid.x: the larger image's cells)
static void launch_cells64(const WindowCall& c) {
  long total = 0;
  for (int i = 0; i < c.images; ++i) total = std::max(total, (long)c.N * c.im[i].h_c * c.im[i].w_c);
  with_window(c.W, [&](auto w) {
    auto launch = [&](auto merge) {
      hipLaunchKernelGGL((k_gather_cellorder64<decltype(w)::value, decltype(merge)::value>),
                         dim3(cell_blocks(total), c.images), dim3(256), 0, (hipStream_t)c.stream, cell_args(c));
    };
    if (c.merge) launch(std::true_type{});
    else launch(std::false_type{});
  });
}
template <bool MERGE>
static void launch_list64(const WindowCall& c) {
  const WindowImage& im = c.im[0];
  with_window(c.W, [&](auto w) {
    hipLaunchKernelGGL((k_gather_nchw64<decltype(w)::value, MERGE>), dim3(list_blocks(c.m_max)), dim3(256), 0,
                       (hipStream_t)c.stream, (const float*)im.feat, im.Hf, im.Wf, c.stride, c.pad, im.w_c, c.b_ids, im.ids,
                       c.d_count, c.m_max, im.out, (const half8*)c.wpack, im.ctx, MERGE ? im.h_c * im.w_c : 0);
  });
}
// half-precision maps (an autocast backbone's hand-over) are read as they are - every value is exact in float32 - by
// the generic kernels; no up-cast pass over the whole map in front of the crop
template <int DT>
static void launch_generic_gather(const WindowCall& c) {
  const WindowImage& im = c.im[0];
  auto launch = [&](auto kernel, size_t smem) {
    hipLaunchKernelGGL(kernel, dim3(c.m_max), dim3(256), smem, (hipStream_t)c.stream,
                       (const typename MapElem<DT>::type*)im.feat, c.Cf, im.Hf, im.Wf, c.W, c.stride, c.pad, im.w_c, c.b_ids,
                       im.ids, c.d_count, c.m_max, im.out);
  };
  if (c.layout == 0) launch(k_gather_nchw<DT>, (size_t)c.W * c.W * (c.Cf + 1) * sizeof(float));
  else launch(k_gather_nhwc<DT>, 0);
}

// What every crop entry point does with its record.  The cases stand in the order in which the kernels have always been
// instantiated, the generic kernels' element types included (F32 first: not with_map_dtype's order), so that the device
// code object keeps its layout.
static int run_window_call(const WindowCall& c) {
  const int status = window_status(c);
  if (status != FM_OK || c.m_max == 0) return status;
  const WindowImage& im = c.im[0];
  switch (window_route(c)) {
    case WindowRoute::Cells64: launch_cells64(c); break;
    case WindowRoute::List64: launch_list64<false>(c); break;
    case WindowRoute::Nhwc64Copy:
      with_window(c.W, [&](auto w) {
        hipLaunchKernelGGL(k_gather_nhwc64<decltype(w)::value>, dim3(list_blocks(c.m_max)), dim3(256), 0, (hipStream_t)c.stream,
                           (const float*)im.feat, im.Hf, im.Wf, c.stride, c.pad, im.w_c, c.b_ids, im.ids, c.d_count, c.m_max,
                           im.out);
      });
      break;
    case WindowRoute::Generic:
      if (c.dtype == FM_F32) launch_generic_gather<FM_F32>(c);
      else if (c.dtype == FM_F16) launch_generic_gather<FM_F16>(c);
      else launch_generic_gather<FM_BF16>(c);
      break;
    case WindowRoute::List64Merge: launch_list64<true>(c); break;
    case WindowRoute::Nhwc64Merge:
      with_window(c.W, [&](auto w) {
        with_map_dtype(c.dtype, [&](auto dt) {
          hipLaunchKernelGGL((k_gather_merge_nhwc64<decltype(w)::value, decltype(dt)::value>),
                             dim3(list_blocks(c.m_max), c.images), dim3(256), 0, (hipStream_t)c.stream, merge_nhwc_args(c));
        });
      });
      break;
    default: break;       // (FineMaps: fm_fine_match_maps_dtype launches its own)
  }
  return (int)hipGetLastError();
}

extern "C" int fm_gather_windows_dtype(const void* feat_f, int map_dtype, int N, int Cf, int Hf, int Wf, int layout, int W,
                                       int stride, int pad, int w_c, const int64_t* b_ids, const int64_t* ids,
                                       const int32_t* d_count, int m_max, float* out, void* stream) {
  return run_window_call({1, {{feat_f, Hf, Wf, 0, w_c, ids, nullptr, 0, nullptr, out, nullptr}}, N, Cf, W, stride, pad, layout,
                          map_dtype, b_ids, d_count, m_max, nullptr, stream, /*cells*/ false, /*merge*/ false, /*free_size*/ true});
}

extern "C" int fm_gather_windows(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout, int W, int stride,
                                 int pad, int w_c, const int64_t* b_ids, const int64_t* ids, const int32_t* d_count,
                                 int m_max, float* out, void* stream) {
  return fm_gather_windows_dtype(feat_f, FM_F32, N, Cf, Hf, Wf, layout, W, stride, pad, w_c, b_ids, ids, d_count, m_max, out,
                                 stream);
}

extern "C" int fm_gather_windows_cells(const float* feat_f, int N, int Cf, int Hf, int Wf, int W, int stride, int pad,
                                       int h_c, int w_c, const int32_t* cell_to_match, int cell_pitch,
                                       const int32_t* ties, const int64_t* b_ids, const int64_t* ids,
                                       const int32_t* d_count, int m_max, float* out, void* stream) {
  return run_window_call({1, {{feat_f, Hf, Wf, h_c, w_c, ids, cell_to_match, cell_pitch, ties, out, nullptr}}, N, Cf, W, stride,
                          pad, 0, FM_F32, b_ids, d_count, m_max, nullptr, stream, /*cells*/ true});
}

// merge_feat.weight[:, :64] (row-major [64, 128], fine_preprocess.py:26) -> MFMA B fragments, f16 hi and lo:
// packed[((nt*4 + ks)*2 + plane)*64 + lane][j] = plane(W_w[32*nt + lane%32][16*ks + 8*(lane/32) + j])
__global__ __launch_bounds__(256) void k_merge_pack(const float* __restrict__ merge_w, half8* __restrict__ packed) {
  const int idx = blockIdx.x * 256 + threadIdx.x;       // (nt, ks, lane): 2 * 4 * 64 = 512
  if (idx >= 512) return;
  const int lane = idx & 63, ks = (idx >> 6) & 3, nt = idx >> 8;
  const float* src = merge_w + (32 * nt + (lane & 31)) * 128 + 16 * ks + 8 * (lane >> 5);
  half8 hh, ll;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float x = src[j] * kMergeWgtScale;
    // a weight beyond the fixed scale (|w| >= 16) would turn into +-inf here and into a wrong finite number or NaN
    // somewhere downstream: make it NaN for certain - every output that touches it then says so
    if (!(fabsf(x) <= 65504.f)) x = __builtin_nanf("");
    split_f16(x, hh, ll, j);
  }
  packed[((nt * 4 + ks) * 2 + 0) * 64 + lane] = hh;
  packed[((nt * 4 + ks) * 2 + 1) * 64 + lane] = ll;
}

extern "C" int fm_merge_pack_weights(const float* merge_w, int Cf, void* packed, void* stream) {
  if (!merge_w || !packed) return FM_E_NULL;
  if (Cf != 64) return FM_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_merge_pack, dim3(2), dim3(256), 0, (hipStream_t)stream, merge_w, (half8*)packed);
  return (int)hipGetLastError();
}

extern "C" int fm_gather_merge_windows(const float* feat_f, int N, int Cf, int Hf, int Wf, int W, int stride, int pad,
                                       int h_c, int w_c, const int32_t* cell_to_match, int cell_pitch,
                                       const int32_t* ties, const void* packed_w, const float* ctx_bias,
                                       const int64_t* b_ids, const int64_t* ids, const int32_t* d_count, int m_max,
                                       float* out, void* stream) {
  return run_window_call({1, {{feat_f, Hf, Wf, h_c, w_c, ids, cell_to_match, cell_pitch, ties, out, ctx_bias}}, N, Cf, W, stride,
                          pad, 0, FM_F32, b_ids, d_count, m_max, packed_w, stream,
                          /*cells, else list order*/ cell_to_match != nullptr, /*merge*/ true});
}

extern "C" int fm_gather_windows_pair(const float* feat_f0, const float* feat_f1, int N, int Cf, int Hf0, int Wf0,
                                      int Hf1, int Wf1, int W, int stride, int pad, int h0c, int w0c, int h1c, int w1c,
                                      const int32_t* cell0, int pitch0, const int32_t* ties0, const int32_t* cell1,
                                      int pitch1, const int32_t* ties1, const void* packed_w, const float* ctx0,
                                      const float* ctx1, const int64_t* b_ids, const int64_t* i_ids,
                                      const int64_t* j_ids, const int32_t* d_count, int m_max, float* out0,
                                      float* out1, void* stream) {
  return run_window_call({2, {{feat_f0, Hf0, Wf0, h0c, w0c, i_ids, cell0, pitch0, ties0, out0, ctx0},
                              {feat_f1, Hf1, Wf1, h1c, w1c, j_ids, cell1, pitch1, ties1, out1, ctx1}},
                          N, Cf, W, stride, pad, 0, FM_F32, b_ids, d_count, m_max, packed_w, stream,
                          /*cells*/ true, /*merge, else the plain crop*/ packed_w != nullptr});
}

extern "C" int fm_gather_merge_windows_nhwc(const void* feat_f0, const void* feat_f1, int map_dtype, int N, int Cf, int Hf0,
                                            int Wf0, int Hf1, int Wf1, int W, int stride, int pad, int h0c, int w0c,
                                            int h1c, int w1c, const void* packed_w, const float* ctx0, const float* ctx1,
                                            const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                            const int32_t* d_count, int m_max, float* out0, float* out1, void* stream) {
  return run_window_call({feat_f1 ? 2 : 1, {{feat_f0, Hf0, Wf0, h0c, w0c, i_ids, nullptr, 0, nullptr, out0, ctx0},
                                            {feat_f1, Hf1, Wf1, h1c, w1c, j_ids, nullptr, 0, nullptr, out1, ctx1}},
                          N, Cf, W, stride, pad, 1, map_dtype, b_ids, d_count, m_max, packed_w, stream, /*cells*/ false,
                          /*merge*/ true});
}

extern "C" int fm_fine_match(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW, int Cf,
                             const float* mix0, const float* mix1, const float* mkpts0_c, const float* mkpts1_c,
                             float scale_f, float* out0, float* out1, void* stream) {
  if (m_max == 0) return FM_OK;
  if (!win0 || !win1 || !mix0 || !mix1 || !mkpts0_c || !mkpts1_c || !out0 || !out1) return FM_E_NULL;
  if (m_max < 0) return FM_E_SHAPE;
  if (Cf != 64 || (WW != 25 && WW != 49)) return FM_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (m_max + 3) / 4;
  with_window(WW == 25 ? 5 : 7, [&](auto w) {
    hipLaunchKernelGGL(k_fine<decltype(w)::value>, dim3(blocks), dim3(256), 0, st, win0, win1, m_max, d_count, mix0, mix1,
                       mkpts0_c, mkpts1_c, scale_f, out0, out1);
  });
  return (int)hipGetLastError();
}

// Scratch of fm_fine_match_maps for NCHW maps: the channels-last copies k_fine_maps reads.  float32 maps: image 1's
// only (image 0 is read as it is: map[0] is empty).  Half-precision maps: both images' (2-byte elements), image 0's
// first, image 1's 256-byte aligned.  Byte regions: the element type is the call's (launch_channels_last_copy<T>).
struct FineMapsScratch { Region<char> map[2]; size_t total; };
static FineMapsScratch fine_maps_layout(int N, int Cf, int Hf0, int Wf0, int Hf1, int Wf1, int map_dtype) {
  const size_t elem = map_dtype == FM_F32 ? 4 : 2;
  FineMapsScratch s;
  Carver c;
  c.take(s.map[0], map_dtype == FM_F32 ? 0 : (size_t)N * Cf * elem * (size_t)Hf0 * Wf0);
  c.take(s.map[1], (size_t)N * Cf * elem * (size_t)Hf1 * Wf1);
  s.total = c.o;
  return s;
}

extern "C" size_t fm_fine_maps_scratch_bytes_dtype(int N, int Cf, int Hf0, int Wf0, int Hf1, int Wf1, int layout, int map_dtype) {
  if (layout != 0 || N <= 0 || Cf <= 0 || Hf0 <= 0 || Wf0 <= 0 || Hf1 <= 0 || Wf1 <= 0) return 0;
  return fine_maps_layout(N, Cf, Hf0, Wf0, Hf1, Wf1, map_dtype).total;
}

// [N, 64, Hf, Wf] -> [N, Hf, Wf, 64] of T (k_nchw_to_nhwc64): one workgroup per piece, or grid_cap of them in strides
template <typename T>
static void launch_channels_last_copy(const void* src, void* dst, int N, int Hf, int Wf, int grid_cap, hipStream_t st) {
  const long pieces = (long)((Wf + 63) / 64) * Hf * N;
  hipLaunchKernelGGL(k_nchw_to_nhwc64<T>, dim3((unsigned)(pieces < grid_cap ? pieces : grid_cap)), dim3(256), 0, st,
                     (const T*)src, (T*)dst, Hf, Wf, N);
}
extern "C" size_t fm_fine_maps_scratch_bytes(int N, int Cf, int Hf0, int Wf0, int Hf1, int Wf1, int layout) {
  return fm_fine_maps_scratch_bytes_dtype(N, Cf, Hf0, Wf0, Hf1, Wf1, layout, FM_F32);
}

extern "C" int fm_fine_match_maps_dtype(const void* feat_f0, const void* feat_f1, int map_dtype, int layout, int N, int Cf,
                                        int Hf0, int Wf0, int Hf1, int Wf1, int W, int stride, int pad, int w0c, int w1c,
                                        const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                        const int32_t* d_count, int m_max, const float* mix0, const float* mix1,
                                        const float* mkpts0_c, const float* mkpts1_c, float scale_f, void* scratch,
                                        float* out0, float* out1, void* stream) {
  const WindowCall c{2, {{feat_f0, Hf0, Wf0, 0, w0c, i_ids, nullptr, 0, nullptr, out0, nullptr},
                         {feat_f1, Hf1, Wf1, 0, w1c, j_ids, nullptr, 0, nullptr, out1, nullptr}},
                     N, Cf, W, stride, pad, layout, map_dtype, b_ids, d_count, m_max, nullptr, stream, /*cells*/ false,
                     /*merge*/ false, /*free_size*/ false, /*fine*/ true, !mix0 || !mix1 || !mkpts0_c || !mkpts1_c, scratch};
  const int status = window_status(c);
  if (status != FM_OK || m_max == 0) return status;
  const bool prepared = layout == FM_LAYOUT_NCHW_PREPARED, nchw = layout != 1;
  hipStream_t st = (hipStream_t)stream;
  const void *m0 = feat_f0, *m1 = feat_f1;      // the maps k_fine_maps reads
  int grid_cap = kFineGridCap;
#ifdef FM_TUNE_ENV
  if (const char* e = getenv("FM_FINE_GRID")) grid_cap = atoi(e) > 0 ? atoi(e) / 8 * 8 : kFineGridCap;
#endif
  if (nchw) {          // NCHW: channels-last copies (coalesced on both sides), element type kept
    const FineMapsScratch sc = fine_maps_layout(N, Cf, Hf0, Wf0, Hf1, Wf1, map_dtype);
    void* s0 = sc.map[0].in(scratch);
    void* s1 = sc.map[1].in(scratch);
    if (map_dtype == FM_F32) {     // image 0 is read as it is; image 1's copy may have been made by the coarse call
      if (!prepared) launch_channels_last_copy<float>(feat_f1, s1, N, Hf1, Wf1, grid_cap, st);
    } else {
      launch_channels_last_copy<unsigned short>(feat_f0, s0, N, Hf0, Wf0, grid_cap, st);
      launch_channels_last_copy<unsigned short>(feat_f1, s1, N, Hf1, Wf1, grid_cap, st);
      m0 = s0;
    }
    m1 = s1;
  }
  const int blocks = list_blocks(m_max) < grid_cap ? list_blocks(m_max) : grid_cap;
  with_window(W, [&](auto w) {
    with_map_dtype(map_dtype, [&](auto dt) {
      auto launch = [&](auto nchw0) {
        hipLaunchKernelGGL((k_fine_maps<decltype(w)::value, decltype(nchw0)::value, decltype(dt)::value>), dim3(blocks),
                           dim3(256), 0, st, (const float*)m0, (const float*)m1, Hf0, Wf0, Hf1, Wf1, stride, pad, w0c, w1c,
                           b_ids, i_ids, j_ids, d_count, m_max, mix0, mix1, mkpts0_c, mkpts1_c, scale_f, out0, out1);
      };
      // float32 NCHW: image 0 straight from the map; every other form reads two channels-last maps
      if constexpr (decltype(dt)::value == FM_F32) {
        if (nchw) launch(std::true_type{});
        else launch(std::false_type{});
      } else {
        launch(std::false_type{});
      }
    });
  });
  return (int)hipGetLastError();
}

extern "C" int fm_fine_match_maps(const float* feat_f0, const float* feat_f1, int layout, int N, int Cf, int Hf0, int Wf0,
                                  int Hf1, int Wf1, int W, int stride, int pad, int w0c, int w1c, const int64_t* b_ids,
                                  const int64_t* i_ids, const int64_t* j_ids, const int32_t* d_count, int m_max,
                                  const float* mix0, const float* mix1, const float* mkpts0_c, const float* mkpts1_c,
                                  float scale_f, void* scratch, float* out0, float* out1, void* stream) {
  return fm_fine_match_maps_dtype(feat_f0, feat_f1, FM_F32, layout, N, Cf, Hf0, Wf0, Hf1, Wf1, W, stride, pad, w0c, w1c,
                                  b_ids, i_ids, j_ids, d_count, m_max, mix0, mix1, mkpts0_c, mkpts1_c, scale_f, scratch,
                                  out0, out1, stream);
}
