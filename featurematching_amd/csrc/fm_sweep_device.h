// The tiled sweep of the coarse level's training kernels, once: k_dsm_bwd (dsm_grad.hip) and k_closs_sweep
// (coarse_loss.hip) are instantiations of sweep_tiles below, differ in their policy type alone and are launched from one
// site, launch_sweep (fm_internal.h).
//
// A workgroup of 256 threads owns 32 rows of the "owner" image (X, R rows) and sweeps the z-th share of the other image
// (Y, T rows) in tiles of 32 descriptors; grid (ceil(R / 32), N, Z).  Per tile it recomputes the 32 x 32 dot products in
// float32 and turns each into one value (written transposed into Dt).  kDsmStats: it stores the tile's column sums as its
// row tile's partial of u and goes on; v_out / u_out are then the partial arrays, and it ends with the row sums into its z
// slice's partial of v.  kDsmSparse, kDsmDense: it accumulates Dt . Ys into its rows' gradient and ends with its partial
// gradient into part[z][b][row][c_in].
//   kDsmSparse : D = -(A w_y + B w_x), the weights w / sum folded into one factor per row / column
//   kDsmStats  : gc = g conf, conf = A B                          (no gradient phase)
//   kDsmDense  : D = 2 gc - A w_y - B w_x                         (1 / sum and w kept apart)
// with A = exp2(k2 x + ofs_y) / sum_y, B = exp2(k2 x + ofs_x) / sum_x and x the dot product.
//
// The policy says what the two kernels do not share:
//   pol.dots<C>(Xs, Ys, tx, ty, sv)       how a dot product is summed: sv[q] (0 on entry) += Xs[ty + 8 q] . Ys[tx]
//   pol.fetch_g(...), pol.g_from_lds(...) where g comes from, when it is loaded: before / behind the tile's barrier
//   pol.gc(g, conf, kept), pol.keep(ok, kept)  g conf of one entry; what else a kDsmStats sweep keeps of the entry
//   pol.sums_done(Dt, part_index)         what a kDsmStats workgroup still does once its row sums are out
//
// Every expression is written as the two kernels had it before they were joined, operand order and the place of each
// `ok ? ... : 0` included: which products the compiler packs and which it contracts into fused multiply-adds - that is,
// the rounding of D - follows from that shape.  After an edit, compare with the parent build as
// profiles/sweep_shared_parent_vs_change.txt does ("One sweep, two policies").
#pragma once
#include "fm_device.h"

namespace fm {

enum { kDsmSparse = 0, kDsmStats = 1, kDsmDense = 2 };

// LDS of a sweep (floats): Xs [32][C + 4] | Ys [32][C + 4] | Dt [32 (l)][36], D transposed | Gs [32][33], the tile of a
// loaded G (kernels that have one).  Row pitch C + 4: 16-byte reads of 16 consecutive rows hit all banks.
constexpr int kSweepTile = 32;
constexpr int kSweepDtPitch = 36, kSweepGsPitch = 33;
constexpr int sweep_pitch(int C) { return C + 4; }
constexpr int sweep_dt_at(int C) { return 2 * kSweepTile * sweep_pitch(C); }
constexpr int sweep_gs_at(int C) { return sweep_dt_at(C) + kSweepTile * kSweepDtPitch; }
constexpr int sweep_lds_bytes(int C, bool g_tile) {
  return (sweep_gs_at(C) + (g_tile ? kSweepTile * kSweepGsPitch : 0)) * 4;
}

// 32 rows of src from row0 on (rows beyond `rows` and float4 groups beyond c_in / 4: zeros) into dst [32][C + 4]
template <int C>
__device__ __forceinline__ void sweep_load_tile(float* dst, const float* src, int row0, int rows, int c_in) {
  constexpr int P = sweep_pitch(C);
  const int tid = threadIdx.x, vpr = c_in >> 2;
#pragma unroll
  for (int p = 0; p < 32 * (C / 4) / 256; ++p) {
    const int idx = p * 256 + tid, row = idx / (C / 4), v4 = idx % (C / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < rows && v4 < vpr) v = reinterpret_cast<const float4*>(src + (long)(row0 + row) * c_in)[v4];
    *reinterpret_cast<float4*>(&dst[row * P + 4 * v4]) = v;
  }
}

// gradient phase: acc[r][e] += sum_l Dt[l][8 rg + r] Ys[l][4 c4 + e]
template <int C>
__device__ __forceinline__ void sweep_accumulate(const float* Ys, const float* Dt, int c4, int rg, float (&acc)[8][4]) {
  constexpr int P = sweep_pitch(C);
  if (4 * c4 < C) {
#pragma unroll 4
    for (int ll = 0; ll < 32; ++ll) {
      const float4 y = *reinterpret_cast<const float4*>(&Ys[ll * P + 4 * c4]);
      const float4 d0 = *reinterpret_cast<const float4*>(&Dt[ll * kSweepDtPitch + 8 * rg]);
      const float4 d1 = *reinterpret_cast<const float4*>(&Dt[ll * kSweepDtPitch + 8 * rg + 4]);
      const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        acc[r][0] = __builtin_fmaf(d[r], y.x, acc[r][0]);
        acc[r][1] = __builtin_fmaf(d[r], y.y, acc[r][1]);
        acc[r][2] = __builtin_fmaf(d[r], y.z, acc[r][2]);
        acc[r][3] = __builtin_fmaf(d[r], y.w, acc[r][3]);
      }
    }
  }
}

// column sums of this tile's g conf: 32 threads add the 32 owner rows of their column in a fixed order and store the sum
// as the partial of this workgroup's row tile, u_part[blockIdx.x][b][T] - a tile of columns belongs to one z slice, so
// every element has one writer; k_sweep_fold_sums adds the row tiles up in index order (no atomics)
__device__ __forceinline__ void sweep_column_sums(const float* Dt, int b, int l0, int T, float* u_part) {
  const int tid = threadIdx.x;
  if (tid < 32 && l0 + tid < T) {
    float cs = 0.f;
#pragma unroll 8
    for (int rr = 0; rr < 32; ++rr) cs += Dt[tid * kSweepDtPitch + rr];
    u_part[((long)blockIdx.x * gridDim.y + b) * T + l0 + tid] = cs;
  }
}

// row sums: the 32 columns a row's partial sums sit in are the 32 lanes of a half wave; one partial per z slice,
// v_part[z][b][R] (a slice without a tile stores 0), folded in index order by k_sweep_fold_sums
__device__ __forceinline__ void sweep_row_sums(const float (&vacc)[4], int b, int k0, int R, float* v_part) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float t = vacc[q];
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) t += __shfl_xor(t, m);
    const int k = k0 + ty + 8 * q;
    if (tx == 0 && k < R) v_part[((long)blockIdx.z * gridDim.y + b) * R + k] = t;
  }
}

// the workgroup's partial gradient of its rows into part[z][b], [R][c_in]
__device__ __forceinline__ void sweep_store_partial(const float (&acc)[8][4], int k0, int R, int c_in, int c4, int rg,
                                                    float* part) {
  if (c4 < (c_in >> 2)) {
    float* out = part + (((long)blockIdx.z * gridDim.y + blockIdx.y) * R) * c_in;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = k0 + 8 * rg + r;
      if (k < R) reinterpret_cast<float4*>(out + (long)k * c_in)[c4] = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
  }
}

// C = padded channel count (64 / 128 / 256), c_in <= C the rows' real length; the statistics and weights are those of
// the owner image (x) and of the other image (y)
template <int C, int MODE, class Pol>
__device__ __forceinline__ void sweep_tiles(const float* X, const float* Y, int R, int T, int c_in, const float* ofs_x,
                                            const float* sum_x, int pitch_x, const float* ofs_y, const float* sum_y,
                                            int pitch_y, const float* w_x, const float* w_y, float k2, float* part,
                                            float* v_out, float* u_out, Pol& pol) {
  constexpr int P = sweep_pitch(C);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Xs = sm;
  float* Ys = sm + kSweepTile * P;
  float* Dt = sm + sweep_dt_at(C);
  const int tid = threadIdx.x, b = blockIdx.y, k0 = blockIdx.x * 32;
  const int ntiles = (T + 31) / 32, Z = gridDim.z, z = blockIdx.z;
  const int t_lo = (int)((long)ntiles * z / Z), t_hi = (int)((long)ntiles * (z + 1) / Z);
  const float* Xb = X + (long)b * R * c_in;
  const float* Yb = Y + (long)b * T * c_in;
  sweep_load_tile<C>(Xs, Xb, k0, R, c_in);
  const int tx = tid & 31, ty = tid >> 5;                 // similarity phase: column tx, rows ty + 8 q
  float ox[4], wx[4], isx[4], vacc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + ty + 8 * q;
    ox[q] = k < R ? ofs_x[(long)b * pitch_x + k] : 0.f;
    isx[q] = k < R ? 1.0f / sum_x[(long)b * pitch_x + k] : 0.f;
    if (MODE == kDsmSparse) wx[q] = k < R ? w_x[(long)b * R + k] / sum_x[(long)b * pitch_x + k] : 0.f;
    else wx[q] = (MODE == kDsmDense && k < R) ? w_x[(long)b * R + k] : 0.f;
    vacc[q] = 0.f;
  }
  const int c4 = tid & 63, rg = tid >> 6;                 // gradient phase: channels 4 c4 .. + 3, rows 8 rg .. + 7
  float acc[8][4];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
  for (int t = t_lo; t < t_hi; ++t) {
    const int l0 = t * 32;
    __syncthreads();                                      // the previous tile's readers are done with Ys and Dt
    sweep_load_tile<C>(Ys, Yb, l0, T, c_in);
    const int l = l0 + tx;
    const float oy = l < T ? ofs_y[(long)b * pitch_y + l] : 0.f;
    const float isy = l < T ? 1.0f / sum_y[(long)b * pitch_y + l] : 0.f;
    float wy;
    if (MODE == kDsmSparse) wy = l < T ? w_y[(long)b * T + l] / sum_y[(long)b * pitch_y + l] : 0.f;
    else wy = (MODE == kDsmDense && l < T) ? w_y[(long)b * T + l] : 0.f;
    float gq[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE != kDsmSparse) pol.fetch_g(gq, k0, l0, R, T);
    __syncthreads();
    if (MODE != kDsmSparse) pol.g_from_lds(gq);
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
    pol.template dots<C>(Xs, Ys, tx, ty, sv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = l < T && k0 + ty + 8 * q < R;
      if (MODE == kDsmSparse) {
        const float a = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[q], k2, oy)) * wy;
        const float bt = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[q], k2, ox[q])) * wx[q];
        Dt[tx * kSweepDtPitch + ty + 8 * q] = ok ? -(a + bt) : 0.f;
      } else {
        // (conf_from of coarse_loss.hip, written out: called here it changes what k_dsm_bwd<C, kDsmDense> compiles to)
        const float ar = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[q], k2, oy)) * isy;       // softmax over the owner's rows
        const float br = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[q], k2, ox[q])) * isx[q]; // ... over the other image's
        const float conf = ar * br;
        float kept = 0.f;                                 // (what the policy keeps of an entry besides gc)
        const float gc = ok ? pol.gc(gq[q], conf, kept) : 0.f;
        if (MODE == kDsmStats) { vacc[q] += gc; pol.keep(ok, kept); Dt[tx * kSweepDtPitch + ty + 8 * q] = gc; }
        else Dt[tx * kSweepDtPitch + ty + 8 * q] = ok ? 2.0f * gc - ar * wy - br * wx[q] : 0.f;
      }
    }
    __syncthreads();
    if (MODE == kDsmStats) {
      sweep_column_sums(Dt, b, l0, T, u_out);
      continue;
    }
    sweep_accumulate<C>(Ys, Dt, c4, rg, acc);
  }
  if (MODE == kDsmStats) {
    sweep_row_sums(vacc, b, k0, R, v_out);
    pol.sums_done(Dt, ((long)z * gridDim.y + b) * gridDim.x + blockIdx.x);
    return;
  }
  sweep_store_partial(acc, k0, R, c_in, c4, rg, part);
}

}  // namespace fm
