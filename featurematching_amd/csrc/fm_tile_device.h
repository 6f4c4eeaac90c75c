// The float32 tile products of the fine training layers (encoder_tail.hip, qkv_proj.hip, window_merge.hip) and the fold
// of per-workgroup slabs they share with linear_attn.hip.  Defined once: layout L, the fragment order, the transposed
// exchange image, the opaque zero and the two-groups-ahead prefetch are explained here and nowhere else.
//
// Layout L.  A wave owns 32 tokens.  Every product runs on v_mfma_f32_32x32x2_f32 (exact float32, one rounding per
// product, a k-ordered fmaf chain) and is computed TRANSPOSED, out^T [channel][token] = M [out][in] in^T: the token is
// the column of the 32x32 result tile, so it sits on the lane (lane & 31) and a token's channels sit in the registers of
// the two lanes `lane` and `lane ^ 32`.  A 64-channel vector of a token is 32 registers per lane,
//     register R of lane half h = lane >> 5  <->  channel 8 (R >> 2) + 4 h + (R & 3)
// which is the C/D map of the instruction (row = (r & 3) + 8 (r >> 2) + 4 h of tile R >> 4) and, read the other way, its
// B operand of k-step R: half 0 supplies channel k0, half 1 channel k1, and since the order of a sum's terms is free,
// register R of one product's result IS the B operand of step R of the next.  A chain of products never leaves the
// registers, and rows of a [T, 64] tensor are loaded and stored straight in layout L as 16-byte pieces.
// Fragments.  The A operand of step R is M[32 ot + (lane & 31)][channel(R, h)]: a pack kernel writes a matrix once per
// call in that order, [out tile][R >> 2][lane][R & 3], so a lane's operands of four k-steps are one 16-byte load.
// Exchange image.  A weight gradient sums over TOKENS, which sit on lanes: each of a backward's four waves writes its
// tile's operands transposed into an LDS image [channel][token] (rows of kTilePitch = 33 floats, an odd pitch: the lanes
// of the products' loads walk down a column and then share no bank) and, between two barriers, every wave multiplies
// ITS output tiles over all four images, in wave order.  Per workgroup one slab of partial sums; fold_slabs adds the
// slabs in a fixed order.
#pragma once
#include "fm_wave_device.h"

namespace fm {

constexpr int kTile = 32;                        // tokens of a wave's tile (the N of the MFMA)
constexpr int kTilePitch = 33;                   // floats of a row of the exchange image
constexpr int kTileFwdWaves = 8, kTileFwdChunk = kTileFwdWaves * kTile;     // 256 tokens per workgroup and round
constexpr int kTileBwdWaves = 4, kTileBwdChunk = kTileBwdWaves * kTile;     // 128
constexpr int kTileMaxGroups = 256;              // workgroups of a kernel (one per CU; the rest by grid stride)
constexpr int kTileMaxT = 1 << 24;               // tokens of one call (fmatch.h)

// workgroups of a kernel whose chunk holds `chunk` tokens
static inline int token_groups(long T, int chunk) {
  const long c = (T + chunk - 1) / chunk;
  return (int)(c < kTileMaxGroups ? c : kTileMaxGroups);
}

// frag[idx] of one matrix: [ot][q][lane][e] = M[32 ot + (lane & 31)][8 q + 4 (lane >> 5) + e], M = W [O][I] (kin = I
// k-steps' channels) or W^T (kin = O)
__device__ __forceinline__ float frag_value(const float* __restrict__ W, int I, int kin, bool tr, int idx) {
  const int e = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8, nq = kin >> 3;
  const int row = 32 * (rest / nq) + (lane & 31), col = 8 * (rest % nq) + 4 * (lane >> 5) + e;
  return tr ? W[col * I + row] : W[row * I + col];
}

// 0, but not to the compiler: added to the base of the fragments (and of parameters in LDS) once per round of the token
// loop, it keeps their loads - the same addresses in every round - from being hoisted out of the loop (896 registers'
// worth in k_et_bwd) and spilled
__device__ __forceinline__ int opaque_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

// acc[ot] = rows 32 ot .. of M in^T for the wave's 32 tokens; in[R] in layout L (NK registers = 2 NK channels)
template <int NO, int NK>
__device__ __forceinline__ void tile_mm(const float4* __restrict__ F, const float (&in)[NK], f32x16 (&acc)[NO], int lane) {
#pragma unroll
  for (int ot = 0; ot < NO; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ot][r] = 0.f;
  // The fragments of group q + 2 are requested before the products of group q and nothing crosses a group's end
  // (sched_barrier): the loads from L2 then stay two groups ahead of their use.  Left to the scheduler the encoder
  // tail's backward is a third slower (forward + backward at 196 000 tokens 0.63 against 0.47 ms), the forward, whose
  // fragments are in LDS, the same.
  constexpr int NQ = NK / 4, AHEAD = 2;
  float4 w[AHEAD + 1][NO];
#pragma unroll
  for (int q = 0; q < AHEAD && q < NQ; ++q)
#pragma unroll
    for (int ot = 0; ot < NO; ++ot) w[q][ot] = F[(ot * NQ + q) * 64 + lane];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q + AHEAD < NQ) {
#pragma unroll
      for (int ot = 0; ot < NO; ++ot) w[(q + AHEAD) % (AHEAD + 1)][ot] = F[(ot * NQ + q + AHEAD) * 64 + lane];
    }
#pragma unroll
    for (int ot = 0; ot < NO; ++ot) {
      const float4 f = w[q % (AHEAD + 1)][ot];
      acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.x, in[4 * q], acc[ot], 0, 0, 0);
      acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.y, in[4 * q + 1], acc[ot], 0, 0, 0);
      acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.z, in[4 * q + 2], acc[ot], 0, 0, 0);
      acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.w, in[4 * q + 3], acc[ot], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// rows t0 .. t0 + 31 of a [T, 64] tensor <-> layout L (32 registers); rows past T read as 0 and are not written
__device__ __forceinline__ void tile_load(const float* __restrict__ p, size_t t0, int T, int lane, float* __restrict__ v) {
  const size_t tok = t0 + (lane & 31);
  const bool live = tok < (size_t)T;
  const float4* s = reinterpret_cast<const float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 r = live ? s[2 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
  }
}
__device__ __forceinline__ void tile_store(float* __restrict__ p, size_t t0, int T, int lane, const float (&v)[32]) {
  const size_t tok = t0 + (lane & 31);
  if (tok >= (size_t)T) return;
  float4* s = reinterpret_cast<float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 8; ++q) s[2 * q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// the two tiles of an accumulator -> rows t0 .. of a [T, 64] tensor
__device__ __forceinline__ void tile_store(float* __restrict__ p, size_t t0, int T, int lane, const f32x16& a,
                                           const f32x16& b) {
  const size_t tok = t0 + (lane & 31);
  if (tok >= (size_t)T) return;
  float4* s = reinterpret_cast<float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[2 * q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    s[2 * q + 8] = make_float4(b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]);
  }
}
// the same + the 64 floats at `bias` (the lane's pieces of them; NULL: + 0) -> row tok of [T, 64], if live
__device__ __forceinline__ void tile_store(float* __restrict__ p, size_t tok, bool live, int lane,
                                           const float* __restrict__ bias, const f32x16& a, const f32x16& b) {
  if (!live) return;
  float4* s = reinterpret_cast<float4*>(p + tok * 64 + 4 * (lane >> 5));
  const float4* c = reinterpret_cast<const float4*>(bias ? bias + 4 * (lane >> 5) : nullptr);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 lo = bias ? c[2 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 hi = bias ? c[2 * q + 8] : make_float4(0.f, 0.f, 0.f, 0.f);
    s[2 * q] = make_float4(a[4 * q] + lo.x, a[4 * q + 1] + lo.y, a[4 * q + 2] + lo.z, a[4 * q + 3] + lo.w);
    s[2 * q + 8] = make_float4(b[4 * q] + hi.x, b[4 * q + 1] + hi.y, b[4 * q + 2] + hi.z, b[4 * q + 3] + hi.w);
  }
}

// the wave's image: row (row0 + channel) <- v (NR registers in layout L), column = token
template <int NR>
__device__ __forceinline__ void tile_put(float* __restrict__ E, int row0, int lane, const float* __restrict__ v) {
  float* e = E + (row0 + 4 * (lane >> 5)) * kTilePitch + (lane & 31);
#pragma unroll
  for (int R = 0; R < NR; ++R) e[(8 * (R >> 2) + (R & 3)) * kTilePitch] = v[R];
}
// acc[j][out][in] += sum over the chunk's tokens of rows rowA.. (out) times rows rowB + 32 j.. (in): the WAVES images
// (IMAGE floats each) in index order, the tokens of each in order
template <int NB, int WAVES, int IMAGE>
__device__ __forceinline__ void tile_wgrad(const float* __restrict__ E, int rowA, int rowB, int lane, f32x16 (&acc)[NB]) {
  const int at = (lane & 31) * kTilePitch + (lane >> 5);
  for (int w = 0; w < WAVES; ++w) {
    const float* pa = E + w * IMAGE + rowA * kTilePitch + at;
    const float* pb = E + w * IMAGE + rowB * kTilePitch + at;
#pragma unroll 4
    for (int s = 0; s < kTile / 2; ++s) {
      const float va = pa[2 * s];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, pb[j * 32 * kTilePitch + 2 * s], acc[j], 0, 0, 0);
    }
  }
}
// tile -> slab: D[i][j] at col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void tile_out(float* __restrict__ dst, int ld, int lane, const f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * ld + (lane & 31)] = acc[r];
}

// The sum of n_part slabs of slab_floats floats at one entry (p = the entry in slab 0), by a workgroup of 256 threads
// that folds 32 neighbouring entries (entry = threadIdx.x & 31): slice j = threadIdx.x >> 5 of its 8 adds slabs j,
// j + 8, ... in index order (8 short chains of loads in place of one long one), then slice 0 adds the 8 slices in index
// order.  True, with *v set, in the threads of slice 0; the others are done.  These sums decide the weight gradients'
// bits: the order is part of the interface.
__device__ __forceinline__ bool fold_slabs(const float* __restrict__ p, int n_part, int slab_floats, float (&red)[8][32],
                                           float* __restrict__ v) {
  const int x = threadIdx.x & 31, j = threadIdx.x >> 5;
  float s = 0.f;
#pragma unroll 4
  for (int c = j; c < n_part; c += 8) s += p[(size_t)c * slab_floats];
  red[j][x] = s;
  __syncthreads();
  if (j != 0) return false;
  *v = ((((((red[0][x] + red[1][x]) + red[2][x]) + red[3][x]) + red[4][x]) + red[5][x]) + red[6][x]) + red[7][x];
  return true;
}

}  // namespace fm
