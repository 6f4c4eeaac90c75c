// The tail of an encoder layer (transformer.py, EncoderLayer.forward: everything behind the attention) and its gradient,
// fused: the context layers' training path at the fine level, d_model = 64.  Per token t, float32 throughout:
//     m = a Wm^T        mu1, r1 = mean(m), 1 / sqrt(var(m) + eps1)     nh = (m - mu1) r1      n1 = nh g1 + b1
//     c = [x, n1]       p = c W1^T      h = max(p, 0)      o = h W2^T
//     mu2, r2 likewise with eps2        oh = (o - mu2) r2  y = x + oh g2 + b2
// and from gy:
//     db2 = sum_t gy    dg2 = sum_t gy oh     doh = gy g2      do = r2 (doh - mean(doh) - oh mean(doh oh))
//     dW2 = sum_t do^T h     dh = do W2       dp = dh [p > 0]
//     dW1 = sum_t dp^T c     dc = dp W1       dx = gy + dc[:64]      dn1 = dc[64:]
//     db1 = sum_t dn1   dg1 = sum_t dn1 nh    dnh = dn1 g1     dm = r1 (dnh - mean(dnh) - nh mean(dnh nh))
//     dWm = sum_t dm^T a     da = dm Wm
// (biased variance, as nn.LayerNorm).  Every product runs on v_mfma_f32_32x32x2_f32: exact float32, one rounding per
// product, a k-ordered fmaf chain.
//
// Tiling.  A wave owns 32 tokens.  The products are computed TRANSPOSED, out^T [channel][token] = W [out][in] in^T: the
// token is the column of the 32x32 result tile, so it sits on the lane (lane & 31) and a token's channels sit in the
// registers of the two lanes `lane` and `lane ^ 32`.  A 64-channel vector of a token is 32 registers per lane,
//     register R of lane half h = lane >> 5  <->  channel 8 (R >> 2) + 4 h + (R & 3)                     ("layout L")
// which is the C/D map of the instruction (row = (r & 3) + 8 (r >> 2) + 4 h of tile R >> 4) and, read the other way,
// its B operand of k-step R: half 0 supplies channel k0, half 1 channel k1, and since the order of a sum's terms is
// free, register R of one product's result IS the B operand of step R of the next.  The chain m -> n1 -> p -> h -> o
// (and do -> dh -> dp -> dc -> dm -> da) never leaves the registers, a LayerNorm sum is 32 in-lane adds and one
// exchange with lane ^ 32, and x, a, gy are loaded straight into layout L as 16-byte pieces.  The A operand of step R
// is W[32 ot + (lane & 31)][channel(R, h)]: k_et_pack writes the three matrices and their transposes once per call in
// that order ("fragments": [out tile][R >> 2][lane][R & 3], one 16-byte load per lane = 4 k-steps).
//   k_et_fwd : 8 waves; the forward fragments (112 KB) in LDS; nothing is kept for the backward.
//   k_et_bwd : 4 waves; recomputes the chain from x and a; fragments from L2 (the LDS is the exchange below).
//     The weight gradients sum over TOKENS, which sit on lanes: each wave writes its tile's operands transposed into an
//     LDS image [channel][token] (three stages per 128-token chunk: (do, h, gy oh), (dp, c), (dm, a, dn1, dn1 nh); 256
//     rows of 33 floats per wave) and, between two barriers, every wave multiplies ITS share of the output tiles (7 of
//     the 28: 112 accumulator registers) over all four images.  The LayerNorm gradients are row sums of the wave's own
//     image, lane = channel.  Per workgroup one slab of partial sums; k_et_fold adds the slabs in a fixed order.
// No atomics, grids that depend on T alone, fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_wave_device.h"

namespace fm {

constexpr int kEtTile = 32;                      // tokens of a wave's tile (the N of the MFMA)
constexpr int kEtFwdWaves = 8, kEtFwdChunk = kEtFwdWaves * kEtTile;     // 256 tokens per workgroup and round
constexpr int kEtBwdWaves = 4, kEtBwdChunk = kEtBwdWaves * kEtTile;     // 128
constexpr int kEtMaxGroups = 256;                // workgroups of either kernel (one per CU; the rest by grid stride)
constexpr int kEtMaxT = 1 << 24;                 // tokens of one call (fmatch.h)
// fragments, in floats: Wm | W1 | W2 (the forward's) | Wm^T | W1^T | W2^T
constexpr int kEtFm = 0, kEtF1 = 4096, kEtF2 = 20480, kEtFwdFrag = 28672;
constexpr int kEtFmT = 28672, kEtF1T = 32768, kEtF2T = 49152, kEtFrag = 57344;
// a slab of partial parameter gradients, in floats: dW1 | dW2 | dWm | dg1 | db1 | dg2 | db2
constexpr int kEtS1 = 0, kEtS2 = 16384, kEtSm = 24576, kEtSln = 28672, kEtSlab = 28928;
constexpr int kEtPitch = 33, kEtImage = 256 * kEtPitch;      // floats of an exchange row / of a wave's image
constexpr int kEtFwdLds = (kEtFwdFrag + 256) * 4;
constexpr int kEtBwdLds = (256 + kEtBwdWaves * 4 * 64 + kEtBwdWaves * kEtImage) * 4;
static_assert(kEtSlab % 32 == 0, "k_et_fold's grid covers a slab exactly");
static_assert(kEtBwdLds <= 160 * 1024 && kEtFwdLds <= 160 * 1024, "one workgroup per CU");

// frag[idx] of one matrix: [ot][q][lane][e] = M[32 ot + (lane & 31)][8 q + 4 (lane >> 5) + e], M = W [O][I] or W^T
__device__ __forceinline__ float et_frag(const float* __restrict__ W, int I, int kin, bool tr, int idx) {
  const int e = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8, nq = kin >> 3;
  const int row = 32 * (rest / nq) + (lane & 31), col = 8 * (rest % nq) + 4 * (lane >> 5) + e;
  return tr ? W[col * I + row] : W[row * I + col];
}
__global__ __launch_bounds__(256) void k_et_pack(const float* __restrict__ wm, const float* __restrict__ w1,
                                                 const float* __restrict__ w2, int n, float* __restrict__ frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v;
  if (i < kEtF1) v = et_frag(wm, 64, 64, false, i - kEtFm);
  else if (i < kEtF2) v = et_frag(w1, 128, 128, false, i - kEtF1);
  else if (i < kEtFmT) v = et_frag(w2, 128, 128, false, i - kEtF2);
  else if (i < kEtF1T) v = et_frag(wm, 64, 64, true, i - kEtFmT);
  else if (i < kEtF2T) v = et_frag(w1, 128, 128, true, i - kEtF1T);
  else v = et_frag(w2, 128, 64, true, i - kEtF2T);
  frag[i] = v;
}

// 0, but not to the compiler: added to the base of the fragments and parameters once per round of the token loop, it keeps
// their loads - the same addresses in every round - from being hoisted out of the loop (896 registers' worth) and spilled
__device__ __forceinline__ int et_opaque_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

// acc[ot] = rows 32 ot .. of M in^T for the wave's 32 tokens; in[R] in layout L (NK registers = 2 NK channels)
template <int NO, int NK>
__device__ __forceinline__ void et_mm(const float4* __restrict__ F, const float (&in)[NK], f32x16 (&acc)[NO], int lane) {
#pragma unroll
  for (int ot = 0; ot < NO; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ot][r] = 0.f;
  // The fragments of group q + 2 are requested before the products of group q and nothing crosses a group's end
  // (sched_barrier): the loads from L2 then stay two groups ahead of their use.  Left to the scheduler the backward is
  // a third slower (forward + backward at 196 000 tokens 0.63 against 0.47 ms), the forward, whose fragments are in
  // LDS, the same.
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
template <int NO>
__device__ __forceinline__ void et_unpack(const f32x16 (&acc)[NO], float (&v)[16 * NO]) {
#pragma unroll
  for (int R = 0; R < 16 * NO; ++R) v[R] = acc[R >> 4][R & 15];
}

// sum over a token's 64 channels: the lane's 32 registers, then the other half's (the same bits in both lanes)
__device__ __forceinline__ float et_sum64(const float (&v)[32]) {
  float s = v[0];
#pragma unroll
  for (int R = 1; R < 32; ++R) s += v[R];
  return pair_op<32, OpAdd>(s);
}
// v <- (v - mean) r, r = 1 / sqrt(var + eps) returned
__device__ __forceinline__ float et_normalize(float (&v)[32], float eps) {
  const float mean = et_sum64(v) * (1.f / 64.f);
  float sq[32];
#pragma unroll
  for (int R = 0; R < 32; ++R) { v[R] -= mean; sq[R] = v[R] * v[R]; }
  const float r = 1.f / sqrtf(et_sum64(sq) * (1.f / 64.f) + eps);
#pragma unroll
  for (int R = 0; R < 32; ++R) v[R] *= r;
  return r;
}
// out = r (d - mean(d) - nh mean(d nh)): the gradient through (v - mean) r given d = the gradient of nh
__device__ __forceinline__ void et_normalize_grad(const float (&d)[32], const float (&nh)[32], float r, float (&out)[32]) {
  float t[32];
#pragma unroll
  for (int R = 0; R < 32; ++R) t[R] = d[R] * nh[R];
  const float m1 = et_sum64(d) * (1.f / 64.f), m2 = et_sum64(t) * (1.f / 64.f);
#pragma unroll
  for (int R = 0; R < 32; ++R) out[R] = r * (d[R] - m1 - nh[R] * m2);
}
// a per-channel parameter vector (LDS, 64 floats) in layout L
__device__ __forceinline__ void et_param(const float* __restrict__ p, int lane, float (&v)[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 r = *reinterpret_cast<const float4*>(p + 8 * q + 4 * (lane >> 5));
    v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
  }
}
// rows t0 .. t0 + 31 of a [T, 64] tensor <-> layout L; rows past T read as 0 and are not written
__device__ __forceinline__ void et_load(const float* __restrict__ p, size_t t0, int T, int lane, float (&v)[32]) {
  const size_t tok = t0 + (lane & 31);
  const bool live = tok < (size_t)T;
  const float4* s = reinterpret_cast<const float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 r = live ? s[2 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
  }
}
__device__ __forceinline__ void et_store(float* __restrict__ p, size_t t0, int T, int lane, const float (&v)[32]) {
  const size_t tok = t0 + (lane & 31);
  if (tok >= (size_t)T) return;
  float4* s = reinterpret_cast<float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 8; ++q) s[2 * q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// c = [x, n1], n1 = nh g1 + b1
__device__ __forceinline__ void et_concat(const float* __restrict__ lnp, int lane, const float (&x)[32],
                                          const float (&nh)[32], float (&c)[64]) {
  float g[32], b[32];
  et_param(lnp, lane, g);
  et_param(lnp + 64, lane, b);
#pragma unroll
  for (int R = 0; R < 32; ++R) { c[R] = x[R]; c[32 + R] = fmaf(nh[R], g[R], b[R]); }
}

// the forward chain of one tile.  lnp (LDS) = g1 | b1 | g2 | b2.  Leaves nh, r1, h, oh, r2.
__device__ __forceinline__ void et_chain(const float4* __restrict__ Fm, const float4* __restrict__ F1,
                                         const float4* __restrict__ F2, const float* __restrict__ lnp,
                                         const float (&x)[32], const float (&a)[32], float eps1, float eps2, int lane,
                                         float (&nh)[32], float& r1, float (&hh)[64], float (&oh)[32],
                                         float& r2) {
  f32x16 m[2];
  et_mm<2, 32>(Fm, a, m, lane);
  et_unpack<2>(m, nh);
  r1 = et_normalize(nh, eps1);
  float c[64];
  et_concat(lnp, lane, x, nh, c);
  f32x16 p[4];
  et_mm<4, 64>(F1, c, p, lane);
  et_unpack<4>(p, hh);
#pragma unroll
  for (int R = 0; R < 64; ++R) hh[R] = fmaxf(hh[R], 0.f);
  f32x16 o[2];
  et_mm<2, 64>(F2, hh, o, lane);
  et_unpack<2>(o, oh);
  r2 = et_normalize(oh, eps2);
}

__device__ __forceinline__ void et_stage_params(float* __restrict__ lnp, const float* __restrict__ g1,
                                                const float* __restrict__ b1, const float* __restrict__ g2,
                                                const float* __restrict__ b2, int tid) {
  if (tid < 256) {
    const float* src = tid < 64 ? g1 : tid < 128 ? b1 : tid < 192 ? g2 : b2;
    lnp[tid] = src[tid & 63];
  }
}

__global__ __launch_bounds__(kEtFwdWaves * 64) void k_et_fwd(const float* __restrict__ x, const float* __restrict__ a,
                                                             const float* __restrict__ frag, const float* __restrict__ g1,
                                                             const float* __restrict__ b1, const float* __restrict__ g2,
                                                             const float* __restrict__ b2, int T, float eps1, float eps2,
                                                             float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float et_lds[];
  float* lnp = et_lds + kEtFwdFrag;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kEtFwdFrag / 4; i += kEtFwdWaves * 64)
    reinterpret_cast<float4*>(et_lds)[i] = reinterpret_cast<const float4*>(frag)[i];
  et_stage_params(lnp, g1, b1, g2, b2, tid);
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(et_lds);
  const int chunks = (T + kEtFwdChunk - 1) / kEtFwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kEtFwdChunk + wave * kEtTile;
    if (t0 >= (size_t)T) continue;
    const float4* F = F0 + et_opaque_zero();
    float vx[32], va[32], nh[32], hh[64], oh[32], r1, r2;
    et_load(x, t0, T, lane, vx);
    et_load(a, t0, T, lane, va);
    et_chain(F + kEtFm / 4, F + kEtF1 / 4, F + kEtF2 / 4, lnp, vx, va, eps1, eps2, lane, nh, r1, hh, oh, r2);
    float g[32], b[32];
    et_param(lnp + 128, lane, g);
    et_param(lnp + 192, lane, b);
#pragma unroll
    for (int R = 0; R < 32; ++R) oh[R] = vx[R] + fmaf(oh[R], g[R], b[R]);
    et_store(y, t0, T, lane, oh);
  }
}

// the wave's image: row (row0 + channel) <- v, column = token
template <int NR>
__device__ __forceinline__ void et_put(float* __restrict__ E, int row0, int lane, const float (&v)[NR]) {
  float* e = E + (row0 + 4 * (lane >> 5)) * kEtPitch + (lane & 31);
#pragma unroll
  for (int R = 0; R < NR; ++R) e[(8 * (R >> 2) + (R & 3)) * kEtPitch] = v[R];
}
// acc[j][out][in] += sum over the chunk's 128 tokens of rows rowA.. (out) times rows rowB + 32 j.. (in)
template <int NB>
__device__ __forceinline__ void et_wgrad(const float* __restrict__ E, int rowA, int rowB, int lane, f32x16 (&acc)[NB]) {
  const int at = (lane & 31) * kEtPitch + (lane >> 5);
  for (int w = 0; w < kEtBwdWaves; ++w) {
    const float* pa = E + w * kEtImage + rowA * kEtPitch + at;
    const float* pb = E + w * kEtImage + rowB * kEtPitch + at;
#pragma unroll 4
    for (int s = 0; s < kEtTile / 2; ++s) {
      const float va = pa[2 * s];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, pb[j * 32 * kEtPitch + 2 * s], acc[j], 0, 0, 0);
    }
  }
}
// lane = channel: the sum of row (row0 + lane) of the wave's image over its 32 tokens, in token order
__device__ __forceinline__ float et_row_sum(const float* __restrict__ E, int row0, int lane) {
  const float* e = E + (row0 + lane) * kEtPitch;
  float s = e[0];
#pragma unroll
  for (int t = 1; t < kEtTile; ++t) s += e[t];
  return s;
}
// tile -> slab: D[i][j] at col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void et_tile_out(float* __restrict__ dst, int ld, int lane, const f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * ld + (lane & 31)] = acc[r];
}

// WGRAD = false: dx and da only (no exchange, no barriers, `part` unused)
template <bool WGRAD>
__global__ __launch_bounds__(kEtBwdWaves * 64) void k_et_bwd(const float* __restrict__ x, const float* __restrict__ a,
                                                             const float* __restrict__ gy, const float* __restrict__ frag,
                                                             const float* __restrict__ g1, const float* __restrict__ b1,
                                                             const float* __restrict__ g2, const float* __restrict__ b2,
                                                             int T, float eps1, float eps2, float* __restrict__ dx,
                                                             float* __restrict__ da, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float et_lds[];
  float* lnp0_ = et_lds;                                 // g1 | b1 | g2 | b2
  float* red = lnp0_ + 256;                                // [wave][dg1 | db1 | dg2 | db2][64]
  float* E = red + kEtBwdWaves * 256;                    // [wave][256 rows][kEtPitch]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* Ew = E + wave * kEtImage;
  et_stage_params(lnp0_, g1, b1, g2, b2, tid);
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(frag);
  const float* lnp0 = lnp0_;
  f32x16 acc2[2], acc1[4], accm[1];
  float s_g1 = 0.f, s_b1 = 0.f, s_g2 = 0.f, s_b2 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc2[0][r] = acc2[1][r] = accm[0][r] = 0.f;
    acc1[0][r] = acc1[1][r] = acc1[2][r] = acc1[3][r] = 0.f;
  }
  const int chunks = (T + kEtBwdChunk - 1) / kEtBwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kEtBwdChunk + wave * kEtTile;     // past T in the last chunk: a tile of zeros
    const int zero = et_opaque_zero();
    const float4* F = F0 + zero;
    const float* lnp = lnp0 + zero;
    float nh[32], hh[64], oh[32], dv[32], r1, r2;
    {
      float vx[32], va[32];
      et_load(x, t0, T, lane, vx);
      et_load(a, t0, T, lane, va);
      et_chain(F + kEtFm / 4, F + kEtF1 / 4, F + kEtF2 / 4, lnp, vx, va, eps1, eps2, lane, nh, r1, hh, oh, r2);
    }
    {                                                    // do
      float g[32], w[32];
      et_load(gy, t0, T, lane, g);
      if (WGRAD) {
#pragma unroll
        for (int R = 0; R < 32; ++R) w[R] = g[R] * oh[R];
        et_put<32>(Ew, 192, lane, w);
      }
      et_param(lnp + 128, lane, w);
#pragma unroll
      for (int R = 0; R < 32; ++R) g[R] *= w[R];
      et_normalize_grad(g, oh, r2, dv);
    }
    if (WGRAD) {                                         // stage 1: dW2 = do^T h, dg2, db2
      et_put<32>(Ew, 0, lane, dv);
      et_put<64>(Ew, 64, lane, hh);
      __syncthreads();
      et_wgrad<2>(E, 32 * (wave >> 1), 64 + 64 * (wave & 1), lane, acc2);
      s_g2 += et_row_sum(Ew, 192, lane);
      float s = 0.f;
      for (int t = 0; t < kEtTile; ++t)
        if (t0 + t < (size_t)T) s += gy[(t0 + t) * 64 + lane];
      s_b2 += s;
      __syncthreads();
    }
    float dp[64];
    {
      f32x16 dh[4];
      et_mm<4, 32>(F + kEtF2T / 4, dv, dh, lane);
      et_unpack<4>(dh, dp);
#pragma unroll
      for (int R = 0; R < 64; ++R) dp[R] = hh[R] > 0.f ? dp[R] : 0.f;
    }
    if (WGRAD) {                                         // stage 2: dW1 = dp^T c
      et_put<64>(Ew, 0, lane, dp);
      float vx[32], c[64];                               // (x again: 32 registers less through the products between)
      et_load(x, t0, T, lane, vx);
      et_concat(lnp, lane, vx, nh, c);
      et_put<64>(Ew, 128, lane, c);
      __syncthreads();
      et_wgrad<4>(E, 32 * wave, 128, lane, acc1);
      __syncthreads();
    }
    float dn[32];
    {
      f32x16 dc[4];
      et_mm<4, 64>(F + kEtF1T / 4, dp, dc, lane);
      float g[32];
      et_load(gy, t0, T, lane, g);
#pragma unroll
      for (int R = 0; R < 32; ++R) { g[R] += dc[R >> 4][R & 15]; dn[R] = dc[2 + (R >> 4)][R & 15]; }
      et_store(dx, t0, T, lane, g);
    }
    float dm[32];
    {
      float w[32];
      if (WGRAD) {
        et_put<32>(Ew, 128, lane, dn);
#pragma unroll
        for (int R = 0; R < 32; ++R) w[R] = dn[R] * nh[R];
        et_put<32>(Ew, 192, lane, w);
      }
      et_param(lnp, lane, w);
#pragma unroll
      for (int R = 0; R < 32; ++R) dn[R] *= w[R];
      et_normalize_grad(dn, nh, r1, dm);
    }
    if (WGRAD) {                                         // stage 3: dWm = dm^T a, dg1, db1
      float va[32];
      et_load(a, t0, T, lane, va);
      et_put<32>(Ew, 0, lane, dm);
      et_put<32>(Ew, 64, lane, va);
      __syncthreads();
      et_wgrad<1>(E, 32 * (wave >> 1), 64 + 32 * (wave & 1), lane, accm);
      s_b1 += et_row_sum(Ew, 128, lane);
      s_g1 += et_row_sum(Ew, 192, lane);
      __syncthreads();
    }
    {
      f32x16 dd[2];
      et_mm<2, 32>(F + kEtFmT / 4, dm, dd, lane);
      float w[32];
      et_unpack<2>(dd, w);
      et_store(da, t0, T, lane, w);
    }
  }
  if (WGRAD) {
    float* slab = part + (size_t)blockIdx.x * kEtSlab;
#pragma unroll
    for (int j = 0; j < 4; ++j) et_tile_out(slab + kEtS1 + 32 * wave * 128 + 32 * j, 128, lane, acc1[j]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      et_tile_out(slab + kEtS2 + 32 * (wave >> 1) * 128 + 32 * (2 * (wave & 1) + j), 128, lane, acc2[j]);
    et_tile_out(slab + kEtSm + 32 * (wave >> 1) * 64 + 32 * (wave & 1), 64, lane, accm[0]);
    float* rw = red + wave * 256;
    rw[lane] = s_g1; rw[64 + lane] = s_b1; rw[128 + lane] = s_g2; rw[192 + lane] = s_b2;
    __syncthreads();
    slab[kEtSln + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];      // the waves in index order
  }
}

// the seven parameter gradients = the sum of the n_part slabs, in a fixed order (k_la_fold's: 8 slices of every 8th
// slab, then the slices in index order)
struct EtGrads { float *w_merge, *ln1_w, *ln1_b, *w_mlp0, *w_mlp2, *ln2_w, *ln2_b; };
__global__ __launch_bounds__(256) void k_et_fold(const float* __restrict__ part, int n_part, EtGrads d) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, j = threadIdx.x >> 5, i = blockIdx.x * 32 + x;
  const float* p = part + i;
  float s = 0.f;
#pragma unroll 4
  for (int c = j; c < n_part; c += 8) s += p[(size_t)c * kEtSlab];
  red[j][x] = s;
  __syncthreads();
  if (j != 0) return;
  const float v = ((((((red[0][x] + red[1][x]) + red[2][x]) + red[3][x]) + red[4][x]) + red[5][x]) + red[6][x]) + red[7][x];
  if (i < kEtS2) d.w_mlp0[i] = v;
  else if (i < kEtSm) d.w_mlp2[i - kEtS2] = v;
  else if (i < kEtSln) d.w_merge[i - kEtSm] = v;
  else if (i < kEtSln + 64) d.ln1_w[i - kEtSln] = v;
  else if (i < kEtSln + 128) d.ln1_b[i - kEtSln - 64] = v;
  else if (i < kEtSln + 192) d.ln2_w[i - kEtSln - 128] = v;
  else d.ln2_b[i - kEtSln - 192] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool et_route(int T, int d) { return d == 64 && T <= kEtMaxT; }
static int et_groups(int T, int chunk) {
  const int c = (T + chunk - 1) / chunk;
  return c < kEtMaxGroups ? c : kEtMaxGroups;
}
// Workspace of either call: the fragments | one slab per workgroup of the backward
struct EtWs { Region<float> frag, part; size_t total; };
static EtWs et_layout(int T) {
  EtWs w;
  Carver c;
  c.take(w.frag, kEtFrag);
  c.take(w.part, (size_t)et_groups(T, kEtBwdChunk) * kEtSlab);
  w.total = c.pad();
  return w;
}

// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct EtCall {
  const float *x, *a, *w_merge, *ln1_w, *ln1_b, *w_mlp0, *w_mlp2, *ln2_w, *ln2_b;
  int T, d; float eps1, eps2;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float* y;                                        // forward
  const float* d_y; float *d_x, *d_a; EtGrads g;   // backward
};

// the ONLY copy of the two entry points' argument checks; *wgrad is set with FM_OK.  (No route keeps a state: the
// state pointers are never looked at.)
static int et_status(const EtCall& c, bool* wgrad) {
  if (!c.x || !c.a || !c.w_merge || !c.ln1_w || !c.ln1_b || !c.w_mlp0 || !c.w_mlp2 || !c.ln2_w || !c.ln2_b) return FM_E_NULL;
  if (c.backward ? (!c.d_y || !c.d_x || !c.d_a) : !c.y) return FM_E_NULL;
  const int given = !!c.g.w_merge + !!c.g.ln1_w + !!c.g.ln1_b + !!c.g.w_mlp0 + !!c.g.w_mlp2 + !!c.g.ln2_w + !!c.g.ln2_b;
  if (given != 0 && given != 7) return FM_E_NULL;
  if (c.T <= 0 || c.d <= 0) return FM_E_SHAPE;
  if (!et_route(c.T, c.d) || !(c.eps1 > 0.f) || !(c.eps2 > 0.f)) return FM_E_UNSUPPORTED;
  if (!c.workspace || !workspace_ok(c.workspace, c.workspace_bytes, et_layout(c.T).total)) return FM_E_WORKSPACE;
  *wgrad = given == 7;
  return FM_OK;
}

static int et_run(const EtCall& c) {
  bool wgrad = false;
  const int status = et_status(c, &wgrad);
  if (status != FM_OK) return status;
  hipStream_t st = (hipStream_t)c.stream;
  const EtWs w = et_layout(c.T);
  float* frag = w.frag.in(c.workspace);
  const int n_frag = c.backward ? kEtFrag : kEtFwdFrag;
  hipLaunchKernelGGL(k_et_pack, dim3(n_frag / 256), dim3(256), 0, st, c.w_merge, c.w_mlp0, c.w_mlp2, n_frag, frag);
  if (!c.backward) {
    static unsigned long long lds_fwd = 0;
    const hipError_t e = ensure_dynamic_lds(k_et_fwd, kEtFwdLds, &lds_fwd);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_et_fwd, dim3(et_groups(c.T, kEtFwdChunk)), dim3(kEtFwdWaves * 64), kEtFwdLds, st, c.x, c.a,
                       (const float*)frag, c.ln1_w, c.ln1_b, c.ln2_w, c.ln2_b, c.T, c.eps1, c.eps2, c.y);
    return (int)hipGetLastError();
  }
  const int groups = et_groups(c.T, kEtBwdChunk);
  float* part = w.part.in(c.workspace);
  if (wgrad) {
    static unsigned long long lds_bwd = 0;
    const hipError_t e = ensure_dynamic_lds(k_et_bwd<true>, kEtBwdLds, &lds_bwd);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_et_bwd<true>, dim3(groups), dim3(kEtBwdWaves * 64), kEtBwdLds, st, c.x, c.a, c.d_y,
                       (const float*)frag, c.ln1_w, c.ln1_b, c.ln2_w, c.ln2_b, c.T, c.eps1, c.eps2, c.d_x, c.d_a, part);
    hipLaunchKernelGGL(k_et_fold, dim3(kEtSlab / 32), dim3(256), 0, st, (const float*)part, groups, c.g);
  } else {
    hipLaunchKernelGGL(k_et_bwd<false>, dim3(groups), dim3(kEtBwdWaves * 64), 256 * 4, st, c.x, c.a, c.d_y,
                       (const float*)frag, c.ln1_w, c.ln1_b, c.ln2_w, c.ln2_b, c.T, c.eps1, c.eps2, c.d_x, c.d_a, part);
  }
  return (int)hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_encoder_tail_state_bytes(int T, int d) {
  (void)T; (void)d;
  return 0;                                        // the backward recomputes the chain: nothing is kept
}

extern "C" size_t fm_encoder_tail_workspace_bytes(int T, int d) {
  if (T <= 0 || d <= 0 || !et_route(T, d)) return 0;
  return et_layout(T).total;
}

extern "C" int fm_encoder_tail_forward(const float* x, const float* a, const float* w_merge, const float* ln1_w,
                                       const float* ln1_b, const float* w_mlp0, const float* w_mlp2, const float* ln2_w,
                                       const float* ln2_b, int T, int d, float eps1, float eps2, void* workspace,
                                       size_t workspace_bytes, float* state, float* y, void* stream) {
  (void)state;
  EtCall c = {};
  c.x = x; c.a = a; c.w_merge = w_merge; c.ln1_w = ln1_w; c.ln1_b = ln1_b; c.w_mlp0 = w_mlp0; c.w_mlp2 = w_mlp2;
  c.ln2_w = ln2_w; c.ln2_b = ln2_b;
  c.T = T; c.d = d; c.eps1 = eps1; c.eps2 = eps2;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.y = y;
  return et_run(c);
}

extern "C" int fm_encoder_tail_backward(const float* x, const float* a, const float* w_merge, const float* ln1_w,
                                        const float* ln1_b, const float* w_mlp0, const float* w_mlp2, const float* ln2_w,
                                        const float* ln2_b, const float* d_y, const float* state, int T, int d, float eps1,
                                        float eps2, void* workspace, size_t workspace_bytes, float* d_x, float* d_a,
                                        float* d_w_merge, float* d_ln1_w, float* d_ln1_b, float* d_w_mlp0, float* d_w_mlp2,
                                        float* d_ln2_w, float* d_ln2_b, void* stream) {
  (void)state;
  EtCall c = {};
  c.x = x; c.a = a; c.w_merge = w_merge; c.ln1_w = ln1_w; c.ln1_b = ln1_b; c.w_mlp0 = w_mlp0; c.w_mlp2 = w_mlp2;
  c.ln2_w = ln2_w; c.ln2_b = ln2_b;
  c.T = T; c.d = d; c.eps1 = eps1; c.eps2 = eps2;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.d_y = d_y; c.d_x = d_x; c.d_a = d_a;
  c.g = {d_w_merge, d_ln1_w, d_ln1_b, d_w_mlp0, d_w_mlp2, d_ln2_w, d_ln2_b};
  return et_run(c);
}
