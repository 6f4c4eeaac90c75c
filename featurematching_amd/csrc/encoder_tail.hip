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
// Tiling: fm_tile_device.h's (layout L, fragments, the exchange image).  The chain m -> n1 -> p -> h -> o (and do -> dh ->
// dp -> dc -> dm -> da) never leaves the registers, a LayerNorm sum is 32 in-lane adds and one exchange with lane ^ 32,
// and k_et_pack writes the three matrices and their transposes as fragments once per call.
//   k_et_fwd : 8 waves; the forward fragments (112 KB) in LDS; nothing is kept for the backward.
//   k_et_bwd : 4 waves; recomputes the chain from x and a; fragments from L2 (the LDS is the exchange).  Three stages
//     per 128-token chunk: (do, h, gy oh), (dp, c), (dm, a, dn1, dn1 nh); 256 image rows per wave; every wave multiplies
//     ITS share of the output tiles (7 of the 28: 112 accumulator registers) over all four images.  The LayerNorm
//     gradients are row sums of the wave's own image, lane = channel.  k_et_fold adds the workgroups' slabs.
// No atomics, grids that depend on T alone, fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

// fragments, in floats: Wm | W1 | W2 (the forward's) | Wm^T | W1^T | W2^T
constexpr int kEtFm = 0, kEtF1 = 4096, kEtF2 = 20480, kEtFwdFrag = 28672;
constexpr int kEtFmT = 28672, kEtF1T = 32768, kEtF2T = 49152, kEtFrag = 57344;
// a slab of partial parameter gradients, in floats: dW1 | dW2 | dWm | dg1 | db1 | dg2 | db2
constexpr int kEtS1 = 0, kEtS2 = 16384, kEtSm = 24576, kEtSln = 28672, kEtSlab = 28928;
constexpr int kEtImage = 256 * kTilePitch;       // floats of a wave's image
constexpr int kEtFwdLds = (kEtFwdFrag + 256) * 4;
constexpr int kEtBwdLds = (256 + kTileBwdWaves * 4 * 64 + kTileBwdWaves * kEtImage) * 4;
static_assert(kEtSlab % 32 == 0, "k_et_fold's grid covers a slab exactly");
static_assert(kEtBwdLds <= 160 * 1024 && kEtFwdLds <= 160 * 1024, "one workgroup per CU");

__global__ __launch_bounds__(256) void k_et_pack(const float* __restrict__ wm, const float* __restrict__ w1,
                                                 const float* __restrict__ w2, int n, float* __restrict__ frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v;
  if (i < kEtF1) v = frag_value(wm, 64, 64, false, i - kEtFm);
  else if (i < kEtF2) v = frag_value(w1, 128, 128, false, i - kEtF1);
  else if (i < kEtFmT) v = frag_value(w2, 128, 128, false, i - kEtF2);
  else if (i < kEtF1T) v = frag_value(wm, 64, 64, true, i - kEtFmT);
  else if (i < kEtF2T) v = frag_value(w1, 128, 128, true, i - kEtF1T);
  else v = frag_value(w2, 128, 64, true, i - kEtF2T);
  frag[i] = v;
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
  tile_mm<2, 32>(Fm, a, m, lane);
  et_unpack<2>(m, nh);
  r1 = et_normalize(nh, eps1);
  float c[64];
  et_concat(lnp, lane, x, nh, c);
  f32x16 p[4];
  tile_mm<4, 64>(F1, c, p, lane);
  et_unpack<4>(p, hh);
#pragma unroll
  for (int R = 0; R < 64; ++R) hh[R] = fmaxf(hh[R], 0.f);
  f32x16 o[2];
  tile_mm<2, 64>(F2, hh, o, lane);
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

__global__ __launch_bounds__(kTileFwdWaves * 64) void k_et_fwd(const float* __restrict__ x, const float* __restrict__ a,
                                                               const float* __restrict__ frag, const float* __restrict__ g1,
                                                               const float* __restrict__ b1, const float* __restrict__ g2,
                                                               const float* __restrict__ b2, int T, float eps1, float eps2,
                                                               float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float et_lds[];
  float* lnp = et_lds + kEtFwdFrag;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kEtFwdFrag / 4; i += kTileFwdWaves * 64)     // (written out: a helper moves the loop in the kernel)
    reinterpret_cast<float4*>(et_lds)[i] = reinterpret_cast<const float4*>(frag)[i];
  et_stage_params(lnp, g1, b1, g2, b2, tid);
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(et_lds);
  const int chunks = (T + kTileFwdChunk - 1) / kTileFwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kTileFwdChunk + wave * kTile;
    if (t0 >= (size_t)T) continue;
    const float4* F = F0 + opaque_zero();
    float vx[32], va[32], nh[32], hh[64], oh[32], r1, r2;
    tile_load(x, t0, T, lane, vx);
    tile_load(a, t0, T, lane, va);
    et_chain(F + kEtFm / 4, F + kEtF1 / 4, F + kEtF2 / 4, lnp, vx, va, eps1, eps2, lane, nh, r1, hh, oh, r2);
    float g[32], b[32];
    et_param(lnp + 128, lane, g);
    et_param(lnp + 192, lane, b);
#pragma unroll
    for (int R = 0; R < 32; ++R) oh[R] = vx[R] + fmaf(oh[R], g[R], b[R]);
    tile_store(y, t0, T, lane, oh);
  }
}

// lane = channel: the sum of row (row0 + lane) of the wave's image over its 32 tokens, in token order
__device__ __forceinline__ float et_row_sum(const float* __restrict__ E, int row0, int lane) {
  const float* e = E + (row0 + lane) * kTilePitch;
  float s = e[0];
#pragma unroll
  for (int t = 1; t < kTile; ++t) s += e[t];
  return s;
}

// WGRAD = false: dx and da only (no exchange, no barriers, `part` unused)
template <bool WGRAD>
__global__ __launch_bounds__(kTileBwdWaves * 64) void k_et_bwd(const float* __restrict__ x, const float* __restrict__ a,
                                                               const float* __restrict__ gy, const float* __restrict__ frag,
                                                               const float* __restrict__ g1, const float* __restrict__ b1,
                                                               const float* __restrict__ g2, const float* __restrict__ b2,
                                                               int T, float eps1, float eps2, float* __restrict__ dx,
                                                               float* __restrict__ da, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float et_lds[];
  float* lnp0_ = et_lds;                                 // g1 | b1 | g2 | b2
  float* red = lnp0_ + 256;                                // [wave][dg1 | db1 | dg2 | db2][64]
  float* E = red + kTileBwdWaves * 256;                    // [wave][256 rows][kTilePitch]
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
  const int chunks = (T + kTileBwdChunk - 1) / kTileBwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kTileBwdChunk + wave * kTile;     // past T in the last chunk: a tile of zeros
    const int zero = opaque_zero();
    const float4* F = F0 + zero;
    const float* lnp = lnp0 + zero;
    float nh[32], hh[64], oh[32], dv[32], r1, r2;
    {
      float vx[32], va[32];
      tile_load(x, t0, T, lane, vx);
      tile_load(a, t0, T, lane, va);
      et_chain(F + kEtFm / 4, F + kEtF1 / 4, F + kEtF2 / 4, lnp, vx, va, eps1, eps2, lane, nh, r1, hh, oh, r2);
    }
    {                                                    // do
      float g[32], w[32];
      tile_load(gy, t0, T, lane, g);
      if (WGRAD) {
#pragma unroll
        for (int R = 0; R < 32; ++R) w[R] = g[R] * oh[R];
        tile_put<32>(Ew, 192, lane, w);
      }
      et_param(lnp + 128, lane, w);
#pragma unroll
      for (int R = 0; R < 32; ++R) g[R] *= w[R];
      et_normalize_grad(g, oh, r2, dv);
    }
    if (WGRAD) {                                         // stage 1: dW2 = do^T h, dg2, db2
      tile_put<32>(Ew, 0, lane, dv);
      tile_put<64>(Ew, 64, lane, hh);
      __syncthreads();
      tile_wgrad<2, kTileBwdWaves, kEtImage>(E, 32 * (wave >> 1), 64 + 64 * (wave & 1), lane, acc2);
      s_g2 += et_row_sum(Ew, 192, lane);
      float s = 0.f;
      for (int t = 0; t < kTile; ++t)
        if (t0 + t < (size_t)T) s += gy[(t0 + t) * 64 + lane];
      s_b2 += s;
      __syncthreads();
    }
    float dp[64];
    {
      f32x16 dh[4];
      tile_mm<4, 32>(F + kEtF2T / 4, dv, dh, lane);
      et_unpack<4>(dh, dp);
#pragma unroll
      for (int R = 0; R < 64; ++R) dp[R] = hh[R] > 0.f ? dp[R] : 0.f;
    }
    if (WGRAD) {                                         // stage 2: dW1 = dp^T c
      tile_put<64>(Ew, 0, lane, dp);
      float vx[32], c[64];                               // (x again: 32 registers less through the products between)
      tile_load(x, t0, T, lane, vx);
      et_concat(lnp, lane, vx, nh, c);
      tile_put<64>(Ew, 128, lane, c);
      __syncthreads();
      tile_wgrad<4, kTileBwdWaves, kEtImage>(E, 32 * wave, 128, lane, acc1);
      __syncthreads();
    }
    float dn[32];
    {
      f32x16 dc[4];
      tile_mm<4, 64>(F + kEtF1T / 4, dp, dc, lane);
      float g[32];
      tile_load(gy, t0, T, lane, g);
#pragma unroll
      for (int R = 0; R < 32; ++R) { g[R] += dc[R >> 4][R & 15]; dn[R] = dc[2 + (R >> 4)][R & 15]; }
      tile_store(dx, t0, T, lane, g);
    }
    float dm[32];
    {
      float w[32];
      if (WGRAD) {
        tile_put<32>(Ew, 128, lane, dn);
#pragma unroll
        for (int R = 0; R < 32; ++R) w[R] = dn[R] * nh[R];
        tile_put<32>(Ew, 192, lane, w);
      }
      et_param(lnp, lane, w);
#pragma unroll
      for (int R = 0; R < 32; ++R) dn[R] *= w[R];
      et_normalize_grad(dn, nh, r1, dm);
    }
    if (WGRAD) {                                         // stage 3: dWm = dm^T a, dg1, db1
      float va[32];
      tile_load(a, t0, T, lane, va);
      tile_put<32>(Ew, 0, lane, dm);
      tile_put<32>(Ew, 64, lane, va);
      __syncthreads();
      tile_wgrad<1, kTileBwdWaves, kEtImage>(E, 32 * (wave >> 1), 64 + 32 * (wave & 1), lane, accm);
      s_b1 += et_row_sum(Ew, 128, lane);
      s_g1 += et_row_sum(Ew, 192, lane);
      __syncthreads();
    }
    {
      f32x16 dd[2];
      tile_mm<2, 32>(F + kEtFmT / 4, dm, dd, lane);
      float w[32];
      et_unpack<2>(dd, w);
      tile_store(da, t0, T, lane, w);
    }
  }
  if (WGRAD) {
    float* slab = part + (size_t)blockIdx.x * kEtSlab;
#pragma unroll
    for (int j = 0; j < 4; ++j) tile_out(slab + kEtS1 + 32 * wave * 128 + 32 * j, 128, lane, acc1[j]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      tile_out(slab + kEtS2 + 32 * (wave >> 1) * 128 + 32 * (2 * (wave & 1) + j), 128, lane, acc2[j]);
    tile_out(slab + kEtSm + 32 * (wave >> 1) * 64 + 32 * (wave & 1), 64, lane, accm[0]);
    float* rw = red + wave * 256;
    rw[lane] = s_g1; rw[64 + lane] = s_b1; rw[128 + lane] = s_g2; rw[192 + lane] = s_b2;
    __syncthreads();
    slab[kEtSln + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];      // the waves in index order
  }
}

// the seven parameter gradients = the sum of the n_part slabs (fold_slabs' order)
struct EtGrads { float *w_merge, *ln1_w, *ln1_b, *w_mlp0, *w_mlp2, *ln2_w, *ln2_b; };
__global__ __launch_bounds__(256) void k_et_fold(const float* __restrict__ part, int n_part, EtGrads d) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, i = blockIdx.x * 32 + x;
  float v;
  if (!fold_slabs(part + i, n_part, kEtSlab, red, &v)) return;
  if (i < kEtS2) d.w_mlp0[i] = v;
  else if (i < kEtSm) d.w_mlp2[i - kEtS2] = v;
  else if (i < kEtSln) d.w_merge[i - kEtSm] = v;
  else if (i < kEtSln + 64) d.ln1_w[i - kEtSln] = v;
  else if (i < kEtSln + 128) d.ln1_b[i - kEtSln - 64] = v;
  else if (i < kEtSln + 192) d.ln2_w[i - kEtSln - 128] = v;
  else d.ln2_b[i - kEtSln - 192] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool et_route(int T, int d) { return d == 64 && T <= kTileMaxT; }
// Workspace of either call: the fragments | one slab per workgroup of the backward
struct EtWs { Region<float> frag, part; size_t total; };
static EtWs et_layout(int T) {
  EtWs w;
  Carver c;
  c.take(w.frag, kEtFrag);
  c.take(w.part, (size_t)token_groups(T, kTileBwdChunk) * kEtSlab);
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
    hipLaunchKernelGGL(k_et_fwd, dim3(token_groups(c.T, kTileFwdChunk)), dim3(kTileFwdWaves * 64), kEtFwdLds, st, c.x, c.a,
                       (const float*)frag, c.ln1_w, c.ln1_b, c.ln2_w, c.ln2_b, c.T, c.eps1, c.eps2, c.y);
    return (int)hipGetLastError();
  }
  const int groups = token_groups(c.T, kTileBwdChunk);
  float* part = w.part.in(c.workspace);
  if (wgrad) {
    static unsigned long long lds_bwd = 0;
    const hipError_t e = ensure_dynamic_lds(k_et_bwd<true>, kEtBwdLds, &lds_bwd);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_et_bwd<true>, dim3(groups), dim3(kTileBwdWaves * 64), kEtBwdLds, st, c.x, c.a, c.d_y,
                       (const float*)frag, c.ln1_w, c.ln1_b, c.ln2_w, c.ln2_b, c.T, c.eps1, c.eps2, c.d_x, c.d_a, part);
    hipLaunchKernelGGL(k_et_fold, dim3(kEtSlab / 32), dim3(256), 0, st, (const float*)part, groups, c.g);
  } else {
    hipLaunchKernelGGL(k_et_bwd<false>, dim3(groups), dim3(kTileBwdWaves * 64), 256 * 4, st, c.x, c.a, c.d_y,
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
