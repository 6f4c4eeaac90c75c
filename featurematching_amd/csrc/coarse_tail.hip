// The tail of an encoder layer at d_model = 256 (transformer.py, EncoderLayer.forward: everything behind the attention)
// and its gradient: the coarse context layers' training path.  The arithmetic is encoder_tail.hip's header with d = 256
// - Wm [256, 256], W1 [512, 512], W2 [256, 512], both LayerNorms over 256 channels, biased variance - float32
// throughout, every product on v_mfma_f32_32x32x2_f32: exact float32, one rounding per product, a k-ordered chain.
//
// The d = 64 design does not carry over: 1.75 MB of weights fit no LDS and a tile's chain fits no register file.  Here
// the C call walks T in chunks of at most kCtChunk = 8192 tokens (equal lengths, a multiple of 64) and a chunk's
// intermediates - m / nh / dm, c = [x, n1], h / dc, o / do, dp, r1: 2048 floats per token + 1 - live in the workspace,
// which is therefore bounded whatever T is.  Per chunk:
//   forward : m = a Wm^T | LN1 -> c | h = max(c W1^T, 0) | o = h W2^T | y = x + LN2(o)                       (5 launches)
//   backward: the first four again, then do (and the dg2, db2 rows) | dW2 = do^T h | dp = (do W2) [h > 0] |
//             dW1 = dp^T c | dc = dp W1 | dx, dm (and the dg1, db1 rows) | dWm = dm^T a | da = dm Wm | two folds
//             (14 launches, 9 without parameter gradients).  Nothing is kept between the two calls: the state is 0 bytes.
// k_ct_gemm is the one product kernel: a workgroup of 4 waves owns a 64 x 64 tile of the result, each wave a 32 x 32
// accumulator; panels of 32 k-steps of both operands stream through LDS (2 x 32 x 68 floats = 17 KB, the next panel's
// global loads in flight in registers while the present one is multiplied), stored k-major so that an operand read is 32
// neighbouring floats per half-wave (swizzled: ct_swz).  An operand is read either k-contiguous (activations [tokens, K], nn.Linear weights
// [N, K]) or row-contiguous (W as [K, N] for the data gradients; both operands of a weight gradient, whose k is the
// token).  A weight gradient splits the chunk's tokens in kCtSplit = 512 over blockIdx.z, one slab per split; k_ct_fold
// adds the slabs in fold_slabs' order and, from the second chunk on, adds that to what the gradient holds: kernels of
// one stream, a fixed order.  The LayerNorm kernels take a token per wave (4 channels per lane) and 64 tokens per
// workgroup; their per-channel sums go to one row per workgroup and through the same fold.
// Occupancy: k_ct_gemm takes 17 KB of LDS and under 64 registers, so a CU holds 8 workgroups (8 waves per SIMD, the
// limit) and the barriers of one hide behind the products of the others; a chunk of 8192 tokens is 512 to 1024 tiles.
// No atomics, grids that depend on T alone, fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

constexpr int kCtD = 256, kCtH = 512;
constexpr int kCtChunk = 8192;                   // tokens of a chunk, at most
constexpr int kCtSplit = 512;                    // tokens of one slab of a weight gradient
constexpr int kCtLnTok = 64;                     // tokens of a LayerNorm workgroup: 4 waves x 16
constexpr int kCtBM = 64, kCtBK = 32, kCtPitch = 68;     // the result tile's edge, k-steps of a panel, floats of a panel row
constexpr int kCtMaxT = 1 << 24;
// a slab of partial weight gradients, in floats: dW1 | dW2 | dWm; a row of partial LayerNorm gradients: dg1 | db1 | dg2 | db2
constexpr int kCtS1 = 0, kCtS2 = kCtH * kCtH, kCtSm = kCtS2 + kCtD * kCtH, kCtSlab = kCtSm + kCtD * kCtD;
constexpr int kCtLnRow = 4 * kCtD;
static_assert(kCtChunk % kCtSplit == 0 && kCtSplit % kCtBK == 0 && kCtChunk % kCtLnTok == 0, "whole splits, panels and rows");
static_assert(kCtSlab % 32 == 0 && kCtLnRow % 32 == 0, "k_ct_fold's grid covers a slab exactly");

struct CtGemm {
  const float *A, *B, *aux; float* C;
  int M, N, K, lda, ldb, ldc, kz; size_t cz;     // split z: k in [z kz, (z + 1) kz), written to C + z cz
};

// one thread's two 16-byte pieces of a 64 x 32 panel.  KC: element (r, k) at src[r ld + k], the k range a multiple of 32,
// rows beyond `rows` read as 0; else at src[k ld + r], `rows` a multiple of 64, k beyond kend reads as 0
struct CtPiece { float4 v[2]; };
template <bool KC>
__device__ __forceinline__ CtPiece ct_fetch(const float* __restrict__ src, int ld, int r0, int rows, int k0, int kend, int tid) {
  CtPiece p;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    p.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KC) {
      const int r = r0 + (idx >> 3), k = k0 + 4 * (idx & 7);
      if (r < rows && k < kend) p.v[j] = *reinterpret_cast<const float4*>(src + (size_t)r * ld + k);
    } else {
      const int k = k0 + (idx >> 4), r = r0 + 4 * (idx & 15);
      if (k < kend && r < rows) p.v[j] = *reinterpret_cast<const float4*>(src + (size_t)k * ld + r);
    }
  }
  return p;
}
// ... into the panel S[k][r ^ ct_swz(k)].  The swizzle moves a row by 0, 8, 16 or 24 columns inside its aligned 32: an
// operand read (one k, 32 neighbouring rows) stays a permutation of the 32 banks, a 16-byte piece stays whole, and the
// transposing stores of a wave (8 rows x 8 pieces, k = 4 piece + i) fall on every bank twice instead of on 16 banks four
// times (bank = 16 (piece & 1) + 8 ((row >> 3) ^ (piece >> 1)) + (row & 7) + 4 i mod 32).
__device__ __forceinline__ int ct_swz(int k) { return 8 * ((k >> 3) & 3); }
template <bool KC>
__device__ __forceinline__ void ct_stash(float* __restrict__ S, const CtPiece& p, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    const float4 v = p.v[j];
    if (KC) {
      float* s = S + 4 * (idx & 7) * kCtPitch + ((idx >> 3) ^ ct_swz(4 * (idx & 7)));
      s[0] = v.x; s[kCtPitch] = v.y; s[2 * kCtPitch] = v.z; s[3 * kCtPitch] = v.w;
    } else {
      *reinterpret_cast<float4*>(S + (idx >> 4) * kCtPitch + ((4 * (idx & 15)) ^ ct_swz(idx >> 4))) = v;
    }
  }
}

// C [M, N] = A B over the split's k range, A (m, k) and B (k, n) read as AK / BK say.  EPI 1: max(., 0); EPI 2: zeroed
// where aux (C's shape and pitch) is not > 0.
template <bool AK, bool BK, int EPI>
__global__ __launch_bounds__(256) void k_ct_gemm(CtGemm g) {
  __shared__ __attribute__((aligned(16))) float As[kCtBK * kCtPitch];
  __shared__ __attribute__((aligned(16))) float Bs[kCtBK * kCtPitch];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.y * kCtBM, n0 = blockIdx.x * kCtBM;
  const int kbeg = blockIdx.z * g.kz, kend = min(g.K, kbeg + g.kz);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  CtPiece ra = ct_fetch<AK>(g.A, g.lda, m0, g.M, kbeg, kend, tid);
  CtPiece rb = ct_fetch<BK>(g.B, g.ldb, n0, g.N, kbeg, kend, tid);
  int ao[4], bo[4];                               // per swizzle of the panel's four groups of 8 k-steps
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    ao[v] = (lane >> 5) * kCtPitch + ((32 * (wave >> 1) + (lane & 31)) ^ (8 * v));
    bo[v] = (lane >> 5) * kCtPitch + ((32 * (wave & 1) + (lane & 31)) ^ (8 * v));
  }
  for (int k0 = kbeg; k0 < kend; k0 += kCtBK) {
    ct_stash<AK>(As, ra, tid);
    ct_stash<BK>(Bs, rb, tid);
    __syncthreads();
    if (k0 + kCtBK < kend) {
      ra = ct_fetch<AK>(g.A, g.lda, m0, g.M, k0 + kCtBK, kend, tid);
      rb = ct_fetch<BK>(g.B, g.ldb, n0, g.N, k0 + kCtBK, kend, tid);
    }
#pragma unroll
    for (int kk = 0; kk < kCtBK; kk += 2) {
      const float va = As[ao[(kk >> 3) & 3] + kk * kCtPitch], vb = Bs[bo[(kk >> 3) & 3] + kk * kCtPitch];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va, vb, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  float* C = g.C + (size_t)blockIdx.z * g.cz;
  const int col = n0 + 32 * (wave & 1) + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + 32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row >= g.M) continue;
    const size_t at = (size_t)row * g.ldc + col;
    float v = acc[r];
    if (EPI == 1) v = fmaxf(v, 0.f);
    if (EPI == 2) v = g.aux[at] > 0.f ? v : 0.f;
    C[at] = v;
  }
}

__device__ __forceinline__ float ct_sum4(const float4& v) { return wave_sum((v.x + v.y) + (v.z + v.w)); }
// v <- (v - mean) r over the wave's 256 channels, r = 1 / sqrt(var + eps) returned
__device__ __forceinline__ float ct_normalize(float4& v, float eps) {
  const float mean = ct_sum4(v) * (1.f / kCtD);
  v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
  const float r = 1.f / sqrtf(ct_sum4(make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w)) * (1.f / kCtD) + eps);
  v.x *= r; v.y *= r; v.z *= r; v.w *= r;
  return r;
}
// r (d - mean(d) - nh mean(d nh)): the gradient through (v - mean) r given d = the gradient of nh
__device__ __forceinline__ float4 ct_normalize_grad(const float4& d, const float4& nh, float r) {
  const float m1 = ct_sum4(d) * (1.f / kCtD);
  const float m2 = ct_sum4(make_float4(d.x * nh.x, d.y * nh.y, d.z * nh.z, d.w * nh.w)) * (1.f / kCtD);
  return make_float4(r * (d.x - m1 - nh.x * m2), r * (d.y - m1 - nh.y * m2), r * (d.z - m1 - nh.z * m2),
                     r * (d.w - m1 - nh.w * m2));
}
__device__ __forceinline__ float4 ct_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void ct_st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void ct_acc(float4& s, const float4& u, const float4& v) {
  s.x += u.x * v.x; s.y += u.y * v.y; s.z += u.z * v.z; s.w += u.w * v.w;
}
// the workgroup's row of two per-channel sums: the waves in index order -> row[0 .. 256) = s0, row[256 .. 512) = s1
__device__ __forceinline__ void ct_row_out(float (&red)[4][2 * kCtD], const float4& s0, const float4& s1, float* __restrict__ row) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  ct_st4(&red[wave][4 * lane], s0);
  ct_st4(&red[wave][kCtD + 4 * lane], s1);
  __syncthreads();
  for (int i = tid; i < 2 * kCtD; i += 256) row[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// m [n, 256] -> nh in place (KEEP; with r1 [n]), c [n, 512] = [x, nh g1 + b1]
template <bool KEEP>
__global__ __launch_bounds__(256) void k_ct_ln1(float* m, const float* __restrict__ x, const float* __restrict__ g1,
                                                const float* __restrict__ b1, int n, float eps, float* __restrict__ c,
                                                float* __restrict__ r1) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4 g = ct_ld4(g1 + 4 * lane), b = ct_ld4(b1 + 4 * lane);
  for (int i = 0; i < kCtLnTok / 4; ++i) {
    const int t = blockIdx.x * kCtLnTok + wave * (kCtLnTok / 4) + i;
    if (t >= n) break;
    float4 v = ct_ld4(m + (size_t)t * kCtD + 4 * lane);
    const float r = ct_normalize(v, eps);
    if (KEEP) {
      ct_st4(m + (size_t)t * kCtD + 4 * lane, v);
      if (lane == 0) r1[t] = r;
    }
    ct_st4(c + (size_t)t * kCtH + 4 * lane, ct_ld4(x + (size_t)t * kCtD + 4 * lane));
    ct_st4(c + (size_t)t * kCtH + kCtD + 4 * lane,
           make_float4(fmaf(v.x, g.x, b.x), fmaf(v.y, g.y, b.y), fmaf(v.z, g.z, b.z), fmaf(v.w, g.w, b.w)));
  }
}

// y = x + LN2(o) g2 + b2
__global__ __launch_bounds__(256) void k_ct_ln2_fwd(const float* __restrict__ o, const float* __restrict__ x,
                                                    const float* __restrict__ g2, const float* __restrict__ b2, int n,
                                                    float eps, float* __restrict__ y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4 g = ct_ld4(g2 + 4 * lane), b = ct_ld4(b2 + 4 * lane);
  for (int i = 0; i < kCtLnTok / 4; ++i) {
    const int t = blockIdx.x * kCtLnTok + wave * (kCtLnTok / 4) + i;
    if (t >= n) break;
    float4 v = ct_ld4(o + (size_t)t * kCtD + 4 * lane);
    ct_normalize(v, eps);
    const float4 xv = ct_ld4(x + (size_t)t * kCtD + 4 * lane);
    ct_st4(y + (size_t)t * kCtD + 4 * lane, make_float4(xv.x + fmaf(v.x, g.x, b.x), xv.y + fmaf(v.y, g.y, b.y),
                                                       xv.z + fmaf(v.z, g.z, b.z), xv.w + fmaf(v.w, g.w, b.w)));
  }
}

// o [n, 256] -> do in place; WGRAD: the workgroup's sums of gy oh and gy into rows[blockIdx.x][dg2 | db2]
template <bool WGRAD>
__global__ __launch_bounds__(256) void k_ct_ln2_bwd(float* o, const float* __restrict__ gy, const float* __restrict__ g2,
                                                    int n, float eps, float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float red[4][2 * kCtD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4 g = ct_ld4(g2 + 4 * lane);
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sb = sg;
  for (int i = 0; i < kCtLnTok / 4; ++i) {
    const int t = blockIdx.x * kCtLnTok + wave * (kCtLnTok / 4) + i;
    if (t >= n) break;
    float4 oh = ct_ld4(o + (size_t)t * kCtD + 4 * lane);
    const float r = ct_normalize(oh, eps);
    const float4 d = ct_ld4(gy + (size_t)t * kCtD + 4 * lane);
    ct_acc(sg, d, oh);
    sb.x += d.x; sb.y += d.y; sb.z += d.z; sb.w += d.w;
    ct_st4(o + (size_t)t * kCtD + 4 * lane, ct_normalize_grad(make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w), oh, r));
  }
  if (WGRAD) ct_row_out(red, sg, sb, rows + (size_t)blockIdx.x * kCtLnRow + 2 * kCtD);
}

// dc [n, 512], gy, nh = m [n, 256], r1 -> dx = gy + dc[:, :256]; dm in place of nh from dn1 = dc[:, 256:]; WGRAD: the
// workgroup's sums of dn1 nh and dn1 into rows[blockIdx.x][dg1 | db1]
template <bool WGRAD>
__global__ __launch_bounds__(256) void k_ct_ln1_bwd(const float* __restrict__ dc, const float* __restrict__ gy, float* m,
                                                    const float* __restrict__ r1, const float* __restrict__ g1, int n,
                                                    float* __restrict__ dx, float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float red[4][2 * kCtD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4 g = ct_ld4(g1 + 4 * lane);
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sb = sg;
  for (int i = 0; i < kCtLnTok / 4; ++i) {
    const int t = blockIdx.x * kCtLnTok + wave * (kCtLnTok / 4) + i;
    if (t >= n) break;
    const float4 d0 = ct_ld4(dc + (size_t)t * kCtH + 4 * lane), dn = ct_ld4(dc + (size_t)t * kCtH + kCtD + 4 * lane);
    const float4 gv = ct_ld4(gy + (size_t)t * kCtD + 4 * lane);
    ct_st4(dx + (size_t)t * kCtD + 4 * lane, make_float4(gv.x + d0.x, gv.y + d0.y, gv.z + d0.z, gv.w + d0.w));
    const float4 nh = ct_ld4(m + (size_t)t * kCtD + 4 * lane);
    ct_acc(sg, dn, nh);
    sb.x += dn.x; sb.y += dn.y; sb.z += dn.z; sb.w += dn.w;
    ct_st4(m + (size_t)t * kCtD + 4 * lane,
           ct_normalize_grad(make_float4(dn.x * g.x, dn.y * g.y, dn.z * g.z, dn.w * g.w), nh, r1[t]));
  }
  if (WGRAD) ct_row_out(red, sg, sb, rows + (size_t)blockIdx.x * kCtLnRow);
}

// entries [end[s - 1], end[s]) of a slab belong to dst[s]: dst = (the sum of the n_part slabs, fold_slabs' order)
// (+ what dst holds, if add)
struct CtFold { float* dst[4]; int end[4]; };
__global__ __launch_bounds__(256) void k_ct_fold(const float* __restrict__ part, int n_part, int slab_floats, CtFold f, bool add) {
  __shared__ float red[8][32];
  const int i = blockIdx.x * 32 + (threadIdx.x & 31);
  float v;
  if (!fold_slabs(part + i, n_part, slab_floats, red, &v)) return;
  float* d = i < f.end[0] ? f.dst[0] + i : i < f.end[1] ? f.dst[1] + (i - f.end[0])
           : i < f.end[2] ? f.dst[2] + (i - f.end[1]) : f.dst[3] + (i - f.end[2]);
  *d = add ? *d + v : v;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool ct_route(int T, int d) { return d == kCtD && T <= kCtMaxT; }
// tokens of a chunk: T in equal parts of at most kCtChunk, rounded up to the LayerNorm workgroups' 64
static int ct_chunk_len(int T) {
  const int n = (T + kCtChunk - 1) / kCtChunk;
  return round_up((T + n - 1) / n, kCtLnTok);
}
// Workspace of either call: one chunk's intermediates | the slabs of its weight gradients | its LayerNorm rows
struct CtWs { Region<float> m, c, h, o, dp, r1, slab, rows; size_t total; };
static CtWs ct_layout(int T) {
  const size_t n = T > kCtChunk ? kCtChunk : round_up(T, kCtLnTok);
  CtWs w;
  Carver c;
  c.take(w.m, n * kCtD);
  c.take(w.c, n * kCtH);
  c.take(w.h, n * kCtH);
  c.take(w.o, n * kCtD);
  c.take(w.dp, n * kCtH);
  c.take(w.r1, n);
  c.take(w.slab, (n + kCtSplit - 1) / kCtSplit * kCtSlab);
  c.take(w.rows, n / kCtLnTok * kCtLnRow);
  w.total = c.pad();
  return w;
}

struct CtGrads { float *w_merge, *ln1_w, *ln1_b, *w_mlp0, *w_mlp2, *ln2_w, *ln2_b; };
// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct CtCall {
  const float *x, *a, *w_merge, *ln1_w, *ln1_b, *w_mlp0, *w_mlp2, *ln2_w, *ln2_b;
  int T, d; float eps1, eps2;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float* y;                                        // forward
  const float* d_y; float *d_x, *d_a; CtGrads g;   // backward
};

// the ONLY copy of the two entry points' argument checks; *wgrad is set with FM_OK.  (No state is kept: the state
// pointers are never looked at.)
static int ct_status(const CtCall& c, bool* wgrad) {
  if (!c.x || !c.a || !c.w_merge || !c.ln1_w || !c.ln1_b || !c.w_mlp0 || !c.w_mlp2 || !c.ln2_w || !c.ln2_b) return FM_E_NULL;
  if (c.backward ? (!c.d_y || !c.d_x || !c.d_a) : !c.y) return FM_E_NULL;
  const int given = !!c.g.w_merge + !!c.g.ln1_w + !!c.g.ln1_b + !!c.g.w_mlp0 + !!c.g.w_mlp2 + !!c.g.ln2_w + !!c.g.ln2_b;
  if (given != 0 && given != 7) return FM_E_NULL;
  if (c.T <= 0 || c.d <= 0) return FM_E_SHAPE;
  if (!ct_route(c.T, c.d) || !(c.eps1 > 0.f) || !(c.eps2 > 0.f)) return FM_E_UNSUPPORTED;
  if (!c.workspace || !workspace_ok(c.workspace, c.workspace_bytes, ct_layout(c.T).total)) return FM_E_WORKSPACE;
  *wgrad = given == 7;
  return FM_OK;
}

// C [M, N] (pitch ldc) = A B; kz < K: one slab of cz floats per kz k-steps
template <bool AK, bool BK, int EPI>
static void ct_gemm(hipStream_t st, const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* aux,
                    int M, int N, int K, int kz, size_t cz) {
  const CtGemm g = {A, B, aux, C, M, N, K, lda, ldb, ldc, kz, cz};
  hipLaunchKernelGGL((k_ct_gemm<AK, BK, EPI>), dim3(N / kCtBM, (M + kCtBM - 1) / kCtBM, (K + kz - 1) / kz), dim3(256), 0, st, g);
}
// the three forms: X [n, K] W^T with W [N, K];  X [n, K] W with W [K, N];  U^T V over the n tokens, U [n, M], V [n, N]
template <int EPI>
static void ct_linear(hipStream_t st, const float* X, const float* W, float* Y, const float* aux, int n, int N, int K) {
  ct_gemm<true, true, EPI>(st, X, K, W, K, Y, N, aux, n, N, K, K, 0);
}
template <int EPI>
static void ct_linear_t(hipStream_t st, const float* X, const float* W, float* Y, const float* aux, int n, int N, int K) {
  ct_gemm<true, false, EPI>(st, X, K, W, N, Y, N, aux, n, N, K, K, 0);
}
static void ct_wgrad(hipStream_t st, const float* U, const float* V, float* slab, int n, int M, int N) {
  ct_gemm<false, false, 0>(st, U, M, V, N, slab, N, nullptr, M, N, n, kCtSplit, kCtSlab);
}

static int ct_run(const CtCall& c) {
  bool wgrad = false;
  const int status = ct_status(c, &wgrad);
  if (status != FM_OK) return status;
  hipStream_t st = (hipStream_t)c.stream;
  const CtWs w = ct_layout(c.T);
  float *m = w.m.in(c.workspace), *cc = w.c.in(c.workspace), *h = w.h.in(c.workspace), *o = w.o.in(c.workspace);
  float *dp = w.dp.in(c.workspace), *r1 = w.r1.in(c.workspace), *slab = w.slab.in(c.workspace), *rows = w.rows.in(c.workspace);
  const int len = ct_chunk_len(c.T);
  for (int t0 = 0; t0 < c.T; t0 += len) {
    const int n = c.T - t0 < len ? c.T - t0 : len, groups = (n + kCtLnTok - 1) / kCtLnTok;
    const size_t at = (size_t)t0 * kCtD;
    const float *x = c.x + at, *a = c.a + at;
    ct_linear<0>(st, a, c.w_merge, m, nullptr, n, kCtD, kCtD);
    if (c.backward) hipLaunchKernelGGL(k_ct_ln1<true>, dim3(groups), dim3(256), 0, st, m, x, c.ln1_w, c.ln1_b, n, c.eps1, cc, r1);
    else hipLaunchKernelGGL(k_ct_ln1<false>, dim3(groups), dim3(256), 0, st, m, x, c.ln1_w, c.ln1_b, n, c.eps1, cc, r1);
    ct_linear<1>(st, cc, c.w_mlp0, h, nullptr, n, kCtH, kCtH);
    ct_linear<0>(st, h, c.w_mlp2, o, nullptr, n, kCtD, kCtH);
    if (!c.backward) {
      hipLaunchKernelGGL(k_ct_ln2_fwd, dim3(groups), dim3(256), 0, st, (const float*)o, x, c.ln2_w, c.ln2_b, n, c.eps2, c.y + at);
      continue;
    }
    const float* gy = c.d_y + at;
    if (wgrad) {
      hipLaunchKernelGGL(k_ct_ln2_bwd<true>, dim3(groups), dim3(256), 0, st, o, gy, c.ln2_w, n, c.eps2, rows);
      ct_wgrad(st, o, h, slab + kCtS2, n, kCtD, kCtH);
    } else {
      hipLaunchKernelGGL(k_ct_ln2_bwd<false>, dim3(groups), dim3(256), 0, st, o, gy, c.ln2_w, n, c.eps2, rows);
    }
    ct_linear_t<2>(st, o, c.w_mlp2, dp, h, n, kCtH, kCtD);
    if (wgrad) ct_wgrad(st, dp, cc, slab + kCtS1, n, kCtH, kCtH);
    ct_linear_t<0>(st, dp, c.w_mlp0, h, nullptr, n, kCtH, kCtH);            // dc, where h was
    if (wgrad) {
      hipLaunchKernelGGL(k_ct_ln1_bwd<true>, dim3(groups), dim3(256), 0, st, (const float*)h, gy, m, (const float*)r1, c.ln1_w, n,
                         c.d_x + at, rows);
      ct_wgrad(st, m, a, slab + kCtSm, n, kCtD, kCtD);
    } else {
      hipLaunchKernelGGL(k_ct_ln1_bwd<false>, dim3(groups), dim3(256), 0, st, (const float*)h, gy, m, (const float*)r1, c.ln1_w, n,
                         c.d_x + at, rows);
    }
    ct_linear_t<0>(st, m, c.w_merge, c.d_a + at, nullptr, n, kCtD, kCtD);
    if (wgrad) {
      const CtFold fw = {{c.g.w_mlp0, c.g.w_mlp2, c.g.w_merge, nullptr}, {kCtS2, kCtSm, kCtSlab, kCtSlab}};
      const CtFold fl = {{c.g.ln1_w, c.g.ln1_b, c.g.ln2_w, c.g.ln2_b}, {kCtD, 2 * kCtD, 3 * kCtD, 4 * kCtD}};
      hipLaunchKernelGGL(k_ct_fold, dim3(kCtSlab / 32), dim3(256), 0, st, (const float*)slab, (n + kCtSplit - 1) / kCtSplit,
                         kCtSlab, fw, t0 > 0);
      hipLaunchKernelGGL(k_ct_fold, dim3(kCtLnRow / 32), dim3(256), 0, st, (const float*)rows, groups, kCtLnRow, fl, t0 > 0);
    }
  }
  return (int)hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_coarse_tail_state_bytes(int T, int d) {
  (void)T; (void)d;
  return 0;                                        // the backward recomputes the chain: nothing is kept
}

extern "C" size_t fm_coarse_tail_workspace_bytes(int T, int d) {
  if (T <= 0 || d <= 0 || !ct_route(T, d)) return 0;
  return ct_layout(T).total;
}

extern "C" int fm_coarse_tail_forward(const float* x, const float* a, const float* w_merge, const float* ln1_w,
                                      const float* ln1_b, const float* w_mlp0, const float* w_mlp2, const float* ln2_w,
                                      const float* ln2_b, int T, int d, float eps1, float eps2, void* workspace,
                                      size_t workspace_bytes, float* state, float* y, void* stream) {
  (void)state;
  CtCall c = {};
  c.x = x; c.a = a; c.w_merge = w_merge; c.ln1_w = ln1_w; c.ln1_b = ln1_b; c.w_mlp0 = w_mlp0; c.w_mlp2 = w_mlp2;
  c.ln2_w = ln2_w; c.ln2_b = ln2_b;
  c.T = T; c.d = d; c.eps1 = eps1; c.eps2 = eps2;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.y = y;
  return ct_run(c);
}

extern "C" int fm_coarse_tail_backward(const float* x, const float* a, const float* w_merge, const float* ln1_w,
                                       const float* ln1_b, const float* w_mlp0, const float* w_mlp2, const float* ln2_w,
                                       const float* ln2_b, const float* d_y, const float* state, int T, int d, float eps1,
                                       float eps2, void* workspace, size_t workspace_bytes, float* d_x, float* d_a,
                                       float* d_w_merge, float* d_ln1_w, float* d_ln1_b, float* d_w_mlp0, float* d_w_mlp2,
                                       float* d_ln2_w, float* d_ln2_b, void* stream) {
  (void)state;
  CtCall c = {};
  c.x = x; c.a = a; c.w_merge = w_merge; c.ln1_w = ln1_w; c.ln1_b = ln1_b; c.w_mlp0 = w_mlp0; c.w_mlp2 = w_mlp2;
  c.ln2_w = ln2_w; c.ln2_b = ln2_b;
  c.T = T; c.d = d; c.eps1 = eps1; c.eps2 = eps2;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.d_y = d_y; c.d_x = d_x; c.d_a = d_a;
  c.g = {d_w_merge, d_ln1_w, d_ln1_b, d_w_mlp0, d_w_mlp2, d_ln2_w, d_ln2_b};
  return ct_run(c);
}
