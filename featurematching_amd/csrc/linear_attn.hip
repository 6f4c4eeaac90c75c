// Linear attention with the elu(x) + 1 feature map ("Transformers are RNNs"; the reference's LinearAttention,
// network/module/attentions.py:19-46) and its gradient: the attention core of the context layers' training path
// (transformer.py, `linear_attention`).  float32 on plain FMAs; the work is one read of q, k, v and one write of the result.
//
// Per sample n and head h, phi(x) = x + 1 for x > 0, else exp(x); Q = phi(q) qm, K = phi(k) km, V = v km:
//     A[d][v] = sum_s K[s][d] V[s][v]      Ksum[d] = sum_s K[s][d]
//     Z_l = 1 / (Q_l . Ksum + eps)         out[l][v] = Z_l sum_d Q[l][d] A[d][v]
// and with g = d out:
//     t_l[d]  = sum_v A[d][v] g[l][v]                  dden_l = -Z_l^2 sum_d Q[l][d] t_l[d]     (= -Z_l g_l . out_l)
//     dQ[l][d] = Z_l t_l[d] + dden_l Ksum[d]
//     dA[d][v] = sum_l Q[l][d] Z_l g[l][v]             dKsum[d] = sum_l dden_l Q[l][d]
//     dK[s][d] = sum_v dA[d][v] V[s][v] + dKsum[d]     dV[s][v] = sum_d K[s][d] dA[d][v]
//     dq = dQ phi'(q) qm,  dk = dK phi'(k) km,  dv = dV km;   phi'(x) qm = (P > 1 ? 1 : P) for P = phi(x) qm
// (the reference divides V by S before the sum and multiplies by S after it: a float16 precaution, dropped here).
//
// Two routes (la_route), both with 8 heads:
//   window (D = 8, L, S <= 64: the fine level's [M, 25 | 49, 64]): one wave per sequence, lane = channel = (h, c).  The
//     sequence's rows are staged in LDS once; a lane reads its head's 8-float rows as broadcasts (all lanes of an
//     instruction read ONE row, the 8 heads 8 disjoint bank ranges: no conflict at the plain pitch of 64 floats) and
//     keeps column c of A - in the backward also row c, of A and of dA - in registers.  k_la_win_fwd, one launch;
//     k_la_win_bwd, one launch, recomputes A and Ksum: no state, no workspace.
//   long (D = 32, any L, S: the coarse level's [N, 4800, 256]): 256 threads = 256 channels, work units of kLaUnit rows
//     dealt round-robin over at most kLaMaxUnits workgroups per sample, kLaTile rows in LDS at a time.
//     forward : k_la_kv_part (per-workgroup partials of A | Ksum) -> k_la_fold (in a fixed order; = the call's state)
//               -> k_la_out
//     backward: k_la_bwd_q (dq and per-workgroup partials of dA | dKsum) -> k_la_fold -> k_la_bwd_kv (dk, dv)
//     A slab is [8][33][32] floats per sample: rows 0..31 of a head the matrix, row 32 the vector.
// No atomics: every sum has one owner and a fixed order, so every output is the same bits on every run.
#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

constexpr int kLaWinMax = 64;         // tokens of a window-route sequence
constexpr int kLaWinGrid = 2048;      // workgroups of a window launch (the rest by grid stride)
constexpr int kLaUnit = 32;           // rows of a long-route work unit
constexpr int kLaTile = 16;           // rows staged in LDS at a time
constexpr int kLaMaxUnits = 256;      // workgroups per sample on the long route
constexpr int kLaSlab = 8 * 33 * 32;  // floats of A | Ksum (or dA | dKsum) of one sample
static_assert(kLaUnit % kLaTile == 0 && kLaSlab % 32 == 0, "tiles fill a unit; k_la_fold's grid covers a slab exactly");

__device__ __forceinline__ float la_phi(float x) { return x > 0.f ? x + 1.f : expf(x); }
// phi'(x) * mask from P = phi(x) * mask: P > 1 only on the linear branch; on the other phi' = phi (P = 1: both are 1)
__device__ __forceinline__ float la_dphi(float P) { return P > 1.f ? 1.f : P; }
__device__ __forceinline__ bool la_keep(const unsigned char* __restrict__ mask, size_t at) { return !mask || mask[at] != 0; }

__device__ __forceinline__ float dot8(const float4& a0, const float4& a1, const float (&b)[8]) {
  float s = a0.x * b[0];
  s = fmaf(a0.y, b[1], s); s = fmaf(a0.z, b[2], s); s = fmaf(a0.w, b[3], s);
  s = fmaf(a1.x, b[4], s); s = fmaf(a1.y, b[5], s); s = fmaf(a1.z, b[6], s); s = fmaf(a1.w, b[7], s);
  return s;
}
// acc[i] += row[i] * x
__device__ __forceinline__ void axpy8(float (&acc)[8], const float4& r0, const float4& r1, float x) {
  acc[0] = fmaf(r0.x, x, acc[0]); acc[1] = fmaf(r0.y, x, acc[1]); acc[2] = fmaf(r0.z, x, acc[2]); acc[3] = fmaf(r0.w, x, acc[3]);
  acc[4] = fmaf(r1.x, x, acc[4]); acc[5] = fmaf(r1.y, x, acc[5]); acc[6] = fmaf(r1.z, x, acc[6]); acc[7] = fmaf(r1.w, x, acc[7]);
}
// sum over the 8 lanes of a head (lane ^ 1, ^ 2, ^ 4), the same bits in all 8
__device__ __forceinline__ float head_sum8(float v) {
  v = pair_op<1, OpAdd>(v); v = pair_op<2, OpAdd>(v); v = pair_op<4, OpAdd>(v);
  return v;
}

// ---- window route -------------------------------------------------------------------------------------------------
// rows [R][64] of one tensor of sequence n into LDS: PHI = phi and mask (q, k), else mask only (v, g: g unmasked).
// The R * 64 floats are contiguous: 16 bytes per lane and instruction, all 16 loads (R <= 64) issued before the first
// use - a sequence's waves are few (LDS bounds them), so the bytes in flight per wave are what hides the memory latency.
template <bool PHI>
__device__ __forceinline__ void la_win_stage(float* __restrict__ dst, const float* __restrict__ src,
                                             const unsigned char* __restrict__ mask, size_t n, int R, int lane) {
  const float4* p = reinterpret_cast<const float4*>(src + n * R * 64);
  float4 x[kLaWinMax / 4];
#pragma unroll
  for (int i = 0; i < kLaWinMax / 4; ++i) {
    const int at = i * 64 + lane;                  // float4 index: row at >> 4
    x[i] = at < R * 16 ? p[at] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < kLaWinMax / 4; ++i) {
    const int at = i * 64 + lane;
    if (at < R * 16) {
      float4 y = x[i];
      if (PHI) y = make_float4(la_phi(y.x), la_phi(y.y), la_phi(y.z), la_phi(y.w));
      if (!la_keep(mask, n * R + (at >> 4))) y = make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4*>(dst)[at] = y;
    }
  }
}

__global__ __launch_bounds__(64) void k_la_win_fwd(const float* __restrict__ q, const float* __restrict__ k,
                                                   const float* __restrict__ v, const unsigned char* __restrict__ qm,
                                                   const unsigned char* __restrict__ km, int N, int L, int S, float eps,
                                                   float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float* Ks = la_lds;                    // [S][64]
  float* Vs = Ks + S * 64;               // [S][64]
  float* Qs = Vs + S * 64;               // [L][64]
  const int lane = threadIdx.x, hb = lane & ~7;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    la_win_stage<true>(Ks, k, km, n, S, lane);
    la_win_stage<false>(Vs, v, km, n, S, lane);
    la_win_stage<true>(Qs, q, qm, n, L, lane);
    __syncthreads();
    float Ac[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, Ksum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int s = 0; s < S; ++s) {
      const float4 k0 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb), k1 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb + 4);
      axpy8(Ac, k0, k1, Vs[s * 64 + lane]);
      axpy8(Ksum, k0, k1, 1.f);
    }
    float* o = out + (size_t)n * L * 64 + lane;
#pragma unroll 2
    for (int l = 0; l < L; ++l) {
      const float4 q0 = *reinterpret_cast<const float4*>(Qs + l * 64 + hb), q1 = *reinterpret_cast<const float4*>(Qs + l * 64 + hb + 4);
      const float z = 1.f / (dot8(q0, q1, Ksum) + eps);
      o[(size_t)l * 64] = dot8(q0, q1, Ac) * z;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_la_win_bwd(const float* __restrict__ q, const float* __restrict__ k,
                                                   const float* __restrict__ v, const unsigned char* __restrict__ qm,
                                                   const unsigned char* __restrict__ km, const float* __restrict__ g, int N,
                                                   int L, int S, float eps, float* __restrict__ dq, float* __restrict__ dk,
                                                   float* __restrict__ dv) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float* Ks = la_lds;                    // [S][64]
  float* Vs = Ks + S * 64;               // [S][64]
  float* Qs = Vs + S * 64;               // [L][64]
  float* Gs = Qs + L * 64;               // [L][64]
  const int lane = threadIdx.x, hb = lane & ~7;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    la_win_stage<true>(Ks, k, km, n, S, lane);
    la_win_stage<false>(Vs, v, km, n, S, lane);
    la_win_stage<true>(Qs, q, qm, n, L, lane);
    la_win_stage<false>(Gs, g, nullptr, n, L, lane);
    __syncthreads();
    // column c and row c of A, Ksum of the head and this lane's own entry of it
    float Ac[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, Ar[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float Ksum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ks = 0.f;
#pragma unroll 2
    for (int s = 0; s < S; ++s) {
      const float4 k0 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb), k1 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb + 4);
      const float4 v0 = *reinterpret_cast<const float4*>(Vs + s * 64 + hb), v1 = *reinterpret_cast<const float4*>(Vs + s * 64 + hb + 4);
      const float ko = Ks[s * 64 + lane];
      axpy8(Ac, k0, k1, Vs[s * 64 + lane]);
      axpy8(Ar, v0, v1, ko);
      axpy8(Ksum, k0, k1, 1.f);
      ks += ko;
    }
    // the pass over the queries: dq, and row c / column c of dA and this lane's dKsum
    float dAr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dAc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dks = 0.f;
    float* oq = dq + (size_t)n * L * 64 + lane;
    for (int l = 0; l < L; ++l) {
      const float4 q0 = *reinterpret_cast<const float4*>(Qs + l * 64 + hb), q1 = *reinterpret_cast<const float4*>(Qs + l * 64 + hb + 4);
      const float4 g0 = *reinterpret_cast<const float4*>(Gs + l * 64 + hb), g1 = *reinterpret_cast<const float4*>(Gs + l * 64 + hb + 4);
      const float qo = Qs[l * 64 + lane], go = Gs[l * 64 + lane];
      const float z = 1.f / (dot8(q0, q1, Ksum) + eps);
      const float t = dot8(g0, g1, Ar);
      const float dden = -z * z * head_sum8(qo * t);
      oq[(size_t)l * 64] = (z * t + dden * ks) * la_dphi(qo);
      axpy8(dAr, g0, g1, qo * z);
      axpy8(dAc, q0, q1, go * z);
      dks = fmaf(dden, qo, dks);
    }
    float* ok = dk + (size_t)n * S * 64 + lane;
    float* ov = dv + (size_t)n * S * 64 + lane;
#pragma unroll 2
    for (int s = 0; s < S; ++s) {
      const float4 k0 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb), k1 = *reinterpret_cast<const float4*>(Ks + s * 64 + hb + 4);
      const float4 v0 = *reinterpret_cast<const float4*>(Vs + s * 64 + hb), v1 = *reinterpret_cast<const float4*>(Vs + s * 64 + hb + 4);
      ok[(size_t)s * 64] = (dot8(v0, v1, dAr) + dks) * la_dphi(Ks[s * 64 + lane]);
      ov[(size_t)s * 64] = la_keep(km, (size_t)n * S + s) ? dot8(k0, k1, dAc) : 0.f;
    }
    __syncthreads();
  }
}

// ---- long route ---------------------------------------------------------------------------------------------------
// thread = channel (h, x) = (tid >> 5, tid & 31); the 32 lanes of a head are one half of a wave (half_all)
__device__ __forceinline__ int la_units(int R) { return (R + kLaUnit - 1) / kLaUnit; }

// sum_i row[i] * b[i] over the 32 floats at row (LDS, 16-byte aligned; a broadcast read for the lanes of a head)
__device__ __forceinline__ float dot32(const float* __restrict__ row, const float (&b)[32]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * i);
    s = fmaf(r.x, b[4 * i], s); s = fmaf(r.y, b[4 * i + 1], s); s = fmaf(r.z, b[4 * i + 2], s); s = fmaf(r.w, b[4 * i + 3], s);
  }
  return s;
}
// b[i] = the 32 contiguous floats at p (global, 16-byte aligned)
__device__ __forceinline__ void load32(float (&b)[32], const float* __restrict__ p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 r = *reinterpret_cast<const float4*>(p + 4 * i);
    b[4 * i] = r.x; b[4 * i + 1] = r.y; b[4 * i + 2] = r.z; b[4 * i + 3] = r.w;
  }
}

// part[n][blockIdx.x] = A | Ksum over this workgroup's units of S.  Thread (h, x) owns column x of A and Ksum[x].
__global__ __launch_bounds__(256) void k_la_kv_part(const float* __restrict__ k, const float* __restrict__ v,
                                                    const unsigned char* __restrict__ km, int S, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ks[kLaTile][256];
  const int tid = threadIdx.x, hb = tid & ~31, n = blockIdx.y;
  const float* kp = k + (size_t)n * S * 256 + tid;
  const float* vp = v + (size_t)n * S * 256 + tid;
  float A[32], ks = 0.f;
#pragma unroll
  for (int d = 0; d < 32; ++d) A[d] = 0.f;
  for (int u = blockIdx.x; u < la_units(S); u += gridDim.x) {
    const int s1 = min(S, (u + 1) * kLaUnit);
    for (int t0 = u * kLaUnit; t0 < s1; t0 += kLaTile) {
      float vo[kLaTile];
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const int s = t0 + r;
        const bool keep = s < s1 && la_keep(km, (size_t)n * S + s);
        const float K = keep ? la_phi(kp[(size_t)s * 256]) : 0.f;
        vo[r] = keep ? vp[(size_t)s * 256] : 0.f;
        Ks[r][tid] = K;
        ks += K;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float4 kk = *reinterpret_cast<const float4*>(&Ks[r][hb + 4 * i]);
          A[4 * i] = fmaf(kk.x, vo[r], A[4 * i]); A[4 * i + 1] = fmaf(kk.y, vo[r], A[4 * i + 1]);
          A[4 * i + 2] = fmaf(kk.z, vo[r], A[4 * i + 2]); A[4 * i + 3] = fmaf(kk.w, vo[r], A[4 * i + 3]);
        }
      }
      __syncthreads();
    }
  }
  float* o = part + ((size_t)n * gridDim.x + blockIdx.x) * kLaSlab + (size_t)(tid >> 5) * 33 * 32 + (tid & 31);
#pragma unroll
  for (int d = 0; d < 32; ++d) o[d * 32] = A[d];
  o[32 * 32] = ks;
}

// dst[n] = sum over the n_part slabs of part[n] (fold_slabs' order, fm_tile_device.h)
__global__ __launch_bounds__(256) void k_la_fold(const float* __restrict__ part, int n_part, float* __restrict__ dst) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, i = blockIdx.x * 32 + x, n = blockIdx.y;
  float v;
  if (fold_slabs(part + (size_t)n * n_part * kLaSlab + i, n_part, kLaSlab, red, &v)) dst[(size_t)n * kLaSlab + i] = v;
}

// out: thread (h, x) holds column x of A and Ksum[x]; the denominator is the one 32-lane sum per token and head
__global__ __launch_bounds__(256) void k_la_out(const float* __restrict__ q, const unsigned char* __restrict__ qm,
                                                const float* __restrict__ state, int L, float eps, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float Qs[kLaTile][256];
  const int tid = threadIdx.x, hb = tid & ~31, n = blockIdx.y;
  const float* st = state + (size_t)n * kLaSlab + (size_t)(tid >> 5) * 33 * 32 + (tid & 31);
  float A[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) A[d] = st[d * 32];
  const float ks = st[32 * 32];
  const float* qp = q + (size_t)n * L * 256 + tid;
  float* op = out + (size_t)n * L * 256 + tid;
  for (int u = blockIdx.x; u < la_units(L); u += gridDim.x) {
    const int l1 = min(L, (u + 1) * kLaUnit);
    for (int t0 = u * kLaUnit; t0 < l1; t0 += kLaTile) {
      float qo[kLaTile];
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const int l = t0 + r;
        qo[r] = l < l1 && la_keep(qm, (size_t)n * L + l) ? la_phi(qp[(size_t)l * 256]) : 0.f;
        Qs[r][tid] = qo[r];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const float z = 1.f / (half_all<OpAdd>(qo[r] * ks) + eps);
        const float o = dot32(&Qs[r][hb], A) * z;
        if (t0 + r < l1) op[(size_t)(t0 + r) * 256] = o;
      }
      __syncthreads();
    }
  }
}

// dq and part[n][blockIdx.x] = dA | dKsum over this workgroup's units of L.  Thread (h, d) holds row d of A and of dA.
__global__ __launch_bounds__(256) void k_la_bwd_q(const float* __restrict__ q, const unsigned char* __restrict__ qm,
                                                  const float* __restrict__ g, const float* __restrict__ state, int L,
                                                  float eps, float* __restrict__ dq, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Qs[kLaTile][256];
  __shared__ __attribute__((aligned(16))) float Gs[kLaTile][256];
  const int tid = threadIdx.x, hb = tid & ~31, n = blockIdx.y;
  const float* st = state + (size_t)n * kLaSlab + (size_t)(tid >> 5) * 33 * 32;
  float Ar[32], dAr[32], dks = 0.f;
  load32(Ar, st + (tid & 31) * 32);
  const float ks = st[32 * 32 + (tid & 31)];
#pragma unroll
  for (int i = 0; i < 32; ++i) dAr[i] = 0.f;
  const float* qp = q + (size_t)n * L * 256 + tid;
  const float* gp = g + (size_t)n * L * 256 + tid;
  float* op = dq + (size_t)n * L * 256 + tid;
  for (int u = blockIdx.x; u < la_units(L); u += gridDim.x) {
    const int l1 = min(L, (u + 1) * kLaUnit);
    for (int t0 = u * kLaUnit; t0 < l1; t0 += kLaTile) {
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const int l = t0 + r;
        Qs[r][tid] = l < l1 && la_keep(qm, (size_t)n * L + l) ? la_phi(qp[(size_t)l * 256]) : 0.f;
        Gs[r][tid] = l < l1 ? gp[(size_t)l * 256] : 0.f;
      }
      __syncthreads();
#pragma unroll 1
      for (int r = 0; r < kLaTile; ++r) {      // (one row at a time: unrolled, the tile's rows would hold 360 registers)
        const float Q = Qs[r][tid];
        const float z = 1.f / (half_all<OpAdd>(Q * ks) + eps);
        float gr[32];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float4 x = *reinterpret_cast<const float4*>(&Gs[r][hb + 4 * i]);
          gr[4 * i] = x.x; gr[4 * i + 1] = x.y; gr[4 * i + 2] = x.z; gr[4 * i + 3] = x.w;
        }
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) t = fmaf(Ar[i], gr[i], t);
        const float dden = -z * z * half_all<OpAdd>(Q * t);
        const float dQ = (z * t + dden * ks) * la_dphi(Q);
        if (t0 + r < l1) op[(size_t)(t0 + r) * 256] = dQ;
        const float c = Q * z;
#pragma unroll
        for (int i = 0; i < 32; ++i) dAr[i] = fmaf(c, gr[i], dAr[i]);
        dks = fmaf(dden, Q, dks);
      }
      __syncthreads();
    }
  }
  // slab entry [h][v][d] = dA[d][v]: consecutive lanes, consecutive addresses
  float* o = part + ((size_t)n * gridDim.x + blockIdx.x) * kLaSlab + (size_t)(tid >> 5) * 33 * 32 + (tid & 31);
#pragma unroll
  for (int i = 0; i < 32; ++i) o[i * 32] = dAr[i];
  o[32 * 32] = dks;
}

// dk, dv.  Thread (h, c) holds row c and column c of dA (dstate entry [h][v][d] = dA[d][v]) and dKsum[c].
__global__ __launch_bounds__(256) void k_la_bwd_kv(const float* __restrict__ k, const float* __restrict__ v,
                                                   const unsigned char* __restrict__ km, const float* __restrict__ dstate,
                                                   int S, float* __restrict__ dk, float* __restrict__ dv) {
  __shared__ __attribute__((aligned(16))) float Ks[kLaTile][256];
  __shared__ __attribute__((aligned(16))) float Vs[kLaTile][256];
  const int tid = threadIdx.x, hb = tid & ~31, n = blockIdx.y;
  const float* st = dstate + (size_t)n * kLaSlab + (size_t)(tid >> 5) * 33 * 32;
  float dAr[32], dAc[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) dAr[i] = st[i * 32 + (tid & 31)];
  load32(dAc, st + (tid & 31) * 32);
  const float dks = st[32 * 32 + (tid & 31)];
  const float* kp = k + (size_t)n * S * 256 + tid;
  const float* vp = v + (size_t)n * S * 256 + tid;
  float* ok = dk + (size_t)n * S * 256 + tid;
  float* ov = dv + (size_t)n * S * 256 + tid;
  for (int u = blockIdx.x; u < la_units(S); u += gridDim.x) {
    const int s1 = min(S, (u + 1) * kLaUnit);
    for (int t0 = u * kLaUnit; t0 < s1; t0 += kLaTile) {
      float ko[kLaTile];
      bool keep[kLaTile];
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const int s = t0 + r;
        keep[r] = s < s1 && la_keep(km, (size_t)n * S + s);
        ko[r] = keep[r] ? la_phi(kp[(size_t)s * 256]) : 0.f;
        Ks[r][tid] = ko[r];
        Vs[r][tid] = keep[r] ? vp[(size_t)s * 256] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kLaTile; ++r) {
        const float dK = (dot32(&Vs[r][hb], dAr) + dks) * la_dphi(ko[r]);
        const float dV = keep[r] ? dot32(&Ks[r][hb], dAc) : 0.f;
        if (t0 + r < s1) {
          ok[(size_t)(t0 + r) * 256] = dK;
          ov[(size_t)(t0 + r) * 256] = dV;
        }
      }
      __syncthreads();
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
enum LaRoute { kLaNone = 0, kLaWindow, kLaLong };
// the route table (mirrored by ops.linear_attention_supported); the long route's samples are the grid's y
static LaRoute la_route(int N, int L, int S, int H, int D) {
  if (H != 8) return kLaNone;
  if (D == 8 && L <= kLaWinMax && S <= kLaWinMax) return kLaWindow;
  if (D == 32 && N <= 65535) return kLaLong;
  return kLaNone;
}
static int la_groups(int R) {                    // workgroups per sample of a pass over R rows
  const int u = (R + kLaUnit - 1) / kLaUnit;
  return u < kLaMaxUnits ? u : kLaMaxUnits;
}
// Long-route workspace, carved from its start by either call: the forward's partial slabs [N][la_groups(S)]; the
// backward's [N][la_groups(L)] and, directly behind them, the folded dA | dKsum [N]
struct LaWs { int gs, gl; Region<float> part, dstate; size_t total; };
static LaWs la_layout(int N, int L, int S) {
  LaWs w;
  w.gs = la_groups(S);
  w.gl = la_groups(L);
  Carver fwd, bwd;
  fwd.take(w.part, (size_t)N * w.gs * kLaSlab);
  bwd.take(w.part, (size_t)N * w.gl * kLaSlab);
  bwd.take(w.dstate, (size_t)N * kLaSlab, sizeof(float));
  w.total = align256(fwd.o > bwd.o ? fwd.o : bwd.o);
  return w;
}

// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct LaCall {
  const float *q, *k, *v; const unsigned char *q_mask, *kv_mask;
  int N, L, S, H, D; float eps;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float *state_out, *out;                                   // forward
  const float *d_out, *state; float *d_q, *d_k, *d_v;       // backward
};

// the ONLY copy of the two entry points' argument checks; *route is set with FM_OK
static int la_status(const LaCall& c, LaRoute* route) {
  if (!c.q || !c.k || !c.v) return FM_E_NULL;
  if (c.backward ? (!c.d_out || !c.d_q || !c.d_k || !c.d_v) : !c.out) return FM_E_NULL;
  if (c.N <= 0 || c.L <= 0 || c.S <= 0 || c.H <= 0 || c.D <= 0) return FM_E_SHAPE;
  const LaRoute r = la_route(c.N, c.L, c.S, c.H, c.D);
  if (r == kLaNone || !(c.eps > 0.f)) return FM_E_UNSUPPORTED;
  if (r == kLaLong) {
    if (!c.workspace || !(c.backward ? (const void*)c.state : (const void*)c.state_out)) return FM_E_NULL;
    if (!workspace_ok(c.workspace, c.workspace_bytes, la_layout(c.N, c.L, c.S).total)) return FM_E_WORKSPACE;
  }
  *route = r;
  return FM_OK;
}

static int la_run(const LaCall& c) {
  LaRoute route = kLaNone;
  const int status = la_status(c, &route);
  if (status != FM_OK) return status;
  hipStream_t st = (hipStream_t)c.stream;
  if (route == kLaWindow) {
    static unsigned long long lds_fwd = 0, lds_bwd = 0;
    const int smem = (2 * c.S + (c.backward ? 2 : 1) * c.L) * 64 * (int)sizeof(float);
    const dim3 grid(c.N < kLaWinGrid ? c.N : kLaWinGrid);
    if (!c.backward) {
      const hipError_t e = ensure_dynamic_lds(k_la_win_fwd, 3 * kLaWinMax * 256, &lds_fwd);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(k_la_win_fwd, grid, dim3(64), smem, st, c.q, c.k, c.v, c.q_mask, c.kv_mask, c.N, c.L, c.S, c.eps, c.out);
    } else {
      const hipError_t e = ensure_dynamic_lds(k_la_win_bwd, 4 * kLaWinMax * 256, &lds_bwd);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(k_la_win_bwd, grid, dim3(64), smem, st, c.q, c.k, c.v, c.q_mask, c.kv_mask, c.d_out, c.N, c.L, c.S,
                         c.eps, c.d_q, c.d_k, c.d_v);
    }
    return (int)hipGetLastError();
  }
  const LaWs w = la_layout(c.N, c.L, c.S);
  float* part = w.part.in(c.workspace);
  const dim3 fold(kLaSlab / 32, c.N);
  if (!c.backward) {
    hipLaunchKernelGGL(k_la_kv_part, dim3(w.gs, c.N), dim3(256), 0, st, c.k, c.v, c.kv_mask, c.S, part);
    hipLaunchKernelGGL(k_la_fold, fold, dim3(256), 0, st, (const float*)part, w.gs, c.state_out);
    hipLaunchKernelGGL(k_la_out, dim3(w.gl, c.N), dim3(256), 0, st, c.q, c.q_mask, (const float*)c.state_out, c.L, c.eps, c.out);
  } else {
    float* dstate = w.dstate.in(c.workspace);
    hipLaunchKernelGGL(k_la_bwd_q, dim3(w.gl, c.N), dim3(256), 0, st, c.q, c.q_mask, c.d_out, c.state, c.L, c.eps, c.d_q, part);
    hipLaunchKernelGGL(k_la_fold, fold, dim3(256), 0, st, (const float*)part, w.gl, dstate);
    hipLaunchKernelGGL(k_la_bwd_kv, dim3(w.gs, c.N), dim3(256), 0, st, c.k, c.v, c.kv_mask, (const float*)dstate, c.S, c.d_k, c.d_v);
  }
  return (int)hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_linear_attention_state_bytes(int N, int L, int S, int H, int D) {
  if (N <= 0 || L <= 0 || S <= 0 || H <= 0 || D <= 0 || la_route(N, L, S, H, D) != kLaLong) return 0;
  return (size_t)N * kLaSlab * sizeof(float);
}

extern "C" size_t fm_linear_attention_workspace_bytes(int N, int L, int S, int H, int D) {
  if (N <= 0 || L <= 0 || S <= 0 || H <= 0 || D <= 0 || la_route(N, L, S, H, D) != kLaLong) return 0;
  return la_layout(N, L, S).total;
}

extern "C" int fm_linear_attention_forward(const float* q, const float* k, const float* v, const unsigned char* q_mask,
                                           const unsigned char* kv_mask, int N, int L, int S, int H, int D, float eps,
                                           void* workspace, size_t workspace_bytes, float* state, float* out, void* stream) {
  LaCall c = {};
  c.q = q; c.k = k; c.v = v; c.q_mask = q_mask; c.kv_mask = kv_mask;
  c.N = N; c.L = L; c.S = S; c.H = H; c.D = D; c.eps = eps;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.state_out = state; c.out = out;
  return la_run(c);
}

extern "C" int fm_linear_attention_backward(const float* q, const float* k, const float* v, const unsigned char* q_mask,
                                            const unsigned char* kv_mask, const float* d_out, const float* state, int N, int L,
                                            int S, int H, int D, float eps, void* workspace, size_t workspace_bytes, float* d_q,
                                            float* d_k, float* d_v, void* stream) {
  LaCall c = {};
  c.q = q; c.k = k; c.v = v; c.q_mask = q_mask; c.kv_mask = kv_mask;
  c.N = N; c.L = L; c.S = S; c.H = H; c.D = D; c.eps = eps;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.d_out = d_out; c.state = state; c.d_q = d_q; c.d_k = d_k; c.d_v = d_v;
  return la_run(c);
}
