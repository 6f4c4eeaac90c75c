// Full softmax attention (the reference's FullAttention, network/module/attentions.py:48-79, without mask and dropout:
// what EncoderLayer constructs) and its gradient: the 'full' attention core of the context layers' training path
// (transformer.py, `full_attention`).  float32 throughout, every product on v_mfma_f32_32x32x2_f32 (exact float32); the
// [L, S] scores of a head never reach memory, in either direction.
//
// Per sample n and head h, c = 1 / sqrt(D), g = d out:
//     s[l][s'] = c q_l . k_s'        lse_l = log sum_s' exp(s[l][s'])        p = exp(s - lse_l)
//     out_l = sum_s' p[l][s'] v_s'
//     delta_l = g_l . out_l          dP[l][s'] = g_l . v_s'                  dS = p (dP - delta_l)
//     dv_s' = sum_l p[l][s'] g_l     dk_s' = c sum_l dS[l][s'] q_l           dq_l = c sum_s' dS[l][s'] k_s'
//
// One wave owns a tile of 32 tokens of one (n, h) and walks the other side in tiles of 32; the work units (n, h, tile)
// are flattened into blockIdx.x and taken by grid stride, so no size is bounded by a grid dimension.  Every tile product
// is computed in fm_tile_device.h's orientation: the OWNED token is the column of the 32 x 32 result and sits on the lane
// (lane & 31), the walked tokens are its rows, fa_row(R, lane >> 5) of register R.  A product that sums over the walked
// tokens then takes that result as its B operand register by register ("register R of one product's result IS the B
// operand of step R of the next"): nothing crosses lanes but one lane ^ 32 exchange per row statistic, and there is no LDS.
//   operand with the token on the lane (fa_frag): the lane's half of the head's channels, D / 2 contiguous floats - step
//     t of the D / 2 steps of a q.k or g.v product takes channel t from half 0 and D / 2 + t from half 1;
//   operand with the token in the register (fa_rows): channel = lane & 31 of token fa_row(R, half), 16 coalesced loads of
//     one row each (D = 8: lanes 8..31 supply 0, three quarters of that product's rows are idle).
//   forward  k_fa_fwd   : owns 32 queries, walks the keys with a running maximum and sum (online softmax): S^T = K Q^T,
//                         O^T += V^T P^T.  2 products per tile pair.  Writes out and, if asked, lse [N][H][L].
//   backward k_fa_delta : delta [N][H][L] into the workspace
//            k_fa_bwd_kv: owns 32 keys, walks the queries: S = Q K^T, dP = g V^T, dV^T += g^T P, dK^T += Q^T dS.  4 products.
//            k_fa_bwd_q : owns 32 queries, walks the keys: S^T = K Q^T, dP^T = V g^T, dQ^T += K^T dS^T.  3 products.
// No atomics and no sum across workgroups: every output element has one owner that adds its terms in index order, and the
// grids depend on the shape alone, so every output is the same bits on every call.
#include <math.h>

#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

constexpr int kFaHeads = 8;
constexpr int kFaMaxGrid = 1 << 20;   // workgroups (of one wave) of a sweep's launch; the rest by grid stride
constexpr int kFaDeltaGrid = 4096;    // workgroups (of 256 threads) of k_fa_delta; the rest by grid stride

// row of a 32 x 32 product that register R of lane half `half` holds
__device__ __forceinline__ int fa_row(int R, int half) { return (R & 3) + 8 * (R >> 2) + 4 * half; }

// The scaled score, rounded to float32 BEFORE anything is subtracted from it, in the forward and in both backward sweeps
// alike (left to the compiler the backward's `s * scale - lse` is one fma and the forward's product is rounded).  The
// backward's p is then the forward's up to one factor per row, and sum_s dS[l][s] = 0 holds to rounding as it does on
// paper; with the two apart by half an ulp of a score of 300, a channel that all keys share (k = 30) lost 1.5e-4 of dq.
// (The pragma takes the product out of fma contraction wherever it is inlined; __fmul_rn is a plain product here.)
__device__ __forceinline__ float fa_scaled(float s, float scale) {
#pragma clang fp contract(off)
  return s * scale;
}

// f[t] = channel (lane >> 5) * D / 2 + t of token t0 + (lane & 31); base = the head's channel 0 of token 0; tokens past
// T read as 0
template <int D>
__device__ __forceinline__ void fa_frag(const float* __restrict__ base, int t0, int T, int lane, float (&f)[D / 2]) {
  const int tok = t0 + (lane & 31);
  const float4* p = reinterpret_cast<const float4*>(base + (size_t)(tok < T ? tok : 0) * (kFaHeads * D) + (lane >> 5) * (D / 2));
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const float4 x = tok < T ? p[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    f[4 * i] = x.x; f[4 * i + 1] = x.y; f[4 * i + 2] = x.z; f[4 * i + 3] = x.w;
  }
}
// r[R] = channel lane & 31 of token t0 + fa_row(R, lane >> 5); channels past D and tokens past T read as 0
template <int D>
__device__ __forceinline__ void fa_rows(const float* __restrict__ base, int t0, int T, int lane, float (&r)[16]) {
  const int c = lane & 31, half = lane >> 5;
#pragma unroll
  for (int R = 0; R < 16; ++R) {
    const int tok = t0 + fa_row(R, half);
    r[R] = (tok < T && c < D) ? base[(size_t)tok * (kFaHeads * D) + c] : 0.f;
  }
}
// r[R] = x[t0 + fa_row(R, lane >> 5)] (one float per token); tokens past T read as 0
__device__ __forceinline__ void fa_stats(const float* __restrict__ x, int t0, int T, int lane, float (&r)[16]) {
#pragma unroll
  for (int R = 0; R < 16; ++R) {
    const int tok = t0 + fa_row(R, lane >> 5);
    r[R] = tok < T ? x[tok] : 0.f;
  }
}
// acc = sum over the head's channels of a (token = row) times b (token = column)
template <int D>
__device__ __forceinline__ f32x16 fa_dot(const float (&a)[D / 2], const float (&b)[D / 2]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int t = 0; t < D / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
  return acc;
}
// acc[channel][column] += sum over the 32 row tokens of rows[R] (channel on the lane) times x[R]
__device__ __forceinline__ void fa_acc(f32x16& acc, const float (&rows)[16], const f32x16& x) {
#pragma unroll
  for (int R = 0; R < 16; ++R) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rows[R], x[R], acc, 0, 0, 0);
}
// acc^T (channel fa_row(R, half), token on the lane) times f -> channels of token tok of the head at base, if live
template <int D>
__device__ __forceinline__ void fa_store(float* __restrict__ base, int tok, int T, int lane, const f32x16& acc, float f) {
  if (tok >= T) return;
  float4* p = reinterpret_cast<float4*>(base + (size_t)tok * (kFaHeads * D) + 4 * (lane >> 5));
#pragma unroll
  for (int g = 0; g < D / 8; ++g) p[2 * g] = make_float4(acc[4 * g] * f, acc[4 * g + 1] * f, acc[4 * g + 2] * f, acc[4 * g + 3] * f);
}

// unit u -> (sample * heads + head, tile) for `tiles` tiles per head
struct FaUnit { size_t nh; int h, t0; };
__device__ __forceinline__ FaUnit fa_unit(long u, int tiles) {
  FaUnit x;
  x.nh = (size_t)(u / tiles);
  x.h = (int)(x.nh & (kFaHeads - 1));
  x.t0 = (int)(u % tiles) * kTile;
  return x;
}
// channel 0 of head h of token 0 of the unit's sample, in a [N, T, H * D] tensor
template <int D, class T>
__device__ __forceinline__ T* fa_head(T* p, const FaUnit& x, int tokens) {
  return p + (x.nh >> 3) * (size_t)tokens * (kFaHeads * D) + x.h * D;
}

template <int D>
__global__ __launch_bounds__(64) void k_fa_fwd(const float* __restrict__ q, const float* __restrict__ k,
                                               const float* __restrict__ v, int L, int S, long units, float scale,
                                               float* __restrict__ lse, float* __restrict__ out) {
  const int lane = threadIdx.x, half = lane >> 5, tiles = (L + kTile - 1) / kTile;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const FaUnit x = fa_unit(u, tiles);
    const float* kb = fa_head<D>(k, x, S);
    const float* vb = fa_head<D>(v, x, S);
    float qf[D / 2];
    fa_frag<D>(fa_head<D>(q, x, L), x.t0, L, lane, qf);
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int s0 = 0; s0 < S; s0 += kTile) {
      float kf[D / 2], vr[16];
      fa_frag<D>(kb, s0, S, lane, kf);
      fa_rows<D>(vb, s0, S, lane, vr);
      f32x16 sc = fa_dot<D>(kf, qf);                 // S^T [key][query]
      float tm = -INFINITY;
#pragma unroll
      for (int R = 0; R < 16; ++R) {
        sc[R] = s0 + fa_row(R, half) < S ? fa_scaled(sc[R], scale) : -INFINITY;
        tm = fmaxf(tm, sc[R]);
      }
      // (key s0 is live, so the pair's maximum is finite; m = -inf only before the first tile, where alpha = 0)
      const float mn = fmaxf(m, pair_op<32, OpMax>(tm));
      const float alpha = expf(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int R = 0; R < 16; ++R) {
        sc[R] = expf(sc[R] - mn);
        ps += sc[R];
      }
      l = l * alpha + pair_op<32, OpAdd>(ps);
      m = mn;
#pragma unroll
      for (int R = 0; R < 16; ++R) o[R] *= alpha;
      fa_acc(o, vr, sc);                             // O^T [channel][query] += V^T P^T
    }
    const int tok = x.t0 + (lane & 31);
    fa_store<D>(fa_head<D>(out, x, L), tok, L, lane, o, 1.f / l);
    if (lse && half == 0 && tok < L) lse[x.nh * L + tok] = m + logf(l);
  }
}

// delta [N][H][L] = sum over a head's channels of g * out; thread i = (n, l, h), h fastest: neighbouring reads
template <int D>
__global__ __launch_bounds__(256) void k_fa_delta(const float* __restrict__ g, const float* __restrict__ out, int L,
                                                  long total, float* __restrict__ delta) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const float4* a = reinterpret_cast<const float4*>(g + (size_t)i * D);
    const float4* b = reinterpret_cast<const float4*>(out + (size_t)i * D);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D / 4; ++j) {
      const float4 x = a[j], y = b[j];
      s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    const long tok = i >> 3, n = tok / L;
    delta[((size_t)n * kFaHeads + (i & 7)) * L + (tok - n * L)] = s;
  }
}

// p and dS of one tile pair from its scores and dP (in place): row statistics per register (ROWS: the walked tokens are
// the queries) or per lane; entries outside the problem are 0
template <bool ROWS>
__device__ __forceinline__ void fa_p_ds(f32x16& sc, f32x16& dp, const float (&ls)[16], const float (&dl)[16], int row0,
                                        int rows, bool col_live, int half, float scale) {
#pragma unroll
  for (int R = 0; R < 16; ++R) {
    const bool live = col_live && row0 + fa_row(R, half) < rows;
    const float p = live ? expf(fa_scaled(sc[R], scale) - ls[ROWS ? R : 0]) : 0.f;
    sc[R] = p;
    dp[R] = p * (dp[R] - dl[ROWS ? R : 0]);
  }
}

template <int D>
__global__ __launch_bounds__(64) void k_fa_bwd_kv(const float* __restrict__ q, const float* __restrict__ k,
                                                  const float* __restrict__ v, const float* __restrict__ g,
                                                  const float* __restrict__ lse, const float* __restrict__ delta, int L,
                                                  int S, long units, float scale, float* __restrict__ dk,
                                                  float* __restrict__ dv) {
  const int lane = threadIdx.x, half = lane >> 5, tiles = (S + kTile - 1) / kTile;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const FaUnit x = fa_unit(u, tiles);
    const float* qb = fa_head<D>(q, x, L);
    const float* gb = fa_head<D>(g, x, L);
    const float* lb = lse + x.nh * L;
    const float* db = delta + x.nh * L;
    const int key = x.t0 + (lane & 31);
    float kf[D / 2], vf[D / 2];
    fa_frag<D>(fa_head<D>(k, x, S), x.t0, S, lane, kf);
    fa_frag<D>(fa_head<D>(v, x, S), x.t0, S, lane, vf);
    f32x16 dkt, dvt;
#pragma unroll
    for (int r = 0; r < 16; ++r) dkt[r] = dvt[r] = 0.f;
    for (int l0 = 0; l0 < L; l0 += kTile) {
      float qf[D / 2], gf[D / 2], qr[16], gr[16], ls[16], dl[16];
      fa_frag<D>(qb, l0, L, lane, qf);
      fa_frag<D>(gb, l0, L, lane, gf);
      fa_rows<D>(qb, l0, L, lane, qr);
      fa_rows<D>(gb, l0, L, lane, gr);
      fa_stats(lb, l0, L, lane, ls);
      fa_stats(db, l0, L, lane, dl);
      f32x16 sc = fa_dot<D>(qf, kf);                 // S [query][key]
      f32x16 dp = fa_dot<D>(gf, vf);                 // dP [query][key]
      fa_p_ds<true>(sc, dp, ls, dl, l0, L, key < S, half, scale);
      fa_acc(dvt, gr, sc);                           // dV^T [channel][key] += g^T P
      fa_acc(dkt, qr, dp);                           // dK^T [channel][key] += Q^T dS
    }
    fa_store<D>(fa_head<D>(dk, x, S), key, S, lane, dkt, scale);
    fa_store<D>(fa_head<D>(dv, x, S), key, S, lane, dvt, 1.f);
  }
}

template <int D>
__global__ __launch_bounds__(64) void k_fa_bwd_q(const float* __restrict__ q, const float* __restrict__ k,
                                                 const float* __restrict__ v, const float* __restrict__ g,
                                                 const float* __restrict__ lse, const float* __restrict__ delta, int L,
                                                 int S, long units, float scale, float* __restrict__ dq) {
  const int lane = threadIdx.x, half = lane >> 5, tiles = (L + kTile - 1) / kTile;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const FaUnit x = fa_unit(u, tiles);
    const float* kb = fa_head<D>(k, x, S);
    const float* vb = fa_head<D>(v, x, S);
    const int tok = x.t0 + (lane & 31);
    float qf[D / 2], gf[D / 2];
    fa_frag<D>(fa_head<D>(q, x, L), x.t0, L, lane, qf);
    fa_frag<D>(fa_head<D>(g, x, L), x.t0, L, lane, gf);
    float ls[16], dl[16];                            // ([0] alone is used: the query is the lane's)
    ls[0] = tok < L ? lse[x.nh * L + tok] : 0.f;
    dl[0] = tok < L ? delta[x.nh * L + tok] : 0.f;
    f32x16 dqt;
#pragma unroll
    for (int r = 0; r < 16; ++r) dqt[r] = 0.f;
    for (int s0 = 0; s0 < S; s0 += kTile) {
      float kf[D / 2], vf[D / 2], kr[16];
      fa_frag<D>(kb, s0, S, lane, kf);
      fa_frag<D>(vb, s0, S, lane, vf);
      fa_rows<D>(kb, s0, S, lane, kr);
      f32x16 sc = fa_dot<D>(kf, qf);                 // S^T [key][query]
      f32x16 dp = fa_dot<D>(vf, gf);                 // dP^T [key][query]
      fa_p_ds<false>(sc, dp, ls, dl, s0, S, tok < L, half, scale);
      fa_acc(dqt, kr, dp);                           // dQ^T [channel][query] += K^T dS^T
    }
    fa_store<D>(fa_head<D>(dq, x, L), tok, L, lane, dqt, scale);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool fa_positive(int N, int L, int S, int H, int D) { return N > 0 && L > 0 && S > 0 && H > 0 && D > 0; }
// the served shapes (mirrored by ops.full_attention_supported): 8 heads of 8 or 32 channels, tensors below 2^31 elements
static bool fa_supported(int N, int L, int S, int H, int D) {
  if (H != kFaHeads || (D != 8 && D != 32)) return false;
  return (long long)N * (L > S ? L : S) * H * D < (1ll << 31);
}
static size_t fa_table_bytes(int N, int L) { return align256((size_t)N * L * kFaHeads * sizeof(float)); }
static int fa_grid(long units, int cap = kFaMaxGrid) { return (int)(units < cap ? units : cap); }

// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct FaCall {
  const float *q, *k, *v;
  int N, L, S, H, D;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float *state_out, *out;                                            // forward
  const float *out_in, *d_out, *state; float *d_q, *d_k, *d_v;       // backward
};

// the ONLY copy of the two entry points' argument checks
static int fa_status(const FaCall& c) {
  if (!c.q || !c.k || !c.v) return FM_E_NULL;
  if (c.backward ? (!c.out_in || !c.d_out || !c.state || !c.d_q || !c.d_k || !c.d_v) : !c.out) return FM_E_NULL;
  const bool shape = fa_positive(c.N, c.L, c.S, c.H, c.D), served = shape && fa_supported(c.N, c.L, c.S, c.H, c.D);
  if (served && !c.workspace) return FM_E_NULL;      // (the workspace's size query is non-zero exactly for these)
  if (!shape) return FM_E_SHAPE;
  if (!served) return FM_E_UNSUPPORTED;
  if (!workspace_ok(c.workspace, c.workspace_bytes, fa_table_bytes(c.N, c.L))) return FM_E_WORKSPACE;
  return FM_OK;
}

template <int D>
static int fa_launch(const FaCall& c) {
  hipStream_t st = (hipStream_t)c.stream;
  const float scale = 1.0f / sqrtf((float)D);
  const long ql = (long)c.N * kFaHeads * ((c.L + kTile - 1) / kTile), kl = (long)c.N * kFaHeads * ((c.S + kTile - 1) / kTile);
  if (!c.backward) {
    hipLaunchKernelGGL(k_fa_fwd<D>, dim3(fa_grid(ql)), dim3(64), 0, st, c.q, c.k, c.v, c.L, c.S, ql, scale, c.state_out, c.out);
    return (int)hipGetLastError();
  }
  float* delta = static_cast<float*>(c.workspace);
  const long rows = (long)c.N * c.L * kFaHeads;
  hipLaunchKernelGGL(k_fa_delta<D>, dim3(fa_grid((rows + 255) / 256, kFaDeltaGrid)), dim3(256), 0, st, c.d_out, c.out_in, c.L, rows, delta);
  hipLaunchKernelGGL(k_fa_bwd_kv<D>, dim3(fa_grid(kl)), dim3(64), 0, st, c.q, c.k, c.v, c.d_out, c.state, (const float*)delta,
                     c.L, c.S, kl, scale, c.d_k, c.d_v);
  hipLaunchKernelGGL(k_fa_bwd_q<D>, dim3(fa_grid(ql)), dim3(64), 0, st, c.q, c.k, c.v, c.d_out, c.state, (const float*)delta,
                     c.L, c.S, ql, scale, c.d_q);
  return (int)hipGetLastError();
}

static int fa_run(const FaCall& c) {
  const int status = fa_status(c);
  if (status != FM_OK) return status;
  return c.D == 8 ? fa_launch<8>(c) : fa_launch<32>(c);
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_full_attention_state_bytes(int N, int L, int S, int H, int D) {
  return fa_positive(N, L, S, H, D) && fa_supported(N, L, S, H, D) ? fa_table_bytes(N, L) : 0;
}

extern "C" size_t fm_full_attention_workspace_bytes(int N, int L, int S, int H, int D) {
  return fa_positive(N, L, S, H, D) && fa_supported(N, L, S, H, D) ? fa_table_bytes(N, L) : 0;
}

extern "C" int fm_full_attention_forward(const float* q, const float* k, const float* v, int N, int L, int S, int H, int D,
                                         void* workspace, size_t workspace_bytes, float* state, float* out, void* stream) {
  FaCall c = {};
  c.q = q; c.k = k; c.v = v;
  c.N = N; c.L = L; c.S = S; c.H = H; c.D = D;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.state_out = state; c.out = out;
  return fa_run(c);
}

extern "C" int fm_full_attention_backward(const float* q, const float* k, const float* v, const float* out, const float* d_out,
                                          const float* state, int N, int L, int S, int H, int D, void* workspace,
                                          size_t workspace_bytes, float* d_q, float* d_k, float* d_v, void* stream) {
  FaCall c = {};
  c.q = q; c.k = k; c.v = v;
  c.N = N; c.L = L; c.S = S; c.H = H; c.D = D;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.out_in = out; c.d_out = d_out; c.state = state; c.d_q = d_q; c.d_k = d_k; c.d_v = d_v;
  return fa_run(c);
}
