// The q / k / v projections of an encoder layer (transformer.py, EncoderLayer.forward: the three nn.Linear(64, 64,
// bias=False) lines in front of the attention) and their gradient, fused: the context layers' training path at the fine
// level, d_model = 64.  Float32 throughout:
//     q = x Wq^T          k = src Wk^T          v = src Wv^T
//     d_x   = gq Wq                    (+ gk Wk + gv Wv when src is x)
//     d_src = gk Wk + gv Wv            (cross layers only)
//     dWq = sum_t gq^T x     dWk = sum_t gk^T src     dWv = sum_t gv^T src
// Every product runs on v_mfma_f32_32x32x2_f32: exact float32, one rounding per product, a k-ordered fmaf chain.
//
// Tiling: fm_tile_device.h's (layout L, fragments, the exchange image).  The three matrices are ONE matrix to the
// kernels, packed by k_qp_pack once per call:
//   forward  : [Wq; Wk; Wv], 192 x 64 - six output tiles over one load of x (self mode), or its rows 0..63 over x and its
//              rows 64..191 over src (cross mode);
//   backward : [Wq^T | Wk^T | Wv^T], 64 x 192, over the 96 registers (gq, gk, gv) of a token: the three data-gradient
//              products are one k-ordered sum in the accumulator (self mode), or Wq^T over gq and [Wk^T | Wv^T] over (gk, gv).
//   k_qp_fwd : 8 waves; the fragments (48 KB) in LDS.
//   k_qp_bwd : 4 waves; fragments from L2 (the LDS is the exchange).  Image rows: the one to three gradients, then the
//     input (256 per wave); every wave multiplies ITS output tile (wave >> 1, wave & 1) of each of dWq, dWk, dWv over all
//     four images: 3 of the 12 tiles, 48 accumulator registers.  k_qp_fold adds the workgroups' slabs.
// Self mode (src == x) walks the chunks of x; cross mode walks the chunks of x, then those of src, in one grid: a chunk
// is the one kind or the other for the whole workgroup.  No atomics, grids that depend on Tx, Ts and the mode alone,
// fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

constexpr int kQpMat = 4096;                     // floats of one 64 x 64 matrix
// fragments, in floats: the forward's [Wq; Wk; Wv] | the backward's (self: [Wq^T | Wk^T | Wv^T]; cross: Wq^T, then
// [Wk^T | Wv^T])
constexpr int kQpFwdFrag = 3 * kQpMat, kQpFrag = 6 * kQpMat;
constexpr int kQpSlab = 3 * kQpMat;              // a slab of partial weight gradients, in floats: dWq | dWk | dWv
constexpr int kQpImage = 256 * kTilePitch;       // floats of a wave's image
constexpr int kQpFwdLds = kQpFwdFrag * 4;
constexpr int kQpBwdLds = kTileBwdWaves * kQpImage * 4;
static_assert(kQpSlab % 32 == 0, "k_qp_fold's grid covers a slab exactly");
static_assert(kQpBwdLds <= 160 * 1024 && kQpFwdLds <= 160 * 1024, "one workgroup per CU");

// k_qp_pack.  Forward (tr = false): the fragments of the 192 x 64 matrix [Wq; Wk; Wv] - output tiles 2 m, 2 m + 1 are
// those of matrix m.  Backward (tr = true): of a 64 x 64 nmat matrix [W_first^T | ...], nmat = 3 from Wq on (self mode),
// else Wq^T alone at float 0 and [Wk^T | Wv^T] at float kQpMat - k-groups 8 m .. 8 m + 7 of an output tile are those of
// W_{first + m}^T.
__global__ __launch_bounds__(256) void k_qp_pack(const float* __restrict__ wq, const float* __restrict__ wk,
                                                 const float* __restrict__ wv, int tr, int self, float* __restrict__ frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * kQpMat) return;
  int idx = i, first = 0, nmat = 3;
  if (tr && !self) {
    if (i < kQpMat) nmat = 1;
    else { idx = i - kQpMat; first = 1; nmat = 2; }
  }
  const int nq = tr ? 8 * nmat : 8, ot = (idx >> 8) / nq, q = (idx >> 8) % nq;
  const int m = first + (tr ? q >> 3 : ot >> 1);
  const float* W = m == 0 ? wq : m == 1 ? wk : wv;
  frag[i] = frag_value(W, 64, 64, tr != 0, (((tr ? ot : ot & 1) * 8 + (q & 7)) << 8) + (idx & 255));
}

// What a chunk of the grid's walk is: self mode - chunk `ch` of x, all three products; cross mode - the chunks of x (the
// q side), then those of src (the k / v side).  side: 0 = all three, 1 = q alone, 2 = k and v.
struct QpChunk { int side, T; size_t t0; };
template <bool SELF>
__device__ __forceinline__ QpChunk qp_chunk(int ch, int chunks_x, int Tx, int Ts, int chunk) {
  if (SELF) return {0, Tx, (size_t)ch * chunk};
  if (ch < chunks_x) return {1, Tx, (size_t)ch * chunk};
  return {2, Ts, (size_t)(ch - chunks_x) * chunk};
}

template <bool SELF>
__global__ __launch_bounds__(kTileFwdWaves * 64) void k_qp_fwd(const float* __restrict__ x, const float* __restrict__ src,
                                                               const float* __restrict__ frag, int Tx, int Ts,
                                                               float* __restrict__ q, float* __restrict__ k,
                                                               float* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) float qp_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kQpFwdFrag / 4; i += kTileFwdWaves * 64)     // (written out: a helper moves the loop in the kernel)
    reinterpret_cast<float4*>(qp_lds)[i] = reinterpret_cast<const float4*>(frag)[i];
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(qp_lds);
  const int chunks_x = (Tx + kTileFwdChunk - 1) / kTileFwdChunk;
  const int chunks = SELF ? chunks_x : chunks_x + (Ts + kTileFwdChunk - 1) / kTileFwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const QpChunk c = qp_chunk<SELF>(ch, chunks_x, Tx, Ts, kTileFwdChunk);
    const size_t t0 = c.t0 + wave * kTile;
    if (t0 >= (size_t)c.T) continue;
    const float4* F = F0 + opaque_zero();
    float in[32];
    if (c.side == 0) {
      tile_load(x, t0, c.T, lane, in);
      f32x16 acc[6];
      tile_mm<6, 32>(F, in, acc, lane);
      tile_store(q, t0, c.T, lane, acc[0], acc[1]);
      tile_store(k, t0, c.T, lane, acc[2], acc[3]);
      tile_store(v, t0, c.T, lane, acc[4], acc[5]);
    } else if (c.side == 1) {
      tile_load(x, t0, c.T, lane, in);
      f32x16 acc[2];
      tile_mm<2, 32>(F, in, acc, lane);
      tile_store(q, t0, c.T, lane, acc[0], acc[1]);
    } else {
      tile_load(src, t0, c.T, lane, in);
      f32x16 acc[4];
      tile_mm<4, 32>(F + kQpMat / 4, in, acc, lane);
      tile_store(k, t0, c.T, lane, acc[0], acc[1]);
      tile_store(v, t0, c.T, lane, acc[2], acc[3]);
    }
  }
}

// One chunk of the backward: NG gradients g[0 .. NG) [T, 64] against the fragments FT of [W_0^T | .. | W_{NG-1}^T]; `in`
// is their common input, `out` its gradient.  WGRAD: wacc[j] += this wave's tile of sum_t g[j]^T in over the chunk.
template <int NG, bool WGRAD>
__device__ __forceinline__ void qp_bwd_chunk(const float* const (&g)[NG], const float4* __restrict__ FT,
                                             const float* __restrict__ in, float* __restrict__ out, size_t t0, int T,
                                             int wave, int lane, float* __restrict__ E, f32x16 (*__restrict__ wacc)[1]) {
  float gv[32 * NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) tile_load(g[j], t0, T, lane, gv + 32 * j);
  if (WGRAD) {
    float vin[32];
    tile_load(in, t0, T, lane, vin);
    float* Ew = E + wave * kQpImage;
#pragma unroll
    for (int j = 0; j < NG; ++j) tile_put<32>(Ew, 64 * j, lane, gv + 32 * j);
    tile_put<32>(Ew, 64 * NG, lane, vin);
  }
  {
    f32x16 acc[2];
    tile_mm<2, 32 * NG>(FT, gv, acc, lane);
    tile_store(out, t0, T, lane, acc[0], acc[1]);
  }
  if (WGRAD) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NG; ++j)
      tile_wgrad<1, kTileBwdWaves, kQpImage>(E, 64 * j + 32 * (wave >> 1), 64 * NG + 32 * (wave & 1), lane, wacc[j]);
    __syncthreads();
  }
}

// WGRAD = false: d_x (and d_src) only - no exchange, no barriers, no LDS, `part` unused
template <bool SELF, bool WGRAD>
__global__ __launch_bounds__(kTileBwdWaves * 64) void k_qp_bwd(const float* __restrict__ x, const float* __restrict__ src,
                                                               const float* __restrict__ gq, const float* __restrict__ gk,
                                                               const float* __restrict__ gv, const float* __restrict__ frag,
                                                               int Tx, int Ts, float* __restrict__ d_x,
                                                               float* __restrict__ d_src, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float qp_lds[];     // [wave][256 rows][kTilePitch]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float4* F0 = reinterpret_cast<const float4*>(frag);
  f32x16 wacc[3][1];                                                 // this wave's tile of dWq, dWk, dWv
#pragma unroll
  for (int r = 0; r < 16; ++r) wacc[0][0][r] = wacc[1][0][r] = wacc[2][0][r] = 0.f;
  const int chunks_x = (Tx + kTileBwdChunk - 1) / kTileBwdChunk;
  const int chunks = SELF ? chunks_x : chunks_x + (Ts + kTileBwdChunk - 1) / kTileBwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const QpChunk c = qp_chunk<SELF>(ch, chunks_x, Tx, Ts, kTileBwdChunk);
    const size_t t0 = c.t0 + wave * kTile;                         // past T in the last chunk: a tile of zeros
    const float4* F = F0 + opaque_zero();
    if (c.side == 0) {
      const float* const g[3] = {gq, gk, gv};
      qp_bwd_chunk<3, WGRAD>(g, F, x, d_x, t0, c.T, wave, lane, qp_lds, wacc);
    } else if (c.side == 1) {
      const float* const g[1] = {gq};
      qp_bwd_chunk<1, WGRAD>(g, F, x, d_x, t0, c.T, wave, lane, qp_lds, wacc);
    } else {
      const float* const g[2] = {gk, gv};
      qp_bwd_chunk<2, WGRAD>(g, F + kQpMat / 4, src, d_src, t0, c.T, wave, lane, qp_lds, wacc + 1);
    }
  }
  if (WGRAD) {
    float* slab = part + (size_t)blockIdx.x * kQpSlab + 32 * (wave >> 1) * 64 + 32 * (wave & 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) tile_out(slab + j * kQpMat, 64, lane, wacc[j][0]);
  }
}

// the three weight gradients = the sum of the n_part slabs (fold_slabs' order)
__global__ __launch_bounds__(256) void k_qp_fold(const float* __restrict__ part, int n_part, float* __restrict__ d_wq,
                                                 float* __restrict__ d_wk, float* __restrict__ d_wv) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, i = blockIdx.x * 32 + x;
  float v;
  if (!fold_slabs(part + i, n_part, kQpSlab, red, &v)) return;
  if (i < kQpMat) d_wq[i] = v;
  else if (i < 2 * kQpMat) d_wk[i - kQpMat] = v;
  else d_wv[i - 2 * kQpMat] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool qp_route(int Tx, int Ts, int d) { return d == 64 && Tx <= kTileMaxT && Ts <= kTileMaxT; }
static int qp_chunks(int T, int chunk) { return (T + chunk - 1) / chunk; }
// workgroups of a kernel whose chunk holds `chunk` tokens
static int qp_groups(int Tx, int Ts, bool self, int chunk) {
  const int c = qp_chunks(Tx, chunk) + (self ? 0 : qp_chunks(Ts, chunk));
  return c < kTileMaxGroups ? c : kTileMaxGroups;
}
// Workspace of either call: the fragments | one slab per workgroup of the backward.  The query does not know the mode:
// the slabs are counted for cross mode, which has no fewer workgroups than self mode.
struct QpWs { Region<float> frag, part; size_t total; };
static QpWs qp_layout(int Tx, int Ts) {
  QpWs w;
  Carver c;
  c.take(w.frag, kQpFrag);
  c.take(w.part, (size_t)qp_groups(Tx, Ts, false, kTileBwdChunk) * kQpSlab);
  w.total = c.pad();
  return w;
}

// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct QpCall {
  const float *x, *src, *wq, *wk, *wv;
  int Tx, Ts, d;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float *q, *k, *v;                                              // forward
  const float *gq, *gk, *gv; float *d_x, *d_src, *d_wq, *d_wk, *d_wv;     // backward
  bool self() const { return src == x; }
};

// the ONLY copy of the two entry points' argument checks; *wgrad is set with FM_OK
static int qp_status(const QpCall& c, bool* wgrad) {
  if (!c.x || !c.src || !c.wq || !c.wk || !c.wv) return FM_E_NULL;
  if (c.backward ? (!c.gq || !c.gk || !c.gv || !c.d_x) : (!c.q || !c.k || !c.v)) return FM_E_NULL;
  const int given = !!c.d_wq + !!c.d_wk + !!c.d_wv;
  if (given != 0 && given != 3) return FM_E_NULL;
  if (c.backward && !c.self() && !c.d_src) return FM_E_NULL;
  if (c.Tx <= 0 || c.Ts <= 0 || c.d <= 0) return FM_E_SHAPE;
  if (c.self() && c.Ts != c.Tx) return FM_E_SHAPE;
  if (!qp_route(c.Tx, c.Ts, c.d)) return FM_E_UNSUPPORTED;
  if (!c.workspace || !workspace_ok(c.workspace, c.workspace_bytes, qp_layout(c.Tx, c.Ts).total)) return FM_E_WORKSPACE;
  *wgrad = given == 3;
  return FM_OK;
}

// f(bool_c<self>, bool_c<wgrad>): the four instantiations of the backward
template <bool V> using bool_c = std::integral_constant<bool, V>;
template <typename F>
static int qp_with_mode(bool self, bool wgrad, F&& f) {
  if (self) return wgrad ? f(bool_c<true>{}, bool_c<true>{}) : f(bool_c<true>{}, bool_c<false>{});
  return wgrad ? f(bool_c<false>{}, bool_c<true>{}) : f(bool_c<false>{}, bool_c<false>{});
}

static int qp_run(const QpCall& c) {
  bool wgrad = false;
  const int status = qp_status(c, &wgrad);
  if (status != FM_OK) return status;
  hipStream_t st = (hipStream_t)c.stream;
  const QpWs w = qp_layout(c.Tx, c.Ts);
  const bool self = c.self();
  float* frag = w.frag.in(c.workspace) + (c.backward ? kQpFwdFrag : 0);
  hipLaunchKernelGGL(k_qp_pack, dim3(3 * kQpMat / 256), dim3(256), 0, st, c.wq, c.wk, c.wv, (int)c.backward, (int)self, frag);
  if (!c.backward) {
    return qp_with_mode(self, false, [&](auto S, auto) -> int {
      constexpr bool kSelf = decltype(S)::value;
      static unsigned long long lds_fwd = 0;
      const hipError_t e = ensure_dynamic_lds(k_qp_fwd<kSelf>, kQpFwdLds, &lds_fwd);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(k_qp_fwd<kSelf>, dim3(qp_groups(c.Tx, c.Ts, self, kTileFwdChunk)), dim3(kTileFwdWaves * 64),
                         kQpFwdLds, st, c.x, c.src, (const float*)frag, c.Tx, c.Ts, c.q, c.k, c.v);
      return (int)hipGetLastError();
    });
  }
  const int groups = qp_groups(c.Tx, c.Ts, self, kTileBwdChunk);
  float* part = w.part.in(c.workspace);
  return qp_with_mode(self, wgrad, [&](auto S, auto G) -> int {
    constexpr bool kSelf = decltype(S)::value, kWgrad = decltype(G)::value;
    const int lds = kWgrad ? kQpBwdLds : 0;
    if (kWgrad) {
      static unsigned long long lds_bwd = 0;
      const hipError_t e = ensure_dynamic_lds(k_qp_bwd<kSelf, kWgrad>, lds, &lds_bwd);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((k_qp_bwd<kSelf, kWgrad>), dim3(groups), dim3(kTileBwdWaves * 64), lds, st, c.x, c.src, c.gq, c.gk,
                       c.gv, (const float*)frag, c.Tx, c.Ts, c.d_x, c.d_src, part);
    if (kWgrad)
      hipLaunchKernelGGL(k_qp_fold, dim3(kQpSlab / 32), dim3(256), 0, st, (const float*)part, groups, c.d_wq, c.d_wk, c.d_wv);
    return (int)hipGetLastError();
  });
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_qkv_projection_workspace_bytes(int Tx, int Ts, int d) {
  if (Tx <= 0 || Ts <= 0 || d <= 0 || !qp_route(Tx, Ts, d)) return 0;
  return qp_layout(Tx, Ts).total;
}

extern "C" int fm_qkv_projection_forward(const float* x, const float* src, const float* wq, const float* wk,
                                         const float* wv, int Tx, int Ts, int d, void* workspace, size_t workspace_bytes,
                                         float* q, float* k, float* v, void* stream) {
  QpCall c = {};
  c.x = x; c.src = src; c.wq = wq; c.wk = wk; c.wv = wv;
  c.Tx = Tx; c.Ts = Ts; c.d = d;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.q = q; c.k = k; c.v = v;
  return qp_run(c);
}

extern "C" int fm_qkv_projection_backward(const float* x, const float* src, const float* wq, const float* wk,
                                          const float* wv, const float* gq, const float* gk, const float* gv, int Tx, int Ts,
                                          int d, void* workspace, size_t workspace_bytes, float* d_x, float* d_src,
                                          float* d_wq, float* d_wk, float* d_wv, void* stream) {
  QpCall c = {};
  c.x = x; c.src = src; c.wq = wq; c.wk = wk; c.wv = wv;
  c.Tx = Tx; c.Ts = Ts; c.d = d;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.gq = gq; c.gk = gk; c.gv = gv;
  c.d_x = d_x; c.d_src = d_src; c.d_wq = d_wq; c.d_wk = d_wk; c.d_wv = d_wv;
  return qp_run(c);
}
