// The q / k / v projections of an encoder layer (transformer.py, EncoderLayer.forward: the three nn.Linear(64, 64,
// bias=False) lines in front of the attention) and their gradient, fused: the context layers' training path at the fine
// level, d_model = 64.  Float32 throughout:
//     q = x Wq^T          k = src Wk^T          v = src Wv^T
//     d_x   = gq Wq                    (+ gk Wk + gv Wv when src is x)
//     d_src = gk Wk + gv Wv            (cross layers only)
//     dWq = sum_t gq^T x     dWk = sum_t gk^T src     dWv = sum_t gv^T src
// Every product runs on v_mfma_f32_32x32x2_f32: exact float32, one rounding per product, a k-ordered fmaf chain.
//
// Tiling: encoder_tail.hip's.  A wave owns 32 tokens; the products are computed transposed, out^T [channel][token] =
// M [out][in] in^T, the token on the lane (lane & 31), a token's 64 channels in 32 registers of the lanes `lane` and
// `lane ^ 32` ("layout L": register R of lane half h <-> channel 8 (R >> 2) + 4 h + (R & 3)), loaded and stored as 16-byte
// pieces.  The A operand of k-step R is M[32 ot + (lane & 31)][channel(R, h)]: k_qp_pack writes the matrices in that order
// once per call ("fragments": [out tile][R >> 2][lane][R & 3]).  The three matrices are ONE matrix to the kernels:
//   forward  : [Wq; Wk; Wv], 192 x 64 - six output tiles over one load of x (self mode), or its rows 0..63 over x and its
//              rows 64..191 over src (cross mode);
//   backward : [Wq^T | Wk^T | Wv^T], 64 x 192, over the 96 registers (gq, gk, gv) of a token: the three data-gradient
//              products are one k-ordered sum in the accumulator (self mode), or Wq^T over gq and [Wk^T | Wv^T] over (gk, gv).
//   k_qp_fwd : 8 waves; the fragments (48 KB) in LDS.
//   k_qp_bwd : 4 waves; fragments from L2 (the LDS is the exchange below).  The weight gradients sum over TOKENS, which
//     sit on lanes: each wave writes its tile's operands transposed into an LDS image [channel][token] (rows: the one to
//     three gradients, then the input; 256 rows of 33 floats per wave) and, between two barriers, every wave multiplies
//     ITS output tile (wave >> 1, wave & 1) of each of dWq, dWk, dWv over all four images: 3 of the 12 tiles, 48
//     accumulator registers.  Per workgroup one slab of partial sums; k_qp_fold adds the slabs in a fixed order.
// Self mode (src == x) walks the chunks of x; cross mode walks the chunks of x, then those of src, in one grid: a chunk
// is the one kind or the other for the whole workgroup.  No atomics, grids that depend on Tx, Ts and the mode alone,
// fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_wave_device.h"

namespace fm {

constexpr int kQpTile = 32;                      // tokens of a wave's tile (the N of the MFMA)
constexpr int kQpFwdWaves = 8, kQpFwdChunk = kQpFwdWaves * kQpTile;     // 256 tokens per workgroup and round
constexpr int kQpBwdWaves = 4, kQpBwdChunk = kQpBwdWaves * kQpTile;     // 128
constexpr int kQpMaxGroups = 256;                // workgroups of either kernel (one per CU; the rest by grid stride)
constexpr int kQpMaxT = 1 << 24;                 // tokens of either side of one call (fmatch.h)
constexpr int kQpMat = 4096;                     // floats of one 64 x 64 matrix
// fragments, in floats: the forward's [Wq; Wk; Wv] | the backward's (self: [Wq^T | Wk^T | Wv^T]; cross: Wq^T, then
// [Wk^T | Wv^T])
constexpr int kQpFwdFrag = 3 * kQpMat, kQpFrag = 6 * kQpMat;
constexpr int kQpSlab = 3 * kQpMat;              // a slab of partial weight gradients, in floats: dWq | dWk | dWv
constexpr int kQpPitch = 33, kQpImage = 256 * kQpPitch;      // floats of an exchange row / of a wave's image
constexpr int kQpFwdLds = kQpFwdFrag * 4;
constexpr int kQpBwdLds = kQpBwdWaves * kQpImage * 4;
static_assert(kQpSlab % 32 == 0, "k_qp_fold's grid covers a slab exactly");
static_assert(kQpBwdLds <= 160 * 1024 && kQpFwdLds <= 160 * 1024, "one workgroup per CU");

// k_qp_pack.  Forward (tr = false): frag[idx], [ot][q][lane][e] = M[32 ot + (lane & 31)][8 q + 4 (lane >> 5) + e] of the
// 192 x 64 matrix M = [Wq; Wk; Wv].  Backward (tr = true): a 64 x 64 nmat matrix [W_first^T | ...], nmat = 3 from Wq on
// (self mode), else Wq^T alone at float 0 and [Wk^T | Wv^T] at float kQpMat.
__global__ __launch_bounds__(256) void k_qp_pack(const float* __restrict__ wq, const float* __restrict__ wk,
                                                 const float* __restrict__ wv, int tr, int self, float* __restrict__ frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * kQpMat) return;
  int idx = i, first = 0, nmat = 3;
  if (tr && !self) {
    if (i < kQpMat) nmat = 1;
    else { idx = i - kQpMat; first = 1; nmat = 2; }
  }
  const int e = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8;
  const int nq = tr ? 8 * nmat : 8;
  const int row = 32 * (rest / nq) + (lane & 31), col = 8 * (rest % nq) + 4 * (lane >> 5) + e;
  const int m = first + (tr ? col >> 6 : row >> 6);
  const float* W = m == 0 ? wq : m == 1 ? wk : wv;
  frag[i] = tr ? W[(col & 63) * 64 + row] : W[(row & 63) * 64 + col];
}

// 0, but not to the compiler: added to the base of the fragments once per round of the token loop, it keeps their loads -
// the same addresses in every round - from being hoisted out of the loop and spilled (encoder_tail.hip's note)
__device__ __forceinline__ int qp_opaque_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

// acc[ot] = rows 32 ot .. of M in^T for the wave's 32 tokens; in[R] in layout L (NK registers = 2 NK channels).  The
// fragments of group q + 2 are requested before the products of group q and nothing crosses a group's end
// (sched_barrier), so that loads from L2 stay two groups ahead of their use.
template <int NO, int NK>
__device__ __forceinline__ void qp_mm(const float4* __restrict__ F, const float (&in)[NK], f32x16 (&acc)[NO], int lane) {
#pragma unroll
  for (int ot = 0; ot < NO; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ot][r] = 0.f;
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

// rows t0 .. t0 + 31 of a [T, 64] tensor <-> layout L; rows past T read as 0 and are not written
__device__ __forceinline__ void qp_load(const float* __restrict__ p, size_t t0, int T, int lane, float* __restrict__ v) {
  const size_t tok = t0 + (lane & 31);
  const bool live = tok < (size_t)T;
  const float4* s = reinterpret_cast<const float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 r = live ? s[2 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
  }
}
// tiles a, a + 1 of an accumulator -> rows t0 .. of a [T, 64] tensor
__device__ __forceinline__ void qp_store(float* __restrict__ p, size_t t0, int T, int lane, const f32x16& a, const f32x16& b) {
  const size_t tok = t0 + (lane & 31);
  if (tok >= (size_t)T) return;
  float4* s = reinterpret_cast<float4*>(p + tok * 64 + 4 * (lane >> 5));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[2 * q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    s[2 * q + 8] = make_float4(b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]);
  }
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
__global__ __launch_bounds__(kQpFwdWaves * 64) void k_qp_fwd(const float* __restrict__ x, const float* __restrict__ src,
                                                             const float* __restrict__ frag, int Tx, int Ts,
                                                             float* __restrict__ q, float* __restrict__ k,
                                                             float* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) float qp_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kQpFwdFrag / 4; i += kQpFwdWaves * 64)
    reinterpret_cast<float4*>(qp_lds)[i] = reinterpret_cast<const float4*>(frag)[i];
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(qp_lds);
  const int chunks_x = (Tx + kQpFwdChunk - 1) / kQpFwdChunk;
  const int chunks = SELF ? chunks_x : chunks_x + (Ts + kQpFwdChunk - 1) / kQpFwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const QpChunk c = qp_chunk<SELF>(ch, chunks_x, Tx, Ts, kQpFwdChunk);
    const size_t t0 = c.t0 + wave * kQpTile;
    if (t0 >= (size_t)c.T) continue;
    const float4* F = F0 + qp_opaque_zero();
    float in[32];
    if (c.side == 0) {
      qp_load(x, t0, c.T, lane, in);
      f32x16 acc[6];
      qp_mm<6, 32>(F, in, acc, lane);
      qp_store(q, t0, c.T, lane, acc[0], acc[1]);
      qp_store(k, t0, c.T, lane, acc[2], acc[3]);
      qp_store(v, t0, c.T, lane, acc[4], acc[5]);
    } else if (c.side == 1) {
      qp_load(x, t0, c.T, lane, in);
      f32x16 acc[2];
      qp_mm<2, 32>(F, in, acc, lane);
      qp_store(q, t0, c.T, lane, acc[0], acc[1]);
    } else {
      qp_load(src, t0, c.T, lane, in);
      f32x16 acc[4];
      qp_mm<4, 32>(F + kQpMat / 4, in, acc, lane);
      qp_store(k, t0, c.T, lane, acc[0], acc[1]);
      qp_store(v, t0, c.T, lane, acc[2], acc[3]);
    }
  }
}

// the wave's image: row (row0 + channel) <- v (32 registers in layout L), column = token
__device__ __forceinline__ void qp_put(float* __restrict__ E, int row0, int lane, const float* __restrict__ v) {
  float* e = E + (row0 + 4 * (lane >> 5)) * kQpPitch + (lane & 31);
#pragma unroll
  for (int R = 0; R < 32; ++R) e[(8 * (R >> 2) + (R & 3)) * kQpPitch] = v[R];
}
// acc[out][in] += sum over the chunk's 128 tokens of rows rowA.. (out) times rows rowB.. (in): the waves' images in index
// order, the tokens of each in order
__device__ __forceinline__ void qp_wgrad(const float* __restrict__ E, int rowA, int rowB, int lane, f32x16& acc) {
  const int at = (lane & 31) * kQpPitch + (lane >> 5);
  for (int w = 0; w < kQpBwdWaves; ++w) {
    const float* pa = E + w * kQpImage + rowA * kQpPitch + at;
    const float* pb = E + w * kQpImage + rowB * kQpPitch + at;
#pragma unroll 4
    for (int s = 0; s < kQpTile / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s], pb[2 * s], acc, 0, 0, 0);
  }
}
// tile -> slab: D[i][j] at col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void qp_tile_out(float* __restrict__ dst, int lane, const f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 64 + (lane & 31)] = acc[r];
}

// One chunk of the backward: NG gradients g[0 .. NG) [T, 64] against the fragments FT of [W_0^T | .. | W_{NG-1}^T]; `in`
// is their common input, `out` its gradient.  WGRAD: wacc[j] += this wave's tile of sum_t g[j]^T in over the chunk.
template <int NG, bool WGRAD>
__device__ __forceinline__ void qp_bwd_chunk(const float* const (&g)[NG], const float4* __restrict__ FT,
                                             const float* __restrict__ in, float* __restrict__ out, size_t t0, int T,
                                             int wave, int lane, float* __restrict__ E, f32x16* __restrict__ wacc) {
  float gv[32 * NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) qp_load(g[j], t0, T, lane, gv + 32 * j);
  if (WGRAD) {
    float vin[32];
    qp_load(in, t0, T, lane, vin);
    float* Ew = E + wave * kQpImage;
#pragma unroll
    for (int j = 0; j < NG; ++j) qp_put(Ew, 64 * j, lane, gv + 32 * j);
    qp_put(Ew, 64 * NG, lane, vin);
  }
  {
    f32x16 acc[2];
    qp_mm<2, 32 * NG>(FT, gv, acc, lane);
    qp_store(out, t0, T, lane, acc[0], acc[1]);
  }
  if (WGRAD) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NG; ++j) qp_wgrad(E, 64 * j + 32 * (wave >> 1), 64 * NG + 32 * (wave & 1), lane, wacc[j]);
    __syncthreads();
  }
}

// WGRAD = false: d_x (and d_src) only - no exchange, no barriers, no LDS, `part` unused
template <bool SELF, bool WGRAD>
__global__ __launch_bounds__(kQpBwdWaves * 64) void k_qp_bwd(const float* __restrict__ x, const float* __restrict__ src,
                                                             const float* __restrict__ gq, const float* __restrict__ gk,
                                                             const float* __restrict__ gv, const float* __restrict__ frag,
                                                             int Tx, int Ts, float* __restrict__ d_x,
                                                             float* __restrict__ d_src, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float qp_lds[];     // [wave][256 rows][kQpPitch]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float4* F0 = reinterpret_cast<const float4*>(frag);
  f32x16 wacc[3];                                                    // this wave's tile of dWq, dWk, dWv
#pragma unroll
  for (int r = 0; r < 16; ++r) wacc[0][r] = wacc[1][r] = wacc[2][r] = 0.f;
  const int chunks_x = (Tx + kQpBwdChunk - 1) / kQpBwdChunk;
  const int chunks = SELF ? chunks_x : chunks_x + (Ts + kQpBwdChunk - 1) / kQpBwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const QpChunk c = qp_chunk<SELF>(ch, chunks_x, Tx, Ts, kQpBwdChunk);
    const size_t t0 = c.t0 + wave * kQpTile;                         // past T in the last chunk: a tile of zeros
    const float4* F = F0 + qp_opaque_zero();
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
    for (int j = 0; j < 3; ++j) qp_tile_out(slab + j * kQpMat, lane, wacc[j]);
  }
}

// the three weight gradients = the sum of the n_part slabs, in a fixed order (k_et_fold's: 8 slices of every 8th slab,
// then the slices in index order)
__global__ __launch_bounds__(256) void k_qp_fold(const float* __restrict__ part, int n_part, float* __restrict__ d_wq,
                                                 float* __restrict__ d_wk, float* __restrict__ d_wv) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, j = threadIdx.x >> 5, i = blockIdx.x * 32 + x;
  const float* p = part + i;
  float s = 0.f;
#pragma unroll 4
  for (int c = j; c < n_part; c += 8) s += p[(size_t)c * kQpSlab];
  red[j][x] = s;
  __syncthreads();
  if (j != 0) return;
  const float v = ((((((red[0][x] + red[1][x]) + red[2][x]) + red[3][x]) + red[4][x]) + red[5][x]) + red[6][x]) + red[7][x];
  if (i < kQpMat) d_wq[i] = v;
  else if (i < 2 * kQpMat) d_wk[i - kQpMat] = v;
  else d_wv[i - 2 * kQpMat] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------
static bool qp_route(int Tx, int Ts, int d) { return d == 64 && Tx <= kQpMaxT && Ts <= kQpMaxT; }
static int qp_chunks(int T, int chunk) { return (T + chunk - 1) / chunk; }
// workgroups of a kernel whose chunk holds `chunk` tokens
static int qp_groups(int Tx, int Ts, bool self, int chunk) {
  const int c = qp_chunks(Tx, chunk) + (self ? 0 : qp_chunks(Ts, chunk));
  return c < kQpMaxGroups ? c : kQpMaxGroups;
}
// Workspace of either call: the fragments | one slab per workgroup of the backward.  The query does not know the mode:
// the slabs are counted for cross mode, which has no fewer workgroups than self mode.
struct QpWs { Region<float> frag, part; size_t total; };
static QpWs qp_layout(int Tx, int Ts) {
  QpWs w;
  Carver c;
  c.take(w.frag, kQpFrag);
  c.take(w.part, (size_t)qp_groups(Tx, Ts, false, kQpBwdChunk) * kQpSlab);
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
      hipLaunchKernelGGL(k_qp_fwd<kSelf>, dim3(qp_groups(c.Tx, c.Ts, self, kQpFwdChunk)), dim3(kQpFwdWaves * 64),
                         kQpFwdLds, st, c.x, c.src, (const float*)frag, c.Tx, c.Ts, c.q, c.k, c.v);
      return (int)hipGetLastError();
    });
  }
  const int groups = qp_groups(c.Tx, c.Ts, self, kQpBwdChunk);
  float* part = w.part.in(c.workspace);
  return qp_with_mode(self, wgrad, [&](auto S, auto G) -> int {
    constexpr bool kSelf = decltype(S)::value, kWgrad = decltype(G)::value;
    const int lds = kWgrad ? kQpBwdLds : 0;
    if (kWgrad) {
      static unsigned long long lds_bwd = 0;
      const hipError_t e = ensure_dynamic_lds(k_qp_bwd<kSelf, kWgrad>, lds, &lds_bwd);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((k_qp_bwd<kSelf, kWgrad>), dim3(groups), dim3(kQpBwdWaves * 64), lds, st, c.x, c.src, c.gq, c.gk,
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
