// Window crop + context merge of FinePreprocess as one differentiable op (modules.py, FinePreprocess.forward: the crop,
// then merge_feat over cat[window, expand(down_proj(coarse descriptors))]), per image, float32 throughout.  The
// position-independent half of merge_feat - its columns 64.., the bias and down_proj - arrives as one row per match:
//     win[m, r, c] = feat_f[b_m, c, stride y - pad + r / W, stride x - pad + r % W]      (0 outside the map)
//     out[m, r, :] = Ww win[m, r, :] + ctx[m, :]
//     d_ctx[m, :]  = sum_r g[m, r, :]
//     d_Ww         = sum_{m, r} g[m, r, :]^T win[m, r, :]       (win cropped again from the map)
//     d_feat       = crop adjoint of (g Ww)
// Every product runs on v_mfma_f32_32x32x2_f32: exact float32, one rounding per product, a k-ordered fmaf chain.
//
// Tiling: fm_tile_device.h's (layout L, fragments, the exchange image).  A token is one (m, r) pair, T = m_max W W of
// them; a wave owns 32 consecutive tokens.  k_wm_pack writes M = Ww (forward) or Ww^T (backward) as fragments once per call.
// The loader (wm_crop) is the crop: a lane's token gives (b, y0 + r / W, x0 + r % W); NCHW reads one float per register
// and lane - the 32 lanes of a register's load walk runs of W consecutive pixels of one channel plane - channels-last
// reads the token's 256-byte record as 16-byte pieces, as tile_load does.  A pixel outside the map, a row whose sample or
// cell lies outside the batch or the grid (the crop's adjoint leaves such a row out as well) and a token past T read 0.
//   k_wm_fwd  : 8 waves; the fragments (16 KB) in LDS; writes out alone.
//   k_wm_bwd  : 4 waves; fragments from L2.  g Ww goes to the workspace as [m_max, WW, 64]: the map's gradient is
//     fm_gather_windows_backward (fine_grad.hip: CSR of matches per cell, one wave per pixel, a fixed order) on it.  The
//     weight gradient: each wave writes g and the cropped window into its image (128 rows per wave) and every wave
//     multiplies ITS tile (wave >> 1, wave & 1) of d_Ww over all four images; k_wm_fold adds the workgroups' slabs.
//     WGRAD = false: no crop, no exchange, no barriers, no LDS.  DATA = false (d_feat == NULL): no product, no g Ww, no
//     crop backward.
//   k_wm_dctx : one wave per match at a time, lane = channel, r ascending: one owner per row.
// No float atomics, grids that depend on the arguments alone (at most 256 workgroups, a grid stride over the chunks),
// fixed summation orders: the same inputs give the same bits.
#include "fm_internal.h"
#include "fm_tile_device.h"

namespace fm {

constexpr int kWmMat = 4096;                     // floats of the 64 x 64 matrix: its fragments, a slab of partial sums
constexpr int kWmImage = 128 * kTilePitch;       // floats of a wave's image
constexpr int kWmFwdLds = kWmMat * 4;
constexpr int kWmBwdLds = kTileBwdWaves * kWmImage * 4;
static_assert(kWmMat % 32 == 0, "k_wm_fold's grid covers a slab exactly");
static_assert(kWmBwdLds <= 160 * 1024 && kWmFwdLds <= 160 * 1024, "one workgroup per CU");

// the fragments of M = Ww (tr = 0) or Ww^T (tr = 1)
__global__ __launch_bounds__(256) void k_wm_pack(const float* __restrict__ w, int tr, float* __restrict__ frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kWmMat) frag[i] = frag_value(w, 64, 64, tr != 0, i);
}

// the map and the grid of one call
struct WmMap {
  const float* feat; int N, Hf, Wf, layout, stride, pad, h_c, w_c;
  const int64_t *b_ids, *ids;
};

// token tok = m WW + r -> the window element (m, r) of the map in layout L; 0 where the crop reads nothing
template <int W>
__device__ __forceinline__ void wm_crop(const WmMap& g, size_t tok, bool live, int lane, float* __restrict__ v) {
  constexpr int WW = W * W;
  bool in = false;
  long at = 0;                                       // NCHW: float (b, channel 0, py, px); channels-last: float (b, py, px, 0)
  if (live) {
    const int m = (int)(tok / WW), r = (int)(tok - (size_t)m * WW);
    const int64_t b = g.b_ids[m], id = g.ids[m];
    if (b >= 0 && b < g.N && id >= 0 && id < (int64_t)g.h_c * g.w_c) {
      const int y = (int)(id / g.w_c), x = (int)(id - (int64_t)y * g.w_c);
      const int py = g.stride * y - g.pad + r / W, px = g.stride * x - g.pad + r % W;
      in = py >= 0 && py < g.Hf && px >= 0 && px < g.Wf;
      at = g.layout == 0 ? ((long)b * 64 * g.Hf + py) * g.Wf + px : (((long)b * g.Hf + py) * g.Wf + px) * 64;
    }
  }
  const int h = lane >> 5;
  if (g.layout == 0) {
    const long plane = (long)g.Hf * g.Wf;
    const float* s = g.feat + at + 4 * h * plane;
#pragma unroll
    for (int R = 0; R < 32; ++R) v[R] = in ? s[(8 * (R >> 2) + (R & 3)) * plane] : 0.f;
  } else {
    const float4* s = reinterpret_cast<const float4*>(g.feat + at + 4 * h);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 r = in ? s[2 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * q] = r.x; v[4 * q + 1] = r.y; v[4 * q + 2] = r.z; v[4 * q + 3] = r.w;
    }
  }
}

template <int W>
__global__ __launch_bounds__(kTileFwdWaves * 64) void k_wm_fwd(WmMap g, const float* __restrict__ frag,
                                                               const float* __restrict__ ctx, int T, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float wm_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kWmMat / 4; i += kTileFwdWaves * 64)     // (written out: a helper moves the loop in the kernel)
    reinterpret_cast<float4*>(wm_lds)[i] = reinterpret_cast<const float4*>(frag)[i];
  __syncthreads();
  const float4* F0 = reinterpret_cast<const float4*>(wm_lds);
  const int chunks = (T + kTileFwdChunk - 1) / kTileFwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kTileFwdChunk + wave * kTile;
    if (t0 >= (size_t)T) continue;
    const size_t tok = t0 + (lane & 31);
    const bool live = tok < (size_t)T;
    const float4* F = F0 + opaque_zero();
    float in[32];
    wm_crop<W>(g, tok, live, lane, in);
    f32x16 acc[2];
    tile_mm<2, 32>(F, in, acc, lane);
    tile_store(out, tok, live, lane, live ? ctx + (tok / (W * W)) * 64 : nullptr, acc[0], acc[1]);
  }
}

// WGRAD = false: g Ww only - no crop, no exchange, no barriers, no LDS, `part` unused.  DATA = false (the map wants no
// gradient): no product, `frag` and `gw` unused.
template <int W, bool WGRAD, bool DATA>
__global__ __launch_bounds__(kTileBwdWaves * 64) void k_wm_bwd(WmMap g, const float* __restrict__ frag,
                                                               const float* __restrict__ grad, int T, float* __restrict__ gw,
                                                               float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float wm_lds[];     // [wave][128 rows][kTilePitch]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float4* F0 = reinterpret_cast<const float4*>(frag);
  f32x16 wacc[1];                                                    // this wave's tile of d_Ww
#pragma unroll
  for (int r = 0; r < 16; ++r) wacc[0][r] = 0.f;
  const int chunks = (T + kTileBwdChunk - 1) / kTileBwdChunk;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const size_t t0 = (size_t)ch * kTileBwdChunk + wave * kTile;     // past T in the last chunk: a tile of zeros
    const size_t tok = t0 + (lane & 31);
    const bool live = tok < (size_t)T;
    const float4* F = F0 + opaque_zero();
    float gv[32];
    tile_load(grad, t0, T, lane, gv);
    if (WGRAD) {
      float vin[32];
      wm_crop<W>(g, tok, live, lane, vin);
      float* Ew = wm_lds + wave * kWmImage;
      tile_put<32>(Ew, 0, lane, gv);
      tile_put<32>(Ew, 64, lane, vin);
    }
    if (DATA) {
      f32x16 acc[2];
      tile_mm<2, 32>(F, gv, acc, lane);
      tile_store(gw, tok, live, lane, nullptr, acc[0], acc[1]);      // (+ 0 as it was: -0 is stored as +0)
    }
    if (WGRAD) {
      __syncthreads();
      tile_wgrad<1, kTileBwdWaves, kWmImage>(wm_lds, 32 * (wave >> 1), 64 + 32 * (wave & 1), lane, wacc);
      __syncthreads();
    }
  }
  if (WGRAD) tile_out(part + (size_t)blockIdx.x * kWmMat + 32 * (wave >> 1) * 64 + 32 * (wave & 1), 64, lane, wacc[0]);
}

// d_Ww = the sum of the n_part slabs (fold_slabs' order)
__global__ __launch_bounds__(256) void k_wm_fold(const float* __restrict__ part, int n_part, float* __restrict__ d_w) {
  __shared__ float red[8][32];
  const int x = threadIdx.x & 31, i = blockIdx.x * 32 + x;
  float v;
  if (fold_slabs(part + i, n_part, kWmMat, red, &v)) d_w[i] = v;
}

// d_ctx[m][lane] = sum_r g[m][r][lane], r ascending
__global__ __launch_bounds__(256) void k_wm_dctx(const float* __restrict__ grad, int m_max, int WW, float* __restrict__ d_ctx) {
  const int lane = threadIdx.x & 63;
  for (int m = blockIdx.x * 4 + (threadIdx.x >> 6); m < m_max; m += gridDim.x * 4) {
    const float* p = grad + (size_t)m * WW * 64 + lane;
    float s = 0.f;
#pragma unroll 7
    for (int r = 0; r < WW; ++r) s += p[r * 64];
    d_ctx[(size_t)m * 64 + lane] = s;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
// what the workspace query knows of a call: the batch, the grid, the list and the window
static bool wm_sizes_ok(int N, int h_c, int w_c, int m_max, int W) { return N > 0 && h_c > 0 && w_c > 0 && m_max >= 0 && W > 0; }
static bool wm_route(int N, int h_c, int w_c, int m_max, int W) {
  return (W == 5 || W == 7) && (long)m_max * W * W <= kTileMaxT && (long)N * h_c * w_c < (1L << 31) - 1;
}
// Workspace of either call: the fragments of Ww, then of Ww^T | one slab per workgroup of the backward | g Ww
// [m_max, WW, 64] | the crop backward's own workspace (its CSR)
struct WmWs { Region<float> frag, part, gw; Region<char> crop; size_t crop_bytes, total; };
static WmWs wm_layout(int N, int h_c, int w_c, int m_max, int W) {
  WmWs w;
  Carver c;
  const size_t T = (size_t)m_max * W * W;
  c.take(w.frag, 2 * kWmMat);
  c.take(w.part, (size_t)token_groups((long)T, kTileBwdChunk) * kWmMat);
  c.take(w.gw, T * 64);
  w.crop_bytes = fm_gather_windows_backward_workspace_bytes(N, h_c, w_c, m_max);
  c.take(w.crop, w.crop_bytes);
  w.total = c.pad();
  return w;
}

// One call of either entry point as the C ABI takes it; what an entry point does not have stays NULL.
struct WmCall {
  const float* feat_f; int N, Cf, Hf, Wf, layout, W, stride, pad, h_c, w_c;
  const float *w_win, *ctx; const int64_t *b_ids, *ids; int m_max;
  void* workspace; size_t workspace_bytes; void* stream;
  bool backward;
  float* out;                                                     // forward
  const float* g; float *d_feat, *d_w_win, *d_ctx;                // backward (d_feat and d_w_win may be NULL)
};

// the ONLY copy of the two entry points' argument checks (m_max == 0 is FM_OK before them)
static int wm_status(const WmCall& c) {
  if (!c.feat_f || !c.w_win || !c.ctx || !c.b_ids || !c.ids) return FM_E_NULL;
  if (c.backward ? (!c.g || !c.d_ctx) : !c.out) return FM_E_NULL;
  if (!crop_shape_ok(c.N, c.Hf, c.Wf, c.stride, c.m_max) || !wm_sizes_ok(c.N, c.h_c, c.w_c, c.m_max, c.W) || c.Cf <= 0)
    return FM_E_SHAPE;
  if (c.Cf != 64 || c.pad < 0 || (c.layout != 0 && c.layout != 1) || !wm_route(c.N, c.h_c, c.w_c, c.m_max, c.W))
    return FM_E_UNSUPPORTED;
  if ((long)c.N * c.Hf >= (1L << 31) / (((long)c.Wf + 7) / 8)) return FM_E_UNSUPPORTED;      // (the crop backward's grid)
  if (!c.workspace || !workspace_ok(c.workspace, c.workspace_bytes, wm_layout(c.N, c.h_c, c.w_c, c.m_max, c.W).total))
    return FM_E_WORKSPACE;
  return FM_OK;
}

template <int W>
static int wm_launch(const WmCall& c, const WmWs& w, const WmMap& map, int T, hipStream_t st) {
  float* frag = w.frag.in(c.workspace) + (c.backward ? kWmMat : 0);
  hipLaunchKernelGGL(k_wm_pack, dim3(kWmMat / 256), dim3(256), 0, st, c.w_win, (int)c.backward, frag);
  if (!c.backward) {
    static unsigned long long lds_fwd = 0;
    const hipError_t e = ensure_dynamic_lds(k_wm_fwd<W>, kWmFwdLds, &lds_fwd);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wm_fwd<W>, dim3(token_groups(T, kTileFwdChunk)), dim3(kTileFwdWaves * 64), kWmFwdLds, st, map,
                       (const float*)frag, c.ctx, T, c.out);
    return (int)hipGetLastError();
  }
  const int groups = token_groups(T, kTileBwdChunk);
  float* part = w.part.in(c.workspace);
  float* gw = w.gw.in(c.workspace);
  const dim3 grid(groups), block(kTileBwdWaves * 64);
  if (c.d_w_win) {
    static unsigned long long lds_data = 0, lds_only = 0;
    const hipError_t e = c.d_feat ? ensure_dynamic_lds(k_wm_bwd<W, true, true>, kWmBwdLds, &lds_data)
                                  : ensure_dynamic_lds(k_wm_bwd<W, true, false>, kWmBwdLds, &lds_only);
    if (e != hipSuccess) return (int)e;
    if (c.d_feat)
      hipLaunchKernelGGL((k_wm_bwd<W, true, true>), grid, block, kWmBwdLds, st, map, (const float*)frag, c.g, T, gw, part);
    else
      hipLaunchKernelGGL((k_wm_bwd<W, true, false>), grid, block, kWmBwdLds, st, map, (const float*)frag, c.g, T, gw, part);
    hipLaunchKernelGGL(k_wm_fold, dim3(kWmMat / 32), dim3(256), 0, st, (const float*)part, groups, c.d_w_win);
  } else if (c.d_feat) {
    hipLaunchKernelGGL((k_wm_bwd<W, false, true>), grid, block, 0, st, map, (const float*)frag, c.g, T, gw, part);
  }
  const int rows = (c.m_max + 3) / 4;
  hipLaunchKernelGGL(k_wm_dctx, dim3(rows < kTileMaxGroups ? rows : kTileMaxGroups), dim3(256), 0, st, c.g, c.m_max, W * W,
                     c.d_ctx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !c.d_feat) return (int)e;
  // the map's gradient: the crop's adjoint of g Ww (every element of d_feat written, +0 where no window reads)
  return fm_gather_windows_backward(gw, c.b_ids, c.ids, nullptr, c.m_max, c.N, 64, c.Hf, c.Wf, c.layout, W, c.stride, c.pad,
                                    c.h_c, c.w_c, w.crop.in(c.workspace), w.crop_bytes, c.d_feat, c.stream);
}

static int wm_run(const WmCall& c) {
  if (c.m_max == 0) return FM_OK;
  const int status = wm_status(c);
  if (status != FM_OK) return status;
  const WmWs w = wm_layout(c.N, c.h_c, c.w_c, c.m_max, c.W);
  const WmMap map = {c.feat_f, c.N, c.Hf, c.Wf, c.layout, c.stride, c.pad, c.h_c, c.w_c, c.b_ids, c.ids};
  const int T = c.m_max * c.W * c.W;
  int result = FM_OK;
  with_window(c.W, [&](auto w_c) { result = wm_launch<decltype(w_c)::value>(c, w, map, T, (hipStream_t)c.stream); });
  return result;
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_window_merge_workspace_bytes(int N, int h_c, int w_c, int m_max, int W) {
  if (!wm_sizes_ok(N, h_c, w_c, m_max, W) || !wm_route(N, h_c, w_c, m_max, W)) return 0;
  return wm_layout(N, h_c, w_c, m_max, W).total;
}

extern "C" int fm_window_merge_forward(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout, int W, int stride,
                                       int pad, int h_c, int w_c, const float* w_win, const float* ctx, const int64_t* b_ids,
                                       const int64_t* ids, int m_max, void* workspace, size_t workspace_bytes, float* out,
                                       void* stream) {
  WmCall c = {};
  c.feat_f = feat_f; c.N = N; c.Cf = Cf; c.Hf = Hf; c.Wf = Wf; c.layout = layout; c.W = W; c.stride = stride; c.pad = pad;
  c.h_c = h_c; c.w_c = w_c; c.w_win = w_win; c.ctx = ctx; c.b_ids = b_ids; c.ids = ids; c.m_max = m_max;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.out = out;
  return wm_run(c);
}

extern "C" int fm_window_merge_backward(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout, int W, int stride,
                                        int pad, int h_c, int w_c, const float* w_win, const float* ctx, const int64_t* b_ids,
                                        const int64_t* ids, int m_max, const float* g, void* workspace,
                                        size_t workspace_bytes, float* d_feat, float* d_w_win, float* d_ctx, void* stream) {
  WmCall c = {};
  c.feat_f = feat_f; c.N = N; c.Cf = Cf; c.Hf = Hf; c.Wf = Wf; c.layout = layout; c.W = W; c.stride = stride; c.pad = pad;
  c.h_c = h_c; c.w_c = w_c; c.w_win = w_win; c.ctx = ctx; c.b_ids = b_ids; c.ids = ids; c.m_max = m_max;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.backward = true;
  c.g = g; c.d_feat = d_feat; c.d_w_win = d_w_win; c.d_ctx = d_ctx;
  return wm_run(c);
}
