// Training surface of the fine stage: the backward of the fine matching (network/utils/fine_matching_new.py:50-79) and
// of the window crop (network/module/fine_preprocess.py:43-50, F.unfold + select).
//
// fm_fine_match_backward, per match and direction (direction 0 shown; direction 1 swaps the windows), t = 1/sqrt(64),
// g = d_out0[m], Wh = W/2, (gx, gy) = the kornia grid:
//     q = sum_r mix[r] win0[r,:] + mix[WW]      s[r] = t q . win1[r,:]      h = softmax(s)
//     co = (sum h gx, sum h gy)     var = (sum h gx^2, sum h gy^2) - co^2
//     dvar_k = g[2] / (2 sqrt(var_k)) if var_k >= 1e-10 else 0   (what torch.clamp(min=1e-10) passes back)
//     dco_k  = g[k] Wh scale_f - 2 co_k dvar_k
//     dh[r]  = dco_x gx + dco_y gy + dvar_x gx^2 + dvar_y gy^2,   ds[r] = h[r] (dh[r] - sum_r' h[r'] dh[r'])
//     dq     = t sum_r ds[r] win1[r,:]
//     d_win1[r,:] += t ds[r] q      d_win0[r,:] += mix[r] dq      d_mix[r] += dq . win0[r,:]      d_mix[WW] += sum dq
// One wave per match, lane = channel, as k_fine: q, the similarities and the heat map are recomputed with the forward's
// own device code (fm_fine_device.h: the same products, transpose-reduce, wave maximum and __expf), so the gradient is
// that of the function the forward evaluated.  sum_r h dh follows from the forward's five sums (E[gx], E[gy], E[gx^2],
// E[gy^2]) without another reduction.  d_mix is a sum over matches: per-match partials go to a workspace and a second
// kernel adds them in a fixed order - no float atomics, every output bitwise reproducible.
//
// fm_gather_windows_backward: the adjoint of the crop, d_feat[b, :, y, x] = sum of d_win[m, r, :] over every (match,
// window position) that read pixel (y, x) of sample b.  Gather form: a CSR of matches per (b, cell) - integer count,
// scan, fill, each cell's list sorted by match index - then one wave per output pixel visits the at most
// ceil(W/stride)^2 cells whose windows cover it (row-major) and their matches in ascending index, lane = channel (the
// window rows are 256-byte channel records at Cf = 64).  The fixed order makes the sums bitwise reproducible without
// float atomics; the unfold of every cell ([N, L, WW, Cf], 60 MB per image at 640x480) and its fold never exist.
// Pixels are staged in an LDS tile [pixel][channel] (odd pitch) and leave coalesced in either layout: NCHW as runs of
// one channel along x, channels-last as one contiguous block.
// float32 vector arithmetic throughout (a training path; its bar is float64 autograd, tests/test_gpu_fine_grad.py).
#include "fm_device.h"
#include "fm_fine_device.h"

namespace fm {

// ---- fine matching backward ----
template <int W>
__global__ __launch_bounds__(256) void k_fine_bwd(const float* __restrict__ win0, const float* __restrict__ win1, int m_max,
                                                  const int32_t* __restrict__ d_count, const float* __restrict__ mix0,
                                                  const float* __restrict__ mix1, float scale_f,
                                                  const float* __restrict__ d_out0, const float* __restrict__ d_out1,
                                                  float* __restrict__ d_win0, float* __restrict__ d_win1,
                                                  float* __restrict__ part) {
  constexpr int WW = W * W, CF = 64, NP = WW > 32 ? 64 : 32, NPART = 2 * (WW + 1);
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= m_max) return;
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  float* g0 = d_win0 + (long)m * WW * CF + lane;
  float* g1 = d_win1 + (long)m * WW * CF + lane;
  float* pm = part + (long)m * NPART;
  if (m >= M) {                                      // rows beyond the count: zero gradients, zero partials
#pragma unroll
    for (int r = 0; r < WW; ++r) { g0[r * CF] = 0.f; g1[r * CF] = 0.f; }
    for (int k = lane; k < NPART; k += 64) pm[k] = 0.f;
    return;
  }
  const float* p0 = win0 + (long)m * WW * CF + lane;
  const float* p1 = win1 + (long)m * WW * CF + lane;
  float f0[WW], f1[WW];
#pragma unroll
  for (int r = 0; r < WW; ++r) { f0[r] = p0[r * CF]; f1[r] = p1[r * CF]; }
  // the forward, recomputed with its own code
  const Mix2 q = fine_mix<W>(f0, f1, mix0, mix1);
  const Sims2 s = fine_sims<W>(f0, f1, q.q0, q.q1, lane);
  const Heat2 e = heat_exp2(s.sim0, s.sim1, s.on, kFineInvSqrtC);
  const float t = heat_sums2<W>(e.e0, e.e1, s.pos);
  float gx, gy;
  grid_xy<W>(s.pos, gx, gy);
  // ds of both directions at this lane's window position (0 in lanes that hold none)
  float ds[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float* g = (d ? d_out1 : d_out0) + (long)m * 3;
    const float inv = 1.0f / heat_sum(t, 5 * d);
    const float cx = heat_sum(t, 5 * d + 1) * inv, cy = heat_sum(t, 5 * d + 2) * inv;
    const float ex2 = heat_sum(t, 5 * d + 3) * inv, ey2 = heat_sum(t, 5 * d + 4) * inv;
    const float vx = ex2 - cx * cx, vy = ey2 - cy * cy;
    const float dvx = vx >= 1e-10f ? g[2] * 0.5f / sqrtf(vx) : 0.f;
    const float dvy = vy >= 1e-10f ? g[2] * 0.5f / sqrtf(vy) : 0.f;
    const float k = (float)(W / 2) * scale_f;
    const float dcx = g[0] * k - 2.f * cx * dvx, dcy = g[1] * k - 2.f * cy * dvy;
    // (both sums as the SAME explicit fma chain: left to the compiler the two expressions contract in different orders
    // and a one-hot heat map - cx == gx, cy == gy bit for bit, ds = 0 exactly - got an ulp of dh as its gradient)
    const float hdh = __builtin_fmaf(dvy, ey2, __builtin_fmaf(dvx, ex2, __builtin_fmaf(dcy, cy, dcx * cx)));   // sum_r h dh
    const float dh = __builtin_fmaf(dvy * gy, gy, __builtin_fmaf(dvx * gx, gx, __builtin_fmaf(dcy, gy, dcx * gx)));
    ds[d] = s.on ? (d ? e.e1 : e.e0) * inv * (dh - hdh) : 0.f;
  }
  // lane = channel again: ds[r] is read from the lane that holds position r (tr_index: r itself, or 2r at NP = 32)
  auto ds_at = [&](int d, int r) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ds[d]), NP == 64 ? r : 2 * r));
  };
  float dq0 = 0.f, dq1 = 0.f;
#pragma unroll
  for (int r = 0; r < WW; ++r) { dq0 = __builtin_fmaf(ds_at(0, r), f1[r], dq0); dq1 = __builtin_fmaf(ds_at(1, r), f0[r], dq1); }
  dq0 *= kFineInvSqrtC;                              // (an exact power of two)
  dq1 *= kFineInvSqrtC;
  // per-match d_mix partials: [dq0 . f0[r] (r < WW), sum dq0] and the same of direction 1, one transpose-reduce each
  float pr[NP];
#pragma unroll
  for (int r = 0; r < NP; ++r) pr[r] = r < WW ? dq0 * f0[r] : (r == WW ? dq0 : 0.f);
  const float dm0 = transpose_reduce<NP>(pr, lane);
#pragma unroll
  for (int r = 0; r < NP; ++r) pr[r] = r < WW ? dq1 * f1[r] : (r == WW ? dq1 : 0.f);
  const float dm1 = transpose_reduce<NP>(pr, lane);
  if (s.pos <= WW && (NP == 64 || !(lane & 1))) { pm[s.pos] = dm0; pm[WW + 1 + s.pos] = dm1; }
  const float tq0 = kFineInvSqrtC * q.q0, tq1 = kFineInvSqrtC * q.q1;
#pragma unroll
  for (int r = 0; r < WW; ++r) {
    g0[r * CF] = __builtin_fmaf(mix0[r], dq0, ds_at(1, r) * tq1);
    g1[r * CF] = __builtin_fmaf(mix1[r], dq1, ds_at(0, r) * tq0);
  }
}

// d_mix[col] = sum over matches of part[m][col], m ascending in each thread's stride, then a fixed-order wave and
// workgroup sum: one workgroup per column (2 (WW + 1) of them).
__global__ __launch_bounds__(256) void k_fine_mix_reduce(const float* __restrict__ part, int m_max,
                                                         const int32_t* __restrict__ d_count, int WW,
                                                         float* __restrict__ d_mix0, float* __restrict__ d_mix1) {
  __shared__ float wsum[4];
  const int col = blockIdx.x, ncol = 2 * (WW + 1);
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  float s = 0.f;
  for (int m = threadIdx.x; m < M; m += 256) s += part[(long)m * ncol + col];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (col <= WW) d_mix0[col] = v;
    else d_mix1[col - WW - 1] = v;
  }
}

// ---- window crop backward ----
__device__ __forceinline__ int floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

// a match's CSR slot: (b, cell) inside the maps and the cell grid, else -1 (such a row reads nothing here)
__device__ __forceinline__ long csr_cell(const int64_t* b_ids, const int64_t* ids, int m, int N, int cells) {
  const int64_t b = b_ids[m], id = ids[m];
  if (b < 0 || b >= N || id < 0 || id >= cells) return -1;
  return (long)b * cells + (long)id;
}

__global__ __launch_bounds__(256) void k_csr_count(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ ids,
                                                   const int32_t* __restrict__ d_count, int m_max, int N, int cells,
                                                   int* __restrict__ cnt) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  if (m >= M) return;
  const long c = csr_cell(b_ids, ids, m, N, cells);
  if (c >= 0) atomicAdd(&cnt[c], 1);                 // (integer: exact in any order)
}

// counts [n] -> exclusive starts [n + 1] in place, and a copy of the starts as fill cursors.  One workgroup: each
// thread scans a contiguous chunk, the chunk totals are scanned in LDS.
__global__ __launch_bounds__(1024) void k_csr_scan(int* __restrict__ start, int* __restrict__ cursor, int n) {
  __shared__ int tot[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024;
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += start[i];
  tot[tid] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? tot[tid - off] : 0;
    __syncthreads();
    tot[tid] += v;
    __syncthreads();
  }
  int run = tot[tid] - s;
  for (int i = lo; i < hi; ++i) {
    const int c = start[i];
    start[i] = run;
    cursor[i] = run;
    run += c;
  }
  if (tid == 1023) start[n] = tot[1023];
}

__global__ __launch_bounds__(256) void k_csr_fill(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ ids,
                                                  const int32_t* __restrict__ d_count, int m_max, int N, int cells,
                                                  int* __restrict__ cursor, int* __restrict__ list) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int M = d_count ? min(d_count[0], m_max) : m_max;
  if (m >= M) return;
  const long c = csr_cell(b_ids, ids, m, N, cells);
  if (c >= 0) list[atomicAdd(&cursor[c], 1)] = m;
}

// each cell's matches in ascending index (the fill's order is the atomics' arrival order); lists are short - one or
// two windows per cell, a few hundred for a supervision id drawn that often
__global__ __launch_bounds__(256) void k_csr_sort(const int* __restrict__ start, int* __restrict__ list, int n) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int lo = start[c], hi = start[c + 1];
  for (int i = lo + 1; i < hi; ++i) {
    const int v = list[i];
    int j = i - 1;
    while (j >= lo && list[j] > v) { list[j + 1] = list[j]; --j; }
    list[j + 1] = v;
  }
}

// One workgroup per (sample, row y, TX pixels of the row); one wave per pixel, lane = channel (NCH channels per lane:
// Cf <= 64 NCH).  grid N * Hf * ceil(Wf / TX).
template <int NCH>
__global__ __launch_bounds__(256) void k_crop_bwd(const float* __restrict__ d_win, int Cf, int Hf, int Wf, int layout, int W,
                                                  int stride, int pad, int h_c, int w_c, const int* __restrict__ start,
                                                  const int* __restrict__ list, float* __restrict__ d_feat) {
  constexpr int TX = 64 / NCH;
  __shared__ float tile[TX * (64 * NCH + 1)];
  const int P = Cf + 1;                              // odd pitch: the NCHW read-out below walks the pixels of a channel
  const int tiles_x = (Wf + TX - 1) / TX;
  const int x0 = (int)(blockIdx.x % tiles_x) * TX;
  const int row = (int)(blockIdx.x / tiles_x), y = row % Hf, b = row / Hf;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int WW = W * W, cells = h_c * w_c;
  // cells whose window covers row y: cy stride - pad <= y <= cy stride - pad + W - 1
  const int cy_lo = max(0, floor_div(y + pad - W + stride, stride)), cy_hi = min(h_c - 1, floor_div(y + pad, stride));
  for (int px = wv; px < TX; px += 4) {
    const int x = x0 + px;
    float acc[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) acc[k] = 0.f;
    if (x < Wf) {
      const int cx_lo = max(0, floor_div(x + pad - W + stride, stride)), cx_hi = min(w_c - 1, floor_div(x + pad, stride));
      for (int cy = cy_lo; cy <= cy_hi; ++cy)
        for (int cx = cx_lo; cx <= cx_hi; ++cx) {
          const long cell = (long)b * cells + cy * w_c + cx;
          const int r = (y - (cy * stride - pad)) * W + (x - (cx * stride - pad));
          const int lo = start[cell], hi = start[cell + 1];
          for (int j = lo; j < hi; ++j) {
            const float* src = d_win + ((long)list[j] * WW + r) * Cf;
#pragma unroll
            for (int k = 0; k < NCH; ++k)
              if (lane + 64 * k < Cf) acc[k] += src[lane + 64 * k];
          }
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k)
      if (lane + 64 * k < Cf) tile[px * P + lane + 64 * k] = acc[k];
  }
  __syncthreads();
  if (layout == 0) {
    float* dst = d_feat + (long)b * Cf * Hf * Wf + (long)y * Wf + x0;
    for (int idx = threadIdx.x; idx < Cf * TX; idx += 256) {
      const int c = idx / TX, px = idx - c * TX;
      if (x0 + px < Wf) dst[(long)c * Hf * Wf + px] = tile[px * P + c];
    }
  } else {
    float* dst = d_feat + (((long)b * Hf + y) * Wf + x0) * Cf;
    const int n = min(TX, Wf - x0) * Cf;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
      const int px = idx / Cf, c = idx - px * Cf;
      dst[idx] = tile[px * P + c];
    }
  }
}

}  // namespace fm

using namespace fm;

// Workspace of fm_fine_match_backward: every match's share of the 2 (WW + 1) mix-weight gradients (k_fine_mix_reduce sums them)
struct FineBwdWs { Region<float> part; size_t total; };
static FineBwdWs fine_bwd_layout(int m_max, int WW) {
  FineBwdWs w;
  Carver c;
  c.take(w.part, (size_t)m_max * 2 * (WW + 1));
  w.total = c.pad();
  return w;
}

extern "C" size_t fm_fine_match_backward_workspace_bytes(int m_max, int WW) {
  return m_max >= 0 && WW > 0 ? fine_bwd_layout(m_max, WW).total : 0;
}

extern "C" int fm_fine_match_backward(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW,
                                      int Cf, const float* mix0, const float* mix1, float scale_f, const float* d_out0,
                                      const float* d_out1, void* workspace, size_t workspace_bytes, float* d_win0,
                                      float* d_win1, float* d_mix0, float* d_mix1, void* stream) {
  if (m_max == 0) return FM_OK;
  if (!win0 || !win1 || !mix0 || !mix1 || !d_out0 || !d_out1 || !workspace || !d_win0 || !d_win1 || !d_mix0 || !d_mix1)
    return FM_E_NULL;
  if (m_max < 0) return FM_E_SHAPE;
  if (Cf != 64 || (WW != 25 && WW != 49)) return FM_E_UNSUPPORTED;
  const FineBwdWs ws = fine_bwd_layout(m_max, WW);
  if (!workspace_ok(workspace, workspace_bytes, ws.total)) return FM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* part = ws.part.in(workspace);
  const int blocks = (m_max + 3) / 4;
  with_window(WW == 25 ? 5 : 7, [&](auto w) {
    hipLaunchKernelGGL(k_fine_bwd<decltype(w)::value>, dim3(blocks), dim3(256), 0, st, win0, win1, m_max, d_count, mix0,
                       mix1, scale_f, d_out0, d_out1, d_win0, d_win1, part);
  });
  hipLaunchKernelGGL(k_fine_mix_reduce, dim3(2 * (WW + 1)), dim3(256), 0, st, part, m_max, d_count, WW, d_mix0, d_mix1);
  return (int)hipGetLastError();
}

// Workspace of fm_gather_windows_backward, the CSR of matches per cell: starts [N cells + 1] | fill cursors [N cells] |
// match list [m_max], int32, each 256-byte aligned.  counts: where k_csr_count adds up the cells' counts, zeroed per call.
struct CropBwdWs { Region<int> start, cursor, list; Span counts; size_t total; };
static CropBwdWs crop_bwd_layout(int N, int h_c, int w_c, int m_max) {
  const size_t n = (size_t)N * h_c * w_c;
  CropBwdWs w;
  Carver c;
  c.take(w.start, n + 1);
  w.counts = Span{w.start.at, w.start.bytes(n)};      // the first n of start
  c.take(w.cursor, n);
  c.take(w.list, m_max);
  w.total = c.pad();
  return w;
}

extern "C" size_t fm_gather_windows_backward_workspace_bytes(int N, int h_c, int w_c, int m_max) {
  return N > 0 && h_c > 0 && w_c > 0 && m_max >= 0 ? crop_bwd_layout(N, h_c, w_c, m_max).total : 0;
}

extern "C" int fm_gather_windows_backward(const float* d_win, const int64_t* b_ids, const int64_t* ids,
                                          const int32_t* d_count, int m_max, int N, int Cf, int Hf, int Wf, int layout,
                                          int W, int stride, int pad, int h_c, int w_c, void* workspace,
                                          size_t workspace_bytes, float* d_feat, void* stream) {
  if (m_max == 0) return FM_OK;
  if (!d_win || !b_ids || !ids || !workspace || !d_feat) return FM_E_NULL;
  if (!crop_shape_ok(N, Hf, Wf, stride, m_max) || !generic_window_shape_ok(Cf, W) || h_c <= 0 || w_c <= 0) return FM_E_SHAPE;
  if (!generic_window_supported(Cf, W, layout)) return FM_E_UNSUPPORTED;
  if ((long)N * h_c * w_c >= (1L << 31) - 1 || (long)N * Hf >= (1L << 31) / ((Wf + 7) / 8)) return FM_E_UNSUPPORTED;
  const CropBwdWs ws = crop_bwd_layout(N, h_c, w_c, m_max);
  if (!workspace_ok(workspace, workspace_bytes, ws.total)) return FM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int cells = h_c * w_c, n = N * cells;
  int* start = ws.start.in(workspace);
  int* cursor = ws.cursor.in(workspace);
  int* list = ws.list.in(workspace);
  hipError_t e = hipMemsetAsync(ws.counts.in(workspace), 0, ws.counts.bytes, st);
  if (e != hipSuccess) return (int)e;
  const int mb = (m_max + 255) / 256, cb = (n + 255) / 256;
  hipLaunchKernelGGL(k_csr_count, dim3(mb), dim3(256), 0, st, b_ids, ids, d_count, m_max, N, cells, start);
  hipLaunchKernelGGL(k_csr_scan, dim3(1), dim3(1024), 0, st, start, cursor, n);
  hipLaunchKernelGGL(k_csr_fill, dim3(mb), dim3(256), 0, st, b_ids, ids, d_count, m_max, N, cells, cursor, list);
  hipLaunchKernelGGL(k_csr_sort, dim3(cb), dim3(256), 0, st, start, list, n);
  const int nch = (Cf + 63) / 64;
  const int tx = nch == 1 ? 64 : nch == 2 ? 32 : nch <= 4 ? 16 : 8;
  const dim3 grid((unsigned)((long)N * Hf * ((Wf + tx - 1) / tx)));
#define FM_CROP_BWD(NC)                                                                                                  \
  hipLaunchKernelGGL(k_crop_bwd<NC>, grid, dim3(256), 0, st, d_win, Cf, Hf, Wf, layout, W, stride, pad, h_c, w_c, start, \
                     list, d_feat)
  if (nch == 1) FM_CROP_BWD(1);
  else if (nch == 2) FM_CROP_BWD(2);
  else if (nch <= 4) FM_CROP_BWD(4);
  else FM_CROP_BWD(8);
#undef FM_CROP_BWD
  return (int)hipGetLastError();
}
