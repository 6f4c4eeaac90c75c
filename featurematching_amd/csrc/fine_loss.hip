// The reference's fine loss (Loss.compute_fine_loss, losses/loss.py:70-98) and its gradient, decided and reduced on the
// device: the reference syncs the host twice (expec_f_0.sum() == 0, torch.where) and launches about thirty small kernels
// for M rows of three floats.
//
// Per image d, with inv_m = 1 / max(std_m, 1e-10) and nz = {m : gt[m, 0] != 0}:
//     loss_d = sum_{m in nz} (|xy_m - gt_m|^2 / 49) inv_m / (mean_all(inv) |nz|)
//            = A_d coef_d,   A_d = sum_nz |xy - gt|^2 inv,   B_d = sum_all inv,   coef_d = 1 / (49 (B_d / M) |nz|)
//     loss_f = loss_0 + loss_1;  0 (and zero gradients) when the sum of all entries of expec0 is exactly 0 (loss.py:72-75);
//     NaN when nz is empty (the reference's mean of an empty set)
//     d expec_d[m, :2] = d_loss 2 (xy_m - gt_m) inv_m coef_d for m in nz, 0 elsewhere; the std column gets exactly 0 (the
//     weights are detached)
//
//   forward : k_floss_partial (7 sums per workgroup, double from the first addition, fixed order) -> k_floss_finish (one
//             workgroup folds the partials in index order, writes loss_out and the record the backward reads)
//   backward: k_floss_grad (one thread per row)
// No atomics: the same bits on every run.
#include "fm_internal.h"

namespace fm {

constexpr int kFlossMaxBlocks = 256;
enum { kSumE0 = 0, kA0, kB0, kN0, kA1, kB1, kN1, kFlossSums };        // a workgroup's partial sums (pitch 8 doubles)
// the record k_floss_finish leaves at the head of the workspace (doubles)
enum { kRecLoss = 0, kRecLoss0, kRecLoss1, kRecCoef0, kRecCoef1, kRecRows, kRecNz0, kRecNz1, kRecZero, kFlossRec };

__device__ __forceinline__ int floss_rows(int m_max, const int32_t* d_count) {
  if (!d_count) return m_max;
  const int c = d_count[0];
  return c < 0 ? 0 : (c < m_max ? c : m_max);
}

// 1 / max(std, 1e-10) as torch.clamp(min=...) decides it: a NaN stays a NaN
__device__ __forceinline__ double floss_inv(float std_) {
  const double s = (double)std_;
  return 1.0 / (s < 1e-10 ? 1e-10 : s);
}

__global__ __launch_bounds__(256) void k_floss_partial(const float* __restrict__ e0, const float* __restrict__ e1, int stride,
                                                       const float2* __restrict__ gt0, const float2* __restrict__ gt1,
                                                       int m_max, const int32_t* __restrict__ d_count,
                                                       double* __restrict__ part) {
  __shared__ double red[4][kFlossSums];
  const int M = floss_rows(m_max, d_count);
  double s[kFlossSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int m = blockIdx.x * 256 + threadIdx.x; m < M; m += gridDim.x * 256) {
    const float* r0 = e0 + (size_t)m * stride;
    const float* r1 = e1 + (size_t)m * stride;
    const float x0 = r0[0], y0 = r0[1], s0 = r0[2], x1 = r1[0], y1 = r1[1], s1 = r1[2];
    const float2 g0 = gt0[m], g1 = gt1[m];
    s[kSumE0] += ((double)x0 + (double)y0) + (double)s0;
    const double i0 = floss_inv(s0), i1 = floss_inv(s1);
    s[kB0] += i0;
    s[kB1] += i1;
    if (g0.x != 0.f) {
      const double dx = (double)x0 - (double)g0.x, dy = (double)y0 - (double)g0.y;
      s[kA0] += (dx * dx + dy * dy) * i0;
      s[kN0] += 1.0;
    }
    if (g1.x != 0.f) {
      const double dx = (double)x1 - (double)g1.x, dy = (double)y1 - (double)g1.y;
      s[kA1] += (dx * dx + dy * dy) * i1;
      s[kN1] += 1.0;
    }
  }
  // butterfly within each wave, then the four waves in index order
#pragma unroll
  for (int q = 0; q < kFlossSums; ++q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[q] += __shfl_xor(s[q], d);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < kFlossSums; ++q) red[tid >> 6][q] = s[q];
  }
  __syncthreads();
  if (tid < kFlossSums) part[blockIdx.x * 8 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64) void k_floss_finish(const double* __restrict__ part, int n_part, int m_max,
                                                     const int32_t* __restrict__ d_count, double* __restrict__ rec,
                                                     float* __restrict__ loss_out) {
  const int q = threadIdx.x;
  __shared__ double tot[kFlossSums];
  if (q < kFlossSums) {
    double s = 0.0;
    for (int b = 0; b < n_part; ++b) s += part[b * 8 + q];
    tot[q] = s;
  }
  __syncthreads();
  if (q != 0) return;
  const double M = (double)floss_rows(m_max, d_count);
  const bool zero = tot[kSumE0] == 0.0;                      // loss.py:72 (an empty list sums to 0 as well)
  const double coef0 = 1.0 / (49.0 * (tot[kB0] / M) * tot[kN0]), coef1 = 1.0 / (49.0 * (tot[kB1] / M) * tot[kN1]);
  // |nz| = 0: the reference's mean over an empty set, 0 / 0
  const double l0 = tot[kN0] > 0.0 ? tot[kA0] * coef0 : __builtin_nan(""), l1 = tot[kN1] > 0.0 ? tot[kA1] * coef1 : __builtin_nan("");
  const double loss = zero ? 0.0 : l0 + l1;
  rec[kRecLoss] = loss;
  rec[kRecLoss0] = zero ? 0.0 : l0;
  rec[kRecLoss1] = zero ? 0.0 : l1;
  rec[kRecCoef0] = coef0;
  rec[kRecCoef1] = coef1;
  rec[kRecRows] = M;
  rec[kRecNz0] = tot[kN0];
  rec[kRecNz1] = tot[kN1];
  rec[kRecZero] = zero ? 1.0 : 0.0;
  loss_out[0] = (float)loss;
  loss_out[1] = (float)rec[kRecLoss0];
  loss_out[2] = (float)rec[kRecLoss1];
}

__global__ __launch_bounds__(256) void k_floss_grad(const float* __restrict__ e0, const float* __restrict__ e1, int stride,
                                                    const float2* __restrict__ gt0, const float2* __restrict__ gt1,
                                                    int m_max, const double* __restrict__ rec,
                                                    const float* __restrict__ d_loss, float* __restrict__ d_e0,
                                                    float* __restrict__ d_e1) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= m_max) return;
  float o0x = 0.f, o0y = 0.f, o1x = 0.f, o1y = 0.f;
  if (m < (int)rec[kRecRows] && rec[kRecZero] == 0.0) {
    const double g2 = 2.0 * (double)d_loss[0];
    const float* r0 = e0 + (size_t)m * stride;
    const float* r1 = e1 + (size_t)m * stride;
    const float2 g0 = gt0[m], g1 = gt1[m];
    if (g0.x != 0.f) {
      const double w = g2 * floss_inv(r0[2]) * rec[kRecCoef0];
      o0x = (float)(w * ((double)r0[0] - (double)g0.x));
      o0y = (float)(w * ((double)r0[1] - (double)g0.y));
    }
    if (g1.x != 0.f) {
      const double w = g2 * floss_inv(r1[2]) * rec[kRecCoef1];
      o1x = (float)(w * ((double)r1[0] - (double)g1.x));
      o1y = (float)(w * ((double)r1[1] - (double)g1.y));
    }
  }
  d_e0[3 * (size_t)m] = o0x; d_e0[3 * (size_t)m + 1] = o0y; d_e0[3 * (size_t)m + 2] = 0.f;
  d_e1[3 * (size_t)m] = o1x; d_e1[3 * (size_t)m + 1] = o1y; d_e1[3 * (size_t)m + 2] = 0.f;
}

// Workspace: the record (kFlossRec doubles; record: its 256 bytes, zeroed by a forward call without matches) | 8 doubles
// per workgroup of k_floss_partial
struct FlossWs { Region<double> rec, part; Span record; int blocks; size_t total; };
static FlossWs floss_layout(int m_max) {
  FlossWs w;
  w.blocks = (m_max + 255) / 256;
  if (w.blocks > kFlossMaxBlocks) w.blocks = kFlossMaxBlocks;
  if (w.blocks < 1) w.blocks = 1;
  Carver c;
  c.take(w.rec, kFlossRec);
  w.record = c.since(w.rec.at, 256);
  c.take(w.part, (size_t)w.blocks * 8);
  w.total = c.pad();
  return w;
}
static_assert(kFlossRec * sizeof(double) <= 256, "the record's span");

static int floss_check(const float* e0, const float* e1, int stride, const float* gt0, const float* gt1, int m_max,
                       void* workspace, size_t workspace_bytes, FlossWs* w) {
  if (!e0 || !e1 || !gt0 || !gt1 || !workspace) return FM_E_NULL;
  if (m_max < 0 || stride < 3) return FM_E_SHAPE;
  *w = floss_layout(m_max);
  if (!workspace_ok(workspace, workspace_bytes, w->total)) return FM_E_WORKSPACE;
  return FM_OK;
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_fine_loss_workspace_bytes(int m_max) { return m_max >= 0 ? floss_layout(m_max).total : 0; }

extern "C" int fm_fine_loss_forward(const float* expec0, const float* expec1, int row_stride, const float* gt0,
                                    const float* gt1, int m_max, const int32_t* d_count, void* workspace,
                                    size_t workspace_bytes, float* loss_out, void* stream) {
  if (!loss_out) return FM_E_NULL;
  FlossWs w;
  const int r = floss_check(expec0, expec1, row_stride, gt0, gt1, m_max, workspace, workspace_bytes, &w);
  if (r != FM_OK) return r;
  hipStream_t st = (hipStream_t)stream;
  double* rec = w.rec.in(workspace);
  if (m_max == 0) {                                // the reference's `return 0.`: zeros, no launch
    hipError_t e = hipMemsetAsync(loss_out, 0, 3 * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(w.record.in(workspace), 0, w.record.bytes, st);
    return (int)e;
  }
  double* part = w.part.in(workspace);
  hipLaunchKernelGGL(k_floss_partial, dim3(w.blocks), dim3(256), 0, st, expec0, expec1, row_stride,
                     reinterpret_cast<const float2*>(gt0), reinterpret_cast<const float2*>(gt1), m_max, d_count, part);
  hipLaunchKernelGGL(k_floss_finish, dim3(1), dim3(64), 0, st, (const double*)part, w.blocks, m_max, d_count, rec, loss_out);
  return (int)hipGetLastError();
}

extern "C" int fm_fine_loss_backward(const float* expec0, const float* expec1, int row_stride, const float* gt0,
                                     const float* gt1, int m_max, void* workspace, size_t workspace_bytes,
                                     const float* d_loss, float* d_expec0, float* d_expec1, void* stream) {
  if (!d_loss || !d_expec0 || !d_expec1) return FM_E_NULL;
  FlossWs w;
  const int r = floss_check(expec0, expec1, row_stride, gt0, gt1, m_max, workspace, workspace_bytes, &w);
  if (r != FM_OK) return r;
  if (m_max == 0) return FM_OK;
  hipLaunchKernelGGL(k_floss_grad, dim3((m_max + 255) / 256), dim3(256), 0, (hipStream_t)stream, expec0, expec1, row_stride,
                     reinterpret_cast<const float2*>(gt0), reinterpret_cast<const float2*>(gt1), m_max,
                     w.rec.in(workspace), d_loss, d_expec0, d_expec1);
  return (int)hipGetLastError();
}
