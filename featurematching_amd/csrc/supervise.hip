// Ground-truth supervision on the device: the reference's data_preprocess (datasets/data_preprocessing.py:9-64), which
// copies the correspondences to the host, calls np.unique twice and copies back.
//
// K correspondences (kp0[k], kp1[k]) in pixels; cell = floor(coord / cell size) per axis.  Of all correspondences in one
// image-1 cell the one with the smallest input index survives (np.unique's return_index; the reference's second np.unique
// finds nothing left to remove).  Survivors leave in np.unique(axis=0)'s order: sorted by (cx1, cy1), cx1 the major key.
// Survivor t carries i = cx0 + cy0 w0c, j = cx1 + cy1 w1c, the cell corners, the original points, and fills the two
// per-cell tables fine_mtx_0[i] / fine_mtx_1[j].  The j are distinct; the i are not (two image-1 cells may map to one
// image-0 cell): the survivor with the largest t wins, as the reference's CPU index_put does.
//
//   k_spv_mark   : per correspondence, integer atomicMin of k into first[j] - order independent
//   k_spv_count  : occupied cells per block of 1024 scan positions (position p = cx1 h1c + cy1: the output order)
//   k_spv_scan   : one workgroup, exclusive scan of the block counts, K' -> d_count[0]
//   k_spv_emit   : rank within the block + the block's offset = t; writes survivor t, fine_mtx_1[j], integer atomicMax of
//                  t into last[i]
//   k_spv_table0 : fine_mtx_0[i_t] = fine_kp0[t] where last[i_t] == t
// Integer atomics only: every output is the same bits on every run.  Five small launches instead of one with fences
// (a last-workgroup hand-off costs more than the launches it saves on this part).
#include "fm_internal.h"

namespace fm {

constexpr int kSpvScanBlock = 1024;      // scan positions per workgroup: 256 threads x 4 consecutive positions

// cell of a coordinate: c = floor(x / cell); false when it lies outside [0, n) (NaN fails every comparison).  The sign
// is taken from the coordinate itself: a negative denormal divides to -0, whose floor would pass as cell 0.
__device__ __forceinline__ bool spv_cell(float x, float cell, int n, int& c) {
  const float f = floorf(x / cell);
  if (!(x >= 0.f && f < (float)n)) return false;
  c = (int)f;
  return true;
}

__global__ __launch_bounds__(256) void k_spv_mark(const float2* __restrict__ kp0, const float2* __restrict__ kp1, int K,
                                                  int h0c, int w0c, int h1c, int w1c, float cell,
                                                  unsigned* __restrict__ first, int32_t* __restrict__ d_count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const float2 a = kp0[k], b = kp1[k];
  int cx0 = 0, cy0 = 0, cx1 = 0, cy1 = 0;
  const bool ok = spv_cell(a.x, cell, w0c, cx0) && spv_cell(a.y, cell, h0c, cy0) && spv_cell(b.x, cell, w1c, cx1) &&
                  spv_cell(b.y, cell, h1c, cy1);
  if (!ok) { atomicOr(&d_count[1], FM_DEV_RANGE); return; }
  atomicMin(&first[cx1 + cy1 * w1c], (unsigned)k);
}

// scan position p = cx1 * h1c + cy1 -> cell j = cx1 + cy1 * w1c
__device__ __forceinline__ int spv_cell_of(int p, int h1c, int w1c) {
  const int cx = p / h1c;
  return cx + (p - cx * h1c) * w1c;
}

// occupied positions among the 4 this thread owns (bit q: position base + q), base = 4 * global thread index
__device__ __forceinline__ unsigned spv_occupied(const unsigned* __restrict__ first, int base, int S, int h1c, int w1c) {
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = base + q;
    if (p < S && first[spv_cell_of(p, h1c, w1c)] != 0xffffffffu) m |= 1u << q;
  }
  return m;
}

// exclusive prefix of v over the workgroup's 256 threads (thread order); total in *sum.  red: 4 ints of LDS
__device__ __forceinline__ int spv_block_excl(int v, int* red, int* sum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += red[w];
  *sum = red[0] + red[1] + red[2] + red[3];
  return before + inc - v;
}

__global__ __launch_bounds__(256) void k_spv_count(const unsigned* __restrict__ first, int S, int h1c, int w1c,
                                                   int* __restrict__ block_cnt) {
  __shared__ int red[4];
  const unsigned m = spv_occupied(first, (blockIdx.x * 256 + threadIdx.x) * 4, S, h1c, w1c);
  int total;
  spv_block_excl(__popc(m), red, &total);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// block_cnt[b] <- survivors before block b; d_count[0] = K'.  One workgroup; chunks of 256 blocks with a running carry.
__global__ __launch_bounds__(256) void k_spv_scan(int* __restrict__ block_cnt, int nb, int32_t* __restrict__ d_count) {
  __shared__ int red[4];
  int carry = 0;
  for (int at = 0; at < nb; at += 256) {
    const int b = at + threadIdx.x;
    const int v = b < nb ? block_cnt[b] : 0;
    int total;
    const int ex = spv_block_excl(v, red, &total);
    if (b < nb) block_cnt[b] = carry + ex;
    carry += total;
    __syncthreads();                             // red is rewritten by the next chunk
  }
  if (threadIdx.x == 0) d_count[0] = carry;
}

struct SpvOut {
  int64_t *i_ids, *j_ids;
  float2 *coarse_kp0, *coarse_kp1, *fine_kp0, *fine_kp1;
  float *lists_f0, *lists_f1;
  float2 *fine_mtx_0, *fine_mtx_1;
};

__global__ __launch_bounds__(256) void k_spv_emit(const float2* __restrict__ kp0, const float2* __restrict__ kp1,
                                                  const unsigned* __restrict__ first, const int* __restrict__ block_ofs,
                                                  int S, int h1c, int w0c, int w1c, float cell, int cap, SpvOut o,
                                                  int* __restrict__ last) {
  __shared__ int red[4];
  const int base = (blockIdx.x * 256 + threadIdx.x) * 4;
  const unsigned m = spv_occupied(first, base, S, h1c, w1c);
  int total;
  int t = block_ofs[blockIdx.x] + spv_block_excl(__popc(m), red, &total);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!(m >> q & 1)) continue;
    if (t < cap) {                               // (always: K' <= min(K, S) = cap; the guard keeps a smaller cap in bounds)
      const int cx1 = (base + q) / h1c, cy1 = (base + q) - cx1 * h1c;
      const int j = cx1 + cy1 * w1c;
      const unsigned k = first[j];
      const float2 a = kp0[k], b = kp1[k];
      const int cx0 = (int)floorf(a.x / cell), cy0 = (int)floorf(a.y / cell);   // in range: k_spv_mark checked k
      const int i = cx0 + cy0 * w0c;
      o.i_ids[t] = i;
      o.j_ids[t] = j;
      o.coarse_kp0[t] = make_float2((float)cx0 * cell, (float)cy0 * cell);
      o.coarse_kp1[t] = make_float2((float)cx1 * cell, (float)cy1 * cell);
      o.fine_kp0[t] = a;
      o.fine_kp1[t] = b;
      o.lists_f0[t] = (float)i;
      o.lists_f1[t] = (float)j;
      o.fine_mtx_1[j] = b;
      atomicMax(&last[i], t);
    }
    ++t;
  }
}

__global__ __launch_bounds__(256) void k_spv_table0(const int32_t* __restrict__ d_count, int cap, SpvOut o,
                                                    const int* __restrict__ last) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n = d_count[0] < cap ? d_count[0] : cap;
  if (t >= n) return;
  const int64_t i = o.i_ids[t];
  if (last[i] == t) o.fine_mtx_0[i] = o.fine_kp0[t];
}

// Workspace: first [S] (0xffffffff = empty) | last [L] (-1 = empty) - tables: the two and their padding, set to 0xff bytes
// per call | block_cnt [ceil(S / 1024)]
struct SpvWs { Region<unsigned> first; Region<int> last, block_cnt; Span tables; int nb; size_t total; };
static SpvWs spv_layout(int L, int S) {
  SpvWs w;
  Carver c;
  c.take(w.first, S);
  c.take(w.last, L);
  w.tables = c.since(w.first.at, 256);
  w.nb = (S + kSpvScanBlock - 1) / kSpvScanBlock;
  c.take(w.block_cnt, w.nb);
  w.total = c.pad();
  return w;
}

constexpr int kSpvMaxCells = 1 << 24;    // lists_f* hold the ids as float32: exact up to 2^24
static bool spv_grid_ok(int h, int w) { return h > 0 && w > 0 && (long)h * w <= kSpvMaxCells; }

}  // namespace fm

using namespace fm;

extern "C" size_t fm_supervise_workspace_bytes(int h0c, int w0c, int h1c, int w1c) {
  return spv_grid_ok(h0c, w0c) && spv_grid_ok(h1c, w1c) ? spv_layout(h0c * w0c, h1c * w1c).total : 0;
}

extern "C" int fm_supervise_matches(const float* kp0, const float* kp1, int K, int h0c, int w0c, int h1c, int w1c, float cell,
                                    void* workspace, size_t workspace_bytes, int64_t* i_ids, int64_t* j_ids,
                                    float* coarse_kp0, float* coarse_kp1, float* fine_kp0, float* fine_kp1, float* lists_f0,
                                    float* lists_f1, float* fine_mtx_0, float* fine_mtx_1, int cap, int32_t* d_count,
                                    void* stream) {
  if (!workspace || !fine_mtx_0 || !fine_mtx_1 || !d_count) return FM_E_NULL;
  if (K > 0 && (!kp0 || !kp1)) return FM_E_NULL;
  if (cap > 0 && (!i_ids || !j_ids || !coarse_kp0 || !coarse_kp1 || !fine_kp0 || !fine_kp1 || !lists_f0 || !lists_f1))
    return FM_E_NULL;
  if (K < 0 || cap < 0 || h0c <= 0 || w0c <= 0 || h1c <= 0 || w1c <= 0) return FM_E_SHAPE;
  if (!spv_grid_ok(h0c, w0c) || !spv_grid_ok(h1c, w1c) || !(cell > 0.f) || !(cell < 3.0e38f)) return FM_E_UNSUPPORTED;
  const int L = h0c * w0c, S = h1c * w1c;
  if (cap < (K < S ? K : S)) return FM_E_SHAPE;            // every survivor must have a row
  const SpvWs w = spv_layout(L, S);
  if (!workspace_ok(workspace, workspace_bytes, w.total)) return FM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned* first = w.first.in(workspace);
  int* last = w.last.in(workspace);
  int* block_cnt = w.block_cnt.in(workspace);
  hipError_t e = hipMemsetAsync(w.tables.in(workspace), 0xff, w.tables.bytes, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, 2 * sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(fine_mtx_0, 0, (size_t)L * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(fine_mtx_1, 0, (size_t)S * 8, st);
  if (e != hipSuccess) return (int)e;
  const float2 *p0 = reinterpret_cast<const float2*>(kp0), *p1 = reinterpret_cast<const float2*>(kp1);
  if (K > 0)
    hipLaunchKernelGGL(k_spv_mark, dim3((K + 255) / 256), dim3(256), 0, st, p0, p1, K, h0c, w0c, h1c, w1c, cell, first, d_count);
  hipLaunchKernelGGL(k_spv_count, dim3(w.nb), dim3(256), 0, st, (const unsigned*)first, S, h1c, w1c, block_cnt);
  hipLaunchKernelGGL(k_spv_scan, dim3(1), dim3(256), 0, st, block_cnt, w.nb, d_count);
  if (cap > 0) {
    const SpvOut o = {i_ids, j_ids, reinterpret_cast<float2*>(coarse_kp0), reinterpret_cast<float2*>(coarse_kp1),
                      reinterpret_cast<float2*>(fine_kp0), reinterpret_cast<float2*>(fine_kp1), lists_f0, lists_f1,
                      reinterpret_cast<float2*>(fine_mtx_0), reinterpret_cast<float2*>(fine_mtx_1)};
    hipLaunchKernelGGL(k_spv_emit, dim3(w.nb), dim3(256), 0, st, p0, p1, (const unsigned*)first, (const int*)block_cnt, S, h1c,
                       w0c, w1c, cell, cap, o, last);
    hipLaunchKernelGGL(k_spv_table0, dim3((cap + 255) / 256), dim3(256), 0, st, (const int32_t*)d_count, cap, o,
                       (const int*)last);
  }
  return (int)hipGetLastError();
}
