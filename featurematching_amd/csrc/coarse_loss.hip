// The reference's coarse loss over ALL entries of conf_matrix (losses/loss.py:44-50 cross entropy, :62-67 focal with dense
// supervision) and its gradient w.r.t. the descriptors, without conf_matrix, conf_matrix_gt or any other [N, L, S] array.
//
// With c = clamp(conf, lo, hi), P the distinct supervised entries, l_neg / l_pos the reference's per-entry terms,
// wn = neg_weight / (N L S - |P|) and wp = pos_weight / |P|:
//     loss = wn ( sum_all l_neg(c) - sum_P l_neg(c_e) ) + wp sum_P l_pos(c_e)
//     G    = dloss/dconf = wn l_neg'(c) [lo <= conf <= hi]                               at every entry
//                        + ( wp l_pos'(c_e) - wn l_neg'(c_e) ) [lo <= conf_e <= hi]      at e in P
// The dense part of G is a function of conf alone, so the tiled sweep of fm_sweep_device.h (a workgroup owns 32 rows, sweeps
// the other image in 32-descriptor tiles, conf = A B from exact float32 dot products and the forward call's softmax
// statistics) forms it in registers; the correction at P is a sparse g_e of the kind fm_dual_softmax_backward takes.
// The backward of the dual softmax is linear in G: both parts land in the same row sums v and column sums u, and one
// pair of gradient sweeps serves them together (D = 2 g conf - A u - B v; the entries' own 2 g_e c_e is k_dsm_entries).
//
//   forward : k_closs_entries (conf, l_pos, l_neg, g_e conf_e at P) -> k_dsm_uv -> k_closs_sweep<.., kSums> on side 0
//             (sum of l_neg, v, u) -> k_closs_finish (the three numbers of loss_out, fixed order)
//   backward: k_closs_sweep<.., kGrad> + k_sweep_combine<true> per side (the upstream gradient d_loss is read on the
//             device by the combine) -> k_closs_scale + k_dsm_entries
// k_closs_sweep and k_dsm_bwd are the one tiled sweep of fm_sweep_device.h (LDS layout, tile loader, gradient phase, row /
// column sums, partial store: there, once) under two policies that differ in three things: how a dot product is summed,
// where g comes from (computed from conf here, loaded from G or folded into the weights there) and what is kept of an
// entry (here also the sum of l_neg).  What guards a change to the shared code: the two kernels' arithmetic instructions,
// registers and LDS, the entry points' bits and a training step's time against the parent build, as recorded in
// profiles/sweep_shared_parent_vs_change.txt.
//
// Two things differ from k_dsm_bwd because the loss is not linear in conf:
//   * the clamp's gate [lo <= conf <= hi] decides whether an entry has a gradient at all, and a peaked entry (conf within
//     1e-6 of 1) is only on the right side of hi when the entry and its two denominators hold the SAME dot product.  The
//     denominators come from the coarse stage's exact phase, so the sweep takes that phase's summation order (k_conf_at:
//     16 partial sums over the float4 groups l, l + 16, l + 32, l + 48, folded as a balanced tree) instead of channel
//     order.  The supervised entries (k_closs_entries) use the same order and the same expression, so l_neg(c_e) is bit for
//     bit the term the sweep added;
//   * the sum of l_neg mixes terms of 1e-6 with terms of 13.8 (a positive at the upper bound): it is kept in double from
//     the first addition, so the subtraction above removes the positives' terms exactly.
#include "fm_sweep_device.h"

namespace fm {

enum { kCeLoss = 0, kFocal2 = 1, kFocalG = 2 };     // cross entropy | focal, gamma = 2 (a multiply) | focal, any gamma > 0
enum { kSums = 0, kGrad = 1 };

struct LossParams {
  float alpha, gamma;
  float wn, wp;          // neg_weight / (N L S - |P|), pos_weight / |P|
  float lo, hi;          // float32 roundings of 1e-6 and 1 - 1e-6: the reference runs its clamp in float32
};

// One of the reference's two per-entry terms: l = -alpha a^gamma log b and q = alpha (a^gamma / b - gamma a^(gamma-1) log b).
//   negatives: a = c, b = 1 - c:  l_neg = l, dl_neg/dc = q;     positives: a = 1 - c, b = c:  l_pos = l, dl_pos/dc = -q
// (cross entropy: l = -log b, q = 1 / b)
template <int KIND>
__device__ __forceinline__ void loss_term(float a, float b, const LossParams& p, float& l, float& q) {
  const float rb = __builtin_amdgcn_rcpf(b);
  if (KIND == kCeLoss) {
    l = -__ocml_log_f32(b);
    q = rb;
  } else {
    const float lg = __ocml_log_f32(b);
    float pw1, g;                        // a^(gamma - 1), gamma
    if (KIND == kFocal2) { pw1 = a; g = 2.0f; }
    else { pw1 = __builtin_amdgcn_exp2f((p.gamma - 1.0f) * __builtin_amdgcn_logf(a)); g = p.gamma; }
    const float pw = pw1 * a;
    l = -p.alpha * pw * lg;
    q = p.alpha * (pw * rb - g * pw1 * lg);
  }
}

// Folds the 16 partial sums of a dot product as row_sum16 (fm_wave_device.h) does across 16 lanes - pairs, quads, halves,
// all: a balanced tree, every level commutative - when they arrive one after the other: lv is a binary counter of
// finished subtrees, x the result after l = 15.  (l is uniform: scalar branches, lv stays in registers.)
__device__ __forceinline__ void dot_fold(int l, float s, float (&lv)[4], float& x) {
  if (!(l & 1)) { lv[0] = s; return; }
  s = lv[0] + s;
  if (!(l & 2)) { lv[1] = s; return; }
  s = lv[1] + s;
  if (!(l & 4)) { lv[2] = s; return; }
  s = lv[2] + s;
  if (!(l & 8)) { lv[3] = s; return; }
  x = lv[3] + s;
}

// conf = softmax over the rows * softmax over the columns, from the raw dot product and the statistics of its row (ox, isx =
// 1 / denominator) and its column (oy, isy).  The entries kernel's copy of the three expressions sweep_tiles
// (fm_sweep_device.h) forms conf with; the two must stay the same, operation for operation, so that l_neg(c_e) is the term
// the sweep added.  One function for both was tried: called from sweep_tiles it changes which products of
// k_dsm_bwd<C, kDsmDense> the compiler packs and contracts, that is, that kernel's roundings.
__device__ __forceinline__ float conf_from(float x, float k2, float ox, float isx, float oy, float isy, float& ar, float& br) {
  ar = __builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, oy)) * isy;
  br = __builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, ox)) * isx;
  return ar * br;
}

// the dense part of G at one entry, times conf; l = l_neg(c)
template <int KIND>
__device__ __forceinline__ float dense_gc(float conf, const LossParams& p, float& l) {
  const float c = fminf(fmaxf(conf, p.lo), p.hi);
  float q;
  loss_term<KIND>(c, 1.0f - c, p, l, q);
  return (conf >= p.lo && conf <= p.hi) ? p.wn * q * conf : 0.f;        // torch's clamp backward: the closed interval
}

// The supervised entries: one thread per entry, the dot product in the sweep's order (see above).
// l_pos[e], l_neg[e] and gc[e] = g_e conf_e with g_e the correction of G at e.
template <int KIND>
__global__ __launch_bounds__(256) void k_closs_entries(const float* __restrict__ f0, const float* __restrict__ f1, int L, int S,
                                                       int c_in, float k2, const float* __restrict__ nm_r,
                                                       const float* __restrict__ sum_r, int pitch_r,
                                                       const float* __restrict__ nm_c, const float* __restrict__ sum_c,
                                                       int pitch_c, const int64_t* __restrict__ b_ids,
                                                       const int64_t* __restrict__ i_ids, const int64_t* __restrict__ j_ids,
                                                       int K, LossParams p, float* __restrict__ l_pos,
                                                       float* __restrict__ l_neg, float* __restrict__ gc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= K) return;
  const long b = b_ids[e], i = i_ids[e], j = j_ids[e];
  const float4* ra = reinterpret_cast<const float4*>(f0 + (b * L + i) * c_in);
  const float4* rb = reinterpret_cast<const float4*>(f1 + (b * S + j) * c_in);
  const int vpr = c_in >> 2;
  float lv[4], x = 0.f;                       // the exact phase's order: see dot_fold
#pragma unroll
  for (int l = 0; l < 16; ++l) {
    float sl = 0.f;
    for (int v4 = l; v4 < vpr; v4 += 16) {
      const float4 a = ra[v4], y = rb[v4];
      sl = __builtin_fmaf(a.x, y.x, sl);
      sl = __builtin_fmaf(a.y, y.y, sl);
      sl = __builtin_fmaf(a.z, y.z, sl);
      sl = __builtin_fmaf(a.w, y.w, sl);
    }
    dot_fold(l, sl, lv, x);
  }
  float ar, br;
  const float conf = conf_from(x, k2, nm_r[b * pitch_r + i], 1.0f / sum_r[b * pitch_r + i], nm_c[b * pitch_c + j],
                               1.0f / sum_c[b * pitch_c + j], ar, br);
  const float c = fminf(fmaxf(conf, p.lo), p.hi);
  float ln, qn, lp, qp;
  loss_term<KIND>(c, 1.0f - c, p, ln, qn);
  loss_term<KIND>(1.0f - c, c, p, lp, qp);
  l_pos[e] = lp;
  l_neg[e] = ln;
  gc[e] = (conf >= p.lo && conf <= p.hi) ? (-p.wp * qp - p.wn * qn) * conf : 0.f;
}

// The tiled sweep (fm_sweep_device.h; grid (ceil(R / 32), N, Z)) with g computed from conf.
//   kSums : per entry gc = g conf with g the dense part of G; row sums and column sums as partials folded in index order
//           (as kDsmStats: no atomics), l_neg(c) into a per-thread sum (double), one partial per workgroup into loss_part in a
//           fixed order.  Side 0 only.
//   kGrad : D = 2 gc - A w_y - B w_x accumulated into the rows' gradient, partials per z into `part`.
template <int KIND>
struct ClossSweepPolicy {
  const LossParams& p;
  double* __restrict__ loss_part;
  double lacc;
  float lv[4][4];            // dot_fold's counters (kept here, not in dots: per call they would be set up per tile)
  // the exact phase's order: partial sum pl over the float4 groups pl, pl + 16, ... (see above), folded by dot_fold
  template <int C>
  __device__ __forceinline__ void dots(const float* Xs, const float* Ys, int tx, int ty, float (&sv)[4]) {
    constexpr int P = sweep_pitch(C);
#pragma unroll 1                                          // (unrolled, the loads of all 16 partial sums are hoisted: spills)
    for (int pl = 0; pl < 16; ++pl) {
      float sl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 4 * pl; c < C; c += 64) {
        const float4 y = *reinterpret_cast<const float4*>(&Ys[tx * P + c]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 x = *reinterpret_cast<const float4*>(&Xs[(ty + 8 * q) * P + c]);
          sl[q] = __builtin_fmaf(x.x, y.x, sl[q]);
          sl[q] = __builtin_fmaf(x.y, y.y, sl[q]);
          sl[q] = __builtin_fmaf(x.z, y.z, sl[q]);
          sl[q] = __builtin_fmaf(x.w, y.w, sl[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) dot_fold(pl, sl[q], lv[q], sv[q]);
    }
  }
  __device__ __forceinline__ void fetch_g(float (&)[4], int, int, int, int) const {}
  __device__ __forceinline__ void g_from_lds(float (&)[4]) const {}
  __device__ __forceinline__ float gc(float, float conf, float& ln) const { return dense_gc<KIND>(conf, p, ln); }
  __device__ __forceinline__ void keep(bool ok, float ln) { lacc += ok ? (double)ln : 0.0; }
  // the workgroup's sum of l_neg: butterfly within each wave, then the four waves in index order - the same bits
  // every run
  __device__ __forceinline__ void sums_done(float* Dt, long part_index) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) lacc += __shfl_xor(lacc, m);
    __syncthreads();                                      // the last tile's column sums are done with Dt
    double* red = reinterpret_cast<double*>(Dt);
    if ((tid & 63) == 0) red[tid >> 6] = lacc;
    __syncthreads();
    if (tid == 0) loss_part[part_index] = ((red[0] + red[1]) + red[2]) + red[3];
  }
};

template <int C, int MODE, int KIND>
__global__ __launch_bounds__(256) void k_closs_sweep(const float* __restrict__ X, const float* __restrict__ Y, int R, int T,
                                                     int c_in, const float* __restrict__ ofs_x, const float* __restrict__ sum_x,
                                                     int pitch_x, const float* __restrict__ ofs_y,
                                                     const float* __restrict__ sum_y, int pitch_y,
                                                     const float* __restrict__ w_x, const float* __restrict__ w_y, float k2,
                                                     LossParams p, float* __restrict__ part, float* __restrict__ v_out,
                                                     float* __restrict__ u_out, double* __restrict__ loss_part) {
  ClossSweepPolicy<KIND> pol = {p, loss_part, 0.0, {}};
  sweep_tiles<C, MODE == kSums ? kDsmStats : kDsmDense>(X, Y, R, T, c_in, ofs_x, sum_x, pitch_x, ofs_y, sum_y, pitch_y, w_x,
                                                          w_y, k2, part, v_out, u_out, pol);
}

// sum of n numbers in double, in an order that depends on n alone: thread t adds elements t, t + 256, ..., then a tree
template <typename T>
__device__ __forceinline__ double block_sum_fixed(const T* __restrict__ x, long n, double* red) {
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)x[i];
  __syncthreads();
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  return red[0];
}

// loss_out = {loss, mean of l_pos over P, mean of l_neg over the negatives}; one workgroup.  leave: the listed entries are
// positives and leave the negatives' sum (0: the stand-in entry of an empty supervision)
__global__ __launch_bounds__(256) void k_closs_finish(const double* __restrict__ loss_part, long n_part,
                                                      const float* __restrict__ l_pos, const float* __restrict__ l_neg, int K,
                                                      double inv_pos, double inv_neg, float pos_weight, float neg_weight,
                                                      int leave, float* __restrict__ loss_out) {
  __shared__ double red[256];
  const double all = block_sum_fixed(loss_part, n_part, red);
  const double neg_p = block_sum_fixed(l_neg, K, red);
  const double pos_p = block_sum_fixed(l_pos, K, red);
  if (threadIdx.x == 0) {
    const double pos_mean = pos_p * inv_pos, neg_mean = (leave ? all - neg_p : all) * inv_neg;
    loss_out[0] = (float)((double)pos_weight * pos_mean + (double)neg_weight * neg_mean);
    loss_out[1] = (float)pos_mean;
    loss_out[2] = (float)neg_mean;
  }
}

__global__ __launch_bounds__(256) void k_closs_scale(const float* __restrict__ gc, int K, const float* __restrict__ d_loss,
                                                     float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < K) out[e] = gc[e] * d_loss[0];
}

// one call of either entry point past its status (dsm_status) and carve: the loss's own arithmetic
struct ClossCall {
  ClossWs w;                                  // (layout: fm_internal.h)
  LossParams lp;
  int kind;                                   // kCeLoss / kFocal2 / kFocalG
  DsmEntries e;                               // Ke entries (the workspace's zeros when the supervision is empty), no gc yet
  float pos_weight, neg_weight;               // as they count: 0 where the reference's degenerate cases set them to 0
  double inv_pos, inv_neg;
  bool stand_in;                              // empty supervision: the one listed entry is loss.py:38's (0, 0, 0)
};

static ClossCall closs_begin(const DsmCall& c) {
  ClossCall q;
  const LossSpec& l = c.loss; const int K = c.e.K;
  q.w = closs_layout(c.N, c.L, c.S, c.C, K);
  // loss.py:37-42: without a positive, entry (0, 0, 0) stands in with weight 0 - in pos_mask only: neg_mask was taken
  // before, so the entry stays among the negatives; without a negative the negatives' weight is 0
  q.stand_in = K == 0;
  q.pos_weight = K > 0 ? l.pos_weight : 0.f;
  const double n_neg = (double)c.N * c.L * c.S - (double)K;
  q.neg_weight = n_neg > 0 ? l.neg_weight : 0.f;
  q.inv_pos = 1.0 / (double)q.w.Ke;
  q.inv_neg = n_neg > 0 ? 1.0 / n_neg : 0.0;
  q.kind = l.kind == FM_LOSS_CROSS_ENTROPY ? kCeLoss : (l.gamma == 2.0f ? kFocal2 : kFocalG);
  q.lp = {l.alpha, l.gamma, (float)(q.neg_weight * q.inv_neg), (float)(q.pos_weight * q.inv_pos), 1e-6f, 1.0f - 1e-6f};
  const int64_t* zeros = q.w.zero_ids.in(c.workspace);
  q.e = q.stand_in ? DsmEntries{zeros, zeros, zeros, nullptr, 1} : DsmEntries{c.e.b_ids, c.e.i_ids, c.e.j_ids, nullptr, K};
  return q;
}

template <typename F>
static hipError_t with_kind(int kind, F&& f) {
  return kind == kCeLoss ? f(int_c<kCeLoss>{}) : kind == kFocal2 ? f(int_c<kFocal2>{}) : f(int_c<kFocalG>{});
}

// the tiled sweep of one side (0: owner = image 0, 1: image 1), then the combine of its partials (kGrad) or loss_out (kSums)
static int closs_sweep(int mode, int side, const DsmCall& c, const DsmProblem& p, const ClossCall& q) {
  const DsmSide o = dsm_side(p, c.s, side);
  const dim3 grid = dsm_sweep_grid(o);
  double* loss_part = q.w.loss_part.in(c.workspace);
  auto launch = [&](auto cc, auto mm, auto kk) {
    constexpr int CC = decltype(cc)::value, MM = decltype(mm)::value, KK = decltype(kk)::value;
    const bool sums = MM == kSums;               // (side 0: its sums go out as partials, folded into v and u below)
    return launch_sweep<&k_closs_sweep<CC, MM, KK>>(o, sweep_lds_bytes(CC, false), c.st(), q.lp, p.part, sums ? p.vpart : p.v,
                                                    sums ? p.upart : p.u, loss_part);
  };
  const hipError_t e = with_padded_channels(p.C, [&](auto cc) {
    return with_kind(q.kind, [&](auto kk) {
      return mode == kSums ? launch(cc, int_c<kSums>{}, kk) : launch(cc, int_c<kGrad>{}, kk);
    });
  });
  if (e != hipSuccess) return (int)e;
  if (mode != kSums) return (int)launch_sweep_combine(o, grid.z, c.d_loss, side ? c.d_feat1 : c.d_feat0, true, c.st());
  const hipError_t ef = launch_sweep_fold_sums(p, c.st());
  if (ef != hipSuccess) return (int)ef;
  hipLaunchKernelGGL(k_closs_finish, dim3(1), dim3(256), 0, c.st(), loss_part, (long)grid.x * grid.y * grid.z,
                     q.w.l_pos.in(c.workspace), q.w.l_neg.in(c.workspace), q.w.Ke, q.inv_pos, q.inv_neg, q.pos_weight,
                     q.neg_weight, q.stand_in ? 0 : 1, c.loss_out);
  return (int)hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_coarse_loss_workspace_bytes(int N, int L, int S, int C, int K) {
  return N > 0 && L > 0 && S > 0 && K >= 0 && valid_channels(C) ? closs_layout(N, L, S, C, K).total : 0;
}

extern "C" int fm_coarse_loss_forward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                      const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c,
                                      const float* sum_c, int pitch_c, int kind, float alpha, float gamma, float pos_weight,
                                      float neg_weight, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K,
                                      void* workspace, size_t workspace_bytes, float* loss_out, void* stream) {
  DsmCall c = {feat0, feat1, N, L, S, C, temperature, {nm_r, sum_r, pitch_r, nm_c, sum_c, pitch_c}, {b_ids, i_ids, j_ids, nullptr, K},
               nullptr, workspace, workspace_bytes, stream, nullptr, loss_out};
  c.listed = c.needs_ws = c.is_loss = true; c.loss = {kind, alpha, gamma, pos_weight, neg_weight}; c.missing = !loss_out;
  int r = dsm_status(c);
  if (r != FM_OK) return r;
  DsmProblem p;
  r = dsm_begin(c, &p);
  if (r != FM_OK) return r;
  ClossCall q = closs_begin(c);
  if (q.stand_in) r = (int)hipMemsetAsync(q.w.zeros.in(workspace), 0, q.w.zeros.bytes, c.st());
  if (r != FM_OK) return r;
  float* gc = q.w.gc.in(workspace);
  LossParams lp_e = q.lp;                     // the listed entries leave the negatives - the stand-in does not
  if (q.stand_in) lp_e.wn = 0.f;
  const hipError_t e = with_kind(q.kind, [&](auto kk) {
    hipLaunchKernelGGL((k_closs_entries<decltype(kk)::value>), dim3((q.e.K + 255) / 256), dim3(256), 0, c.st(), feat0, feat1, L, S,
                       C, p.k2, nm_r, sum_r, pitch_r, nm_c, sum_c, pitch_c, q.e.b_ids, q.e.i_ids, q.e.j_ids, q.e.K, lp_e,
                       q.w.l_pos.in(workspace), q.w.l_neg.in(workspace), gc);
    return hipGetLastError();
  });
  if (e != hipSuccess) return (int)e;
  q.e.gc = gc;
  r = (int)launch_dsm_uv(q.e, L, S, p.v, p.u, c.st());
  if (r != FM_OK) return r;
  return closs_sweep(kSums, 0, c, p, q);
}

extern "C" int fm_coarse_loss_backward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                       const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c,
                                       const float* sum_c, int pitch_c, int kind, float alpha, float gamma, float pos_weight,
                                       float neg_weight, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                       int K, void* workspace, size_t workspace_bytes, const float* d_loss, float* d_feat0,
                                       float* d_feat1, void* stream) {
  DsmCall c = {feat0, feat1, N, L, S, C, temperature, {nm_r, sum_r, pitch_r, nm_c, sum_c, pitch_c}, {b_ids, i_ids, j_ids, nullptr, K},
               nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, d_loss, d_feat0, d_feat1};
  c.listed = c.needs_ws = c.is_loss = true; c.loss = {kind, alpha, gamma, pos_weight, neg_weight};
  c.missing = !d_loss || !d_feat0 || !d_feat1;
  int r = dsm_status(c);
  if (r != FM_OK) return r;
  const DsmProblem p = dsm_carve(c);          // (v and u are the forward call's)
  ClossCall q = closs_begin(c);
  float* gcs = q.w.gcs.in(workspace);
  hipLaunchKernelGGL(k_closs_scale, dim3((q.e.K + 255) / 256), dim3(256), 0, c.st(), q.w.gc.in(workspace), q.e.K, d_loss,
                     gcs);
  q.e.gc = gcs;
  r = (int)launch_dsm_entries(p, q.e, d_feat0, d_feat1, c.st());      // (first: the sweeps' combine adds on top)
  for (int side = 0; side < 2 && r == FM_OK; ++side) r = closs_sweep(kGrad, side, c, p, q);
  return r;
}
