// Training surface of the coarse stage: the dual softmax at chosen entries and its backward,
// without any [N, L, S] temporary.
//
// The reference's coarse loss (losses/loss.py:27-67, `sparse_spvs`: the default) reads data['conf_matrix'] only at the
// supervised entries; its gradient w.r.t. the descriptors goes through conf = A * B, A = softmax(sim, dim 1) (over i),
// B = softmax(sim, dim 2) (over j), sim = f0 . f1^T / (C T) (network/utils/coarse_matching_new.py:64-68).  With
// g_e = dL/dconf_e at the supervised entries e = (b, i, j) and c_e = conf_e:
//     dL/dsim_kl = 2 g c [kl supervised] - A_kl u_l - B_kl v_k,      u_l = sum_e[j_e = l] g_e c_e,   v_k = sum_e[i_e = k] g_e c_e
//     dL/df0 = dL/dsim . f1 / (C T),     dL/df1 = dL/dsim^T . f0 / (C T)
// A and B follow from the softmax statistics the coarse stage leaves in its workspace (stabilisers and denominators:
// A_kl = exp2(k2 x_kl + nm_c[l]) / sum_c[l], B_kl = exp2(k2 x_kl + nm_r[k]) / sum_r[k], x = raw dot product, k2 = log2(e) /
// (C T); kept apart - folded into one offset nm - log2(sum) the float32 rounding of ~230 - 230 would cost 1e-5 of a conf
// near 1), so the backward is two
// launches of ONE kernel with the roles of the images swapped: a workgroup owns 32 rows of the "owner" image, sweeps the
// other image in tiles of 32 descriptors, recomputes the 32 x 32 similarities of the tile in float32 (exact products,
// fused multiply-adds in channel order), turns them into D = -(A u + B v) and accumulates D . other into its rows'
// gradient - the dense matrix never exists.  The supervised entries' own term 2 g c is K rows: a third, tiny kernel.
// float32 vector arithmetic on purpose: a training-only path whose bar is the agreement with float64 autograd
// (tests), not the matrix cores.
//
// This file: the training kernels (k_conf_at, k_dsm_uv, k_dsm_bwd, k_sweep_combine, k_dsm_entries), the status function
// and the carve of the five training entry points (DsmCall: fm_internal.h) and three of them; coarse_loss.hip has the
// other two.  The forward call's k_exact_lists, k_fix_sums, k_conf_patch live with the dense kernel: coarse_dense.hip.
#include "fm_sweep_device.h"
#include "fm_wave_device.h"

namespace fm {

// conf at K entries: 16 lanes per entry (16 channels per lane, four 16-byte loads per row), the exact float32 dot
// product in a fixed order - the arithmetic of fm_exact_device.h, written out: through that header's helpers with the
// element type fixed at float32 the compiler if-converts the guarded loads (16 instructions fewer, 3 SGPRs more:
// profiles/dsm_call_isa_identity.txt), and the change that tried it was to leave every kernel's instructions alone.
__global__ __launch_bounds__(256) void k_conf_at(const float* __restrict__ f0, const float* __restrict__ f1, int L, int S, int c_in,
                                                 float k2, const float* __restrict__ nm_r, const float* __restrict__ sum_r,
                                                 int pitch_r, const float* __restrict__ nm_c,
                                                 const float* __restrict__ sum_c, int pitch_c,
                                                 const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                 const int64_t* __restrict__ j_ids, int K, float* __restrict__ conf,
                                                 float* __restrict__ xdot) {
  const int e = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
  const int ec = min(e, K - 1);
  const long b = b_ids[ec], i = i_ids[ec], j = j_ids[ec];
  const float4* ra = reinterpret_cast<const float4*>(f0 + (b * L + i) * c_in);
  const float4* rb = reinterpret_cast<const float4*>(f1 + (b * S + j) * c_in);
  const int vpr = c_in >> 2;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v4 = l16 + 16 * q;
    const bool in = v4 < vpr;
    const float4 a = ra[in ? v4 : 0], bb = rb[in ? v4 : 0];
    const float4 az = in ? a : make_float4(0.f, 0.f, 0.f, 0.f);
    s = __builtin_fmaf(az.x, bb.x, s);
    s = __builtin_fmaf(az.y, bb.y, s);
    s = __builtin_fmaf(az.z, bb.z, s);
    s = __builtin_fmaf(az.w, bb.w, s);
  }
  const float x = row_sum16(s);
  if (l16 == 0 && e < K) {
    conf[e] = (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_r[b * pitch_r + i])) / sum_r[b * pitch_r + i]) *
              (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_c[b * pitch_c + j])) / sum_c[b * pitch_c + j]);
    if (xdot) xdot[e] = x;
  }
}

// u_l and v_k of the supervised entries (float atomics: entries that share a row or a column are rare; two of them commute,
// so the order of three or more in one row or column - here and in k_dsm_entries - is all in this file that is not fixed)
__global__ __launch_bounds__(256) void k_dsm_uv(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                const int64_t* __restrict__ j_ids, const float* __restrict__ gc, int K,
                                                int L, int S, float* __restrict__ v, float* __restrict__ u) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= K) return;
  atomicAdd(&v[b_ids[e] * L + i_ids[e]], gc[e]);
  atomicAdd(&u[b_ids[e] * S + j_ids[e]], gc[e]);
}

// dX[k, :] = sum_l D_kl Y[l, :],  D_kl = -(exp2(k2 x_kl + nm_y[l]) w_y[l] / sum_y[l] + exp2(k2 x_kl + nm_x[k]) w_x[k] / sum_x[k]),
// x = X_k . Y_l
// The tiled sweep of fm_sweep_device.h (grid, LDS, phases: there) with the dot products summed in channel order and G,
// where there is one, loaded.  Partial gradients (one per z) go to part[z][b][row][c_in]; k_sweep_combine adds them up
// and scales.
// MODE (a DENSE dL/dconf = G [N, L, S], what the reference's loss over all negatives hands back - losses/loss.py:44-50,
// 62-65 - without any [N, L, S] temporary):
//   kDsmSparse : as above (G lives in w_x / w_y and the entries' own kernel).
//   kDsmStats  : v_k = sum_l G_kl conf_kl and u_l = sum_k G_kl conf_kl with conf recomputed tile by tile from exact float32
//                dot products (conf = A B); no gradient phase.  Launched on side 0 only; no atomics: a row's v is
//                one partial per z slice (<= 4), a COLUMN's u one partial per 32-row tile of the owner image (150 at
//                640x480), each stored by its one workgroup and added up in index order by k_sweep_fold_sums - the
//                dense backward's gradients are the same bits on every run.
//   kDsmDense  : D_kl = 2 G_kl conf_kl - A_kl u_l - B_kl v_k, the whole of dL/dsim, accumulated into the rows' gradient.
// G is read through a transposing LDS tile when the owner image is image 1 (g_t: element (owner row, other row) lives at
// G[other][owner]): both sides read 128-byte row segments of G.  G is read three times in all (92 MB per 640x480 pair
// each), nothing of its size is written.
struct DsmSweepPolicy {
  const float* Gb;           // this sample's G
  int g_t;
  float* Gs;                 // [32][33]: the tile of G
  // exact products, fused multiply-adds in channel order
  template <int C>
  static __device__ __forceinline__ void dots(const float* Xs, const float* Ys, int tx, int ty, float (&sv)[4]) {
    constexpr int P = sweep_pitch(C);
#pragma unroll 4
    for (int c = 0; c < C; c += 4) {
      const float4 y = *reinterpret_cast<const float4*>(&Ys[tx * P + c]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(&Xs[(ty + 8 * q) * P + c]);
        sv[q] = __builtin_fmaf(x.x, y.x, sv[q]);
        sv[q] = __builtin_fmaf(x.y, y.y, sv[q]);
        sv[q] = __builtin_fmaf(x.z, y.z, sv[q]);
        sv[q] = __builtin_fmaf(x.w, y.w, sv[q]);
      }
    }
  }
  // 128-byte row segments of G either way: g_t = 0 -> G[owner k0 + ty + 8q][other l0 + tx] straight into registers;
  // g_t = 1 -> G[other l0 + ty + 8q][owner k0 + tx] into the LDS tile, read back transposed behind the barrier
  __device__ __forceinline__ void fetch_g(float (&gq)[4], int k0, int l0, int R, int T) const {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, l = l0 + tx;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!g_t) {
        const int k = k0 + ty + 8 * q;
        gq[q] = (k < R && l < T) ? Gb[(long)k * T + l] : 0.f;
      } else {
        const int lo = l0 + ty + 8 * q, ko = k0 + tx;
        Gs[(ty + 8 * q) * kSweepGsPitch + tx] = (lo < T && ko < R) ? Gb[(long)lo * R + ko] : 0.f;
      }
    }
  }
  __device__ __forceinline__ void g_from_lds(float (&gq)[4]) const {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (g_t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) gq[q] = Gs[tx * kSweepGsPitch + ty + 8 * q];
    }
  }
  __device__ __forceinline__ float gc(float g, float conf, float&) const { return g * conf; }
  __device__ __forceinline__ void keep(bool, float) const {}
  __device__ __forceinline__ void sums_done(float*, long) const {}
};

template <int C, int MODE>
__global__ __launch_bounds__(256) void k_dsm_bwd(const float* __restrict__ X, const float* __restrict__ Y, int R, int T, int c_in,
                                                 const float* __restrict__ ofs_x, const float* __restrict__ sum_x, int pitch_x,
                                                 const float* __restrict__ ofs_y, const float* __restrict__ sum_y,
                                                 int pitch_y, const float* __restrict__ w_x, const float* __restrict__ w_y,
                                                 float k2, float* __restrict__ part, const float* __restrict__ G, int g_t,
                                                 float* __restrict__ v_out, float* __restrict__ u_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  DsmSweepPolicy pol = {G ? G + (long)blockIdx.y * (g_t ? (long)T * R : (long)R * T) : nullptr, g_t, sm + sweep_gs_at(C)};
  sweep_tiles<C, MODE>(X, Y, R, T, c_in, ofs_x, sum_x, pitch_x, ofs_y, sum_y, pitch_y, w_x, w_y, k2, part, v_out, u_out, pol);
}

// out = scale * sum_z part[z]   (fixed order), D_LOSS: scale * d_loss * sum_z part[z] with d_loss [1] on the device, the
// upstream gradient of the coarse loss's scalar
// ADD: on top of what `out` holds (the entries' own terms, added before the sweeps)
template <bool D_LOSS, bool ADD>
__global__ __launch_bounds__(256) void k_sweep_combine(const float4* __restrict__ part, long n4, int Z, float scale,
                                                       const float* __restrict__ d_loss, float4* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float f = D_LOSS ? scale * d_loss[0] : scale;
  float4 s = part[i];
  for (int z = 1; z < Z; ++z) {
    const float4 v = part[(long)z * n4 + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  float4 r = make_float4(s.x * f, s.y * f, s.z * f, s.w * f);
  if (ADD) { const float4 e = out[i]; r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w; }
  out[i] = r;
}

// v += sum over the z slices' partials, u += sum over the row tiles' partials of a statistics sweep, each in index order
// (vpart [Z][n_v], upart [G][n_u]; one thread per element)
__global__ __launch_bounds__(256) void k_sweep_fold_sums(const float* __restrict__ vpart, long n_v, int Z,
                                                         const float* __restrict__ upart, long n_u, int G,
                                                         float* __restrict__ v, float* __restrict__ u) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_v) {
    float s = vpart[i];
    for (int z = 1; z < Z; ++z) s += vpart[(long)z * n_v + i];
    v[i] += s;
  } else if (i - n_v < n_u) {
    const long k = i - n_v;
    float s = upart[k];
    int g = 1;
    for (; g + 8 <= G; g += 8) {                          // eight loads in flight; the additions stay in index order
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = upart[(long)(g + j) * n_u + k];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += x[j];
    }
    for (; g < G; ++g) s += upart[(long)g * n_u + k];
    u[k] += s;
  }
}

// the supervised entries' own term: d0[b, i, :] += 2 g c / (C T) f1[b, j, :],  d1[b, j, :] += 2 g c / (C T) f0[b, i, :]
// (one wave per entry; float atomics).  Launched FIRST, onto zeroed gradients (launch_dsm_entries clears them), and the
// combine of the sweeps' partials adds its sum on top: the first term lands on 0 exactly and two terms commute, so a row
// or column with up to two entries is the same bits in any arrival order - as k_dsm_uv's sums.  Cost: K C atomics.
__global__ __launch_bounds__(256) void k_dsm_entries(const float* __restrict__ f0, const float* __restrict__ f1, int L, int S,
                                                     int c_in, const int64_t* __restrict__ b_ids,
                                                     const int64_t* __restrict__ i_ids, const int64_t* __restrict__ j_ids,
                                                     const float* __restrict__ gc, int K, float scale2,
                                                     float* __restrict__ d0, float* __restrict__ d1) {
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= K) return;
  const long b = b_ids[e], i = i_ids[e], j = j_ids[e];
  const float w = gc[e] * scale2;
  for (int c = lane; c < c_in; c += 64) {
    atomicAdd(&d0[(b * L + i) * c_in + c], w * f1[(b * S + j) * c_in + c]);
    atomicAdd(&d1[(b * S + j) * c_in + c], w * f0[(b * L + i) * c_in + c]);
  }
}

int dsm_zsplit(int N, int R) {
  const int wgs = N * ((R + 31) / 32);
  int z = (512 + wgs - 1) / wgs;
  return z < 1 ? 1 : (z > 4 ? 4 : z);
}

hipError_t launch_dsm_uv(const DsmEntries& e, int L, int S, float* v, float* u, hipStream_t st) {
  hipLaunchKernelGGL(k_dsm_uv, dim3((e.K + 255) / 256), dim3(256), 0, st, e.b_ids, e.i_ids, e.j_ids, e.gc, e.K, L, S, v, u);
  return hipGetLastError();
}

hipError_t launch_dsm_entries(const DsmProblem& p, const DsmEntries& e, float* d_feat0, float* d_feat1, hipStream_t st) {
  hipError_t z = hipMemsetAsync(d_feat0, 0, (size_t)p.N * p.L * p.C * sizeof(float), st);
  if (z == hipSuccess) z = hipMemsetAsync(d_feat1, 0, (size_t)p.N * p.S * p.C * sizeof(float), st);
  if (z != hipSuccess) return z;
  hipLaunchKernelGGL(k_dsm_entries, dim3((e.K + 3) / 4), dim3(256), 0, st, p.feat0, p.feat1, p.L, p.S, p.C, e.b_ids, e.i_ids,
                     e.j_ids, e.gc, e.K, 2.0f * p.inv_ct, d_feat0, d_feat1);
  return hipGetLastError();
}

// NULL pointers, sizes, what the kernels are not built for, the workspace: the order all five had.  conf_at (empty_ok)
// answers K == 0 first and looks at its lists whatever K's sign, the others need theirs only with K > 0.
int dsm_status(const DsmCall& c) {
  const DsmStats& s = c.s;
  if (c.empty_ok && c.e.K == 0) return FM_OK;
  if (c.missing || !c.feat0 || !c.feat1 || !s.ofs_r || !s.ofs_c || !s.sum_r || !s.sum_c) return FM_E_NULL;
  if (c.needs_ws && !c.workspace) return FM_E_NULL;
  if (c.listed && (c.e.K > 0 || c.empty_ok) && (!c.e.b_ids || !c.e.i_ids || !c.e.j_ids || (c.with_gc && !c.e.gc)))
    return FM_E_NULL;
  if ((c.listed && c.e.K < 0) || !(c.N > 0 && c.L > 0 && c.S > 0) || s.pitch_r < c.L || s.pitch_c < c.S) return FM_E_SHAPE;
  if (!valid_channels(c.C) || !(c.temperature > 0.f)) return FM_E_UNSUPPORTED;
  if (c.is_loss) {
    if ((c.loss.kind != FM_LOSS_CROSS_ENTROPY && c.loss.kind != FM_LOSS_FOCAL) || !(c.loss.gamma > 0.f)) return FM_E_UNSUPPORTED;
    if ((double)c.e.K > (double)c.N * c.L * c.S) return FM_E_SHAPE;      // more distinct entries than the matrix has
  }
  if (!c.needs_ws) return FM_OK;
  const size_t need = c.is_loss ? closs_layout(c.N, c.L, c.S, c.C, c.e.K).total : dsm_bwd_layout(c.N, c.L, c.S, c.C).total;
  return workspace_ok(c.workspace, c.workspace_bytes, need) ? FM_OK : FM_E_WORKSPACE;
}

DsmProblem dsm_carve(const DsmCall& c) {
  const float inv_ct = inv_ct_of(c.C, c.temperature);
  const DsmBwdWs w = dsm_bwd_layout(c.N, c.L, c.S, c.C);
  return {c.feat0, c.feat1, c.N, c.L, c.S, c.C, k2_of(inv_ct), inv_ct, w.v.in(c.workspace), w.u.in(c.workspace),
          w.part.in(c.workspace), w.vpart.in(c.workspace), w.upart.in(c.workspace)};
}

int dsm_begin(const DsmCall& c, DsmProblem* p) {
  *p = dsm_carve(c);
  const Span sums = dsm_bwd_layout(c.N, c.L, c.S, c.C).sums;
  return (int)hipMemsetAsync(sums.in(c.workspace), 0, sums.bytes, c.st());
}

hipError_t launch_sweep_combine(const DsmSide& o, int Z, const float* d_loss, float* d_out, bool add, hipStream_t st) {
  const long n4 = (long)o.p.N * o.p.L * o.p.C / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256));
  auto* combine = d_loss ? (add ? k_sweep_combine<true, true> : k_sweep_combine<true, false>)
                         : (add ? k_sweep_combine<false, true> : k_sweep_combine<false, false>);
  hipLaunchKernelGGL(combine, grid, dim3(256), 0, st, (const float4*)o.p.part, n4, Z, o.p.inv_ct, d_loss, (float4*)d_out);
  return hipGetLastError();
}

hipError_t launch_sweep_fold_sums(const DsmProblem& p, hipStream_t st) {
  const long n_v = (long)p.N * p.L, n_u = (long)p.N * p.S;
  hipLaunchKernelGGL(k_sweep_fold_sums, dim3((unsigned)((n_v + n_u + 255) / 256)), dim3(256), 0, st, p.vpart, n_v,
                     dsm_zsplit(p.N, p.L), p.upart, n_u, (p.L + 31) / 32, p.v, p.u);
  return hipGetLastError();
}

// the tiled sweep of one side (0: owner = image 0, 1: owner = image 1) in one of its three modes + the combine of its partials
static int dsm_sweep(int mode, int side, const DsmProblem& p, const DsmCall& c) {
  const DsmSide o = dsm_side(p, c.s, side);
  auto launch = [&](auto cc, auto mm) {
    constexpr int CC = decltype(cc)::value, MM = decltype(mm)::value;
    const bool stats = MM == kDsmStats;          // (side 0: its sums go out as partials, folded into v and u below)
    return launch_sweep<&k_dsm_bwd<CC, MM>>(o, sweep_lds_bytes(CC, true), c.st(), p.part, c.G, side, stats ? p.vpart : p.v,
                                            stats ? p.upart : p.u);
  };
  const hipError_t e = with_padded_channels(p.C, [&](auto cc) {
    if (mode == kDsmSparse) return launch(cc, int_c<kDsmSparse>{});
    return mode == kDsmStats ? launch(cc, int_c<kDsmStats>{}) : launch(cc, int_c<kDsmDense>{});
  });
  if (e != hipSuccess) return (int)e;
  if (mode != kDsmStats)      // (a sparse call's entries have put their own terms into the gradients already)
    return (int)launch_sweep_combine(o, dsm_sweep_grid(o).z, nullptr, side ? c.d_feat1 : c.d_feat0,
                                     mode == kDsmSparse && c.e.K > 0, c.st());
  return (int)launch_sweep_fold_sums(p, c.st());
}

}  // namespace fm

using namespace fm;

extern "C" int fm_dual_softmax_conf_at(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                       const float* ofs_r, const float* sum_r, int pitch_r, const float* ofs_c,
                                       const float* sum_c, int pitch_c,
                                       const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K, float* conf,
                                       void* stream) {
  DsmCall c = {feat0, feat1, N, L, S, C, temperature, {ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c}, {b_ids, i_ids, j_ids, nullptr, K},
               nullptr, nullptr, 0, stream, conf};
  c.listed = c.empty_ok = true; c.missing = !conf;
  const int status = dsm_status(c);
  if (status != FM_OK || K == 0) return status;
  hipLaunchKernelGGL(k_conf_at, dim3((K + 15) / 16), dim3(256), 0, c.st(), feat0, feat1, L, S, C, k2_of(inv_ct_of(C, temperature)),
                     ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c, b_ids, i_ids, j_ids, K, conf, (float*)nullptr);
  return (int)hipGetLastError();
}

extern "C" size_t fm_dual_softmax_backward_workspace_bytes(int N, int L, int S, int C) {
  return N > 0 && L > 0 && S > 0 && valid_channels(C) ? dsm_bwd_layout(N, L, S, C).total : 0;
}

// Backward of the dual softmax for a DENSE dL/dconf (losses/loss.py:44-50, 62-65: the loss terms over all negatives):
// G = dL/dconf [N, L, S] float32 [dev], the softmax statistics as in fm_dual_softmax_backward.  Three tiled sweeps (row /
// column sums of G conf; the two gradients), no [N, L, S] temporary: the workspace is fm_dual_softmax_backward_workspace_bytes.
extern "C" int fm_dual_softmax_backward_dense(const float* feat0, const float* feat1, int N, int L, int S, int C,
                                              float temperature, const float* ofs_r, const float* sum_r, int pitch_r,
                                              const float* ofs_c, const float* sum_c, int pitch_c, const float* G,
                                              void* workspace, size_t workspace_bytes, float* d_feat0, float* d_feat1,
                                              void* stream) {
  DsmCall c = {feat0, feat1, N, L, S, C, temperature, {ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c}, {}, G,
               workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, d_feat0, d_feat1};
  c.needs_ws = true; c.missing = !G || !d_feat0 || !d_feat1;
  DsmProblem p;
  int r = dsm_status(c);
  if (r == FM_OK) r = dsm_begin(c, &p);
  if (r == FM_OK) r = dsm_sweep(kDsmStats, 0, p, c);
  if (r == FM_OK) r = dsm_sweep(kDsmDense, 0, p, c);
  if (r == FM_OK) r = dsm_sweep(kDsmDense, 1, p, c);
  return r;
}

extern "C" int fm_dual_softmax_backward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                        const float* ofs_r, const float* sum_r, int pitch_r, const float* ofs_c,
                                        const float* sum_c, int pitch_c,
                                        const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const float* gc,
                                        int K, void* workspace, size_t workspace_bytes, float* d_feat0, float* d_feat1,
                                        void* stream) {
  DsmCall c = {feat0, feat1, N, L, S, C, temperature, {ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c}, {b_ids, i_ids, j_ids, gc, K},
               nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, d_feat0, d_feat1};
  c.listed = c.with_gc = c.needs_ws = true; c.missing = !d_feat0 || !d_feat1;
  DsmProblem p;
  int r = dsm_status(c);
  if (r == FM_OK) r = dsm_begin(c, &p);
  if (r == FM_OK && K > 0) r = (int)launch_dsm_uv(c.e, L, S, p.v, p.u, c.st());
  if (r == FM_OK && K > 0) r = (int)launch_dsm_entries(p, c.e, d_feat0, d_feat1, c.st());
  if (r == FM_OK) r = dsm_sweep(kDsmSparse, 0, p, c);
  if (r == FM_OK) r = dsm_sweep(kDsmSparse, 1, p, c);
  return r;
}
