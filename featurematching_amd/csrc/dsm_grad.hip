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
#include "fm_sweep_device.h"
#include "fm_wave_device.h"

namespace fm {

// conf at K entries: 16 lanes per entry (16 channels per lane, four 16-byte loads per row), the exact float32 dot
// product in a fixed order - the arithmetic of k_screen's exact phase.
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

// u_l and v_k of the supervised entries (float atomics: entries that share a row or a column are rare, and the order
// in which two of them are added is the only thing that is not fixed)
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
//                dot products (conf = A B); no gradient phase.  Launched on side 0 only; v and u by float atomics: a row's
//                v takes one add per z slice (<= 4), a COLUMN's u one add per 32-row tile of the owner image (150 at
//                640x480) in arrival order - the dense backward's gradients are therefore reproducible to float32
//                rounding of those sums (~1e-7 relative), not bit for bit; every other reduction of this file is
//                order-fixed (k_fix_sums, k_sweep_combine).
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
template <bool D_LOSS>
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
  out[i] = make_float4(s.x * f, s.y * f, s.z * f, s.w * f);
}

// the supervised entries' own term: d0[b, i, :] += 2 g c / (C T) f1[b, j, :],  d1[b, j, :] += 2 g c / (C T) f0[b, i, :]
// (one wave per entry; float atomics - see k_dsm_uv)
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

// Dense data['conf_matrix'] (k_dense<C, CONF>: hi/lo-split float16 products, 22 significant bits - 2e-4 in a conf near 1 at
// |sim| ~ 200): every entry that matters takes the exact float32 route.  For the samples the screening kernel served,
// the rows' lists hold every entry with a row term above 2^-32 (all entries with conf > 2.4e-10 are among them) together
// with its exact dot product; their conf is rewritten from that number and the same log-softmax offsets.
// One thread per (row, slot).
__global__ __launch_bounds__(256) void k_conf_patch(const int* __restrict__ rcount, const int* __restrict__ rlist_j,
                                                    const float* __restrict__ rlist_x, const int* __restrict__ rcount_d,
                                                    const int* __restrict__ rlist_j_d, const float* __restrict__ rlist_x_d,
                                                    const float* __restrict__ nm_r,
                                                    const float* __restrict__ sum_r, const float* __restrict__ nm_c,
                                                    const float* __restrict__ sum_c, const int* __restrict__ dense_cnt, int N,
                                                    int L, int S, int Lp, int Sp, int slots, float k2, float* __restrict__ conf) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long grow = gid / slots;
  const int slot = (int)(gid - grow * slots);
  if (grow >= (long)N * Lp) return;
  const int b = (int)(grow / Lp), i = (int)(grow - (long)b * Lp);
  if (i >= L) return;
  const bool dense = dense_cnt[b] > 0;         // the dense kernel's lists, made exact by k_exact_lists
  if (slot >= min((dense ? rcount_d : rcount)[grow], slots)) return;
  const float x = (dense ? rlist_x_d : rlist_x)[grow * slots + slot];
  if (!(x > -INFINITY)) return;                    // a reserved but empty place
  const int j = (dense ? rlist_j_d : rlist_j)[grow * slots + slot];
  const long gcol = (long)b * Sp + j;
  conf[((long)b * L + i) * S + j] = (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_r[grow])) / sum_r[grow]) *
                                    (__builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm_c[gcol])) / sum_c[gcol]);
}

// The samples the DENSE kernel served (flat similarity somewhere in the sample), when every entry is read (conf_matrix,
// softmax statistics): the hi/lo-split float16 products carry 22 bits, 2^-22 |sim| ~ 4e-5 at similarities of ~170 - and
// a peaked row of such a sample (conf ~ 1: the entry IS its row's and its column's denominator) is only right when the
// entry and the two denominators hold the SAME x.  So the lists of such a sample - with a conf_matrix request they are
// formed with min(thr, 0.1): every entry whose two softmax factors both exceed 0.1, i.e. every entry with conf > 0.1 -
// are resolved exactly, entries and denominators together:
//   k_exact_lists : 16 lanes per row list and per column list, its entries in turn: the exact float32 dot product of the caller's
//                   descriptors (the arithmetic of k_conf_at) replaces the list's x; the term's change
//                   exp2(k x + nm) - exp2(k x22 + nm) goes to the screening kernel's list region of the sample (idle)
//   k_fix_sums    : one thread per row / column: adds the changes in index order (same bits every run) to the
//                   denominator, refreshes the log-softmax offset
// The assignment then reads exact x and matching denominators (mconf = the conf_matrix entry), k_conf_patch rewrites the
// listed entries of the dense matrix.  What stays 22-bit has conf <= 0.1: 2 * 2^-22 |sim| conf <= 8e-6 at |sim| ~ 170.
__global__ __launch_bounds__(256) void k_exact_lists(const void* __restrict__ f0, const void* __restrict__ f1, int in_dtype, int c_in,
                                                     const int* __restrict__ rcount, const int* __restrict__ rkey, float* __restrict__ rx,
                                                     float* __restrict__ rdelta, const int* __restrict__ ccount,
                                                     const int* __restrict__ ckey, float* __restrict__ cx, float* __restrict__ cdelta,
                                                     const float* __restrict__ nm_r, const float* __restrict__ nm_c,
                                                     const int* __restrict__ dense_cnt, int N, int L, int S, int Lp, int Sp,
                                                     int slots, float k2) {
  const int side = blockIdx.z;
  const int len = side ? Sp : Lp;
  const long gl = (long)blockIdx.x * 16 + (threadIdx.x >> 4);           // one 16-lane group per list, its slots in turn
  const int l16 = threadIdx.x & 15;
  if (gl >= (long)N * len) return;
  const int b = (int)(gl / len), own = (int)(gl - (long)b * len);
  if (own >= (side ? S : L) || dense_cnt[b] == 0) return;              // (uniform over the group)
  const int n = min((side ? ccount : rcount)[gl], slots);
  const int vpr = c_in >> 2;
  for (int slot = 0; slot < n; ++slot) {
    const long at = gl * slots + slot;
    const int other = (side ? ckey : rkey)[at];
    const int i = side ? other : own, j = side ? own : other;
    const long ro = ((long)b * L + i) * c_in, co = ((long)b * S + j) * c_in;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int v4 = l16 + 16 * q;
      const bool in = v4 < vpr;
      const int vc = in ? v4 : 0;
      float4 a, bb;
      if (in_dtype == FM_F32) {
        a = reinterpret_cast<const float4*>((const float*)f0 + ro)[vc];
        bb = reinterpret_cast<const float4*>((const float*)f1 + co)[vc];
      } else {
        a = half4_to_float4(reinterpret_cast<const uint2*>((const unsigned short*)f0 + ro)[vc], in_dtype);
        bb = half4_to_float4(reinterpret_cast<const uint2*>((const unsigned short*)f1 + co)[vc], in_dtype);
      }
      if (!in) a = make_float4(0.f, 0.f, 0.f, 0.f);
      s = __builtin_fmaf(a.x, bb.x, s);
      s = __builtin_fmaf(a.y, bb.y, s);
      s = __builtin_fmaf(a.z, bb.z, s);
      s = __builtin_fmaf(a.w, bb.w, s);
    }
    const float x = row_sum16(s);
    if (l16 == 0) {
      float* xs = side ? cx : rx;
      const float nm = (side ? nm_c : nm_r)[gl];
      (side ? cdelta : rdelta)[at] = __builtin_amdgcn_exp2f(__builtin_fmaf(x, k2, nm)) - __builtin_amdgcn_exp2f(__builtin_fmaf(xs[at], k2, nm));
      xs[at] = x;
    }
  }
}

__global__ __launch_bounds__(256) void k_fix_sums(const int* __restrict__ rcount, const int* __restrict__ rkey,
                                                  const float* __restrict__ rdelta, const int* __restrict__ ccount,
                                                  const int* __restrict__ ckey, const float* __restrict__ cdelta,
                                                  const float* __restrict__ nm_r, const float* __restrict__ nm_c,
                                                  float* __restrict__ sum_r, float* __restrict__ sum_c, float* __restrict__ nm2_r,
                                                  float* __restrict__ nm2_c, const int* __restrict__ dense_cnt, int Lp, int Sp,
                                                  int slots) {
  const int side = blockIdx.z, b = blockIdx.y;
  const int len = side ? Sp : Lp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= len || dense_cnt[b] == 0) return;
  const long gl = (long)b * len + idx;
  const int n = min((side ? ccount : rcount)[gl], slots);
  if (n == 0) return;
  const int* key = (side ? ckey : rkey) + gl * slots;
  const float* d = (side ? cdelta : rdelta) + gl * slots;
  float acc = 0.f;
  int last = -1;
  for (int t = 0; t < n; ++t) {           // in index order (the lists are filled in the order the waves arrive)
    int best = 0x7fffffff, at = 0;
    for (int q = 0; q < n; ++q) { const int kq = key[q]; if (kq > last && kq < best) { best = kq; at = q; } }
    acc += d[at];
    last = best;
  }
  float* sum = side ? sum_c : sum_r;
  const float v = sum[gl] + acc;
  sum[gl] = v;
  (side ? nm2_c : nm2_r)[gl] = (side ? nm_c : nm_r)[gl] - __log2f(v);
}

hipError_t launch_exact_lists(const CoarseWs& w, char* base, float inv_ct, const void* feat0, const void* feat1, int in_dtype,
                              int c_in, hipStream_t st) {
  // the dense kernel's lists; every term's change goes to the same slot of the sparse kernel's x arrays (idle for the
  // samples the dense kernel redid), where k_fix_sums reads it
  const CandList &rows = w.cand_b, &cols = w.ccand_b;
  float *rdelta = w.cand.x.in(base), *cdelta = w.ccand.x.in(base);
  const long groups = (long)w.N * max(w.Lp, w.Sp);
  hipLaunchKernelGGL(k_exact_lists, dim3((unsigned)((groups + 15) / 16), 1, 2), dim3(256), 0, st, feat0, feat1, in_dtype, c_in,
                     rows.count.in(base), rows.idx.in(base), rows.x.in(base), rdelta, cols.count.in(base), cols.idx.in(base),
                     cols.x.in(base), cdelta, w.nmr.in(base), w.nmc.in(base), w.dense_cnt.in(base), w.N, w.L, w.S, w.Lp, w.Sp,
                     w.slots, inv_ct * kLog2e);
  hipLaunchKernelGGL(k_fix_sums, dim3((max(w.Lp, w.Sp) + 255) / 256, w.N, 2), dim3(256), 0, st, rows.count.in(base),
                     rows.idx.in(base), rdelta, cols.count.in(base), cols.idx.in(base), cdelta, w.nmr.in(base), w.nmc.in(base),
                     w.rsum.in(base), w.csum.in(base), w.nmr2.in(base), w.nmc2.in(base), w.dense_cnt.in(base), w.Lp, w.Sp, w.slots);
  return hipGetLastError();
}

hipError_t launch_conf_patch(const CoarseWs& w, char* base, float inv_ct, float* conf, hipStream_t st) {
  const long total = (long)w.N * w.Lp * w.slots;
  hipLaunchKernelGGL(k_conf_patch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w.cand.count.in(base),
                     w.cand.idx.in(base), w.cand.x.in(base), w.cand_b.count.in(base), w.cand_b.idx.in(base), w.cand_b.x.in(base),
                     w.nmr.in(base), w.rsum.in(base), w.nmc.in(base), w.csum.in(base), w.dense_cnt.in(base), w.N, w.L, w.S, w.Lp,
                     w.Sp, w.slots, inv_ct * kLog2e, conf);
  return hipGetLastError();
}

int dsm_zsplit(int N, int R) {
  const int wgs = N * ((R + 31) / 32);
  int z = (512 + wgs - 1) / wgs;
  return z < 1 ? 1 : (z > 4 ? 4 : z);
}

hipError_t launch_dsm_uv(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const float* gc, int K, int L, int S,
                         float* v, float* u, hipStream_t st) {
  hipLaunchKernelGGL(k_dsm_uv, dim3((K + 255) / 256), dim3(256), 0, st, b_ids, i_ids, j_ids, gc, K, L, S, v, u);
  return hipGetLastError();
}

hipError_t launch_dsm_entries(const DsmProblem& p, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                              const float* gc, int K, float* d_feat0, float* d_feat1, hipStream_t st) {
  hipLaunchKernelGGL(k_dsm_entries, dim3((K + 3) / 4), dim3(256), 0, st, p.feat0, p.feat1, p.L, p.S, p.C, b_ids, i_ids, j_ids, gc,
                     K, 2.0f * p.inv_ct, d_feat0, d_feat1);
  return hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" int fm_dual_softmax_conf_at(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                       const float* ofs_r, const float* sum_r, int pitch_r, const float* ofs_c,
                                       const float* sum_c, int pitch_c,
                                       const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K, float* conf,
                                       void* stream) {
  if (K == 0) return FM_OK;
  if (!feat0 || !feat1 || !ofs_r || !ofs_c || !sum_r || !sum_c || !b_ids || !i_ids || !j_ids || !conf) return FM_E_NULL;
  if (!(N > 0 && L > 0 && S > 0) || K < 0 || pitch_r < L || pitch_c < S) return FM_E_SHAPE;
  if (!valid_channels(C) || !(temperature > 0.f)) return FM_E_UNSUPPORTED;
  // (the SAME two roundings as the k2 the statistics were formed with - inv_ct * kLog2e in every coarse launch: the
  // stabilisers are -k2 x_max, and a k2 one ulp away leaves (k2 - k2') x in both exponents: 4.5e-5 of a conf near 1 at
  // |sim| ~ 160 and C = 36 or 100, where kLog2e / (C T) and kLog2e * (1 / (C T)) round differently)
  const float inv_ct = 1.0f / ((float)C * temperature);
  const float k2 = inv_ct * kLog2e;
  hipLaunchKernelGGL(k_conf_at, dim3((K + 15) / 16), dim3(256), 0, (hipStream_t)stream, feat0, feat1, L, S, C, k2, ofs_r,
                     sum_r, pitch_r, ofs_c, sum_c, pitch_c, b_ids, i_ids, j_ids, K, conf, (float*)nullptr);
  return (int)hipGetLastError();
}

extern "C" size_t fm_dual_softmax_backward_workspace_bytes(int N, int L, int S, int C) {
  return N > 0 && L > 0 && S > 0 && valid_channels(C) ? dsm_bwd_layout(N, L, S, C).total : 0;
}

// what every backward entry point does after its NULL checks: the remaining argument checks and the carved workspace ...
int fm::dsm_carve(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature, const DsmStats& s,
                  void* workspace, size_t workspace_bytes, DsmProblem* p) {
  if (!(N > 0 && L > 0 && S > 0) || s.pitch_r < L || s.pitch_c < S) return FM_E_SHAPE;
  if (!valid_channels(C) || !(temperature > 0.f)) return FM_E_UNSUPPORTED;
  const DsmBwdWs w = dsm_bwd_layout(N, L, S, C);
  if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return FM_E_WORKSPACE;
  const float inv_ct = 1.0f / ((float)C * temperature);
  *p = {feat0, feat1, N, L, S, C, kLog2e * inv_ct, inv_ct, span_ptr<float>(workspace, w.v), span_ptr<float>(workspace, w.u),
        span_ptr<float>(workspace, w.part)};
  return FM_OK;
}

// ... and, for a call that forms v and u itself, the two zeroed
int fm::dsm_begin(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature, const DsmStats& s,
                  void* workspace, size_t workspace_bytes, hipStream_t st, DsmProblem* p) {
  const int r = dsm_carve(feat0, feat1, N, L, S, C, temperature, s, workspace, workspace_bytes, p);
  if (r != FM_OK) return r;
  const DsmBwdWs w = dsm_bwd_layout(N, L, S, C);
  return (int)hipMemsetAsync(span_ptr<char>(workspace, w.sums), 0, w.sums.bytes, st);
}

hipError_t fm::launch_sweep_combine(const DsmSide& o, int Z, const float* d_loss, float* d_out, hipStream_t st) {
  const long n4 = (long)o.p.N * o.p.L * o.p.C / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256));
  auto* combine = d_loss ? k_sweep_combine<true> : k_sweep_combine<false>;
  hipLaunchKernelGGL(combine, grid, dim3(256), 0, st, (const float4*)o.p.part, n4, Z, o.p.inv_ct, d_loss, (float4*)d_out);
  return hipGetLastError();
}

// the tiled sweep of one side (0: owner = image 0, 1: owner = image 1) in one of its three modes + the combine of its partials
static int dsm_sweep(int mode, int side, const DsmProblem& p, const DsmStats& s, const float* G, float* d_out, hipStream_t st) {
  const DsmSide o = dsm_side(p, s, side);
  const dim3 grid = dsm_sweep_grid(o);
  auto launch = [&](auto cc, auto mm) -> hipError_t {
    constexpr int CC = decltype(cc)::value, MM = decltype(mm)::value, smem = sweep_lds_bytes(CC, true);
    static unsigned long long lds_set = 0;      // (one per instantiation of this lambda, that is, per kernel)
    const hipError_t e = ensure_dynamic_lds(&k_dsm_bwd<CC, MM>, smem, &lds_set);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dsm_bwd<CC, MM>), grid, dim3(256), smem, st, o.p.feat0, o.p.feat1, o.p.L, o.p.S, p.C, o.s.ofs_r,
                       o.s.sum_r, o.s.pitch_r, o.s.ofs_c, o.s.sum_c, o.s.pitch_c, o.p.v, o.p.u, p.k2, p.part, G, side, p.v, p.u);
    return hipSuccess;
  };
  const hipError_t e = with_padded_channels(p.C, [&](auto cc) {
    if (mode == kDsmSparse) return launch(cc, int_c<kDsmSparse>{});
    return mode == kDsmStats ? launch(cc, int_c<kDsmStats>{}) : launch(cc, int_c<kDsmDense>{});
  });
  if (e != hipSuccess) return (int)e;
  if (mode != kDsmStats) return (int)launch_sweep_combine(o, grid.z, nullptr, d_out, st);
  return (int)hipGetLastError();
}

// Backward of the dual softmax for a DENSE dL/dconf (losses/loss.py:44-50, 62-65: the loss terms over all negatives):
// G = dL/dconf [N, L, S] float32 [dev], the softmax statistics as in fm_dual_softmax_backward.  Three tiled sweeps (row /
// column sums of G conf; the two gradients), no [N, L, S] temporary: the workspace is fm_dual_softmax_backward_workspace_bytes.
extern "C" int fm_dual_softmax_backward_dense(const float* feat0, const float* feat1, int N, int L, int S, int C,
                                              float temperature, const float* ofs_r, const float* sum_r, int pitch_r,
                                              const float* ofs_c, const float* sum_c, int pitch_c, const float* G,
                                              void* workspace, size_t workspace_bytes, float* d_feat0, float* d_feat1,
                                              void* stream) {
  if (!feat0 || !feat1 || !ofs_r || !ofs_c || !sum_r || !sum_c || !G || !workspace || !d_feat0 || !d_feat1) return FM_E_NULL;
  hipStream_t st = (hipStream_t)stream;
  const DsmStats s = {ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c};
  DsmProblem p;
  int r = dsm_begin(feat0, feat1, N, L, S, C, temperature, s, workspace, workspace_bytes, st, &p);
  if (r != FM_OK) return r;
  r = dsm_sweep(kDsmStats, 0, p, s, G, nullptr, st);
  if (r != FM_OK) return r;
  r = dsm_sweep(kDsmDense, 0, p, s, G, d_feat0, st);
  if (r != FM_OK) return r;
  return dsm_sweep(kDsmDense, 1, p, s, G, d_feat1, st);
}

extern "C" int fm_dual_softmax_backward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                        const float* ofs_r, const float* sum_r, int pitch_r, const float* ofs_c,
                                        const float* sum_c, int pitch_c,
                                        const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const float* gc,
                                        int K, void* workspace, size_t workspace_bytes, float* d_feat0, float* d_feat1,
                                        void* stream) {
  if (!feat0 || !feat1 || !ofs_r || !ofs_c || !sum_r || !sum_c || !workspace || !d_feat0 || !d_feat1) return FM_E_NULL;
  if (K > 0 && (!b_ids || !i_ids || !j_ids || !gc)) return FM_E_NULL;
  if (K < 0) return FM_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const DsmStats s = {ofs_r, sum_r, pitch_r, ofs_c, sum_c, pitch_c};
  DsmProblem p;
  int r = dsm_begin(feat0, feat1, N, L, S, C, temperature, s, workspace, workspace_bytes, st, &p);
  if (r != FM_OK) return r;
  if (K > 0) {
    r = (int)launch_dsm_uv(b_ids, i_ids, j_ids, gc, K, L, S, p.v, p.u, st);
    if (r != FM_OK) return r;
  }
  for (int side = 0; side < 2; ++side) {
    r = dsm_sweep(kDsmSparse, side, p, s, nullptr, side ? d_feat1 : d_feat0, st);
    if (r != FM_OK) return r;
  }
  if (K > 0) return (int)launch_dsm_entries(p, b_ids, i_ids, j_ids, gc, K, d_feat0, d_feat1, st);
  return (int)hipGetLastError();
}
