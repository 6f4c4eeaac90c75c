// The exact float32 dot product of one descriptor row of image 0 and one of image 1, as the screening's exact phase
// (k_screen_rows) and the assignment (k_select, for the entries the screening listed without it) both compute it: 16
// lanes per entry, lane l16 takes the 4-vectors l16, l16 + 16, l16 + 32, l16 + 48 of the two rows (zero beyond c_in), one
// fma chain in that order, then the 16 lanes' partial sums by row_sum16.  ONE definition of the load, of the chain's
// link and of the final sum: the two kernels must produce the same bits for the same entry - an entry's x is numerator
// and denominator of its conf, and exactly tied entries must stay tied (coarse_matching_new.py:105-106) whichever kernel
// resolved them.  What differs between the two is only how many of a lane's loads are in flight together.
#pragma once
#include "fm_device.h"
#include "fm_wave_device.h"

namespace fm {

// the caller's descriptors [N][L][c_in] / [N][S][c_in] (in_dtype: FM_F32 / FM_F16 / FM_BF16)
struct DescRows {
  const void* src0; const void* src1;
  int c_in, in_dtype, L, S;
};

// element offsets of row `row` of image 0 / row `col` of image 1 of sample b
__device__ __forceinline__ long desc_row0(const DescRows& d, int b, int row) { return ((long)b * d.L + row) * d.c_in; }
__device__ __forceinline__ long desc_row1(const DescRows& d, int b, int col) { return ((long)b * d.S + col) * d.c_in; }

// this lane's q-th 4-vector (q < 4) of the two rows at element offsets ro / co; image 0's is zero beyond c_in (the load
// is clamped, not predicated)
__device__ __forceinline__ void exact_dot16_load1(const DescRows& d, long ro, long co, int l16, int q, float4& va, float4& vb) {
  const int v4 = l16 + 16 * q;
  const bool in = v4 < (d.c_in >> 2);
  const int vc = in ? v4 : 0;
  float4 ta, tb;
  if (d.in_dtype == FM_F32) {
    ta = reinterpret_cast<const float4*>((const float*)d.src0 + ro)[vc];
    tb = reinterpret_cast<const float4*>((const float*)d.src1 + co)[vc];
  } else {
    ta = half4_to_float4(reinterpret_cast<const uint2*>((const unsigned short*)d.src0 + ro)[vc], d.in_dtype);
    tb = half4_to_float4(reinterpret_cast<const uint2*>((const unsigned short*)d.src1 + co)[vc], d.in_dtype);
  }
  va = in ? ta : make_float4(0.f, 0.f, 0.f, 0.f);
  vb = tb;
}

// one link of the lane's fma chain: the four channels of a 4-vector, in order
__device__ __forceinline__ float exact_dot16_link(float sm, const float4& va, const float4& vb) {
  sm = __builtin_fmaf(va.x, vb.x, sm);
  sm = __builtin_fmaf(va.y, vb.y, sm);
  sm = __builtin_fmaf(va.z, vb.z, sm);
  sm = __builtin_fmaf(va.w, vb.w, sm);
  return sm;
}

// k_screen_rows: all eight loads of an entry issued together (and two entries' worth before the first use) ...
__device__ __forceinline__ void exact_dot16_load(const DescRows& d, int b, int row, int col, int l16, float4 (&av)[4],
                                                 float4 (&bv)[4]) {
  const long ro = desc_row0(d, b, row), co = desc_row1(d, b, col);
#pragma unroll
  for (int q = 0; q < 4; ++q) exact_dot16_load1(d, ro, co, l16, q, av[q], bv[q]);
}
// ... and the product from them: the same bits in all 16 lanes of the entry's DPP row
__device__ __forceinline__ float exact_dot16_sum(const float4 (&av)[4], const float4 (&bv)[4]) {
  float sm = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) sm = exact_dot16_link(sm, av[q], bv[q]);
  return row_sum16(sm);
}

// k_select: the same loads, links and sum with ONE 4-vector pair in flight - a resolved entry is the exception there,
// and eight float4 of load targets on top of the assignment's state cost the kernel two of its five waves per SIMD
__device__ __forceinline__ float exact_dot16_serial(const DescRows& d, int b, int row, int col, int l16) {
  const long ro = desc_row0(d, b, row), co = desc_row1(d, b, col);
  float sm = 0.f;
#pragma nounroll
  for (int q = 0; q < 4; ++q) {
    float4 va, vb;
    exact_dot16_load1(d, ro, co, l16, q, va, vb);
    sm = exact_dot16_link(sm, va, vb);
  }
  return row_sum16(sm);
}

// Bit 30 of a list index (rlist_j / clist_i): the entry was listed WITHOUT its exact dot product - its x is the
// stand-in sigma_0 sigma_1 q (see sure_slack in coarse_screen.hip).  Indices are < 2^30 (defer_exact_on asks for it).
constexpr int kDeferTag = 0x40000000;

// Wave-cooperative: every lane with `need` holds an entry (row, col) of ITS sample b whose x is a stand-in; returns the
// exact product in those lanes and x unchanged in all others.  Four entries per pass, one per group of 16 lanes (as in
// the exact phase of k_screen_rows).  A wave without such a lane pays one ballot; any = whether the wave had one
// (uniform).  Call it where the whole wave is active.
__device__ __forceinline__ float resolve_deferred(const DescRows& d, int b, bool need, int row, int col, float x, int lane,
                                                  bool& any) {
  unsigned long long m = __ballot(need);
  any = m != 0;
  const int sub = lane >> 4, l16 = lane & 15;
  while (m) {                                   // (wave-uniform)
    int src = 0, nsrc = 0;
    unsigned long long mm = m;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (mm) {
        const int l = __builtin_ctzll(mm);
        mm &= mm - 1;
        if (sub == g) src = l;
        nsrc = g + 1;
      } else if (sub == g) {
        src = __builtin_ctzll(m);               // idle group: repeats the first entry, its result is not delivered
      }
    }
    // (the sample too comes from the entry's lane: a lane of a padding row holds a clamped one)
    const int r = __shfl(row, src), c = __shfl(col, src), bs = __shfl(b, src);
    const float v = exact_dot16_serial(d, bs, r, c, l16);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float vg = __shfl(v, 16 * g);
      const int sg = __shfl(src, 16 * g);
      if (g < nsrc && lane == sg) x = vg;
    }
    m = mm;
  }
  return x;
}

}  // namespace fm
