// Device helpers of the fine stage, shared by its forward (fine.hip) and its backward (fine_grad.hip): the
// backward recomputes the forward's similarities and heat maps with these very instructions.
#pragma once
#include "fm_device.h"
#include "fm_wave_device.h"

namespace fm {

constexpr float kFineInvSqrtC = 0.125f;      // 1 / sqrt(Cf), Cf = 64 (exact)

// q0[c] = b0 + sum_r w0[r] F0[r][c], q1 likewise (Linear over the POSITION axis, fine_matching_new.py:50-54)
struct Mix2 { float q0, q1; };
template <int W>
__device__ __forceinline__ Mix2 fine_mix(const float (&f0)[W * W], const float (&f1)[W * W], const float* __restrict__ mix0,
                                         const float* __restrict__ mix1) {
  constexpr int WW = W * W;
  float q0 = mix0[WW], q1 = mix1[WW];
#pragma unroll
  for (int r = 0; r < WW; ++r) { q0 = __builtin_fmaf(mix0[r], f0[r], q0); q1 = __builtin_fmaf(mix1[r], f1[r], q1); }
  return {q0, q1};
}

// sim0[r] = q0 . F1[r], sim1[r] = q1 . F0[r] (fine_matching_new.py:56-57) through one transpose-reduce each: afterwards
// this lane holds the similarities of window position pos; on = it takes part (NP = 32: the even lane of the pair that
// holds a sum)
struct Sims2 { float sim0, sim1; int pos; bool on; };
template <int W>
__device__ __forceinline__ Sims2 fine_sims(const float (&f0)[W * W], const float (&f1)[W * W], float q0, float q1, int lane) {
  constexpr int WW = W * W;
  constexpr int NP = WW > 32 ? 64 : 32;      // butterfly width
  float p[NP];
#pragma unroll
  for (int r = 0; r < NP; ++r) p[r] = r < WW ? q0 * f1[r] : 0.f;
  const float sim0 = transpose_reduce<NP>(p, lane);
#pragma unroll
  for (int r = 0; r < NP; ++r) p[r] = r < WW ? q1 * f0[r] : 0.f;
  const float sim1 = transpose_reduce<NP>(p, lane);
  const int pos = tr_index<NP>(lane);
  return {sim0, sim1, pos, pos < WW && (NP == 64 || !(lane & 1))};
}

// the normalised kornia grid coordinate of window position pos (create_meshgrid)
template <int W>
__device__ __forceinline__ void grid_xy(int pos, float& gx, float& gy) {
  const int wy = pos / W, wx = pos - wy * W;
  gx = ((float)wx / (float)(W - 1) - 0.5f) * 2.f;
  gy = ((float)wy / (float)(W - 1) - 0.5f) * 2.f;
}

// Heat maps of BOTH directions at once.  pos = window position this lane holds (sim0 / sim1 are that position's
// similarities), on = lane takes part.  Per direction: heat = softmax(sim / sqrt(C)), expectation and variance of the
// normalised grid coordinates under it (kornia spatial_expectation2d on create_meshgrid) -> five sums each
// (sum e, sum gx e, sum gy e, sum gx^2 e, sum gy^2 e); the ten sums go through ONE partial transpose-reduce (16 values,
// four two-instruction levels, then two plain levels) instead of ten 6-level butterflies.
// heat_exp2: this lane's unnormalised heat e = exp(sim / sqrt(C) - max) of both directions (0 where !on).
// heat_sums2: the lane-held result t of the ten sums; heat_sum(t, k) is sum k, k = 5 d + {0: e, 1: gx e, 2: gy e,
// 3: gx^2 e, 4: gy^2 e} of direction d (wave-uniform).
struct Heat2 { float e0, e1; };
__device__ __forceinline__ Heat2 heat_exp2(float sim0, float sim1, bool on, float inv_sqrt_c) {
  const float x0 = on ? sim0 * inv_sqrt_c : -INFINITY, x1 = on ? sim1 * inv_sqrt_c : -INFINITY;
  const float m0 = wave_max(x0), m1 = wave_max(x1);
  const float e0 = on ? __expf(x0 - m0) : 0.f, e1 = on ? __expf(x1 - m1) : 0.f;
  return {e0, e1};
}
template <int W>
__device__ __forceinline__ float heat_sums2(float e0, float e1, int pos) {
  float gx, gy;
  grid_xy<W>(pos, gx, gy);
  float q[16] = {e0, gx * e0, gy * e0, gx * gx * e0, gy * gy * e0, e1, gx * e1, gy * e1, gx * gx * e1, gy * gy * e1,
                 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) permlane32_swap(q[k], q[k + 8]);
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] += q[k + 8];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < 4; ++k) permlane16_swap(q[k], q[k + 4]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] += q[k + 4];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < 2; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0x3" : "+v"(q[k]));
#pragma unroll
  for (int k = 0; k < 2; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xc" : "+v"(q[k]) : "v"(q[k + 2]));
  asm volatile("s_nop 1" ::: "memory");
  asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5" : "+v"(q[0]));
  asm volatile("s_nop 1" ::: "memory");
  asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa" : "+v"(q[0]) : "v"(q[1]));
  float t = q[0];                                    // lane bits b5 b4 b3 b2 -> sum 8 b5 + 4 b4 + 2 b3 + b2; fold b1, b0
  // (hipcc's hazard recogniser does not see the asm above as the vector write it is: the wait states the DPP read
  // below needs are given by hand)
  asm volatile("s_nop 1" : "+v"(t));
  t += dpp_mov<0x4E, 0xf>(t, t);                     // lane ^ 2
  t += dpp_mov<0xB1, 0xf>(t, t);                     // lane ^ 1
  // (the sums are read from OTHER lanes below: without this hipcc sinks the last add into the lane-0 branch, where only
  // lane 0 executes it)
  asm volatile("" : "+v"(t));
  return t;
}
__device__ __forceinline__ float heat_sum(const float& t, int k) {
  const int src = 32 * ((k >> 3) & 1) + 16 * ((k >> 2) & 1) + 8 * ((k >> 1) & 1) + 4 * (k & 1);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), src));
}

}  // namespace fm
