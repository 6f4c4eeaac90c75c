// Cross-lane helpers of the fine stage, shared by its forward (fine.hip) and its backward (fine_grad.hip): the
// backward recomputes the forward's similarities and heat maps with these very instructions.
#pragma once
#include "fm_device.h"

namespace fm {

// Cross-lane exchange without LDS: v[lane ^ MASK] via DPP (1, 2, 4, 8) or the gfx950 permlane swaps
// (16, 32), folded straight into the reduction operator.
template <int CTRL, int BANK>
__device__ __forceinline__ float dpp_mov(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                               CTRL, 0xf, BANK, false));
}
struct OpAdd { static __device__ __forceinline__ float f(float a, float b) { return a + b; } };
struct OpMax { static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };

// op(v[lane], v[lane ^ MASK]) in every lane
template <int MASK, class Op>
__device__ __forceinline__ float pair_op(float v) {
  if constexpr (MASK == 1) return Op::f(v, dpp_mov<0xB1, 0xf>(v, v));           // quad_perm [1,0,3,2]
  else if constexpr (MASK == 2) return Op::f(v, dpp_mov<0x4E, 0xf>(v, v));      // quad_perm [2,3,0,1]
  else if constexpr (MASK == 4) {
    float t = dpp_mov<0x104, 0x5>(v, v);      // row_shl:4 into banks 0,2 (lanes with bit 2 clear read lane+4)
    t = dpp_mov<0x114, 0xA>(t, v);            // row_shr:4 into banks 1,3 (lanes with bit 2 set read lane-4)
    return Op::f(v, t);
  } else if constexpr (MASK == 8) return Op::f(v, dpp_mov<0x128, 0xf>(v, v));   // row_ror:8
  else if constexpr (MASK == 16) {
    // v_permlane16_swap a, b: odd rows of a <-> even rows of b.  With a = b = v: a = {r0,r0,r2,r2},
    // b = {r1,r1,r3,r3}, so op(a, b) is the pair result in every lane.  Inline asm because hipcc
    // (ROCm 7.2) returns the first result twice from the builtin when both operands are one value;
    // s_nop 1 = the two wait states between a VALU write of an operand and the swap.
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return Op::f(a, b);
  } else {
    float a = v, b = v;   // lanes 32-63 of a <-> lanes 0-31 of b: a = {lo,lo}, b = {hi,hi}
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return Op::f(a, b);
  }
}

template <class Op>
__device__ __forceinline__ float wave_all(float v) {
  v = pair_op<1, Op>(v); v = pair_op<2, Op>(v); v = pair_op<4, Op>(v);
  v = pair_op<8, Op>(v); v = pair_op<16, Op>(v); v = pair_op<32, Op>(v);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) { return wave_all<OpAdd>(v); }
__device__ __forceinline__ float wave_max(float v) { return wave_all<OpMax>(v); }

// Transpose-reduce: p[k] = this lane's term of sum k (k < NP = 32 or 64) -> every sum ends in ONE lane (NP = 64) or in
// a pair of neighbouring lanes (NP = 32), tr_index(lane) tells which.  Each level halves the registers: a lane keeps one
// half and hands the other to its partner.  Written so that the levels with many pairs cost TWO instructions per pair
// and no select (round 2's butterfly spent five: two DPP moves, two adds, one select):
//   lane ^ 32 : v_permlane32_swap X, Y leaves {X.lo, Y.lo} / {X.hi, Y.hi}; X + Y = X's sum in lanes 0-31, Y's in 32-63
//   lane ^ 16 : v_permlane16_swap likewise for the rows of 16 lanes
//   15 - i    : row_mirror DPP add with bank-masked writes: banks 0-1 keep X, banks 2-3 receive Y's sum (into X)
//   7 - i     : row_half_mirror, banks 0 / 2 keep X, banks 1 / 3 receive Y's
//   3 - i     : inside the quad by select + quad_perm (one or two pairs are left by then)
//   i ^ 1     : NP = 64: one more transposing level; NP = 32: a plain sum (both lanes of a pair hold it)
// (s_nop 1: the two wait states a DPP / permlane operand needs after the VALU write of its register.)
template <int NP>
__device__ __forceinline__ float transpose_reduce(float (&p)[NP], int lane) {
  constexpr int H1 = NP / 2, H2 = NP / 4, H3 = NP / 8, H4 = NP / 16, H5 = NP / 32;
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H1; ++k) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(p[k]), "+v"(p[k + H1]));
#pragma unroll
  for (int k = 0; k < H1; ++k) p[k] += p[k + H1];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H2; ++k) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(p[k]), "+v"(p[k + H2]));
#pragma unroll
  for (int k = 0; k < H2; ++k) p[k] += p[k + H2];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H3; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0x3" : "+v"(p[k]));
#pragma unroll
  for (int k = 0; k < H3; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xc" : "+v"(p[k]) : "v"(p[k + H3]));
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H4; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5" : "+v"(p[k]));
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H4; ++k)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa" : "+v"(p[k]) : "v"(p[k + H4]));
  const bool b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
#pragma unroll
  for (int k = 0; k < H5; ++k) {                 // lane 3 - i of the quad: quad_perm [3,2,1,0]
    const float own = b1 ? p[k + H5] : p[k], other = b1 ? p[k] : p[k + H5];
    p[k] = own + dpp_mov<0x1B, 0xf>(other, other);
  }
  if constexpr (NP == 64) {                      // lane i ^ 1 takes the second of the last two sums
    const float own = b0 ? p[1] : p[0], other = b0 ? p[0] : p[1];
    return own + dpp_mov<0xB1, 0xf>(other, other);
  } else {
    return p[0] + dpp_mov<0xB1, 0xf>(p[0], p[0]);
  }
}
// lane bits b5..b0 -> the sum it holds
template <int NP>
__device__ __forceinline__ int tr_index(int lane) {
  const int b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1, b3 = (lane >> 3) & 1, b2 = (lane >> 2) & 1, b1 = (lane >> 1) & 1;
  if constexpr (NP == 64) return 32 * b5 + 16 * b4 + 8 * b3 + 4 * b2 + 2 * b1 + (lane & 1);
  else return 16 * b5 + 8 * b4 + 4 * b3 + 2 * b2 + b1;
}

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
  for (int k = 0; k < 8; ++k) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(q[k]), "+v"(q[k + 8]));
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] += q[k + 8];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < 4; ++k) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(q[k]), "+v"(q[k + 4]));
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
