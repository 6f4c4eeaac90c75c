// Wave-level device helpers shared by every kernel file: vector types of the matrix-core operands, the XCD workgroup
// remap, cross-lane moves and reductions without LDS (DPP and the gfx950 permlane swaps), the float16 hi / lo split and
// its three-MFMA product.  Defined once: the wait-state rule and the compiler bug the permlane swaps rest on are
// explained at permlane32_swap / permlane16_swap and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

namespace fm {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Workgroups are dealt round-robin over the 8 XCDs (private L2s).  Give each XCD a contiguous range of the n work
// items: neighbouring items share cache lines (the fine stage's windows are sorted by coarse cell, the coarse sweeps'
// workgroups share panels), and one XCD then pulls only its part over the fabric (bijective; speed only).
__device__ __forceinline__ int xcd_contiguous(int bid, int n) {
  const int q = n >> 3, rem = n & 7, x = bid & 7, y = bid >> 3;
  return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + y;
}

// generic pointer into LDS -> the 32-bit LDS address that ds_* / LDS-DMA instructions in inline asm take
template <typename T>
__device__ __forceinline__ unsigned lds_addr(T* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) T*)p; }

// Cross-lane exchange without LDS: v[lane ^ MASK] via DPP (1, 2, 4, 8) or the gfx950 permlane swaps
// (16, 32), folded straight into the reduction operator.  T = float or int.
template <int CTRL, int BANK, class T>
__device__ __forceinline__ T dpp_mov(T old, T v) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                           CTRL, 0xf, BANK, false));
}
// v_permlane32_swap a, b: lanes 32-63 of a <-> lanes 0-31 of b; v_permlane16_swap a, b: odd rows (of 16 lanes) of
// a <-> even rows of b.  Inline asm because hipcc (ROCm 7.2) returns the first result twice from the builtin when
// both operands are one value; s_nop 1 = the two wait states between a VALU write of an operand and the swap.
template <class T>
__device__ __forceinline__ void permlane32_swap(T& a, T& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
template <class T>
__device__ __forceinline__ void permlane16_swap(T& a, T& b) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
struct OpAdd { template <class T> static __device__ __forceinline__ T f(T a, T b) { return a + b; } };
struct OpMax {
  static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ int f(int a, int b) { return max(a, b); }
};
struct OpMin {
  static __device__ __forceinline__ float f(float a, float b) { return fminf(a, b); }
  static __device__ __forceinline__ int f(int a, int b) { return min(a, b); }
};

// op(v[lane], v[lane ^ MASK]) in every lane
template <int MASK, class Op, class T>
__device__ __forceinline__ T pair_op(T v) {
  if constexpr (MASK == 1) return Op::f(v, dpp_mov<0xB1, 0xf>(v, v));           // quad_perm [1,0,3,2]
  else if constexpr (MASK == 2) return Op::f(v, dpp_mov<0x4E, 0xf>(v, v));      // quad_perm [2,3,0,1]
  else if constexpr (MASK == 4) {
    T t = dpp_mov<0x104, 0x5>(v, v);          // row_shl:4 into banks 0,2 (lanes with bit 2 clear read lane+4)
    t = dpp_mov<0x114, 0xA>(t, v);            // row_shr:4 into banks 1,3 (lanes with bit 2 set read lane-4)
    return Op::f(v, t);
  } else if constexpr (MASK == 8) return Op::f(v, dpp_mov<0x128, 0xf>(v, v));   // row_ror:8
  else if constexpr (MASK == 16) {
    T a = v, b = v;       // a = {r0,r0,r2,r2}, b = {r1,r1,r3,r3}: op(a, b) is the pair result in every lane
    permlane16_swap(a, b);
    return Op::f(a, b);
  } else {
    T a = v, b = v;       // a = {lo,lo}, b = {hi,hi}
    permlane32_swap(a, b);
    return Op::f(a, b);
  }
}

// op over the 32 lanes that share lane >> 5, result in every lane of the half (fixed order)
template <class Op, class T>
__device__ __forceinline__ T half_all(T v) {
  v = pair_op<1, Op>(v); v = pair_op<2, Op>(v); v = pair_op<4, Op>(v);
  v = pair_op<8, Op>(v); v = pair_op<16, Op>(v);
  return v;
}
template <class Op, class T>
__device__ __forceinline__ T wave_all(T v) { return pair_op<32, Op>(half_all<Op>(v)); }
__device__ __forceinline__ float wave_sum(float v) { return wave_all<OpAdd>(v); }
__device__ __forceinline__ float wave_max(float v) { return wave_all<OpMax>(v); }

// sum over the 16 lanes of a DPP row, in a fixed order (every lane of the row ends with the same bits)
__device__ __forceinline__ float row_sum16(float v) {
  v = v + dpp_mov<0xB1, 0xf>(v, v);            // quad_perm [1,0,3,2]
  v = v + dpp_mov<0x4E, 0xf>(v, v);            // quad_perm [2,3,0,1]
  v = v + dpp_mov<0x141, 0xf>(v, v);           // row_half_mirror
  v = v + dpp_mov<0x140, 0xf>(v, v);           // row_mirror
  return v;
}

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
  for (int k = 0; k < H1; ++k) permlane32_swap(p[k], p[k + H1]);
#pragma unroll
  for (int k = 0; k < H1; ++k) p[k] += p[k + H1];
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int k = 0; k < H2; ++k) permlane16_swap(p[k], p[k + H2]);
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

// x = hi + lo in float16, both rounded to nearest (x - hi is exact in float32; hi + lo carries 22 significant bits),
// into element e of two float16 vectors
template <class V>
__device__ __forceinline__ void split_f16(float x, V& hi, V& lo, int e) {
  const _Float16 h = (_Float16)x;
  hi[e] = h;
  lo[e] = (_Float16)(x - (float)h);
}
// acc += A.B with both operands split (float32-equivalent product: hi.hi + lo.hi + hi.lo, lo.lo is below 2^-22)
__device__ __forceinline__ void mma3(f32x16& acc, const half8& ah, const half8& al, const half8& bh, const half8& bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
}

}  // namespace fm
