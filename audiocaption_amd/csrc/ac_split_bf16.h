// The split-bf16 operand arithmetic of the library's f32-grade matrix work, defined once for every kernel that uses it.
//
//   operand   x = hi + lo,  hi = RNE_bf16(x),  lo = RNE_bf16(x - hi)      (16 significant bits: 2^-16 relative operand error)
//   product   lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16, in that order, f32 accumulation (lo*lo is dropped)
//
// The host side of the same convention is kernels.split_bf16 (the weight packers pre-split the other operand with it);
// tests/_split_ref.py derives the conv error bars from it and tests/test_gpu_split_bf16.py holds the two splits to the
// same bits.  The wide decode GEMM carries the split one plane further (split3_bf16x4: 24 bits, exact for f32).
#pragma once
#include "ac_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// two floats -> one dword of two bf16 (RNE), `lo` in the low half
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// the two halves of a packed dword widened back to f32
__device__ __forceinline__ float bf16_lo(unsigned pk) { return __builtin_bit_cast(float, pk << 16); }
__device__ __forceinline__ float bf16_hi(unsigned pk) { return __builtin_bit_cast(float, pk & 0xffff0000u); }

// x (4 floats) -> packed hi (2 dwords) and lo (2 dwords) bf16 quadruples: both hi dwords first, then both lo dwords -
// the order the conv kernels that split a staged patch are scheduled around
__device__ __forceinline__ void split_bf16x4(const f32x4 x, u32x2& hi, u32x2& lo) {
  hi.x = cvt_pk_bf16(x[0], x[1]);
  hi.y = cvt_pk_bf16(x[2], x[3]);
  const float h0 = bf16_lo(hi.x), h1 = bf16_hi(hi.x), h2 = bf16_lo(hi.y), h3 = bf16_hi(hi.y);
  lo.x = cvt_pk_bf16(x[0] - h0, x[1] - h1);
  lo.y = cvt_pk_bf16(x[2] - h2, x[3] - h3);
}

// x (2 N floats) -> packed hi (N dwords) and lo (N dwords), one pair after the other: the same values as split_bf16x4 in
// the order the GEMMs that split while staging (csrc/train.hip: N = 4, csrc/pw_gemm.hip: N = 2) are scheduled around
template <int N, typename X, typename V>
__device__ __forceinline__ void split_bf16_pairs(const X& x, V& hi, V& lo) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const unsigned h = cvt_pk_bf16(x[2 * i], x[2 * i + 1]);
    const float h0 = bf16_lo(h), h1 = bf16_hi(h);
    hi[i] = h;
    lo[i] = cvt_pk_bf16(x[2 * i] - h0, x[2 * i + 1] - h1);
  }
}

// x (4 floats) -> three packed bf16 quadruples: p0 = RNE(x), p1 = RNE(x - p0), p2 = RNE(x - p0 - p1)
__device__ __forceinline__ void split3_bf16x4(const f32x4 x, u32x2& p0, u32x2& p1, u32x2& p2) {
  p0.x = cvt_pk_bf16(x[0], x[1]);
  p0.y = cvt_pk_bf16(x[2], x[3]);
  const float r0 = x[0] - bf16_lo(p0.x), r1 = x[1] - bf16_hi(p0.x), r2 = x[2] - bf16_lo(p0.y), r3 = x[3] - bf16_hi(p0.y);
  p1.x = cvt_pk_bf16(r0, r1);
  p1.y = cvt_pk_bf16(r2, r3);
  p2.x = cvt_pk_bf16(r0 - bf16_lo(p1.x), r1 - bf16_hi(p1.x));
  p2.y = cvt_pk_bf16(r2 - bf16_lo(p1.y), r3 - bf16_hi(p1.y));
}

// the three products of one k step: acc += a_lo * b_hi + a_hi * b_lo + a_hi * b_hi
__device__ __forceinline__ f32x16 mfma_bf16x3(const bf16x8 a_hi, const bf16x8 a_lo, const bf16x8 b_hi, const bf16x8 b_lo,
                                              f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
}

}  // namespace
