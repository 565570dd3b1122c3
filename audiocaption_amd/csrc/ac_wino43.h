// The Winograd pieces shared by the F(4,3) split-bf16 conv kernels (csrc/conv3x3_wino43.hip, csrc/conv3x3_block1_w4.hip):
// the input transform of a row quad, the output transform + BN + ReLU of one accumulator register - and the same two
// transforms of F(6,3) for the row-sextet tile form of csrc/conv3x3_wino43.hip.  The operand split they feed is
// csrc/ac_split_bf16.h, the dead-block test and FastDiv csrc/ac_conv_tile.h.
#pragma once
#include "ac_conv_tile.h"
#include "ac_split_bf16.h"

namespace {

__device__ __forceinline__ f32x4 vfma(float a, const f32x4 x, const f32x4 y) {   // a * x + y, one rounding per element
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = __builtin_fmaf(a, x[j], y[j]);
  return r;
}

// F(4,3) input transform: position pos (0..5) of the six rows d0..d5 of a quad (d[r] only touched where pos needs it)
__device__ __forceinline__ f32x4 w4_transform(int pos, const f32x4& d0, const f32x4& d1, const f32x4& d2, const f32x4& d3,
                                              const f32x4& d4, const f32x4& d5) {
  if (pos == 0) return vfma(4.f, d0, vfma(-5.f, d2, d4));
  if (pos == 5) return vfma(4.f, d1, vfma(-5.f, d3, d5));
  if (pos == 1 || pos == 2) {
    const f32x4 t1 = vfma(-4.f, d2, d4), t2 = vfma(-4.f, d1, d3);
    return pos == 1 ? t1 + t2 : t1 - t2;
  }
  const f32x4 t3 = d4 - d2, u = d3 - d1;
  return pos == 3 ? vfma(2.f, u, t3) : vfma(-2.f, u, t3);
}

// F(4,3) output transform of the six position sums of one (pixel, channel) + BatchNorm (scale, shift) + ReLU: four rows
__device__ __forceinline__ void w4_outputs(float m0, float m1, float m2, float m3, float m4, float m5, float sc, float sh,
                                           float (&y)[4]) {
  const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
  y[0] = fmaxf(fmaf((m0 + s12) + s34, sc, sh), 0.f);
  y[1] = fmaxf(fmaf(__builtin_fmaf(2.f, d34, d12), sc, sh), 0.f);
  y[2] = fmaxf(fmaf(__builtin_fmaf(4.f, s34, s12), sc, sh), 0.f);
  y[3] = fmaxf(fmaf(__builtin_fmaf(8.f, d34, d12) + m5, sc, sh), 0.f);
}

// F(6,3) (points 0, +-1, +-2, +-1/2, inf) input transform: position pos (0..7) of the eight rows d0..d7 of a row SEXTET.
// Every constant is a dyadic rational, so the products below are exact and each fma rounds once; positions (1, 2), (3, 4)
// and (5, 6) share their even / odd halves as the F(4,3) pairs do.
__device__ __forceinline__ f32x4 w6_transform(int pos, const f32x4& d0, const f32x4& d1, const f32x4& d2, const f32x4& d3,
                                              const f32x4& d4, const f32x4& d5, const f32x4& d6, const f32x4& d7) {
  if (pos == 0) return vfma(5.25f, d4 - d2, d0 - d6);
  if (pos == 7) return vfma(5.25f, d3 - d5, d7 - d1);
  if (pos == 1 || pos == 2) {
    const f32x4 te = vfma(-4.25f, d4, d2 + d6), to = vfma(-4.25f, d3, d1 + d5);
    return pos == 1 ? te + to : te - to;
  }
  if (pos == 3 || pos == 4) {
    const f32x4 te = vfma(0.25f, d2, vfma(-1.25f, d4, d6)), to = vfma(2.f, d5, vfma(-2.5f, d3, 0.5f * d1));
    return pos == 3 ? te + to : te - to;
  }
  const f32x4 te = vfma(4.f, d2, vfma(-5.f, d4, d6)), to = vfma(2.f, d1, vfma(-2.5f, d3, 0.5f * d5));
  return pos == 5 ? te + to : te - to;
}

// F(6,3) output transform of the eight position sums of one (pixel, channel) + BatchNorm (scale, shift) + ReLU: six rows
__device__ __forceinline__ void w6_outputs(float m0, float m1, float m2, float m3, float m4, float m5, float m6, float m7,
                                           float sc, float sh, float (&y)[6]) {
  const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4, s56 = m5 + m6, d56 = m5 - m6;
  y[0] = fmaxf(fmaf(((m0 + s12) + s34) + s56, sc, sh), 0.f);
  y[1] = fmaxf(fmaf(__builtin_fmaf(0.5f, d56, __builtin_fmaf(2.f, d34, d12)), sc, sh), 0.f);
  y[2] = fmaxf(fmaf(__builtin_fmaf(0.25f, s56, __builtin_fmaf(4.f, s34, s12)), sc, sh), 0.f);
  y[3] = fmaxf(fmaf(__builtin_fmaf(0.125f, d56, __builtin_fmaf(8.f, d34, d12)), sc, sh), 0.f);
  y[4] = fmaxf(fmaf(__builtin_fmaf(0.0625f, s56, __builtin_fmaf(16.f, s34, s12)), sc, sh), 0.f);
  y[5] = fmaxf(fmaf(__builtin_fmaf(0.03125f, d56, __builtin_fmaf(32.f, d34, d12)) + m7, sc, sh), 0.f);
}

}  // namespace
