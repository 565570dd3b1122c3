// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the audio-captioning path.
// Wave size is 64 everywhere; nothing here compiles for another target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AC_WAVE 64

// Error codes of the C ABI (include/audiocaption_hip.h).
#define AC_OK 0
#define AC_ERR_ARG (-1)
#define AC_ERR_LAUNCH (-2)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// v_mfma_f32_32x32x2_f32: D(32x32) += A(32x2) * B(2x32), exact f32 (k-ordered fmaf chain).
// Lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; the result register r
// of lane l is D[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][l & 31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// 64-lane reductions on the DPP cross-lane network (quad permutes, row mirrors) plus four scalar lane
// reads: ~10x cheaper than a ds_bpermute butterfly, which goes through the LDS crossbar at every step.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
constexpr int DPP_QUAD_XOR1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;   // quad_perm [2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;
constexpr int DPP_ROW_MIRROR = 0x140;

// sum / max over each 16-lane row, result in every lane of the row
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<DPP_QUAD_XOR1>(v);
  v += dpp_mov<DPP_QUAD_XOR2>(v);
  v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_mov<DPP_ROW_MIRROR>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<DPP_QUAD_XOR1>(v));
  v = fmaxf(v, dpp_mov<DPP_QUAD_XOR2>(v));
  v = fmaxf(v, dpp_mov<DPP_ROW_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_mov<DPP_ROW_MIRROR>(v));
  return v;
}
__device__ __forceinline__ float lane_read(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  return (lane_read(v, 0) + lane_read(v, 16)) + (lane_read(v, 32) + lane_read(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = row16_max(v);
  return fmaxf(fmaxf(lane_read(v, 0), lane_read(v, 16)), fmaxf(lane_read(v, 32), lane_read(v, 48)));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Reductions over a workgroup of exactly 256 threads (four waves).  Every thread calls, the result lands in every
// thread; sh is 4 words of LDS (per value), and the leading barrier is there because sh may still be read by a previous
// call.  The order of the additions is fixed: lanes by wave_sum, then (wave 0 + wave 1) + (wave 2 + wave 3).
__device__ __forceinline__ float block_max256(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// K sums at once, each in place, behind one pair of barriers
template <typename T, int K>
__device__ __forceinline__ void block_sums256(T (&v)[K], T (*sh)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
}

// swish / sigmoid on the transcendental unit: v_exp_f32 and v_rcp_f32 (1 ulp each), 6 instructions instead of the ~25 of
// expf + an IEEE division.  EfficientNet applies one swish per activation, which made the accurate form the largest VALU
// item of its streaming kernels.  exp2 overflows to +inf for v < -88 (rcp(inf) = 0: the result is -0, the limit).
__device__ __forceinline__ float ac_sigmoid_fast(float v) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896f * v));
}
__device__ __forceinline__ float ac_swish_fast(float v) { return v * ac_sigmoid_fast(v); }
// The accurate forms (expf + IEEE division) for the kernels documented as exact f32 (gemm_general / gemm_nt / gemm_kk).
__device__ __forceinline__ float ac_sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float ac_swish_exact(float v) { return v * ac_sigmoid_exact(v); }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter
// (s_waitcnt vmcnt(0)), which would force every global prefetch in flight to land at each barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: remembered per (launch site, device), so
// that a process which touches a second GPU sets it there as well (a plain function-local flag would skip it and the
// launch would fail with more than 64 KiB of dynamic LDS).  One word per site: bit d = device d has the attribute.
struct AcLdsAttr { unsigned long long done = 0; };
static inline int ac_allow_lds(const void* kernel, int bytes, AcLdsAttr* st) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return AC_ERR_LAUNCH;
  const bool tracked = dev >= 0 && dev < 64;
  if (tracked && ((__atomic_load_n(&st->done, __ATOMIC_ACQUIRE) >> dev) & 1ull)) return AC_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return AC_ERR_LAUNCH;
  if (tracked) __atomic_fetch_or(&st->done, 1ull << dev, __ATOMIC_RELEASE);
  return AC_OK;
}

static inline int ac_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? AC_OK : AC_ERR_LAUNCH;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011): the counter-based generator
// of the on-device samplers.  Ten rounds of two 32x32 -> 64-bit multiplies; the key is bumped by the Weyl constants between
// rounds.  A draw depends on (key, counter) only: no state, so it is the same in any launch order, batch or graph replay.
// ctr[4] is replaced by the output block.  Known answers (Random123 kat_vectors) in tests/test_sampling_cpu.py.
__host__ __device__ inline void ac_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * ctr[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
    ctr[0] = n0;
    ctr[1] = (uint32_t)p1;
    ctr[2] = n2;
    ctr[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The sampler's uniform for (seed, step, row): counter (step, row, 0, 0), key (seed lo, seed hi), word 0 ->
// ((x0 >> 8) + 1) * 2^-24, a float in (0, 1] (24 random bits; exact in f32).
__host__ __device__ inline float ac_sample_uniform(uint64_t seed, uint32_t step, uint32_t row) {
  uint32_t c[4] = {step, row, 0u, 0u};
  ac_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)((c[0] >> 8) + 1u) * 5.9604644775390625e-8f;
}
