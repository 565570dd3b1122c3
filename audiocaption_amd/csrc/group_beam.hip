// Group (diverse) beam search, base.py:363-471 diverse_beam_search: the per-step selection of ONE group.  A search of G
// groups of bdash beams per clip staggers the groups in time; group g at its local position lt scores its rows as a beam
// search does and subtracts, per word, lambda times the number of rows of the groups 0 .. g-1 of the same clip that hold this
// word at position lt (add_diversity, base.py:365-379) - read from those groups' CURRENT token planes, i.e. the history of
// their surviving beams.
//
//   ac_group_beam_select   per row lp = log_softmax(log_softmax(z) / temp), lp -= count * lambda, + cum; the row's best bdash
//                          candidates; then the per-clip merge of the single-model search (ac_beam.h): top_val / top_idx as
//                          ac_trm_beam_update(_all) reads them
//
// The score arithmetic restates beam_row_topk_kernel (csrc/decoder.hip, "The two kernels above as ONE pass per row") in the
// same order: one 256-thread workgroup per row, the row in registers, `bdash` rounds of a workgroup arg-max, the lowest
// index wins ties.  The penalty sits between the second log-softmax and "+ cum"; its product and its subtraction are each
// rounded once (group_penalise below), so that count == 0 or lambda == 0 leaves the bits of the un-penalised score.
#include "ac_beam.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

constexpr int GB_MAX_PREV = AC_GROUP_BEAM_MAX_GROUPS - 1;   // earlier groups of a clip
constexpr int GB_MAX_BDASH = 8;
constexpr int GB_MAX_WORDS = GB_MAX_PREV * GB_MAX_BDASH;    // 56 earlier words of a clip at one position

struct GroupPrev {
  const int* plane[GB_MAX_PREV];   // token planes [B * bdash][tok_ld] of the groups 0 .. n - 1
  int n;
};

__device__ __forceinline__ void gb_argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// lp - (float)count * lambda as one product and one subtraction in f32 (base.py:377: change * diversity_lambda, then the
// subtraction): never a fused multiply-add, whose single rounding gives another float
__device__ __forceinline__ float group_penalise(float lp, int count, float lambda) {
#pragma clang fp contract(off)
  const float pen = (float)count * lambda;
  return lp - pen;
}

template <int NV>
__global__ __launch_bounds__(256) void group_beam_row_kernel(const float* logit, long ldl, const float* cum, float temp,
                                                             float lambda, GroupPrev prev, long tok_ld, int col, int bdash,
                                                             int V, float* cand_val, int* cand_idx) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int s_win;
  __shared__ int s_prev[GB_MAX_WORDS];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int clip = r / bdash;
  const int nprev = prev.n * bdash;            // <= 56
  if (tid < nprev) {
    const int g = tid / bdash, j = tid % bdash;
    const int* plane = prev.plane[0];
#pragma unroll
    for (int q = 1; q < GB_MAX_PREV; ++q)      // unrolled predicate: a runtime index into the argument array goes to scratch
      if (q == g) plane = prev.plane[q];
    s_prev[tid] = plane[(size_t)(clip * bdash + j) * tok_ld + col];
  }
  const float* row = logit + (size_t)r * ldl;
  float x[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) x[k] = tid + 256 * k < V ? row[tid + 256 * k] : -INFINITY;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NV; ++k) m = fmaxf(m, x[k]);
  m = block_max256(m, sh);                     // its barriers also publish s_prev
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (tid + 256 * k < V) s += expf(x[k] - m);
  s = block_sum256(s, sh);
  const float lse1 = m + logf(s);
  const float inv_t = 1.0f / temp;
  const float m2 = (m - lse1) * inv_t;
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (tid + 256 * k < V) s2 += expf((x[k] - lse1) * inv_t - m2);
  s2 = block_sum256(s2, sh);
  const float lse2 = m2 + logf(s2);
  // count[w] of this thread's words: every earlier word is looked at once, its owner found by the unrolled predicate
  int cnt[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) cnt[k] = 0;
  for (int i = 0; i < nprev; ++i) {
    const int w = s_prev[i];
    const bool mine = w >= 0 && (w & 255) == tid;
    const int wk = w >> 8;
#pragma unroll
    for (int k = 0; k < NV; ++k) cnt[k] += (mine && wk == k) ? 1 : 0;
  }
  const float cr = cum[r];
#pragma unroll
  for (int k = 0; k < NV; ++k)
    x[k] = tid + 256 * k < V ? cr + group_penalise((x[k] - lse1) * inv_t - lse2, cnt[k], lambda) : -INFINITY;
  unsigned taken = 0u;
  const int flat0 = (r % bdash) * V;           // index of the row's first entry in the clip's flattened scores
  for (int j = 0; j < bdash; ++j) {
    float v = -INFINITY;
    int idx = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (!((taken >> k) & 1u) && tid + 256 * k < V) gb_argmax_merge(v, idx, x[k], tid + 256 * k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      gb_argmax_merge(v, idx, ov, oi);
    }
    __syncthreads();
    if (lane == 0) { sv[wave] = v; si[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
      v = sv[0]; idx = si[0];
      for (int w = 1; w < 4; ++w) gb_argmax_merge(v, idx, sv[w], si[w]);
      if (idx == 0x7fffffff) idx = j;          // a row without a comparable score left (NaN logits): still a word of the row
      s_win = idx;
      cand_val[(size_t)r * bdash + j] = v;
      cand_idx[(size_t)r * bdash + j] = flat0 + idx;
    }
    __syncthreads();
    const int win = s_win;
    if ((win & 255) == tid) taken |= 1u << (win >> 8);
  }
}

}  // namespace

extern "C" int ac_group_beam_select(const float* logit, long ldl, int B, int bdash, int V, int lt, float temp,
                                    float diversity_lambda, const float* cum, const int* const* prev_tok, int n_prev,
                                    long tok_ld, float* top_val, int* top_idx, float* scratch, void* stream) {
  if (!logit || !cum || !top_val || !top_idx || !scratch) return AC_ERR_ARG;
  if (B <= 0 || bdash < 1 || bdash > GB_MAX_BDASH || n_prev < 0 || n_prev > GB_MAX_PREV) return AC_ERR_ARG;
  // every row offers bdash words, and the row indices of the planes are ints
  if (V < 1 || V > 8192 || bdash > V || ldl < V || lt < 0 || (long)B * bdash > 0x7fffffffL / 8) return AC_ERR_ARG;
  if (!isfinite(temp) || !(temp > 0.f) || !isfinite(diversity_lambda) || !(diversity_lambda >= 0.f)) return AC_ERR_ARG;
  GroupPrev prev = {};
  prev.n = n_prev;
  if (n_prev > 0) {
    if (!prev_tok || tok_ld < (long)lt + 2) return AC_ERR_ARG;   // column lt + 1 is read
    for (int g = 0; g < n_prev; ++g) {
      if (!prev_tok[g]) return AC_ERR_ARG;
      prev.plane[g] = prev_tok[g];
    }
  }
  const int R = B * bdash;
  float* cand_val = scratch;                           // scratch: 2 * B * bdash * bdash words
  int* cand_idx = (int*)(scratch + (size_t)R * bdash);
  const dim3 grid(R), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (V <= 256 * 20)
    hipLaunchKernelGGL(group_beam_row_kernel<20>, grid, block, 0, s, logit, ldl, cum, temp, diversity_lambda, prev, tok_ld,
                       lt + 1, bdash, V, cand_val, cand_idx);
  else
    hipLaunchKernelGGL(group_beam_row_kernel<32>, grid, block, 0, s, logit, ldl, cum, temp, diversity_lambda, prev, tok_ld,
                       lt + 1, bdash, V, cand_val, cand_idx);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  return ac_beam_merge_launch(cand_val, cand_idx, B, bdash, lt == 0 ? 1 : bdash, top_val, top_idx, s);
}
