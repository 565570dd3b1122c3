// Ensemble decoding: the word of a step is chosen for several captioners at once from the mean of their log-softmaxes
// (ensemble.py:94-151 stepwise_forward, :154-276 beam_search).  Every member's decoder step has written its logits [R][V]
// into a plane of its own (ac_trm_step_logits); the kernels here read up to AC_ENS_MAX planes, one 256-thread workgroup per
// row, and keep m = mean_n log_softmax(logit_n) in registers (ac_ens.h) - no member's log-softmax and no m goes to memory.
//
//   ac_ens_greedy_pick       argmax m (lowest index wins ties), stored value m[word], greedy_pick_kernel's bookkeeping on
//                            the buffers the members share (seq, tokens, key mask, unfinished flags, unfinished counts)
//   ac_ens_sample_pick       the sampler of csrc/sample.hip over m with the rules of ensemble.py:412-449
//   ac_ens_beam_step_select  log_softmax(m / temp) + cum per row, the row's best `beam` candidates, then the per-clip merge
//                            of the single-model search (ac_beam.h): top_val / top_idx as ac_trm_beam_update(_all) reads them
#include "ac_beam.h"
#include "ac_ens.h"
#include "ac_sample.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

constexpr int ENS_MAXV = SAMPLE_MAXV;   // a row is held in registers: <= 64 values per thread

__device__ __forceinline__ void ens_argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// workgroup arg-max (lowest index wins ties), the result in every thread.  sv / si: 4 words of LDS each.
__device__ __forceinline__ void ens_block_argmax(float& v, int& idx, float* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    ens_argmax_merge(v, idx, ov, oi);
  }
  __syncthreads();   // sv / si may still be read by a previous call
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = idx; }
  __syncthreads();
  v = sv[0]; idx = si[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) ens_argmax_merge(v, idx, sv[k], si[k]);
}

struct EnsPickParams {
  EnsPlanes ens;
  int V, t, max_len, end_idx, pad_idx;
  int64_t* seq; float* logprob;      // [rows][max_len]
  int* tok; unsigned char* mask;     // [rows][max_len + 1]
  int* unfinished;                   // [rows]
  int* cnt;                          // [max_len]
};

template <int NPT>
__global__ __launch_bounds__(256) void ens_greedy_pick_kernel(EnsPickParams p) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (p.t > 0 && p.cnt[p.t - 1] == 0) return;   // every row had finished after step t - 1: the search is over
  float x[NPT];
  ens_mean<NPT, true>(p.ens, r, p.V, x, sh);
  float v = -INFINITY;
  int idx = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NPT; ++i) ens_argmax_merge(v, idx, x[i], ens_col<NPT, true>(tid, i));
  ens_block_argmax(v, idx, sv, si);
  if (tid == 0) {
    // greedy_pick_kernel's bookkeeping; a row that finished earlier emits end_idx and keeps the initial 0 as its value
    const int prev = p.t == 0 ? 1 : p.unfinished[r];
    const int unf = prev && (idx != p.end_idx);
    const int w = unf ? idx : p.end_idx;
    p.unfinished[r] = unf;
    p.seq[(size_t)r * p.max_len + p.t] = w;
    if (prev) p.logprob[(size_t)r * p.max_len + p.t] = v;   // m[word] (ensemble.py:415), not a log-softmax value
    p.tok[(size_t)r * (p.max_len + 1) + p.t + 1] = w;
    p.mask[(size_t)r * (p.max_len + 1) + p.t + 1] = (w == p.pad_idx) ? 1 : 0;
    if (unf) atomicAdd(&p.cnt[p.t], 1);
  }
}

// Row r: scores log_softmax(m / temp) + cum[r] in registers, then the row's best `beam` of them by `beam` rounds of a
// workgroup arg-max (the clip's best `beam` are among the per-row best `beam`): cand_val / cand_idx [r][beam], the index
// flattened over the clip's rows ((r % beam) * V + word) as beam_row_topk_kernel publishes it.
template <int NPT>
__global__ __launch_bounds__(256) void ens_beam_row_kernel(EnsPlanes ens, const float* cum, float temp, int beam, int V,
                                                           float* cand_val, int* cand_idx) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  float x[NPT];
  ens_mean<NPT, true>(ens, r, V, x, sh);
  const float inv_t = 1.0f / temp;
  float m2 = -INFINITY;
#pragma unroll
  for (int i = 0; i < NPT; ++i) m2 = fmaxf(m2, x[i] * inv_t);
  m2 = block_max256(m2, sh);
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NPT; ++i) s2 += expf(x[i] * inv_t - m2);   // exp(-inf) = 0 beyond V
  const float lse2 = m2 + logf(block_sum256(s2, sh));
  const float cr = cum[r];
#pragma unroll
  for (int i = 0; i < NPT; ++i) x[i] = ens_col<NPT, true>(tid, i) < V ? cr + (x[i] * inv_t - lse2) : -INFINITY;
  unsigned long long taken = 0ull;
  const int flat0 = (r % beam) * V;
  for (int j = 0; j < beam; ++j) {
    float v = -INFINITY;
    int idx = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < NPT; ++i)
      if (!((taken >> i) & 1ull) && ens_col<NPT, true>(tid, i) < V) ens_argmax_merge(v, idx, x[i], ens_col<NPT, true>(tid, i));
    ens_block_argmax(v, idx, sv, si);
    if (tid == 0) {
      cand_val[(size_t)r * beam + j] = v;
      cand_idx[(size_t)r * beam + j] = flat0 + idx;
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i)
      if (ens_col<NPT, true>(tid, i) == idx) taken |= 1ull << i;
  }
}

}  // namespace

extern "C" int ac_ens_greedy_pick(const float* const* logits, int n_models, long ld, int rows, int V, int t, int max_len,
                                  int end_idx, int pad_idx, int64_t* seq, float* logprob, int* tokens,
                                  unsigned char* key_mask, int* unfinished, int* unfinished_cnt, void* stream) {
  EnsPickParams p;
  if (V <= 0 || V > ENS_MAXV || ens_planes(logits, n_models, ld, V, &p.ens) != AC_OK) return AC_ERR_ARG;
  if (rows <= 0 || max_len <= 0 || t < 0 || t >= max_len || !seq || !logprob || !tokens || !key_mask || !unfinished ||
      !unfinished_cnt)
    return AC_ERR_ARG;
  p.V = V; p.t = t; p.max_len = max_len; p.end_idx = end_idx; p.pad_idx = pad_idx;
  p.seq = seq; p.logprob = logprob; p.tok = tokens; p.mask = key_mask; p.unfinished = unfinished; p.cnt = unfinished_cnt;
  const dim3 grid(rows), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (V <= 256 * 20) hipLaunchKernelGGL(ens_greedy_pick_kernel<20>, grid, block, 0, s, p);
  else if (V <= 256 * 32) hipLaunchKernelGGL(ens_greedy_pick_kernel<32>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(ens_greedy_pick_kernel<64>, grid, block, 0, s, p);
  return ac_check_launch();
}

extern "C" int ac_ens_sample_pick(const float* const* logits, int n_models, long ld, int rows, int V, int method, int k,
                                  float top_p, float temp, const uint64_t* seed_dev, int t, int max_len, int end_idx,
                                  int pad_idx, int64_t* seq, float* logprob, int* tokens, unsigned char* key_mask,
                                  int* unfinished, int* unfinished_cnt, int* word_out, void* stream) {
  SampleParams p = {};
  if (V <= 0 || V > ENS_MAXV || ens_planes(logits, n_models, ld, V, &p.ens) != AC_OK) return AC_ERR_ARG;
  if (!(temp > 0.f) || !isfinite(temp) || t < 0 || !logprob) return AC_ERR_ARG;   // ensemble.py divides by temp under every rule
  p.rows = rows; p.V = V; p.method = method; p.k = k; p.top_p = top_p; p.temp = temp; p.seed = seed_dev; p.t = t;
  p.logprob = logprob;
  if (seq) {   // step t of a search: row r's value at logprob[r][t]
    p.logprob = logprob + t; p.ld_lp = max_len;
    p.seq = seq; p.max_len = max_len; p.end_idx = end_idx; p.pad_idx = pad_idx;
    p.tok = tokens; p.mask = key_mask; p.unfinished = unfinished; p.cnt = unfinished_cnt;
  } else {     // the pick alone, as ac_sample_rows: word_out[r], logprob[r]
    p.word = word_out; p.ld_lp = 1;
  }
  return ac_sample_launch(p, (hipStream_t)stream);
}

extern "C" int ac_ens_beam_step_select(const float* const* logits, int n_models, long ld, int B, int beam, int V, int t,
                                       float temp, const float* cum_logprob, float* top_val, int* top_idx,
                                       float* scratch, void* stream) {
  EnsPlanes e;
  if (V <= 0 || V > ENS_MAXV || ens_planes(logits, n_models, ld, V, &e) != AC_OK) return AC_ERR_ARG;
  // beam * beam row candidates per clip are merged by one wave
  if (B <= 0 || beam <= 0 || beam > 8 || beam > V || t < 0 || !(temp > 0.f) || !isfinite(temp) || !cum_logprob ||
      !top_val || !top_idx || !scratch)
    return AC_ERR_ARG;
  const int R = B * beam;
  float* cand_val = scratch;                          // scratch: 2 * B * beam * beam words
  int* cand_idx = (int*)(scratch + (size_t)R * beam);
  const dim3 grid(R), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (V <= 256 * 20) hipLaunchKernelGGL(ens_beam_row_kernel<20>, grid, block, 0, s, e, cum_logprob, temp, beam, V, cand_val, cand_idx);
  else if (V <= 256 * 32) hipLaunchKernelGGL(ens_beam_row_kernel<32>, grid, block, 0, s, e, cum_logprob, temp, beam, V, cand_val, cand_idx);
  else hipLaunchKernelGGL(ens_beam_row_kernel<64>, grid, block, 0, s, e, cum_logprob, temp, beam, V, cand_val, cand_idx);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  return ac_beam_merge_launch(cand_val, cand_idx, B, beam, t == 0 ? 1 : beam, top_val, top_idx, s);
}
