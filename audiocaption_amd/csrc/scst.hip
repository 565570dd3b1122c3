// Self-critical sequence training (rl_model.py:24-62) on the training engine's rollout: the word pick of one rollout
// pass and the policy-gradient loss with its gradient.
//
//   ac_scst_pick  pass t of the rollout: clip n draws a word from softmax(log_softmax(logit[n][t]) / temp) with the sampler
//                 of csrc/sample.hip (plain method, Philox counter (t, n)), or takes the caller's forced word; a clip that
//                 has drawn <end> keeps emitting <end> (base.py:161-166).
//   ac_scst_loss  mask[n][t] = (t == 0 or seq[n][t-1] != <end>), row_loss[n][t] = -(lp[n][t][w] / temp) * reward[n] * mask,
//                 loss = (1 / N) sum row_loss, dlogit = -(reward * mask / (N * temp)) * (onehot(w) - softmax(logit)).
//                 One 256-thread workgroup per (clip, step) row, fp32 wave reductions (like the cross entropy of
//                 csrc/train.hip).
//   ac_scst_group_reward  the reward of K rollouts per clip from their scores [K][N]: against the greedy caption's score,
//                 or against the mean score of the clip's other K - 1 rollouts (leave-one-out).  One thread per clip,
//                 sums in the order j = 0 .. K-1.
#include "ac_sample.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

// Bookkeeping of one rollout pass: the drawn (or forced) word of clip n -> seq[n][t] under the finished-row rule.  With
// forced words the stored log-probability is recomputed here for the forced word (the sampler stored the drawn word's).
__global__ __launch_bounds__(256) void scst_book_kernel(const float* logit, long ld, int V, float temp, int t, int end_idx,
                                                        const int* drawn, const int* forced, long forced_ld, int* done,
                                                        int* seq, long seq_ld, float* logprob, long lp_ld) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const int word = forced ? forced[n * forced_ld + t] : drawn[n];
  if (forced) {
    const float* z = logit + n * ld;
    float m = -INFINITY;
    for (int v = threadIdx.x; v < V; v += 256) m = fmaxf(m, z[v]);
    m = block_max256(m, red);
    float se = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) se += expf(z[v] - m);
    se = block_sum256(se, red);
    // (a forced word outside the vocabulary: NaN instead of a read beyond the row)
    if (threadIdx.x == 0) logprob[n * lp_ld + t] = word >= 0 && word < V ? ((z[word] - m) - logf(se)) / temp : NAN;
  }
  if (threadIdx.x == 0) {
    const int was_done = t == 0 ? 0 : done[n];
    const int w = was_done ? end_idx : word;
    seq[n * seq_ld + t] = w;
    done[n] = was_done || w == end_idx;
  }
}

__global__ __launch_bounds__(256) void scst_loss_kernel(const float* logit, const int* seq, long seq_ld, const float* reward,
                                                        float temp, int end_idx, int N, int T, int V, float* row_loss,
                                                        float* dlogit, const float* gscale_dev) {
  __shared__ float red[4];
  const int row = blockIdx.x, n = row / T, t = row % T;
  const bool live = t == 0 || seq[n * seq_ld + t - 1] != end_idx;
  if (!live) {
    if (threadIdx.x == 0) row_loss[row] = 0.f;
    if (dlogit)
      for (int v = threadIdx.x; v < V; v += 256) dlogit[(long)row * V + v] = 0.f;
    return;
  }
  const float* z = logit + (long)row * V;
  const int w = seq[n * seq_ld + t];
  float m = -INFINITY;
  for (int v = threadIdx.x; v < V; v += 256) m = fmaxf(m, z[v]);
  m = block_max256(m, red);
  float se = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) se += expf(z[v] - m);
  se = block_sum256(se, red);
  const float r = reward[n];
  // (a word outside the vocabulary: NaN instead of a read beyond the row)
  if (threadIdx.x == 0) row_loss[row] = w >= 0 && w < V ? -(((z[w] - m) - logf(se)) / temp) * r : NAN;
  if (dlogit) {
    float g = r / ((float)N * temp);
    if (gscale_dev) g *= gscale_dev[0];
    const float inv = 1.0f / se;
    for (int v = threadIdx.x; v < V; v += 256)
      dlogit[(long)row * V + v] = g * (expf(z[v] - m) * inv - (v == w ? 1.0f : 0.0f));
  }
}

// loss[0] = scale * sum(row_loss), a fixed summation order (one workgroup)
__global__ __launch_bounds__(256) void scst_sum_kernel(const float* x, long n, float scale, float* out) {
  __shared__ float red[4];
  float a = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) a += x[i];
  a = block_sum256(a, red);
  if (threadIdx.x == 0) out[0] = a * scale;
}

// reward[k][n] of clip n (one thread per clip): mode greedy s[k][n] - g[n]; mode mean s[k][n] - (sum_j s[j][n] - s[k][n]) /
// (K - 1), the sum taken once in the order j = 0 .. K-1
__global__ __launch_bounds__(256) void scst_group_reward_kernel(const float* scores, int K, int N, int mode,
                                                                const float* greedy, float* reward) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (mode == AC_SCST_BASELINE_GREEDY) {
    const float g = greedy[n];
    for (int k = 0; k < K; ++k) reward[(long)k * N + n] = scores[(long)k * N + n] - g;
    return;
  }
  float sum = 0.f;
  for (int j = 0; j < K; ++j) sum += scores[(long)j * N + n];
  const float others = (float)(K - 1);
  for (int k = 0; k < K; ++k) {
    const float s = scores[(long)k * N + n];
    reward[(long)k * N + n] = s - (sum - s) / others;
  }
}

}  // namespace

extern "C" int ac_scst_group_reward(const float* scores, int K, int N, int mode, const float* greedy_scores, float* reward,
                                    void* stream) {
  if (!scores || !reward || K < 1 || K > AC_SCST_MAX_ROLLOUTS || N < 1 ||
      (mode != AC_SCST_BASELINE_GREEDY && mode != AC_SCST_BASELINE_MEAN) || (mode == AC_SCST_BASELINE_GREEDY && !greedy_scores) ||
      (mode == AC_SCST_BASELINE_MEAN && K < 2))
    return AC_ERR_ARG;
  hipLaunchKernelGGL(scst_group_reward_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, K, N, mode,
                     greedy_scores, reward);
  return ac_check_launch();
}

extern "C" int ac_scst_pick(const float* logit, long ld, int N, int V, float temp, const uint64_t* seed_dev, int t,
                            int end_idx, const int* forced, long forced_ld, int* done, int* drawn, int* seq, long seq_ld,
                            float* logprob, long lp_ld, void* stream) {
  if (!logit || !seed_dev || !done || !drawn || !seq || !logprob || N <= 0 || ld < V || t < 0 || t >= seq_ld || t >= lp_ld ||
      (forced && t >= forced_ld))
    return AC_ERR_ARG;
  SampleParams p = {};
  p.logit = logit; p.ldl = ld; p.rows = N; p.V = V; p.method = AC_SAMPLE_PLAIN; p.temp = temp;
  p.seed = seed_dev; p.t = t; p.word = drawn; p.logprob = logprob + t; p.ld_lp = lp_ld;
  const int rc = ac_sample_launch(p, (hipStream_t)stream);   // (checks V <= 16384 and temp)
  if (rc != AC_OK) return rc;
  hipLaunchKernelGGL(scst_book_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, logit, ld, V, temp, t, end_idx, drawn,
                     forced, forced_ld, done, seq, seq_ld, logprob, lp_ld);
  return ac_check_launch();
}

extern "C" int ac_scst_loss(const float* logit, const int* seq, long seq_ld, const float* reward, float temp, int end_idx,
                            int N, int T, int V, float* row_loss, float* loss, float* dlogit, const float* gscale_dev,
                            void* stream) {
  if (!logit || !seq || !reward || !row_loss || !loss || N <= 0 || T <= 0 || V <= 0 || V > SAMPLE_MAXV || seq_ld < T ||
      !(temp > 0.f) || !isfinite(temp))
    return AC_ERR_ARG;
  hipLaunchKernelGGL(scst_loss_kernel, dim3(N * T), dim3(256), 0, (hipStream_t)stream, logit, seq, seq_ld, reward, temp,
                     end_idx, N, T, V, row_loss, dlogit, gscale_dev);
  hipLaunchKernelGGL(scst_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_loss, (long)N * T, 1.0f / (float)N,
                     loss);
  return ac_check_launch();
}
