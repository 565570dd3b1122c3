// The condition term of the specificity loss (reference captioning/losses/loss.py:195-219 SpecificityLossWrapper):
//   s[n][t] = sum_v softmax(logit[n][t])_v ws_v                   the expected word specificity of a position
//   c[n]    = scale[n] sum_{t < tgt_len[n] - 1} s[n][t]           scale 1 ("sum") or 1 / (tgt_len[n] - 1) (mean_with_lens)
//   loss    = mean_n (c[n] - cond[n])^2                           torch.nn.MSELoss
//   dlogit[n][t][v] = g (2 / N) (c[n] - cond[n]) m[n][t] scale[n] p_v (ws_v - s[n][t])
// Forward: spec_row_kernel, one workgroup per (n, t) row, one pass for the maximum and one for the two sums (wave
// reductions as in the label-smoothing kernel of csrc/train.hip); it keeps s and the row's log-sum-exp.  spec_clip_kernel,
// one workgroup, sums each clip's at most T values in order and reduces the squared errors: no atomics.  Backward:
// spec_bwd_kernel, one workgroup per row, from the kept s / lse / c - cond; a masked row is written as exact zeros.
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

__device__ __forceinline__ bool row_valid(const int* tgt_len, int n, int t) { return t < tgt_len[n] - 1; }

__global__ __launch_bounds__(256) void spec_row_kernel(const float* logit, const float* ws, const int* tgt_len, int T, int V,
                                                       float* row_s, float* row_lse) {
  __shared__ float red[4];
  const int row = blockIdx.x, n = row / T, t = row % T;
  if (!row_valid(tgt_len, n, t)) {
    if (threadIdx.x == 0) row_s[row] = row_lse[row] = 0.f;
    return;
  }
  const float* z = logit + (long)row * V;
  float m = -INFINITY;
  for (int v = threadIdx.x; v < V; v += 256) m = fmaxf(m, z[v]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float se = 0.f, sw = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float e = expf(z[v] - m);
    se += e;
    sw = fmaf(e, ws[v], sw);
  }
  se = block_sum256(se, red);
  sw = block_sum256(sw, red);
  if (threadIdx.x == 0) {
    row_s[row] = sw / se;
    row_lse[row] = m + logf(se);
  }
}

__device__ __forceinline__ float clip_scale(const int* tgt_len, int n, int mean_reduce) {
  return mean_reduce ? 1.0f / (float)(tgt_len[n] - 1) : 1.0f;
}

__global__ __launch_bounds__(256) void spec_clip_kernel(const float* row_s, const int* tgt_len, const float* cond, int N,
                                                        int T, int mean_reduce, float* diff, float* loss) {
  __shared__ float red[4];
  float sq = 0.f;
  for (int n = threadIdx.x; n < N; n += 256) {
    float c = 0.f;
    for (int t = 0; t < T; ++t) c += row_s[(long)n * T + t];   // masked rows hold 0
    const float e = c * clip_scale(tgt_len, n, mean_reduce) - cond[n];
    diff[n] = e;
    sq = fmaf(e, e, sq);
  }
  sq = block_sum256(sq, red);
  if (threadIdx.x == 0) loss[0] = sq / (float)N;
}

__global__ __launch_bounds__(256) void spec_bwd_kernel(const float* logit, const float* ws, const int* tgt_len,
                                                       const float* row_s, const float* row_lse, const float* diff,
                                                       const float* g_dev, int N, int T, int V, int mean_reduce,
                                                       float* dlogit) {
  const int row = blockIdx.x, n = row / T, t = row % T;
  float* dz = dlogit + (long)row * V;
  if (!row_valid(tgt_len, n, t)) {
    for (int v = threadIdx.x; v < V; v += 256) dz[v] = 0.f;
    return;
  }
  const float* z = logit + (long)row * V;
  const float s = row_s[row], lse = row_lse[row];
  const float k = g_dev[0] * (2.0f / (float)N) * diff[n] * clip_scale(tgt_len, n, mean_reduce);
  for (int v = threadIdx.x; v < V; v += 256) dz[v] = k * expf(z[v] - lse) * (ws[v] - s);
}

bool spec_args_ok(const void* logit, const void* ws, const int* tgt_len, int N, int T, int V) {
  return logit && ws && tgt_len && N > 0 && T > 0 && V > 0 && (long)N * T <= 0x7fffffffL;
}

}  // namespace

extern "C" {

int ac_specificity_loss(const float* logit, const float* word_spec, const int* tgt_len, const float* cond, int N, int T,
                        int V, int mean_reduce, float* row_s, float* row_lse, float* diff, float* loss, void* stream) {
  if (!spec_args_ok(logit, word_spec, tgt_len, N, T, V) || !cond || !row_s || !row_lse || !diff || !loss) return AC_ERR_ARG;
  hipLaunchKernelGGL(spec_row_kernel, dim3(N * T), dim3(256), 0, (hipStream_t)stream, logit, word_spec, tgt_len, T, V, row_s,
                     row_lse);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(spec_clip_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_s, tgt_len, cond, N, T, mean_reduce,
                     diff, loss);
  return ac_check_launch();
}

int ac_specificity_loss_bwd(const float* logit, const float* word_spec, const int* tgt_len, const float* row_s,
                            const float* row_lse, const float* diff, const float* g_dev, int N, int T, int V,
                            int mean_reduce, float* dlogit, void* stream) {
  if (!spec_args_ok(logit, word_spec, tgt_len, N, T, V) || !row_s || !row_lse || !diff || !g_dev || !dlogit)
    return AC_ERR_ARG;
  hipLaunchKernelGGL(spec_bwd_kernel, dim3(N * T), dim3(256), 0, (hipStream_t)stream, logit, word_spec, tgt_len, row_s,
                     row_lse, diff, g_dev, N, T, V, mean_reduce, dlogit);
  return ac_check_launch();
}

}  // extern "C"
