// Repetition and word constraints of a search step: the row of raw logits z [V] a decoder step produced becomes the row z'
// the pick selects from.  With g = tokens[1 .. t], the t words the row has generated (the start token is not one of them):
//
//   1. repetition_penalty rho != 1: every word w of g gets z'[w] = z[w] / rho (z[w] > 0) or z[w] * rho - from z, so a word
//      that occurs five times is penalised once;
//   2. no_repeat_ngram n > 0, t >= n - 1: with p the last n - 1 words of g, every i with i + n - 1 < t and
//      g[i .. i + n - 2] == p bans g[i + n - 1] (overlapping occurrences count; n = 1 bans every word of g);
//   3. bad_words: always banned;
//   4. min_length: end_idx is banned while t < min_length.
//
// Banned: z'[w] = -inf, which the picks (greedy_pick_kernel, sample_kernel, the beam kernels) treat as an absent column -
// their log-softmax renormalises over what is left.
//
// One 256-thread workgroup per row, out of place: copy (16-byte accesses when both planes allow them), barrier, the prefix
// positions write the penalised values (read from the INPUT row: the same value whichever occurrence writes it), barrier,
// the bans.  A row moves 2 V floats; the launch is bound by its own latency.  No allocation, no synchronisation.
#include "ac_logit_rules.h"

#include <math.h>

namespace {

struct RulesParams {
  const float* in; long ld_in;
  float* out; long ld_out;
  int V;
  const int* tok; long ld_tok;   // row r at tok + r * ld_tok: column 0 the start token, columns 1 .. t the generated words
  int t;
  float rho;
  int ngram, min_length, end_idx, n_bad;
  const int* bad;
  const int* cnt; int seg_rows, max_len;   // the search's unfinished counts (null: every row runs)
  int vec;                       // both planes 16-byte aligned with strides that are multiples of 4
};

__global__ __launch_bounds__(256) void logit_rules_kernel(RulesParams p) {
  const int r = blockIdx.x, tid = threadIdx.x;
  // per workgroup, ahead of the barriers: the search of this row's segment has already stopped
  if (p.cnt && p.t > 0 && p.cnt[(size_t)(r / p.seg_rows) * p.max_len + p.t - 1] == 0) return;
  const float* in = p.in + (size_t)r * p.ld_in;
  float* out = p.out + (size_t)r * p.ld_out;
  const int* g = p.tok + (size_t)r * p.ld_tok + 1;
  const int V = p.V, t = p.t;
  if (p.vec) {
    const int n4 = V >> 2;
    for (int c = tid; c < n4; c += 256) ((f32x4*)out)[c] = ((const f32x4*)in)[c];
    for (int c = (n4 << 2) + tid; c < V; c += 256) out[c] = in[c];
  } else {
    for (int c = tid; c < V; c += 256) out[c] = in[c];
  }
  __syncthreads();
  if (p.rho != 1.0f) {
    for (int j = tid; j < t; j += 256) {
      const int w = g[j];
      if ((unsigned)w < (unsigned)V) {
        const float z = in[w];
        out[w] = z > 0.f ? z / p.rho : z * p.rho;
      }
    }
  }
  __syncthreads();
  const int n = p.ngram;
  if (n > 0 && t >= n - 1) {
    const int* tail = g + (t - (n - 1));   // the last n - 1 words
    for (int i = tid; i + n - 1 < t; i += 256) {
      bool same = true;
      for (int q = 0; q < n - 1; ++q) same = same && g[i + q] == tail[q];
      const int w = g[i + n - 1];
      if (same && (unsigned)w < (unsigned)V) out[w] = -INFINITY;
    }
  }
  for (int j = tid; j < p.n_bad; j += 256) {
    const int w = p.bad[j];
    if ((unsigned)w < (unsigned)V) out[w] = -INFINITY;
  }
  if (tid == 0 && t < p.min_length) out[p.end_idx] = -INFINITY;
}

}  // namespace

int ac_logit_rules_check(const ac_logit_rules* q, int V) {
  if (!q || V <= 0 || V > 16384) return AC_ERR_ARG;
  if (!isfinite(q->repetition_penalty) || !(q->repetition_penalty > 0.f)) return AC_ERR_ARG;
  if (q->no_repeat_ngram < 0 || q->min_length < 0 || q->n_bad < 0 || q->n_bad > 256) return AC_ERR_ARG;
  if (q->n_bad > 0 && !q->bad_words) return AC_ERR_ARG;
  if (q->end_idx < 0 || q->end_idx >= V) return AC_ERR_ARG;
  return AC_OK;
}

int ac_logit_rules_launch(const float* logit, long ld_in, float* out, long ld_out, int rows, int V, const int* tokens,
                          long ld_tok, int t, const ac_logit_rules* rules, const int* cnt, int seg_rows, int max_len,
                          hipStream_t s) {
  if (ac_logit_rules_check(rules, V) != AC_OK) return AC_ERR_ARG;
  if (!logit || !out || !tokens || rows <= 0 || ld_in < V || ld_out < V) return AC_ERR_ARG;
  if (t < 0 || (long)t >= ld_tok) return AC_ERR_ARG;   // columns 1 .. t of the token row are read
  if (cnt && (seg_rows <= 0 || max_len <= 0 || t >= max_len)) return AC_ERR_ARG;
  RulesParams p;
  p.in = logit; p.ld_in = ld_in; p.out = out; p.ld_out = ld_out; p.V = V; p.tok = tokens; p.ld_tok = ld_tok; p.t = t;
  p.rho = rules->repetition_penalty; p.ngram = rules->no_repeat_ngram; p.min_length = rules->min_length;
  p.end_idx = rules->end_idx; p.n_bad = rules->n_bad; p.bad = rules->bad_words;
  p.cnt = cnt; p.seg_rows = seg_rows; p.max_len = max_len;
  p.vec = !(((uintptr_t)logit | (uintptr_t)out) & 15) && ld_in % 4 == 0 && ld_out % 4 == 0;
  hipLaunchKernelGGL(logit_rules_kernel, dim3(rows), dim3(256), 0, s, p);
  return ac_check_launch();
}

extern "C" int ac_logit_rules_apply(const float* logit, long ld_in, float* out, long ld_out, int rows, int V,
                                    const int* tokens, long ld_tok, int t, const ac_logit_rules* rules, void* stream) {
  return ac_logit_rules_launch(logit, ld_in, out, ld_out, rows, V, tokens, ld_tok, t, rules, nullptr, 1, 0,
                               (hipStream_t)stream);
}
