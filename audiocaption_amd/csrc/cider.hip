// CIDEr-D (Vedantam et al., CVPR 2015, as pycocoevalcap's cider_scorer.py computes it: n-grams of 1..4 words, sigma 6,
// document frequencies from the scored batch's own references) on token ids, for the reward of self-critical sequence
// training: score(sampled) and score(greedy) per clip, and their difference, without a trip through the host.
//
// A distinct n-gram of the references is identified by the slot it holds in one table over the flat reference words;
// the table, the sentence rule, the counts at a first occurrence and the view of the packed arguments are those of
// ac_ngram.h.  This file owns the document frequencies, every tf * idf formula and the similarity.  Everything after the
// table is integer equality of slots:
//
//   cider_insert_kernel  one workgroup per reference sentence: slot of every n-gram occurrence (atomicCAS claims)
//   cider_df_kernel      one workgroup per key: df[slot] += 1 for the key's first occurrence of each slot (integer atomicAdd)
//   cider_ref_kernel     one workgroup per reference sentence: tf * idf of every occurrence and the norm per order
//   cider_hyp_kernel     one workgroup per (key, set): the sentence of the key's first row (start skipped, cut at the first
//                        end), its tf * idf vector, then the clipped similarity against each reference in turn
//   cider_scatter_kernel score of a row = score of its key; reward = set 0 - set 1
//
// Floating-point sums run over positions in a fixed order (a thread's strided positions, then the wave and workgroup
// tree of block_sum256), and the integer atomics commute, so a call is bitwise repeatable; which occurrence represents an
// n-gram in the table does depend on timing, and nothing downstream depends on it.
#include "ac_ngram.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;

struct CiderArgs : HypView, RefView {
  int n_words, order;
  float inv_2sigma2;
  // workspace
  int* rep;   // [mask + 1] representative occurrence of the slot's n-gram, -1 = empty
  int* df;    // [mask + 1]
  unsigned mask;
  int* bad;        // [0] != 0: an offset or a reference word was out of range
  int* occ;        // [4][W] slot of the n-gram that starts at each reference position (-1: none, or past its sentence)
  float* refw;     // [4][W] tf * idf of that n-gram in its sentence
  float* refnorm;  // [M][4]
  float* key_score;  // [sets][K]
  float* scores;     // [sets][N]
  float* reward;     // [N] or NULL
};

__global__ __launch_bounds__(kThreads) void cider_insert_kernel(CiderArgs a) {
  int b, e;
  if (!sentence_range(a, blockIdx.x, &b, &e)) {
    if (threadIdx.x == 0) a.bad[0] = 1;
    return;
  }
  for (int p = b + threadIdx.x; p < e; p += kThreads) {
    if (a.words[p] < 0 || a.words[p] >= a.n_words) a.bad[0] = 1;
    for (int n = 0; n < a.order; ++n) {
      int slot = -1;
      if (p + n < e) slot = gram_claim(a.rep, a.mask, a.words, a.words + p, n + 1, p * 4 + n);
      a.occ[(long)n * a.W + p] = slot;
    }
  }
}

__global__ __launch_bounds__(kThreads) void cider_df_kernel(CiderArgs a) {
  int s0, s1, b, e, tmp;
  if (!key_range(a, blockIdx.x, &s0, &s1) || s0 == s1 || !sentence_range(a, s0, &b, &tmp) ||
      !sentence_range(a, s1 - 1, &tmp, &e) || e < b) {
    if (threadIdx.x == 0) a.bad[0] = 1;
    return;
  }
  for (int n = 0; n < a.order; ++n) {
    const int* occ = a.occ + (long)n * a.W;
    for (int p = b + threadIdx.x; p < e; p += kThreads) {
      const int slot = occ[p];
      if (slot < 0) continue;
      bool first = true;
      for (int q = b; q < p; ++q)
        if (occ[q] == slot) {
          first = false;
          break;
        }
      if (first) atomicAdd(&a.df[slot], 1);
    }
  }
}

__global__ __launch_bounds__(kThreads) void cider_ref_kernel(CiderArgs a) {
  __shared__ int sl[AC_CIDER_MAX_REF_WORDS];
  __shared__ float red[4];
  const int s = blockIdx.x;
  int b, e;
  if (!sentence_range(a, s, &b, &e) || e - b > AC_CIDER_MAX_REF_WORDS) {
    if (threadIdx.x == 0) a.bad[0] = 1;
    return;
  }
  const int L = e - b;
  const float log_k = logf((float)a.K);
  for (int n = 0; n < a.order; ++n) {
    __syncthreads();
    for (int p = threadIdx.x; p < L; p += kThreads) sl[p] = a.occ[(long)n * a.W + b + p];
    __syncthreads();
    float sq = 0.f;
    for (int p = threadIdx.x; p < L; p += kThreads) {
      const int slot = sl[p];
      float w = 0.f;
      if (slot >= 0) {
        bool first;
        const int tf = slot_count(sl, L, p, &first);
        const int df = a.df[slot];
        w = (float)tf * (log_k - logf((float)(df > 1 ? df : 1)));
        if (first) sq += w * w;
      }
      a.refw[(long)n * a.W + b + p] = w;
    }
    sq = block_sum256(sq, red);
    if (threadIdx.x == 0) a.refnorm[s * 4 + n] = sqrtf(sq);
  }
}

__global__ __launch_bounds__(kThreads) void cider_hyp_kernel(CiderArgs a) {
  __shared__ int hw[AC_CIDER_MAX_HYP_WORDS];
  __shared__ int hslot[4][AC_CIDER_MAX_HYP_WORDS];
  __shared__ float hwt[4][AC_CIDER_MAX_HYP_WORDS];   // tf * idf at the first occurrence of an n-gram, 0 at its repeats
  __shared__ float red[4];
  __shared__ int sh_len;
  const int k = blockIdx.x, set = blockIdx.y;
  // (the row is staged in hslot[0] and hslot[1], which are written for good only later)
  const int L = load_key_sentence(a, a, k, set, hw, hslot[0], hslot[1], &sh_len);
  int s0, s1;
  if (L < 0 || !key_range(a, k, &s0, &s1)) {
    if (threadIdx.x == 0) a.key_score[set * a.K + k] = NAN;
    return;
  }
  const float log_k = logf((float)a.K);
  float norm_h[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < a.order; ++n) {
    float sq = 0.f;
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      bool first;
      const int tf = gram_count(hw, L, p, n + 1, &first);
      const int slot = gram_find(a.rep, a.mask, a.words, hw + p, n + 1);
      const int df = slot >= 0 ? a.df[slot] : 0;
      const float w = (float)tf * (log_k - logf((float)(df > 1 ? df : 1)));
      hslot[n][p] = slot;
      hwt[n][p] = first ? w : 0.f;
      if (first) sq += w * w;
    }
    norm_h[n] = sqrtf(block_sum256(sq, red));
  }
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int len_h = L > 0 ? L - 1 : 0;
  for (int s = s0; s < s1; ++s) {
    int b, e;
    const bool ok = sentence_range(a, s, &b, &e);
    const int len_r = ok && e > b ? e - b - 1 : 0;
    const float d = (float)(len_h - len_r);
    const float penalty = expf(-(d * d) * a.inv_2sigma2);
    for (int n = 0; n < a.order; ++n) {
      const int* occ = a.occ + (long)n * a.W;
      float c = 0.f;
      if (ok)
        for (int p = threadIdx.x; p + n < L; p += kThreads) {
          const float wh = hwt[n][p];
          const int slot = hslot[n][p];
          if (slot < 0 || !(wh > 0.f)) continue;
          for (int q = b; q + n < e; ++q)
            if (occ[q] == slot) {
              const float wr = a.refw[(long)n * a.W + q];
              c += fminf(wh, wr) * wr;
              break;
            }
        }
      float val = block_sum256(c, red);
      const float nr = ok ? a.refnorm[s * 4 + n] : NAN;
      // (the cosine of a clipped vector: at most 1 in exact arithmetic, so rounding may not carry it above)
      if (norm_h[n] != 0.f && nr != 0.f) val = fminf(val / (norm_h[n] * nr), 1.0f);
      acc[n] += val * penalty;
    }
  }
  if (threadIdx.x == 0) {
    const float sum = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    a.key_score[set * a.K + k] = 10.0f * (sum / (float)a.order) / (float)(s1 - s0);
  }
}

__global__ __launch_bounds__(kThreads) void cider_scatter_kernel(CiderArgs a) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= a.N) return;
  const int k = a.row_key[n];
  const bool ok = k >= 0 && k < a.K && a.bad[0] == 0;
  float s01[2] = {0.f, 0.f};
  for (int s = 0; s < a.sets; ++s) {
    const float v = ok ? a.key_score[s * a.K + k] : NAN;
    a.scores[(long)s * a.N + n] = v;
    if (s < 2) s01[s] = v;
  }
  if (a.reward) a.reward[n] = s01[0] - s01[1];
}

struct Layout {
  long slots, rep, df, bad, occ, refw, refnorm, key_score, total;
};

// ref_words <= 2^26 is checked by the callers
inline Layout layout(long ref_words, long sentences, long keys, long sets) {
  Layout l;
  l.slots = gram_slots(ref_words);
  long at = 0;
  l.rep = at; at += align256(4 * l.slots);
  l.occ = at; at += align256(16 * (ref_words > 0 ? ref_words : 1));   // (set to -1 together with rep)
  l.df = at;  at += align256(4 * l.slots);
  l.bad = at; at += 256;                          // (cleared together with df)
  l.refw = at; at += align256(16 * (ref_words > 0 ? ref_words : 1));
  l.refnorm = at; at += align256(16 * sentences);
  l.key_score = at; at += align256(4 * sets * keys);
  l.total = at;
  return l;
}

}  // namespace

extern "C" long ac_cider_workspace_bytes(long ref_words, int sentences, int keys, int sets) {
  if (ref_words < 0 || ref_words > kMaxGramWords || sentences <= 0 || keys <= 0 || keys > sentences || sets <= 0 ||
      sets > AC_CIDER_MAX_SETS)
    return AC_ERR_ARG;
  return layout(ref_words, sentences, keys, sets).total;
}

extern "C" int ac_cider_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                               const int* canon, int vocab_size, int n_words, const int* ref_words, long total_words,
                               const int* sent_off, int sentences, int max_ref_words, const int* key_off, int keys,
                               const int* row_key, const int* first_row, int order, float sigma, void* workspace,
                               long workspace_bytes, float* scores, float* reward, void* stream) {
  CiderArgs a = {};
  const int rc = fill_views(&a, &a, hyp, sets, hyp_ld, N, T, start_idx, end_idx, canon, vocab_size, ref_words, total_words,
                            sent_off, sentences, max_ref_words, key_off, keys, row_key, first_row);
  if (rc != AC_OK) return rc;
  if (n_words < vocab_size || order < 1 || order > 4 || !(sigma > 0.f) || !isfinite(sigma) || !workspace || !scores ||
      (reward && sets < 2) || ((uintptr_t)workspace & 255))
    return AC_ERR_ARG;
  const Layout l = layout(total_words, sentences, keys, sets);
  if (workspace_bytes < l.total) return AC_ERR_ARG;
  char* ws = (char*)workspace;
  a.n_words = n_words; a.order = order; a.inv_2sigma2 = 1.0f / (2.0f * sigma * sigma);
  a.rep = (int*)(ws + l.rep); a.df = (int*)(ws + l.df); a.mask = (unsigned)(l.slots - 1); a.bad = (int*)(ws + l.bad);
  a.occ = (int*)(ws + l.occ); a.refw = (float*)(ws + l.refw); a.refnorm = (float*)(ws + l.refnorm);
  a.key_score = (float*)(ws + l.key_score); a.scores = scores; a.reward = reward;
  hipStream_t st = (hipStream_t)stream;
  // occ starts at -1 as well: a sentence that the insert kernel refuses leaves no slot behind for the later kernels
  if (hipMemsetAsync(a.rep, 0xFF, l.df - l.rep, st) != hipSuccess) return AC_ERR_LAUNCH;
  if (hipMemsetAsync(a.df, 0, l.bad + 256 - l.df, st) != hipSuccess) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(cider_insert_kernel, dim3(sentences), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(cider_df_kernel, dim3(keys), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(cider_ref_kernel, dim3(sentences), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(cider_hyp_kernel, dim3(keys, sets), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(cider_scatter_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a);
  return ac_check_launch();
}
