// BLEU-1..4 and ROUGE-L on token ids, as pycocoevalcap's bleu_scorer.py (option "closest") and rouge.py (beta 1.2)
// compute them on words: the two string metrics of the reference's evaluation (train_eval/base.py) that need neither
// Java nor a language model.  Their arguments - hypothesis planes behind a host array of device pointers, packed references
// per key - their sentence rule and the count of an n-gram at its first occurrence are those of ac_ngram.h; this file owns
// the matching against the references, the LCS and the closed formulas.
//
//   bleu_key_kernel     one workgroup per (key, set): the hypothesis in LDS; tf of every distinct hypothesis n-gram at its
//                       first occurrence; each reference staged in LDS in turn and counted against, the maximum kept per
//                       n-gram; correct[n] = sum min(tf, max); reflen; the four sentence scores in float64
//   bleu_finish_kernel  score of a row = score of its key; integer totals over the keys -> the corpus scores
//   rouge_key_kernel    one workgroup per (key, set), one wave per reference: the LCS by the bit-parallel row update
//                       (Crochemore et al. 2001 / Hyyro 2004) over the full |h| x |r| table, 64 hypothesis positions per
//                       machine word, no banding and no cut-off; then F_beta of the best precision and the best recall
//   rouge_finish_kernel score of a row = score of its key; the mean over the keys
//
// N-grams are compared word by word, never by a hash.  Counts are integers (LDS integer atomics commute), float64 enters
// only in the closed formulas on those integers and in one sum of fixed order (a thread's strided keys, then the threads
// in order), so a call is bitwise repeatable.  A reference word is only ever compared, a hypothesis word indexes `canon`
// after its range check: nothing here is indexed by a word.
#include "ac_ngram.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxOrder = 4;
constexpr int kHypWords64 = AC_CIDER_MAX_HYP_WORDS / 64;

struct MetricArgs : HypView, RefView {
  int order;
  double* key_score;     // workspace: BLEU [sets][K][4], ROUGE-L [sets][K]
  int* ints;             // BLEU stats [sets][K][2 + 2 * order]; ROUGE-L lcs [sets][M]
  double* scores;        // BLEU [sets][order][N]; ROUGE-L [sets][N]
  double* total;         // BLEU corpus [sets][order]; ROUGE-L mean [sets]
};

// The hypothesis of key k and its references, as far as both kernels refuse them alike: a sentence that does not fit the
// LDS staging, a key without a sentence.  Returns the hypothesis' length (load_key_sentence), or -1; uniform over the
// workgroup, every thread of which calls it.
__device__ int load_key(const MetricArgs& a, int k, int set, int* hw, int* raw, int* can, int* sh_len, int* s0, int* s1) {
  const int L = load_key_sentence(a, a, k, set, hw, raw, can, sh_len);
  bool ok = L >= 0 && key_range(a, k, s0, s1) && *s1 > *s0;
  if (ok)
    for (int s = *s0; s < *s1; ++s) {
      int b, e;
      ok = ok && sentence_range(a, s, &b, &e) && e - b <= AC_CIDER_MAX_REF_WORDS;
    }
  return ok ? L : -1;
}

// bleu_scorer.py, one sentence or the corpus: b_k = prod_{j <= k} (correct[j] + tiny) / (guess[j] + small),
// bleu_k = b_k^(1 / (k + 1)), times exp(1 - 1 / ratio) when ratio = (testlen + tiny) / (reflen + small) < 1.
__device__ void bleu_from_counts(long long testlen, long long reflen, const long long* guess, const long long* correct,
                                 int order, double* out) {
  const double tiny = 1e-15, small = 1e-9;
  const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
  const double brevity = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
  double b = 1.0;
  for (int k = 0; k < order; ++k) {
    b *= ((double)correct[k] + tiny) / ((double)guess[k] + small);
    const double v = pow(b, 1.0 / (double)(k + 1));
    out[k] = ratio < 1.0 ? v * brevity : v;
  }
}

__global__ __launch_bounds__(kThreads) void bleu_key_kernel(MetricArgs a) {
  __shared__ int hw[AC_CIDER_MAX_HYP_WORDS];
  __shared__ int rw[AC_CIDER_MAX_REF_WORDS];
  __shared__ int tf[kMaxOrder][AC_CIDER_MAX_HYP_WORDS];   // count in the hypothesis at an n-gram's first occurrence, else 0
  __shared__ int mx[kMaxOrder][AC_CIDER_MAX_HYP_WORDS];   // max over the references of its count there
  __shared__ int sh_len, sh_correct[kMaxOrder];
  const int k = blockIdx.x, set = blockIdx.y;
  const int width = 2 + 2 * a.order;
  int* stats = a.ints + ((long)set * a.K + k) * width;
  double* score = a.key_score + ((long)set * a.K + k) * kMaxOrder;
  int s0, s1;
  const int L = load_key(a, k, set, hw, tf[0], tf[1], &sh_len, &s0, &s1);
  if (L < 0) {
    for (int i = threadIdx.x; i < width; i += kThreads) stats[i] = -1;
    if (threadIdx.x < kMaxOrder) score[threadIdx.x] = NAN;
    return;
  }
  __syncthreads();   // tf[0], tf[1] staged the row: all reads of them are done
  if (threadIdx.x < kMaxOrder) sh_correct[threadIdx.x] = 0;
  for (int n = 0; n < a.order; ++n)
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      bool first;
      const int count = gram_count(hw, L, p, n + 1, &first);
      tf[n][p] = first ? count : 0;
      mx[n][p] = 0;
    }
  for (int s = s0; s < s1; ++s) {
    const int b = a.sent_off[s], R = a.sent_off[s + 1] - b;
    __syncthreads();
    for (int q = threadIdx.x; q < R; q += kThreads) rw[q] = a.words[b + q];
    __syncthreads();
    for (int n = 0; n < a.order; ++n)
      for (int p = threadIdx.x; p + n < L; p += kThreads) {   // (a position belongs to one thread throughout)
        if (tf[n][p] == 0) continue;
        int count = 0;
        for (int q = 0; q + n < R; ++q) {
          bool same = true;
          for (int i = 0; i <= n; ++i) same = same && rw[q + i] == hw[p + i];
          count += same;
        }
        if (count > mx[n][p]) mx[n][p] = count;
      }
  }
  for (int n = 0; n < a.order; ++n) {
    int c = 0;
    for (int p = threadIdx.x; p + n < L; p += kThreads) c += min(tf[n][p], mx[n][p]);
    if (c) atomicAdd(&sh_correct[n], c);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int reflen = 0, best = -1;   // the closest reference length; of two equally close, the smaller
    for (int s = s0; s < s1; ++s) {
      const int R = a.sent_off[s + 1] - a.sent_off[s];
      const int d = R > L ? R - L : L - R;
      if (best < 0 || d < best || (d == best && R < reflen)) {
        best = d;
        reflen = R;
      }
    }
    long long guess[kMaxOrder], correct[kMaxOrder];
    double out[kMaxOrder];
    stats[0] = L;
    stats[1] = reflen;
    for (int n = 0; n < a.order; ++n) {
      guess[n] = L > n ? L - n : 0;
      correct[n] = sh_correct[n];
      stats[2 + n] = (int)guess[n];
      stats[2 + a.order + n] = (int)correct[n];
    }
    bleu_from_counts(L, reflen, guess, correct, a.order, out);
    for (int n = 0; n < a.order; ++n) score[n] = out[n];
  }
}

__global__ __launch_bounds__(kThreads) void bleu_finish_kernel(MetricArgs a) {
  __shared__ unsigned long long tot[2 + 2 * kMaxOrder];
  __shared__ int sh_bad;
  const int set = blockIdx.y;
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < a.N) {
    const int k = a.row_key[n];
    const bool ok = k >= 0 && k < a.K;
    for (int o = 0; o < a.order; ++o)
      a.scores[((long)set * a.order + o) * a.N + n] = ok ? a.key_score[((long)set * a.K + k) * kMaxOrder + o] : NAN;
  }
  if (blockIdx.x != 0) return;
  const int width = 2 + 2 * a.order;
  if (threadIdx.x < width) tot[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) sh_bad = 0;
  __syncthreads();
  unsigned long long part[2 + 2 * kMaxOrder] = {};
  bool bad = false;
  for (int k = threadIdx.x; k < a.K; k += kThreads) {
    const int* st = a.ints + ((long)set * a.K + k) * width;
    if (st[0] < 0) {
      bad = true;
      continue;
    }
#pragma unroll
    for (int i = 0; i < 2 + 2 * kMaxOrder; ++i)
      if (i < width) part[i] += (unsigned long long)st[i];
  }
#pragma unroll
  for (int i = 0; i < 2 + 2 * kMaxOrder; ++i)
    if (i < width && part[i]) atomicAdd(&tot[i], part[i]);
  if (bad) sh_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long guess[kMaxOrder], correct[kMaxOrder];
    double out[kMaxOrder];
    for (int o = 0; o < a.order; ++o) {
      guess[o] = (long long)tot[2 + o];
      correct[o] = (long long)tot[2 + a.order + o];
    }
    bleu_from_counts((long long)tot[0], (long long)tot[1], guess, correct, a.order, out);
    for (int o = 0; o < a.order; ++o) a.total[set * a.order + o] = sh_bad ? NAN : out[o];   // (a key without a score)
  }
}

__global__ __launch_bounds__(kThreads) void rouge_key_kernel(MetricArgs a) {
  __shared__ int hw[AC_CIDER_MAX_HYP_WORDS];
  __shared__ int raw[AC_CIDER_MAX_HYP_WORDS];
  __shared__ int can[AC_CIDER_MAX_HYP_WORDS];
  __shared__ int sh_len;
  __shared__ double best[kThreads / 64][2];
  const int k = blockIdx.x, set = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s0, s1;
  const int L = load_key(a, k, set, hw, raw, can, &sh_len, &s0, &s1);
  if (L < 0) {
    if (threadIdx.x == 0) a.key_score[(long)set * a.K + k] = NAN;
    return;
  }
  const int nw = (L + 63) >> 6;   // machine words that hold the hypothesis positions
  double prec = 0.0, rec = 0.0;
  for (int s = s0 + wave; s < s1; s += kThreads / 64) {   // one wave per reference; nothing below differs between its lanes
    const int b = a.sent_off[s], R = a.sent_off[s + 1] - b;
    // V: bit i of the row is 0 where the LCS table grows between hypothesis positions i and i + 1.  Per reference word c
    // with match mask M (bit i: hw[i] == c): U = V & M, V = (V + U) | (V & ~U), the addition carrying across words.
    unsigned long long V[kHypWords64];
#pragma unroll
    for (int w = 0; w < kHypWords64; ++w) V[w] = ~0ull;
    for (int j = 0; j < R; ++j) {
      const int c = a.words[b + j];
      unsigned long long carry = 0ull;
#pragma unroll
      for (int w = 0; w < kHypWords64; ++w)
        if (w < nw) {
          const int i = w * 64 + lane;
          const unsigned long long M = __ballot(i < L && hw[i] == c);
          const unsigned long long U = V[w] & M;
          const unsigned long long s1_ = V[w] + U;
          const unsigned long long s2_ = s1_ + carry;
          carry = (unsigned long long)((s1_ < V[w]) | (s2_ < s1_));
          V[w] = s2_ | (V[w] & ~U);
        }
    }
    int lcs = 0;
#pragma unroll
    for (int w = 0; w < kHypWords64; ++w)
      if (w < nw) {
        const int rest = L - w * 64;
        const unsigned long long valid = rest >= 64 ? ~0ull : (1ull << rest) - 1ull;
        lcs += __popcll(~V[w] & valid);
      }
    if (lane == 0) a.ints[(long)set * a.M + s] = lcs;
    if (L > 0) prec = fmax(prec, (double)lcs / (double)L);
    if (R > 0) rec = fmax(rec, (double)lcs / (double)R);
  }
  if (lane == 0) {
    best[wave][0] = prec;
    best[wave][1] = rec;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      prec = fmax(prec, best[w][0]);
      rec = fmax(rec, best[w][1]);
    }
    const double beta2 = 1.2 * 1.2;
    a.key_score[(long)set * a.K + k] =
        prec != 0.0 && rec != 0.0 ? ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec) : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void rouge_finish_kernel(MetricArgs a) {
  __shared__ double part[kThreads];
  const int set = blockIdx.y;
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < a.N) {
    const int k = a.row_key[n];
    a.scores[(long)set * a.N + n] = k >= 0 && k < a.K ? a.key_score[(long)set * a.K + k] : NAN;
  }
  if (blockIdx.x != 0) return;
  double sum = 0.0;
  for (int k = threadIdx.x; k < a.K; k += kThreads) sum += a.key_score[(long)set * a.K + k];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = 0.0;
    for (int t = 0; t < kThreads; ++t) sum += part[t];
    a.total[set] = sum / (double)a.K;
  }
}

// what both entry points check, and the arguments both kernels share
int fill(MetricArgs* a, const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
         const int* canon, int vocab_size, const int* ref_words, long total_words, const int* sent_off, int sentences,
         int max_ref_words, const int* key_off, int keys, const int* row_key, const int* first_row, void* workspace,
         long workspace_bytes, const void* ints, const void* scores, const void* total) {
  const int rc = fill_views(a, a, hyp, sets, hyp_ld, N, T, start_idx, end_idx, canon, vocab_size, ref_words, total_words,
                            sent_off, sentences, max_ref_words, key_off, keys, row_key, first_row);
  if (rc != AC_OK) return rc;
  if (!workspace || ((uintptr_t)workspace & 255) || !ints || !scores || !total ||
      workspace_bytes < align256(8L * kMaxOrder * sets * keys))
    return AC_ERR_ARG;
  a->key_score = (double*)workspace; a->ints = (int*)ints; a->scores = (double*)scores; a->total = (double*)total;
  return AC_OK;
}

}  // namespace

extern "C" long ac_capmetrics_workspace_bytes(int keys, int sets) {
  if (keys <= 0 || sets <= 0 || sets > AC_CIDER_MAX_SETS) return AC_ERR_ARG;
  return align256(8L * kMaxOrder * sets * keys);
}

extern "C" int ac_bleu_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                              const int* canon, int vocab_size, const int* ref_words, long total_words,
                              const int* sent_off, int sentences, int max_ref_words, const int* key_off, int keys,
                              const int* row_key, const int* first_row, int order, void* workspace, long workspace_bytes,
                              int* stats, double* scores, double* corpus, void* stream) {
  if (order < 1 || order > kMaxOrder) return AC_ERR_ARG;
  MetricArgs a = {};
  const int rc = fill(&a, hyp, sets, hyp_ld, N, T, start_idx, end_idx, canon, vocab_size, ref_words, total_words, sent_off,
                      sentences, max_ref_words, key_off, keys, row_key, first_row, workspace, workspace_bytes, stats, scores,
                      corpus);
  if (rc != AC_OK) return rc;
  a.order = order;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bleu_key_kernel, dim3(keys, sets), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(bleu_finish_kernel, dim3((N + kThreads - 1) / kThreads, sets), dim3(kThreads), 0, st, a);
  return ac_check_launch();
}

extern "C" int ac_rouge_l_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                                 const int* canon, int vocab_size, const int* ref_words, long total_words,
                                 const int* sent_off, int sentences, int max_ref_words, const int* key_off, int keys,
                                 const int* row_key, const int* first_row, void* workspace, long workspace_bytes, int* lcs,
                                 double* scores, double* mean, void* stream) {
  MetricArgs a = {};
  const int rc = fill(&a, hyp, sets, hyp_ld, N, T, start_idx, end_idx, canon, vocab_size, ref_words, total_words, sent_off,
                      sentences, max_ref_words, key_off, keys, row_key, first_row, workspace, workspace_bytes, lcs, scores,
                      mean);
  if (rc != AC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  // a sentence of a key that the kernel refuses keeps -1
  if (hipMemsetAsync(lcs, 0xFF, 4L * sets * sentences, st) != hipSuccess) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(rouge_key_kernel, dim3(keys, sets), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(rouge_finish_kernel, dim3((N + kThreads - 1) / kThreads, sets), dim3(kThreads), 0, st, a);
  return ac_check_launch();
}
