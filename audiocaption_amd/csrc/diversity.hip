// Diversity of a set of captions on token ids: Self-BLEU (nltk's sentence_bleu with every other caption as a reference,
// weights 1/4 each, SmoothingFunction().method1, as the reference's eval/diversity.py calls it), the distinct n-gram counts
// behind vocabulary size and Distinct-n (diversity.py, diversity_instance.py) and the n-gram richness of
// eval/old_diversity.py.  Self-BLEU by its definition is quadratic in the corpus; one table of the corpus' distinct
// n-grams with four integers per entry makes it linear and yields the other numbers on the way.
//
// A distinct n-gram (n = 1 .. 4) is identified by the slot it holds in one table over the packed words (ac_ngram.h, as
// are the sentence rule and the count of a slot at its first occurrence); this file owns what is kept per slot and the
// scores made of it.  Per slot:
//   max1  the largest count of the n-gram in one sentence       ties  the sentences that hold max1
//   max2  the largest count among the sentences below max1      docs  the sentences that contain it
// so that for sentence i with count tf the largest count among the OTHER sentences is max1 when tf < max1 or ties >= 2,
// and max2 (0 when nobody else has the n-gram) when i alone holds the maximum.
//
//   div_pack_kernel    one workgroup per sentence: start skipped, cut at the first end, canonical ids -> workspace;
//                      the length histogram and the word total
//   div_insert_kernel  one workgroup per sentence: slot of every n-gram occurrence (atomicCAS claims; the claimer counts
//                      the distinct n-gram), count tf at the first occurrence in the sentence, max1 and docs
//   div_second_kernel  one workgroup per sentence: ties and max2
//   div_score_kernel   one workgroup per sentence: the clipped matches, the closest other length from the histogram less
//                      the sentence itself, the float64 score, the sentence's richness term per order
//   div_finish_kernel  the means
//
// The kernel boundaries are the only ordering between workgroups: the words an insert probe compares with were written
// by the launch before it, max1 is final before ties are counted, and so on.  Every probe loop is bounded by the table
// size.  Every count is an integer and integer atomics commute; float64 enters in closed formulas on those integers and in
// sums of fixed order (a thread's strided items, then the threads in order), so a call is bitwise repeatable - which
// occurrence represents an n-gram in the table depends on timing, and nothing downstream depends on it.  A word is
// range-checked before it indexes `canon`; nothing else is indexed by a word.
#include "ac_ngram.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kOrder = 4;
constexpr int kMaxWords = AC_CIDER_MAX_HYP_WORDS;
constexpr int kHist = 1280;        // lengths 0 .. kMaxWords, padded
constexpr int kCounters = 64;      // distinct[4], total words, bad (a word outside the vocabulary), full (no slot found)
constexpr int kTotalWords = 4, kBad = 5, kFull = 6;

struct DivArgs {
  const int* hyp;
  long hyp_ld;
  int N, T, start_idx, end_idx;
  const int* canon;
  int vocab_size;
  long W;           // N * T
  // workspace
  int* rep;         // [mask + 1] representative occurrence of the slot's n-gram, -1 = empty
  int4* cnt;        // [mask + 1] x = max1, y = max2, z = ties, w = docs
  unsigned mask;
  int* len_hist;    // [kHist]
  int* counters;    // [kCounters]
  int* words;       // [N][T] canonical ids, len[row] of them per row
  int* len;         // [N]
  int* occ;         // [4][N][T] slot of the n-gram that starts at a position
  int* tfirst;      // [4][N][T] its count in the sentence at its first occurrence there, 0 at a repeat
  double* rich;     // [N][4] mean over the sentence's distinct n-grams of log(1 / (docs / N))
  // outputs
  int* stats;          // [N][10]
  int* sent_distinct;  // [N][4]
  int* totals;         // [5]
  double* self_bleu;   // [N]
  double* summary;     // [6] (grouped call: [5])
  // ---- the grouped call (ac_diversity_group_scores) ----
  const int* group_off;   // [G + 1] rows [group_off[g], group_off[g + 1]) are group g
  int G;
  int* row_grp;        // workspace [N] group of a row, -1 = in no group of two rows or more
  int* gcount;         // workspace [G][5] words, distinct n-grams of the group
  double* mbleu;       // [N][4]
  int* group_totals;   // [G][5]
  double* group_mean;  // [G][5]
};

__global__ __launch_bounds__(kThreads) void div_pack_kernel(DivArgs a) {
  __shared__ int raw[kMaxWords];
  __shared__ int can[kMaxWords];   // -1: not a vocabulary id
  __shared__ int hw[kMaxWords];
  __shared__ int sh_len;
  const int row = blockIdx.x;
  const int L = load_sentence(a.hyp + (long)row * a.hyp_ld, a.T, a.start_idx, a.end_idx, a.canon, a.vocab_size, hw, raw,
                              can, &sh_len);
  for (int p = threadIdx.x; p < L; p += kThreads) a.words[(long)row * a.T + p] = hw[p];
  if (threadIdx.x == 0) {
    a.len[row] = L;
    if (L < 0) {
      a.counters[kBad] = 1;
    } else {
      atomicAdd(&a.len_hist[L], 1);
      atomicAdd(&a.counters[kTotalWords], L);
    }
  }
}

__global__ __launch_bounds__(kThreads) void div_insert_kernel(DivArgs a) {
  __shared__ int hw[kMaxWords];
  __shared__ int sl[kMaxWords];
  if (a.counters[kBad]) return;   // (written by the launch before: uniform)
  const int row = blockIdx.x;
  const int L = a.len[row];
  const long base = (long)row * a.T;
  for (int p = threadIdx.x; p < L; p += kThreads) hw[p] = a.words[base + p];
  __syncthreads();
  for (int n = 0; n < kOrder; ++n) {
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      bool fresh;
      const int slot = gram_claim(a.rep, a.mask, a.words, hw + p, n + 1, (int)(base + p) * 4 + n, &fresh);
      if (fresh) atomicAdd(&a.counters[n], 1);
      if (slot < 0) a.counters[kFull] = 1;   // (cannot happen below half full; read by the later launches only)
      sl[p] = slot;
    }
    __syncthreads();
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      const int slot = sl[p];
      bool first;
      const int tf = slot_count(sl, L - n, p, &first);
      a.occ[(long)n * a.W + base + p] = slot;
      a.tfirst[(long)n * a.W + base + p] = first ? tf : 0;
      if (first && slot >= 0) {
        atomicMax(&a.cnt[slot].x, tf);
        atomicAdd(&a.cnt[slot].w, 1);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void div_second_kernel(DivArgs a) {
  if (a.counters[kBad] | a.counters[kFull]) return;
  const int row = blockIdx.x;
  const int L = a.len[row];
  const long base = (long)row * a.T;
  for (int n = 0; n < kOrder; ++n)
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      const int tf = a.tfirst[(long)n * a.W + base + p];
      if (tf == 0) continue;
      const int slot = a.occ[(long)n * a.W + base + p];
      if (tf == a.cnt[slot].x)
        atomicAdd(&a.cnt[slot].z, 1);
      else
        atomicMax(&a.cnt[slot].y, tf);
    }
}

__global__ __launch_bounds__(kThreads) void div_score_kernel(DivArgs a) {
  __shared__ int sh_num[kOrder], sh_distinct[kOrder], sh_key;
  __shared__ double part[kOrder][kThreads];
  const int row = blockIdx.x;
  int* stats = a.stats + (long)row * 10;
  if (a.counters[kBad] | a.counters[kFull]) {
    if (threadIdx.x < 10) stats[threadIdx.x] = -1;
    if (threadIdx.x < kOrder) a.sent_distinct[(long)row * kOrder + threadIdx.x] = -1;
    if (threadIdx.x == 0) a.self_bleu[row] = NAN;
    return;
  }
  const int L = a.len[row];
  const long base = (long)row * a.T;
  if (threadIdx.x < kOrder) sh_num[threadIdx.x] = sh_distinct[threadIdx.x] = 0;
  if (threadIdx.x == 0) sh_key = 0x7FFFFFFF;
  __syncthreads();
  for (int n = 0; n < kOrder; ++n) {
    int num = 0, distinct = 0;
    double sum = 0.0;
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      const int tf = a.tfirst[(long)n * a.W + base + p];
      if (tf == 0) continue;
      const int4 c = a.cnt[a.occ[(long)n * a.W + base + p]];
      const int others = tf < c.x || c.z >= 2 ? c.x : c.y;
      num += min(tf, others);
      ++distinct;
      sum += log(1.0 / ((double)c.w / (double)a.N));
    }
    if (num) atomicAdd(&sh_num[n], num);
    if (distinct) atomicAdd(&sh_distinct[n], distinct);
    part[n][threadIdx.x] = sum;
  }
  // the closest length among the other sentences, of two equally close the smaller: the least (distance, length)
  for (int r = threadIdx.x; r <= a.T; r += kThreads)
    if (a.len_hist[r] - (r == L ? 1 : 0) > 0) atomicMin(&sh_key, (r > L ? r - L : L - r) * 2048 + r);
  __syncthreads();
  if (threadIdx.x < kOrder) {
    const int n = threadIdx.x;
    double sum = 0.0;
    for (int t = 0; t < kThreads; ++t) sum += part[n][t];
    a.rich[(long)row * kOrder + n] = sh_distinct[n] > 0 ? sum / (double)sh_distinct[n] : 0.0;
    a.sent_distinct[(long)row * kOrder + n] = sh_distinct[n];
  }
  if (threadIdx.x == 0) {
    const int ref_len = sh_key & 2047;
    stats[0] = L;
    stats[1] = ref_len;
    double log_sum = 0.0;
    for (int n = 0; n < kOrder; ++n) {
      const int den = L > n ? L - n : 1;
      const int num = sh_num[n];
      stats[2 + n] = den;
      stats[2 + kOrder + n] = num;
      const double p = num == 0 ? 0.1 / (double)den : (double)num / (double)den;   // method1, epsilon 0.1
      log_sum += 0.25 * log(p);
    }
    double score = 0.0;
    if (sh_num[0] != 0) {   // (so L > 0)
      const double bp = L > ref_len ? 1.0 : exp(1.0 - (double)ref_len / (double)L);
      score = bp * exp(log_sum);
    }
    a.self_bleu[row] = score;
  }
}

__global__ __launch_bounds__(kThreads) void div_finish_kernel(DivArgs a) {
  __shared__ double part[1 + kOrder][kThreads];
  __shared__ int have[kOrder];
  if (a.counters[kBad] | a.counters[kFull]) {
    if (threadIdx.x < 5) a.totals[threadIdx.x] = -1;
    if (threadIdx.x < 6) a.summary[threadIdx.x] = NAN;
    return;
  }
  if (threadIdx.x < kOrder) have[threadIdx.x] = 0;
  __syncthreads();
  double sum[1 + kOrder] = {};
  int count[kOrder] = {};
  for (int i = threadIdx.x; i < a.N; i += kThreads) {
    sum[0] += a.self_bleu[i];
    const int L = a.len[i];
#pragma unroll
    for (int n = 0; n < kOrder; ++n)
      if (L > n) {
        sum[1 + n] += a.rich[(long)i * kOrder + n];
        ++count[n];
      }
  }
#pragma unroll
  for (int n = 0; n < kOrder; ++n)
    if (count[n]) atomicAdd(&have[n], count[n]);
#pragma unroll
  for (int k = 0; k < 1 + kOrder; ++k) part[k][threadIdx.x] = sum[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double total[1 + kOrder];
    for (int k = 0; k < 1 + kOrder; ++k) {
      total[k] = 0.0;
      for (int t = 0; t < kThreads; ++t) total[k] += part[k][t];
    }
    a.summary[0] = total[0] / (double)a.N;
    double richness = 0.0;
    for (int n = 0; n < kOrder; ++n) {
      const double r = have[n] > 0 ? total[1 + n] / (double)have[n] : NAN;
      a.summary[1 + n] = r;
      richness += r * 0.25;
    }
    a.summary[1 + kOrder] = richness;
    a.totals[0] = a.counters[kTotalWords];
    for (int n = 0; n < kOrder; ++n) a.totals[1 + n] = a.counters[n];
  }
}

// ---- within groups ---------------------------------------------------------------------------------------------------------
// The same table, with the group as a part of an n-gram's identity: the hash mixes it in and a probe also compares the
// group of the representative's row (position / T in the packed words), so the same words in two groups hold two slots
// and div_second_kernel runs unchanged.  "The others" of a sentence are the other rows of its group: the closest length is
// found by a scan of the group's lengths, the sums of a group run over its rows in a fixed order.
constexpr int kBadGroups = 7;   // counters: group_off is not 0 = o[0] <= o[1] <= ... <= o[G] = N

__device__ __forceinline__ int group_gram_claim(const DivArgs& a, int g, const int* w, int len, int id, bool* fresh) {
  int slot = -1;
  *fresh = false;
  unsigned h = (gram_hash(w, len) ^ ((unsigned)g * 0x9E3779B1u)) & a.mask;
  for (unsigned probe = 0; probe <= a.mask; ++probe) {
    const int v = atomicCAS(&a.rep[h], -1, id);
    if (v == -1 || (a.row_grp[(v >> 2) / a.T] == g && gram_is(a.words, v, w, len))) {
      slot = (int)h;
      *fresh = v == -1;
      break;
    }
    h = (h + 1) & a.mask;
  }
  return slot;
}

// one workgroup per group: its rows learn their group.  The offsets are range-checked before they index anything; a group
// of fewer than two rows marks none (its rows and the group read NaN / -1, nothing of them is read)
__global__ __launch_bounds__(kThreads) void divg_rows_kernel(DivArgs a) {
  const int g = blockIdx.x;
  const int b = a.group_off[g], e = a.group_off[g + 1];
  if (b < 0 || e < b || e > a.N || (g == 0 && b != 0) || (g == a.G - 1 && e != a.N)) {
    if (threadIdx.x == 0) a.counters[kBadGroups] = 1;
    return;
  }
  if (e - b < 2) return;
  for (int r = b + threadIdx.x; r < e; r += kThreads) a.row_grp[r] = g;
}

__global__ __launch_bounds__(kThreads) void divg_pack_kernel(DivArgs a) {
  __shared__ int raw[kMaxWords];
  __shared__ int can[kMaxWords];   // -1: not a vocabulary id
  __shared__ int hw[kMaxWords];
  __shared__ int sh_len;
  const int row = blockIdx.x;
  const int g = a.counters[kBadGroups] ? -1 : a.row_grp[row];   // (both written by the launch before: uniform)
  if (g < 0) {
    if (threadIdx.x == 0) a.len[row] = -1;
    return;
  }
  const int L = load_sentence(a.hyp + (long)row * a.hyp_ld, a.T, a.start_idx, a.end_idx, a.canon, a.vocab_size, hw, raw,
                              can, &sh_len);
  for (int p = threadIdx.x; p < L; p += kThreads) a.words[(long)row * a.T + p] = hw[p];
  if (threadIdx.x == 0) {
    a.len[row] = L;
    if (L < 0) a.counters[kBad] = 1;
    else atomicAdd(&a.gcount[g * 5], L);
  }
}

__global__ __launch_bounds__(kThreads) void divg_insert_kernel(DivArgs a) {
  __shared__ int hw[kMaxWords];
  __shared__ int sl[kMaxWords];
  if (a.counters[kBad] | a.counters[kBadGroups]) return;
  const int row = blockIdx.x;
  const int L = a.len[row];        // (-1: a row outside every group)
  if (L <= 0) return;
  const int g = a.row_grp[row];
  const long base = (long)row * a.T;
  for (int p = threadIdx.x; p < L; p += kThreads) hw[p] = a.words[base + p];
  __syncthreads();
  for (int n = 0; n < kOrder; ++n) {
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      bool fresh;
      const int slot = group_gram_claim(a, g, hw + p, n + 1, (int)(base + p) * 4 + n, &fresh);
      if (fresh) atomicAdd(&a.gcount[g * 5 + 1 + n], 1);
      if (slot < 0) a.counters[kFull] = 1;   // (cannot happen below half full; read by the later launches only)
      sl[p] = slot;
    }
    __syncthreads();
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      const int slot = sl[p];
      bool first;
      const int tf = slot_count(sl, L - n, p, &first);
      a.occ[(long)n * a.W + base + p] = slot;
      a.tfirst[(long)n * a.W + base + p] = first ? tf : 0;
      if (first && slot >= 0) {
        atomicMax(&a.cnt[slot].x, tf);
        atomicAdd(&a.cnt[slot].w, 1);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void divg_score_kernel(DivArgs a) {
  __shared__ int sh_num[kOrder], sh_distinct[kOrder], sh_key;
  const int row = blockIdx.x;
  int* stats = a.stats + (long)row * 10;
  const bool bad = a.counters[kBad] | a.counters[kFull] | a.counters[kBadGroups];
  const int L = bad ? -1 : a.len[row];
  if (L < 0) {
    if (threadIdx.x < 10) stats[threadIdx.x] = -1;
    if (threadIdx.x < kOrder) {
      a.sent_distinct[(long)row * kOrder + threadIdx.x] = -1;
      a.mbleu[(long)row * kOrder + threadIdx.x] = NAN;
    }
    if (threadIdx.x == 0) a.self_bleu[row] = NAN;
    return;
  }
  const int g = a.row_grp[row];
  const int gb = a.group_off[g], ge = a.group_off[g + 1];   // (checked by divg_rows_kernel)
  const long base = (long)row * a.T;
  if (threadIdx.x < kOrder) sh_num[threadIdx.x] = sh_distinct[threadIdx.x] = 0;
  if (threadIdx.x == 0) sh_key = 0x7FFFFFFF;
  __syncthreads();
  for (int n = 0; n < kOrder; ++n) {
    int num = 0, distinct = 0;
    for (int p = threadIdx.x; p + n < L; p += kThreads) {
      const int tf = a.tfirst[(long)n * a.W + base + p];
      if (tf == 0) continue;
      const int4 c = a.cnt[a.occ[(long)n * a.W + base + p]];
      const int others = tf < c.x || c.z >= 2 ? c.x : c.y;
      num += min(tf, others);
      ++distinct;
    }
    if (num) atomicAdd(&sh_num[n], num);
    if (distinct) atomicAdd(&sh_distinct[n], distinct);
  }
  // the closest length among the other sentences of the group, of two equally close the smaller
  for (int r = gb + threadIdx.x; r < ge; r += kThreads)
    if (r != row) {
      const int lr = a.len[r];
      atomicMin(&sh_key, (lr > L ? lr - L : L - lr) * 2048 + lr);
    }
  __syncthreads();
  if (threadIdx.x < kOrder) a.sent_distinct[(long)row * kOrder + threadIdx.x] = sh_distinct[threadIdx.x];
  if (threadIdx.x == 0) {
    const int ref_len = sh_key & 2047;
    stats[0] = L;
    stats[1] = ref_len;
    double logp[kOrder];
    for (int n = 0; n < kOrder; ++n) {
      const int den = L > n ? L - n : 1;
      const int num = sh_num[n];
      stats[2 + n] = den;
      stats[2 + kOrder + n] = num;
      const double p = num == 0 ? 0.1 / (double)den : (double)num / (double)den;   // method1, epsilon 0.1
      logp[n] = log(p);
    }
    const double bp = sh_num[0] == 0 || L > ref_len ? 1.0 : exp(1.0 - (double)ref_len / (double)L);
    for (int k = 1; k <= kOrder; ++k) {
      const double wk = 1.0 / (double)k;
      double log_sum = 0.0;
      for (int n = 0; n < k; ++n) log_sum += wk * logp[n];
      const double score = sh_num[0] != 0 ? bp * exp(log_sum) : 0.0;
      a.mbleu[(long)row * kOrder + k - 1] = score;
      if (k == kOrder) a.self_bleu[row] = score;
    }
  }
}

// one workgroup per group: the counts of the group and the means over its sentences (a thread's strided rows, then the
// threads in order)
__global__ __launch_bounds__(kThreads) void divg_group_kernel(DivArgs a) {
  __shared__ double part[1 + kOrder][kThreads];
  const int g = blockIdx.x;
  int rows = 0, gb = 0;
  if (!(a.counters[kBad] | a.counters[kFull] | a.counters[kBadGroups])) {
    gb = a.group_off[g];
    rows = a.group_off[g + 1] - gb;
  }
  if (rows < 2) {
    if (threadIdx.x < 5) {
      a.group_totals[g * 5 + threadIdx.x] = -1;
      a.group_mean[g * 5 + threadIdx.x] = NAN;
    }
    return;
  }
  double sum[1 + kOrder] = {};
  for (int i = threadIdx.x; i < rows; i += kThreads) {
#pragma unroll
    for (int k = 0; k < kOrder; ++k) sum[k] += a.mbleu[(long)(gb + i) * kOrder + k];
    sum[kOrder] += a.self_bleu[gb + i];
  }
#pragma unroll
  for (int k = 0; k < 1 + kOrder; ++k) part[k][threadIdx.x] = sum[k];
  __syncthreads();
  if (threadIdx.x < 1 + kOrder) {
    const int k = threadIdx.x;
    double total = 0.0;
    for (int t = 0; t < kThreads; ++t) total += part[k][t];
    a.group_mean[g * 5 + k] = total / (double)rows;
    a.group_totals[g * 5 + k] = a.gcount[g * 5 + k];
  }
}

// the means over the groups, in the order of the groups within a thread and of the threads
__global__ __launch_bounds__(kThreads) void divg_summary_kernel(DivArgs a) {
  __shared__ double part[1 + kOrder][kThreads];
  double sum[1 + kOrder] = {};
  for (int g = threadIdx.x; g < a.G; g += kThreads)
#pragma unroll
    for (int k = 0; k < 1 + kOrder; ++k) sum[k] += a.group_mean[g * 5 + k];
#pragma unroll
  for (int k = 0; k < 1 + kOrder; ++k) part[k][threadIdx.x] = sum[k];
  __syncthreads();
  if (threadIdx.x < 1 + kOrder) {
    const int k = threadIdx.x;
    double total = 0.0;
    for (int t = 0; t < kThreads; ++t) total += part[k][t];
    a.summary[k] = total / (double)a.G;
  }
}


struct Layout {
  long slots, rep, cnt, len_hist, counters, words, len, occ, tfirst, rich, total;
};

// N * T <= 2^26 is checked by the callers
inline Layout layout(long N, long T) {
  const long W = N * T;
  Layout l;
  l.slots = gram_slots(W);
  long at = 0;
  l.rep = at; at += align256(4 * l.slots);
  l.cnt = at; at += align256(16 * l.slots);
  l.len_hist = at; at += align256(4L * kHist);         // (cleared together with cnt)
  l.counters = at; at += align256(4L * kCounters);     // (and so are these)
  l.words = at; at += align256(4 * W);
  l.len = at; at += align256(4 * N);
  l.occ = at; at += align256(16 * W);
  l.tfirst = at; at += align256(16 * W);
  l.rich = at; at += align256(8L * kOrder * N);
  l.total = at;
  return l;
}

inline bool sizes_ok(int N, int T) {
  return N >= 2 && T >= 1 && T <= kMaxWords && (long)N * T <= kMaxGramWords;
}

}  // namespace

extern "C" long ac_diversity_workspace_bytes(int N, int T) {
  if (!sizes_ok(N, T)) return AC_ERR_ARG;
  return layout(N, T).total;
}

extern "C" int ac_diversity_scores(const int* hyp, long hyp_ld, int N, int T, int start_idx, int end_idx, const int* canon,
                                   int vocab_size, void* workspace, long workspace_bytes, int* stats, int* sent_distinct,
                                   int* totals, double* self_bleu, double* summary, void* stream) {
  if (!hyp || !sizes_ok(N, T) || hyp_ld < T || !canon || vocab_size <= 0 || !workspace || ((uintptr_t)workspace & 255) ||
      !stats || !sent_distinct || !totals || !self_bleu || !summary)
    return AC_ERR_ARG;
  const Layout l = layout(N, T);
  if (workspace_bytes < l.total) return AC_ERR_ARG;
  char* ws = (char*)workspace;
  DivArgs a = {};
  a.hyp = hyp; a.hyp_ld = hyp_ld; a.N = N; a.T = T; a.start_idx = start_idx; a.end_idx = end_idx;
  a.canon = canon; a.vocab_size = vocab_size; a.W = (long)N * T;
  a.rep = (int*)(ws + l.rep); a.cnt = (int4*)(ws + l.cnt); a.mask = (unsigned)(l.slots - 1);
  a.len_hist = (int*)(ws + l.len_hist); a.counters = (int*)(ws + l.counters); a.words = (int*)(ws + l.words);
  a.len = (int*)(ws + l.len); a.occ = (int*)(ws + l.occ); a.tfirst = (int*)(ws + l.tfirst); a.rich = (double*)(ws + l.rich);
  a.stats = stats; a.sent_distinct = sent_distinct; a.totals = totals; a.self_bleu = self_bleu; a.summary = summary;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(a.rep, 0xFF, l.cnt - l.rep, st) != hipSuccess) return AC_ERR_LAUNCH;
  if (hipMemsetAsync(a.cnt, 0, l.words - l.cnt, st) != hipSuccess) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(div_pack_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(div_insert_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(div_second_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(div_score_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(div_finish_kernel, dim3(1), dim3(kThreads), 0, st, a);
  return ac_check_launch();
}

// ---- within groups: the pooled layout (its length histogram unused) plus the group of a row and the counts of a group ----
namespace {

struct GroupLayout { Layout l; long row_grp, gcount, total; };

inline GroupLayout group_layout(long N, long T, long G) {
  GroupLayout gl;
  gl.l = layout(N, T);
  long at = gl.l.total;
  gl.row_grp = at; at += align256(4 * N);
  gl.gcount = at; at += align256(4 * 5 * G);
  gl.total = at;
  return gl;
}

// every group has two rows or more: G <= N / 2 (the offsets themselves live on the device and are checked there)
inline bool group_sizes_ok(int N, int T, int G) { return sizes_ok(N, T) && G >= 1 && G <= N / 2; }

}  // namespace

extern "C" long ac_diversity_group_workspace_bytes(int N, int T, int G) {
  if (!group_sizes_ok(N, T, G)) return AC_ERR_ARG;
  return group_layout(N, T, G).total;
}

extern "C" int ac_diversity_group_scores(const int* hyp, long hyp_ld, int N, int T, int start_idx, int end_idx,
                                         const int* canon, int vocab_size, const int* group_off, int G, void* workspace,
                                         long workspace_bytes, int* stats, int* sent_distinct, double* self_bleu,
                                         double* mbleu, int* group_totals, double* group_mean, double* summary,
                                         void* stream) {
  if (!hyp || !group_sizes_ok(N, T, G) || hyp_ld < T || !canon || vocab_size <= 0 || !group_off || !workspace ||
      ((uintptr_t)workspace & 255) || !stats || !sent_distinct || !self_bleu || !mbleu || !group_totals || !group_mean ||
      !summary)
    return AC_ERR_ARG;
  const GroupLayout gl = group_layout(N, T, G);
  const Layout& l = gl.l;
  if (workspace_bytes < gl.total) return AC_ERR_ARG;
  char* ws = (char*)workspace;
  DivArgs a = {};
  a.hyp = hyp; a.hyp_ld = hyp_ld; a.N = N; a.T = T; a.start_idx = start_idx; a.end_idx = end_idx;
  a.canon = canon; a.vocab_size = vocab_size; a.W = (long)N * T;
  a.rep = (int*)(ws + l.rep); a.cnt = (int4*)(ws + l.cnt); a.mask = (unsigned)(l.slots - 1);
  a.len_hist = (int*)(ws + l.len_hist); a.counters = (int*)(ws + l.counters); a.words = (int*)(ws + l.words);
  a.len = (int*)(ws + l.len); a.occ = (int*)(ws + l.occ); a.tfirst = (int*)(ws + l.tfirst);
  a.group_off = group_off; a.G = G; a.row_grp = (int*)(ws + gl.row_grp); a.gcount = (int*)(ws + gl.gcount);
  a.stats = stats; a.sent_distinct = sent_distinct; a.self_bleu = self_bleu; a.summary = summary;
  a.mbleu = mbleu; a.group_totals = group_totals; a.group_mean = group_mean;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(a.rep, 0xFF, l.cnt - l.rep, st) != hipSuccess) return AC_ERR_LAUNCH;
  if (hipMemsetAsync(a.cnt, 0, l.words - l.cnt, st) != hipSuccess) return AC_ERR_LAUNCH;
  if (hipMemsetAsync(a.row_grp, 0xFF, gl.gcount - gl.row_grp, st) != hipSuccess) return AC_ERR_LAUNCH;
  if (hipMemsetAsync(a.gcount, 0, gl.total - gl.gcount, st) != hipSuccess) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(divg_rows_kernel, dim3(G), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(divg_pack_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(divg_insert_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(div_second_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(divg_score_kernel, dim3(N), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(divg_group_kernel, dim3(G), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(divg_summary_kernel, dim3(1), dim3(kThreads), 0, st, a);
  return ac_check_launch();
}
