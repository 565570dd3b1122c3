// The n-gram core of the scorers on token ids (csrc/cider.hip, csrc/capmetrics.hip, csrc/diversity.hip): the sentence
// rule, the open-addressing table of distinct n-grams, the two "count at the first occurrence" loops, the view of packed
// references and hypothesis planes with its argument checks, and the sizes of the host side.  Integer code only: every
// floating-point formula lives in the kernel that uses it.  Workgroups have 256 threads.
#pragma once
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

// ---- the sentence rule (model_util.py:117-164) ------------------------------------------------------------------------
// The sentence of a row of T token ids into hw (LDS, up to T ints): start skipped, cut at the first end, canonical ids.
// raw / can: LDS staging of T ints each (free again on return); sh_len: one LDS word.  row is null when there is no such
// row.  Returns the length, or -1 for a null row or a word outside the vocabulary (which is never used as an index).
// Every thread of the workgroup calls it.
__device__ __forceinline__ int load_sentence(const int* row, int T, int start_idx, int end_idx, const int* canon,
                                             int vocab_size, int* hw, int* raw, int* can, int* sh_len) {
  if (row)
    for (int t = threadIdx.x; t < T; t += 256) {
      const int w = row[t];
      raw[t] = w;
      can[t] = w >= 0 && w < vocab_size ? canon[w] : -1;
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    int L = 0;
    bool bad = !row;
    for (int t = 0; row && t < T; ++t) {
      const int w = raw[t];
      if (w == end_idx) break;
      if (w == start_idx) continue;
      if (w < 0 || w >= vocab_size) {
        bad = true;
        break;
      }
      hw[L++] = can[t];
    }
    *sh_len = bad ? -1 : L;
  }
  __syncthreads();
  return *sh_len;
}

// ---- the table ----------------------------------------------------------------------------------------------------------
// A distinct n-gram (1 .. 4 words) is identified by the slot it holds in rep[mask + 1].  A slot stores the position of one
// occurrence of the n-gram in the flat `words` (position * 4 + length - 1), -1 while it is empty; a probe compares the
// WORDS at that position with its own, so two n-grams share a slot only if they are equal, whatever the hash does.  The
// table is sized by gram_slots: at most half full.  Every probe is bounded by the table size.
__device__ __forceinline__ unsigned gram_hash(const int* w, int len) {
  unsigned h = 0x811C9DC5u ^ (unsigned)len;
  for (int i = 0; i < len; ++i) h = (h ^ (unsigned)w[i]) * 0x01000193u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return h ^ (h >> 12);
}

// does the slot's representative spell the `len` words at w?
__device__ __forceinline__ bool gram_is(const int* words, int rep, const int* w, int len) {
  if ((rep & 3) != len - 1) return false;
  const int* r = words + (rep >> 2);
  for (int i = 0; i < len; ++i)
    if (r[i] != w[i]) return false;
  return true;
}

// the slot of the `len` words at w, or -1 when the table does not hold them (read only: ends at an empty slot)
__device__ __forceinline__ int gram_find(const int* rep, unsigned mask, const int* words, const int* w, int len) {
  int slot = -1;
  unsigned h = gram_hash(w, len) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const int v = rep[h];
    if (v == -1) break;
    if (gram_is(words, v, w, len)) {
      slot = (int)h;
      break;
    }
    h = (h + 1) & mask;
  }
  return slot;
}

// the slot of the `len` words at w, claimed for the occurrence `id` (atomicCAS) if no equal n-gram holds one yet;
// *fresh (when asked for): this caller claimed it.  -1 only from a full table.
__device__ __forceinline__ int gram_claim(int* rep, unsigned mask, const int* words, const int* w, int len, int id,
                                          bool* fresh = nullptr) {
  int slot = -1;
  if (fresh) *fresh = false;
  unsigned h = gram_hash(w, len) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const int v = atomicCAS(&rep[h], -1, id);
    if (v == -1 || gram_is(words, v, w, len)) {
      slot = (int)h;
      if (fresh) *fresh = v == -1;
      break;
    }
    h = (h + 1) & mask;
  }
  return slot;
}

// ---- counts at the first occurrence ------------------------------------------------------------------------------------
// occurrences among the L words at hw of the `len` words that start at p; *first: none of them starts before p
__device__ __forceinline__ int gram_count(const int* hw, int L, int p, int len, bool* first) {
  int tf = 0;
  bool f = true;
  for (int q = 0; q + len <= L; ++q) {
    bool same = true;
    for (int i = 0; i < len; ++i) same = same && hw[q + i] == hw[p + i];
    if (same) {
      ++tf;
      f = f && q >= p;
    }
  }
  *first = f;
  return tf;
}

// occurrences of sl[p] among the `count` slots at sl; *first: none of them before p
__device__ __forceinline__ int slot_count(const int* sl, int count, int p, bool* first) {
  const int slot = sl[p];
  int tf = 0;
  bool f = true;
  for (int q = 0; q < count; ++q)
    if (sl[q] == slot) {
      ++tf;
      f = f && q >= p;
    }
  *first = f;
  return tf;
}

// ---- hypothesis planes and packed references ---------------------------------------------------------------------------
struct HypView {
  const int* hyp[AC_CIDER_MAX_SETS];   // row n of set s at hyp[s] + n * hyp_ld
  long hyp_ld;
  int sets, N, T, start_idx, end_idx;
  const int* canon;   // [vocab_size] canonical id of a word
  int vocab_size;
};

struct RefView {
  const int* words;      // [W] reference words, canonical ids
  int W;
  const int* sent_off;   // [M + 1]
  int M;
  const int* key_off;    // [K + 1] first sentence of each key
  int K;
  const int* row_key;    // [N]
  const int* first_row;  // [K]
};

// do the words of sentence s lie inside `words`?
__device__ __forceinline__ bool sentence_range(const RefView& r, int s, int* begin, int* end) {
  const int b = r.sent_off[s], e = r.sent_off[s + 1];
  *begin = b;
  *end = e;
  return b >= 0 && e >= b && e <= r.W;
}

// do the sentences of key k lie inside sent_off?  (s0 == s1, a key without a sentence, is in range)
__device__ __forceinline__ bool key_range(const RefView& r, int k, int* s0, int* s1) {
  const int b = r.key_off[k], e = r.key_off[k + 1];
  *s0 = b;
  *s1 = e;
  return b >= 0 && e >= b && e <= r.M;
}

// load_sentence on the first row of key k in plane `set`
__device__ __forceinline__ int load_key_sentence(const HypView& h, const RefView& r, int k, int set, int* hw, int* raw,
                                                 int* can, int* sh_len) {
  const int row = r.first_row[k];
  const int* p = row >= 0 && row < h.N ? h.hyp[set] + (long)row * h.hyp_ld : nullptr;
  return load_sentence(p, h.T, h.start_idx, h.end_idx, h.canon, h.vocab_size, hw, raw, can, sh_len);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static inline long align256(long b) { return (b + 255) & ~255L; }

constexpr long kMaxGramWords = 1L << 26;   // words in one table: positions * 4 + length - 1 stay in int32

// slots of a table over `words` words: at most 4 n-grams per word, so at most half full
static inline long gram_slots(long words) {
  long slots = 64;
  while (slots < 8 * words) slots *= 2;
  return slots;
}

// What every scorer of hypothesis planes against packed references checks of its arguments; fills the two views.
static inline int fill_views(HypView* h, RefView* r, const int* const* hyp, int sets, long hyp_ld, int N, int T,
                             int start_idx, int end_idx, const int* canon, int vocab_size, const int* ref_words,
                             long total_words, const int* sent_off, int sentences, int max_ref_words, const int* key_off,
                             int keys, const int* row_key, const int* first_row) {
  if (!hyp || sets <= 0 || sets > AC_CIDER_MAX_SETS || N <= 0 || T <= 0 || T > AC_CIDER_MAX_HYP_WORDS || hyp_ld < T ||
      !canon || vocab_size <= 0 || !ref_words || total_words < 0 || total_words > kMaxGramWords || !sent_off ||
      sentences <= 0 || max_ref_words < 0 || max_ref_words > AC_CIDER_MAX_REF_WORDS || !key_off || keys <= 0 ||
      keys > sentences || !row_key || !first_row)
    return AC_ERR_ARG;
  for (int s = 0; s < sets; ++s) {
    if (!hyp[s]) return AC_ERR_ARG;
    h->hyp[s] = hyp[s];
  }
  h->hyp_ld = hyp_ld; h->sets = sets; h->N = N; h->T = T; h->start_idx = start_idx; h->end_idx = end_idx;
  h->canon = canon; h->vocab_size = vocab_size;
  r->words = ref_words; r->W = (int)total_words; r->sent_off = sent_off; r->M = sentences; r->key_off = key_off;
  r->K = keys; r->row_key = row_key; r->first_row = first_row;
  return AC_OK;
}
