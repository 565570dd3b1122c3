// Internal interface of the on-device token sampler (csrc/sample.hip), shared with the decode chain (csrc/decoder.hip).
#pragma once
#include "ac_common.h"
#include "ac_ens.h"

// One row of logits -> one sampled word (base.py:214-252 sample_next_word, methods AC_SAMPLE_* of the public header).
// Without `seq` the word goes to word[r] and its log-probability to logprob[r * ld_lp] (ac_sample_rows).  With `seq` the
// kernel also does greedy_pick_kernel's bookkeeping for step t of a decode chain (base.py:157-168): unfinished flag, seq,
// next step's token / mask, unfinished count of the row's segment - and returns at once when no row of that segment was
// left unfinished after step t - 1.
struct SampleParams {
  const float* logit; long ldl;      // row r at logit + r * ldl
  int rows, V, method, k;
  float top_p, temp;
  const uint64_t* seed;              // device word: read by the kernel, so a captured graph replays with a new seed
  int t;                             // step: Philox counter word 0
  int* word;                         // [rows] (ac_sample_rows) or null
  float* logprob; long ld_lp;        // row r at logprob + r * ld_lp
  // decode-chain bookkeeping (null seq: none)
  int64_t* seq; int max_len, end_idx, pad_idx;
  int* tok; unsigned char* mask; int* unfinished; int* cnt;
  int seg_rows;                      // rows per segment of the chain, cnt [segments][max_len] (csrc/decoder.hip struct Live);
                                     // 0: one segment
  // Ensemble decoding (csrc/ensemble.hip): with ens.n > 0 `logit` is not read - the row sampled is the mean of the members'
  // log-softmaxes, formed in registers (ac_ens.h), and the kernel is instantiated with ensemble.py:412-449's rules where
  // they depart from base.py: temp divides the mean before top-p as well; the stored value is x[w] / temp (plain, top-k) or
  // x[w] (gumbel), not a log-softmax value; a row finished before step t stores nothing (its column keeps the initial 0).
  // ens.n == 0 (every single-model call site): base.py's rules, the kernels as they were.
  EnsPlanes ens;
};

constexpr int SAMPLE_MAXV = 16384;   // a row is held in registers: <= 64 logits per thread

int ac_sample_check(int V, int method, int k, float top_p, float temp);   // AC_OK or AC_ERR_ARG
int ac_sample_launch(const SampleParams& p, hipStream_t s);
