// On-device token sampling for the caption decoder (base.py:214-252 sample_next_word): plain temperature sampling, top-k,
// top-p (nucleus) and Gumbel-max.  One 256-thread workgroup per row; thread i holds the contiguous logits
// [i * NPT, (i + 1) * NPT) in registers, so the row is read from memory once and every scan below is in vocabulary order.
//
//   1. max m and, except for top-p, S = sum exp(x - m): lp = x - m - log S is the reference's log_softmax.
//   2. top-k / top-p: the boundary of the kept set by a radix select over the f32 keys, no sort.  Four passes of 8-bit
//      digits, most significant first; each builds a 256-bin LDS histogram of the rows still matching the selected prefix -
//      counts, and for top-p the mass exp(x - m) in 2^-40 fixed point (64-bit integer atomics: exact and independent of the
//      order the atomics land in, so a row is sampled the same way on every run).  A block scan of the bins in descending
//      key order finds the bin holding the k-th element (top-k) or the first element at which the mass ranked ahead of it
//      plus its own reaches p * total (top-p: "cumsum < p shifted right by one").  It ends as soon as the bin is decided.
//      Elements equal to the boundary value are kept in index order (the lower index wins).
//   3. The draw: inverse CDF in vocabulary order over the kept weights exp((x - m) / temp): a block prefix scan, then the
//      first i whose running sum reaches u * total, u in (0, 1] from Philox4x32-10 at counter (step, row, 0, 0), key = seed.
//   4. The word's log-probability as the reference stores it, and (decode chain) greedy_pick_kernel's bookkeeping.
#include "ac_sample.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

// monotone map f32 -> u32: a larger logit has a larger key
__device__ __forceinline__ uint32_t sample_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d) {
  const int lo = __shfl_up((int)(uint32_t)v, d, 64);
  const int hi = __shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ float shfl_up_f32(float v, int d) { return __shfl_up(v, d, 64); }

// Block-wide scan over the 256 threads in thread order: returns the inclusive value, `excl` the exclusive one, `total` the
// block total.  The summation order is fixed, so float results are reproducible; the last thread's inclusive value is `total`
// bit for bit.  sh: 4 words of LDS.  All 256 threads must call it.
template <typename T, typename Up>
__device__ __forceinline__ T block_scan(T v, T* sh, T& excl, T& total, Up up) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = up(v, d);
    if (lane >= d) v += o;
  }
  T ex = up(v, 1);
  if (lane == 0) ex = T(0);
  __syncthreads();   // sh may still be read by a previous call
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  T add = T(0);
  for (int w = 0; w < wave; ++w) add += sh[w];
  total = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  excl = ex + add;
  return v + add;
}

// (min of a, max of b) over the block
__device__ __forceinline__ void block_min_max(int& a, int& b, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a = min(a, __shfl_xor(a, o, 64));
    b = max(b, __shfl_xor(b, o, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = min(min(sh[0], sh[1]), min(sh[2], sh[3]));
  b = max(max(sh[4], sh[5]), max(sh[6], sh[7]));
}

constexpr float SAMPLE_FIX = 1099511627776.0f;   // 2^40: fixed-point scale of the top-p masses (exp(x - m) <= 1)

template <int NPT, bool ENS>
__global__ __launch_bounds__(256) void sample_kernel(SampleParams p) {
  __shared__ unsigned long long hmass[256];
  __shared__ unsigned int hcnt[256];
  __shared__ unsigned long long sh_u[4];
  __shared__ float sh_f[4];
  __shared__ int sh_i[8];
  __shared__ unsigned long long sel_ahead, sel_mass;
  __shared__ unsigned int sel_bin, sel_cnt;
  const int r = blockIdx.x, tid = threadIdx.x, c0 = tid * NPT;
  int* const cnt = p.seq && p.seg_rows > 0 ? p.cnt + (size_t)(r / p.seg_rows) * p.max_len : p.cnt;   // of this row's segment
  if (p.seq && p.t > 0 && cnt[p.t - 1] == 0) return;   // the reference loop of this batch has already stopped (base.py:167)
  float x[NPT];
  if (ENS) {
    ens_mean<NPT, false>(p.ens, r, p.V, x, sh_f);
  } else {
    const float* row = p.logit + (size_t)r * p.ldl;
#pragma unroll
    for (int i = 0; i < NPT; ++i) x[i] = c0 + i < p.V ? row[c0 + i] : -INFINITY;
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NPT; ++i) m = fmaxf(m, x[i]);
  m = block_max256(m, sh_f);

  const bool topk = p.method == AC_SAMPLE_TOPK, topp = p.method == AC_SAMPLE_TOPP;
  // lp / temp for plain and top-k; top-p draws from softmax(logit) and Gumbel-max from softmax(lp): temp has no effect
  // (ENS: ensemble.py:427 divides by temp before the top-p branch as well)
  const float inv_t = (topk || p.method == AC_SAMPLE_PLAIN || (ENS && topp)) ? 1.0f / p.temp : 1.0f;
  float lse = 0.f;
  if (!topp) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NPT; ++i)
      if (c0 + i < p.V) s += expf(x[i] - m);
    lse = logf(block_sum256(s, sh_f));
  }

  // ---- the kept set: key >> shift > prefix, or == prefix and among the first n_tie of those in index order ----
  bool all = true;
  uint32_t prefix = 0, n_tie = 0, bin_cnt = 0;
  int shift = 0;
  if (topk || topp) {
    all = false;
    // top-k: the k-th element; top-p: the first whose mass plus the mass ranked ahead reaches ceil(p * total) (set below from
    // the first pass's histogram, so that every later bin total is an exact part of it)
    unsigned long long target = (unsigned long long)p.k;
    unsigned long long ahead = 0;   // measure (count or mass) of the elements ranked above the selected prefix
    for (shift = 24;; shift -= 8) {
      hmass[tid] = 0;
      hcnt[tid] = 0;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const uint32_t key = sample_key(x[i]);
        if (c0 + i < p.V && (shift == 24 || (key >> (shift + 8)) == prefix)) {
          const uint32_t dg = (key >> shift) & 255u;
          atomicAdd(&hcnt[dg], 1u);
          if (topp) atomicAdd(&hmass[dg], __float2ull_rn(expf((x[i] - m) * inv_t) * SAMPLE_FIX));   // (inv_t = 1 for base.py's top-p) top-k: the count is the measure
        }
      }
      __syncthreads();
      const int b = 255 - tid;                 // thread order = descending key order
      const unsigned long long mb = topk ? (unsigned long long)hcnt[b] : hmass[b];
      unsigned long long ex, tot;
      const unsigned long long in = block_scan(mb, sh_u, ex, tot, shfl_up_u64);
      if (topp && shift == 24) {
        target = (unsigned long long)ceil((double)p.top_p * (double)tot);
        if (target < 1) target = 1;
      }
      if (ahead + ex < target && ahead + in >= target) {   // exactly one bin (integer measures: the totals are exact)
        sel_ahead = ahead + ex;
        sel_mass = mb;
        sel_bin = (uint32_t)b;
        sel_cnt = hcnt[b];
      }
      __syncthreads();
      prefix = (prefix << 8) | sel_bin;
      ahead = sel_ahead;
      bin_cnt = sel_cnt;
      const unsigned long long mbin = sel_mass;
      if (bin_cnt == 1 || (topk && ahead + mbin == target)) {   // the whole bin is kept
        n_tie = bin_cnt;
        break;
      }
      if (shift == 0) {   // one value left: every element of the bin has the same measure e
        const unsigned long long e = mbin / bin_cnt;
        const unsigned long long need = (target - ahead + e - 1) / e;
        n_tie = need < 1 ? 1u : need > bin_cnt ? bin_cnt : (uint32_t)need;
        break;
      }
    }
  }
  // tie rank: only when part of the boundary value's elements is kept
  const bool ranked = !all && n_tie < bin_cnt;
  uint32_t tie_base = 0;
  if (ranked) {
    unsigned long long c = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i)
      if (c0 + i < p.V && (sample_key(x[i]) >> shift) == prefix) ++c;
    unsigned long long ex, tot;
    block_scan(c, sh_u, ex, tot, shfl_up_u64);
    tie_base = (uint32_t)ex;
  }

  // ---- the draw: inverse CDF over the kept weights in vocabulary order ----
  float wsum = 0.f;
  {
    uint32_t tr = tie_base;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      bool keep = c0 + i < p.V;
      if (!all && keep) {
        const uint32_t kk = sample_key(x[i]) >> shift;
        keep = kk > prefix || (kk == prefix && (!ranked || tr++ < n_tie));
      }
      if (keep) wsum += expf((x[i] - m) * inv_t);
    }
  }
  float acc, total;
  block_scan(wsum, sh_f, acc, total, shfl_up_f32);
  const float u = ac_sample_uniform(*p.seed, (uint32_t)p.t, (uint32_t)r);
  const float goal = u * total;
  int cand = 0x7fffffff, last = -1;
  {
    uint32_t tr = tie_base;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      bool keep = c0 + i < p.V;
      if (!all && keep) {
        const uint32_t kk = sample_key(x[i]) >> shift;
        keep = kk > prefix || (kk == prefix && (!ranked || tr++ < n_tie));
      }
      if (keep) {
        const float wv = expf((x[i] - m) * inv_t);
        if (wv > 0.f) {
          acc += wv;
          last = c0 + i;
          if (acc >= goal && cand == 0x7fffffff) cand = c0 + i;
        }
      }
    }
  }
  block_min_max(cand, last, sh_i);
  const int word = cand != 0x7fffffff ? cand : last;   // (rounding of the last partial sums: the last kept word)
  if (word < c0 || word >= c0 + NPT) return;

  // ---- the owner of the word writes it ----
  float xw = 0.f;
#pragma unroll
  for (int i = 0; i < NPT; ++i)
    if (c0 + i == word) xw = x[i];
  float lp;
  if (topp) lp = (xw - m) * inv_t - logf(total);            // log(q_w / sum of the kept q), q = softmax(logit) (ENS: of x / temp)
  else if (ENS) lp = p.method == AC_SAMPLE_GUMBEL ? xw : xw / p.temp;   // ensemble.py:425,:446 gather the mean itself
  else if (p.method == AC_SAMPLE_GUMBEL) lp = (xw - m) - lse;  // lp[w]
  else lp = ((xw - m) - lse) / p.temp;                      // lp[w] / temp (top-k: not renormalised)
  if (!p.seq) {
    p.logprob[(size_t)r * p.ld_lp] = lp;
    p.word[r] = word;
    return;
  }
  // greedy_pick_kernel's bookkeeping (base.py:157-168): a finished row emits end_idx, its logprob keeps the drawn word's
  const int prev = p.t == 0 ? 1 : p.unfinished[r];
  if (!(ENS && !prev)) p.logprob[(size_t)r * p.ld_lp] = lp;
  const int unf = prev && (word != p.end_idx);
  const int w = unf ? word : p.end_idx;
  p.unfinished[r] = unf;
  p.seq[(size_t)r * p.max_len + p.t] = w;
  p.tok[(size_t)r * (p.max_len + 1) + p.t + 1] = w;
  p.mask[(size_t)r * (p.max_len + 1) + p.t + 1] = (w == p.pad_idx) ? 1 : 0;
  if (unf) atomicAdd(&cnt[p.t], 1);
}

}  // namespace

int ac_sample_check(int V, int method, int k, float top_p, float temp) {
  if (V <= 0 || V > SAMPLE_MAXV) return AC_ERR_ARG;
  switch (method) {
    case AC_SAMPLE_PLAIN: return (temp > 0.f && isfinite(temp)) ? AC_OK : AC_ERR_ARG;
    case AC_SAMPLE_TOPK: return (temp > 0.f && isfinite(temp) && k >= 1 && k <= V) ? AC_OK : AC_ERR_ARG;
    case AC_SAMPLE_TOPP: return (top_p > 0.f && top_p < 1.f) ? AC_OK : AC_ERR_ARG;
    case AC_SAMPLE_GUMBEL: return AC_OK;
    default: return AC_ERR_ARG;
  }
}

int ac_sample_launch(const SampleParams& p, hipStream_t s) {
  const bool ens = p.ens.n > 0;
  if (ac_sample_check(p.V, p.method, p.k, p.top_p, p.temp) != AC_OK || p.rows <= 0 || (!ens && !p.logit) || !p.seed || !p.logprob)
    return AC_ERR_ARG;
  if (ens && p.method == AC_SAMPLE_TOPP && !(p.temp > 0.f && isfinite(p.temp))) return AC_ERR_ARG;
  if (!p.seq && !p.word) return AC_ERR_ARG;
  if (p.seq && (!p.tok || !p.mask || !p.unfinished || !p.cnt || p.t < 0 || p.t >= p.max_len)) return AC_ERR_ARG;
  const dim3 grid(p.rows), block(256);
  if (ens) {   // the same kernel over the mean of the members' log-softmaxes (ac_ens.h)
    if (p.V <= 256 * 20) hipLaunchKernelGGL((sample_kernel<20, true>), grid, block, 0, s, p);
    else if (p.V <= 256 * 32) hipLaunchKernelGGL((sample_kernel<32, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((sample_kernel<64, true>), grid, block, 0, s, p);
    return ac_check_launch();
  }
  if (p.V <= 256 * 8) hipLaunchKernelGGL((sample_kernel<8, false>), grid, block, 0, s, p);
  else if (p.V <= 256 * 20) hipLaunchKernelGGL((sample_kernel<20, false>), grid, block, 0, s, p);
  else if (p.V <= 256 * 32) hipLaunchKernelGGL((sample_kernel<32, false>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((sample_kernel<64, false>), grid, block, 0, s, p);
  return ac_check_launch();
}

extern "C" int ac_sample_rows(const float* logit, long ld, int rows, int V, int method, int k, float top_p, float temp,
                              const uint64_t* seed_dev, int step, int* word_out, float* logprob_out, void* stream) {
  if (!logit || !seed_dev || !word_out || !logprob_out || rows <= 0 || ld < V || step < 0) return AC_ERR_ARG;
  SampleParams p = {};
  p.logit = logit; p.ldl = ld; p.rows = rows; p.V = V; p.method = method; p.k = k; p.top_p = top_p; p.temp = temp;
  p.seed = seed_dev; p.t = step; p.word = word_out; p.logprob = logprob_out; p.ld_lp = 1;
  return ac_sample_launch(p, (hipStream_t)stream);
}
