// Token-level knowledge distillation (kd_loss.py:8-49: TokenLevelKdLoss "kl", SupKdLoss over a LabelSmoothingLoss): the
// loss of a student's logits against a frozen teacher's per-token distributions, with its gradient, in one pass per row.
//
//   valid row (n, t), t < tgt_len[n]:
//     row_kd  = -sum_v softmax(z_t / temp)_v * log_softmax(z_s / temp)_v        (not scaled by temp^2, as the reference)
//     row_sup = -sum_v q_v * log_softmax(z_s)_v,  q = 1 - smoothing on the target, smoothing / (V - 1) elsewhere
//     dlogit  = g * [ w * (softmax(z_s) - q) + (1 - w) * (softmax(z_s / temp) - softmax(z_t / temp)) / temp ]
//   masked row: row_kd = row_sup = 0, dlogit = 0, neither logit row is read (a teacher's NaN at a padded position stays out).
//
// One 256-thread workgroup per row.  Both rows are read from global memory ONCE and held in registers: per thread up to
// NV4 chunks of four consecutive words (16-byte loads; the 16-byte aligned body of the row) plus one "edge" word - the
// up to three words before the body and the up to three after it, one per thread of the first six.  Rows of an odd V
// (4981) start 4-byte aligned only; the head is peeled per row.  The row maxima, then eight sums (three log-sum-exps, the
// cross term, the smoothing term, the target's logit and the two counts of words at the maximum) are reduced over the
// workgroup; the gradient pass re-evaluates the exponentials from the registers and stores 16 bytes at a time.  The final
// sums are a second, one-workgroup launch of the same call in a fixed order (no atomics).
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

constexpr int KD_MAXV = 16384;   // ac_scst_loss' limit: two rows of 64 words per thread

template <bool VEC>
__device__ __forceinline__ float4 kd_load4(const float* p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void kd_store4(float* p, float4 v) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}

__device__ __forceinline__ int kd_count(const int* tgt_len, int N, int T) {
  int cnt = 0;
  for (int i = 0; i < N; ++i) cnt += min(tgt_len[i], T);
  return cnt;
}

// VEC: the three base pointers are 16-byte aligned (else every chunk goes word by word and no head is peeled).
template <int NV4, bool VEC>
__global__ __launch_bounds__(256) void kd_loss_kernel(const float* __restrict__ logit, const float* __restrict__ tchr,
                                                      const long long* tgt, long tgt_ld, const int* tgt_len, int N, int T,
                                                      int V, float smoothing, float temp, float w, float* row_sup,
                                                      float* row_kd, float* dlogit, float gscale, const float* gscale_dev) {
  __shared__ float red[8][4];
  const int row = blockIdx.x, n = row / T, t = row % T;
  const int tid = threadIdx.x;
  const long base = (long)row * V;
  // head: words before the first 16-byte boundary of this row; body: n4 chunks of four; tail: the rest (< 4)
  const int head = VEC ? min((int)((4 - (base & 3)) & 3), V) : 0;
  const int n4 = (V - head) >> 2;
  const int tail0 = head + 4 * n4;
  // the edge word of this thread: tid < head -> word tid; head <= tid < head + (V - tail0) -> word tail0 + tid - head
  const int edge = tid < head ? tid : (tid - head < V - tail0 ? tail0 + tid - head : -1);
  float* dz = dlogit ? dlogit + base : nullptr;

  if (!(t < tgt_len[n])) {
    if (tid == 0) { row_sup[row] = 0.f; row_kd[row] = 0.f; }
    if (dz) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int c = 0; c < NV4; ++c) {
        const int i4 = c * 256 + tid;
        if (i4 < n4) kd_store4<VEC>(dz + head + 4 * i4, zero);
      }
      if (edge >= 0) dz[edge] = 0.f;
    }
    return;
  }

  const float* zs_p = logit + base;
  const float* zt_p = tchr + base;
  float4 zs[NV4], zt[NV4];
  float zs_e = -INFINITY, zt_e = -INFINITY;
#pragma unroll
  for (int c = 0; c < NV4; ++c) {
    const int i4 = c * 256 + tid;
    if (i4 < n4) {
      zs[c] = kd_load4<VEC>(zs_p + head + 4 * i4);
      zt[c] = kd_load4<VEC>(zt_p + head + 4 * i4);
    } else {
      zs[c] = zt[c] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);   // exp -> 0; skipped in the linear sums
    }
  }
  if (edge >= 0) { zs_e = zs_p[edge]; zt_e = zt_p[edge]; }

  // ---- row maxima ----
  float mx[2] = {zs_e, zt_e};
#pragma unroll
  for (int c = 0; c < NV4; ++c) {
    mx[0] = fmaxf(mx[0], fmaxf(fmaxf(zs[c].x, zs[c].y), fmaxf(zs[c].z, zs[c].w)));
    mx[1] = fmaxf(mx[1], fmaxf(fmaxf(zt[c].x, zt[c].y), fmaxf(zt[c].z, zt[c].w)));
  }
  mx[0] = wave_max(mx[0]);
  mx[1] = wave_max(mx[1]);
  if ((tid & 63) == 0) { red[0][tid >> 6] = mx[0]; red[1][tid >> 6] = mx[1]; }
  __syncthreads();
  const float ms = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  const float mt = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));

  // ---- the eight sums ----
  const int target = (int)tgt[(long)n * tgt_ld + t];
  const float it = 1.0f / temp;
  const bool one = temp == 1.0f;      // the two student soft-maxes coincide
  // [0] sum exp(a), [1] sum exp(a / temp), [2] sum exp(b / temp), [3] sum exp(b / temp) * a / temp, [4] sum a, [5] a[target],
  // [6] / [7] the number of student / teacher words at the maximum - with a = z_s - max z_s, b = z_t - max z_t.  [0], [1]
  // and [2] leave the words at the maximum (exp = 1) out: log sum exp = log(c) + log1p(r / c), which keeps a row term
  // that is small against 1 (a student that agrees with a confident teacher: r << 1) to f32 precision of ITSELF instead
  // of that of 1 + r; the gradient at a word both put at the maximum is formed from c and r the same way.
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto term = [&](float s, float tt, int v) {
    const float a = s - ms, b = (tt - mt) * it;
    const float e1 = expf(a);
    const float eT = one ? e1 : expf(a * it);
    const float et = expf(b);
    const bool top = a == 0.f;
    acc[0] += top ? 0.f : e1;
    acc[1] += top ? 0.f : eT;
    acc[6] += top ? 1.f : 0.f;
    acc[2] += b == 0.f ? 0.f : et;
    acc[7] += b == 0.f ? 1.f : 0.f;
    acc[3] += et * (a * it);
    acc[4] += a;
    if (v == target) acc[5] += a;
  };
#pragma unroll
  for (int c = 0; c < NV4; ++c) {
    const int i4 = c * 256 + tid;
    if (i4 < n4) {
      const int v = head + 4 * i4;
      term(zs[c].x, zt[c].x, v);
      term(zs[c].y, zt[c].y, v + 1);
      term(zs[c].z, zt[c].z, v + 2);
      term(zs[c].w, zt[c].w, v + 3);
    }
  }
  if (edge >= 0) term(zs_e, zt_e, edge);
  block_sums256(acc, red);
  const float cnt = acc[6], cnt_t = acc[7];
  const float se1 = cnt + acc[0], seT = cnt + acc[1], stT = cnt_t + acc[2];
  const float lse1 = logf(cnt) + log1pf(acc[0] / cnt), lseT = logf(cnt) + log1pf(acc[1] / cnt);
  const float off = smoothing / (float)(V - 1), conf = 1.0f - smoothing;
  if (tid == 0) {
    // -sum_v q_v (a_v - log se1) = log se1 - off * (sum a - a_tgt) - conf * a_tgt                      (sum q = 1)
    row_sup[row] = lse1 - off * (acc[4] - acc[5]) - conf * acc[5];
    // -sum_v p_v (a_v / temp - log seT) = log seT - (1 / stT) sum_v exp(b_v / temp) a_v / temp         (sum p = 1)
    row_kd[row] = lseT - acc[3] / stT;
  }
  if (!dz) return;

  // ---- gradient ----
  if (gscale <= 0.f) gscale = 1.0f / (float)kd_count(tgt_len, N, T);   // "mean", the count taken on the device
  if (gscale_dev) gscale *= gscale_dev[0];
  const float i1 = 1.0f / se1, iT = 1.0f / seT, itc = 1.0f / stT;
  const float gs = gscale * w, gk = gscale * (1.0f - w) * it;
  const bool kd_on = w < 1.0f;        // sup_weight 1: the teacher's values stay out of the gradient altogether
  // softmax(z_s / temp) - softmax(z_t / temp) where both are at their maximum: 1 / seT - 1 / stT without forming 1 + r
  const float both_top = ((cnt_t - cnt) + (acc[2] - acc[1])) * (iT * itc);
  auto grad = [&](float s, float tt, int v) {
    const float a = s - ms;
    const float e1 = expf(a);
    float g = gs * (e1 * i1 - (v == target ? conf : off));
    if (kd_on) {
      const float eT = one ? e1 : expf(a * it);
      const float b = (tt - mt) * it;
      g += gk * (a == 0.f && b == 0.f ? both_top : eT * iT - expf(b) * itc);
    }
    return g;
  };
#pragma unroll
  for (int c = 0; c < NV4; ++c) {
    const int i4 = c * 256 + tid;
    if (i4 < n4) {
      const int v = head + 4 * i4;
      kd_store4<VEC>(dz + v, make_float4(grad(zs[c].x, zt[c].x, v), grad(zs[c].y, zt[c].y, v + 1),
                                         grad(zs[c].z, zt[c].z, v + 2), grad(zs[c].w, zt[c].w, v + 3)));
    }
  }
  if (edge >= 0) dz[edge] = grad(zs_e, zt_e, edge);
}

// loss[1] = scale * sum(row_sup), loss[2] = scale * sum(row_kd), loss[0] = w * loss[1] + (1 - w) * loss[2]; a fixed
// summation order (one workgroup), like sum_scale_kernel of csrc/train.hip
__global__ __launch_bounds__(256) void kd_sum_kernel(const float* row_sup, const float* row_kd, long rows, float scale,
                                                     float w, float* loss, const int* tgt_len, int N, int T) {
  __shared__ float red[2][4];
  if (scale <= 0.f) scale = 1.0f / (float)kd_count(tgt_len, N, T);
  float a[2] = {0.f, 0.f};
  for (long i = threadIdx.x; i < rows; i += 256) {
    a[0] += row_sup[i];
    a[1] += row_kd[i];
  }
  block_sums256(a, red);
  if (threadIdx.x == 0) {
    const float sup = a[0] * scale, kd = a[1] * scale;
    loss[1] = sup;
    loss[2] = kd;
    // (a weight of exactly 0 keeps the other term out: 0 * inf would be NaN)
    loss[0] = (w > 0.f ? w * sup : 0.f) + (w < 1.f ? (1.0f - w) * kd : 0.f);
  }
}

template <int NV4>
void kd_launch(bool vec, dim3 grid, hipStream_t st, const float* logit, const float* tchr, const long long* tgt, long tgt_ld,
               const int* tgt_len, int N, int T, int V, float smoothing, float temp, float w, float* row_sup, float* row_kd,
               float* dlogit, float gscale, const float* gscale_dev) {
  if (vec)
    hipLaunchKernelGGL((kd_loss_kernel<NV4, true>), grid, dim3(256), 0, st, logit, tchr, tgt, tgt_ld, tgt_len, N, T, V,
                       smoothing, temp, w, row_sup, row_kd, dlogit, gscale, gscale_dev);
  else
    hipLaunchKernelGGL((kd_loss_kernel<NV4, false>), grid, dim3(256), 0, st, logit, tchr, tgt, tgt_ld, tgt_len, N, T, V,
                       smoothing, temp, w, row_sup, row_kd, dlogit, gscale, gscale_dev);
}

}  // namespace

extern "C" int ac_kd_loss(const float* logit, const float* tchr_logit, const long long* tgt, long tgt_ld, const int* tgt_len,
                          int N, int T, int V, float smoothing, float temp, float sup_weight, float inv_count, float* row_sup,
                          float* row_kd, float* loss, float* dlogit, float gscale, const float* gscale_dev, void* stream) {
  if (!logit || !tchr_logit || !tgt || !tgt_len || !row_sup || !row_kd || !loss || N <= 0 || T <= 0 || V < 2 || V > KD_MAXV ||
      tgt_ld < T || !(temp > 0.f) || !isfinite(temp) || !(sup_weight >= 0.f && sup_weight <= 1.f))
    return AC_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = (((uintptr_t)logit | (uintptr_t)tchr_logit | (uintptr_t)dlogit) & 15) == 0;
  const dim3 grid(N * T);
  // chunks of four words per thread: a peeled head can leave one chunk less, never one more
  const int nv4 = (V / 4 + 255) / 256;
#define KD_GO(NV4)                                                                                                        \
  kd_launch<NV4>(vec, grid, st, logit, tchr_logit, tgt, tgt_ld, tgt_len, N, T, V, smoothing, temp, sup_weight, row_sup,  \
                 row_kd, dlogit, gscale, gscale_dev)
  if (nv4 <= 1) KD_GO(1);
  else if (nv4 <= 2) KD_GO(2);
  else if (nv4 <= 5) KD_GO(5);
  else if (nv4 <= 8) KD_GO(8);
  else KD_GO(16);
#undef KD_GO
  hipLaunchKernelGGL(kd_sum_kernel, dim3(1), dim3(256), 0, st, row_sup, row_kd, (long)N * T, inv_count, sup_weight, loss,
                     tgt_len, N, T);
  return ac_check_launch();
}
