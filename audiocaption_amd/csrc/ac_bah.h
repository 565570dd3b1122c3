// What the inference (csrc/attn_gru.hip) and the training (csrc/attn_gru_train.hip) entry points of the Bahdanau-attention
// GRU decoder share: the shape limits, the argument check of the weight struct, the workgroup reduction of the attention
// kernels and the exact-f32 product every projection of a decoder step runs on.
#pragma once
#include "ac_common.h"
#include "ac_sample.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

constexpr int BAH_MAX_DIM = 1024;   // emb_dim, d_model, attn_size, attn_emb_dim, fc_emb_dim
constexpr int BAH_MAX_TM = 2048;    // frames of the audio memory (one softmax row in LDS)
constexpr int BAH_MAX_V = SAMPLE_MAXV;

bool bah_shape_ok(const ac_bah_weights* w) {
  if (!w) return false;
  const int dims[5] = {w->emb_dim, w->d_model, w->attn_size, w->attn_emb_dim, w->fc_emb_dim};
  for (int v : dims)
    if (v <= 0 || v > BAH_MAX_DIM || v % 32 != 0) return false;
  if (w->vocab <= 0 || w->vocab > BAH_MAX_V || (w->n_tags != 0 && w->n_tags != 4)) return false;
  if (!w->emb || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->attn_w || !w->attn_b || !w->attn_v || !w->fc_w ||
      !w->fc_b || !w->ctx_w || !w->ctx_b || !w->cls_w || !w->cls_b || (w->n_tags && !w->temb))
    return false;
  return true;
}

size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }   // every carved array starts 16-byte aligned

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();   // sh may still be read by a previous call
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) : (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Y[M][N] = X[M][K] W[N][K]^T + bias on the exact-f32 MFMA GEMM of csrc/train.hip
int gemm(const float* X, long ldx, const float* W, long ldw, const float* bias, float* Y, long ldy, int M, int N, int K,
         void* stream) {
  return ac_gemm(X, ldx, 1, W, 1, ldw, Y, ldy, M, N, K, bias, 0, 0.0f, 1, 0.0f, 0ull, nullptr, 0, nullptr, 0, stream);
}

}  // namespace
