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

// ac_bah_weights.variant: what the third part of the GRU input is, and with it which slots of the struct are in use
//   BAH_CATFC  [embed | ctx_proj(c) | fc_proj(fc_emb)]       every slot (temb with n_tags)
//   BAH_COND   [embed | ctx_proj(c) | cond_emb]              fc_w = condition_embedding.weight [2][E]; fc_b NULL
//   BAH_SPEC   [embed | c | cond]                            w_ih = the first E + A columns of weight_ih_l0 packed to
//                                                            [3d][E + A], fc_w = its last column [3d]; fc_b, ctx_w,
//                                                            ctx_b NULL
// The conditional variants take no tags; a slot a variant does not use must be NULL.
enum { BAH_CATFC = 0, BAH_COND = 1, BAH_SPEC = 2 };

bool bah_shape_ok(const ac_bah_weights* w) {
  if (!w) return false;
  const int dims[5] = {w->emb_dim, w->d_model, w->attn_size, w->attn_emb_dim, w->fc_emb_dim};
  for (int v : dims)
    if (v <= 0 || v > BAH_MAX_DIM || v % 32 != 0) return false;
  if (w->vocab <= 0 || w->vocab > BAH_MAX_V || (w->n_tags != 0 && w->n_tags != 4)) return false;
  if (!w->emb || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->attn_w || !w->attn_b || !w->attn_v || !w->fc_w ||
      !w->cls_w || !w->cls_b || (w->n_tags && !w->temb))
    return false;
  switch (w->variant) {
    case BAH_CATFC: return w->fc_b && w->ctx_w && w->ctx_b;
    case BAH_COND: return !w->fc_b && w->ctx_w && w->ctx_b && !w->n_tags && !w->temb;
    case BAH_SPEC: return !w->fc_b && !w->ctx_w && !w->ctx_b && !w->n_tags && !w->temb;
    default: return false;
  }
}

// Width of the per-step part of the GRU input (xin, the K of the gi product), and the row pitch of w->w_ih
int bah_xw(const ac_bah_weights* w) { return w->variant == BAH_SPEC ? w->emb_dim + w->attn_emb_dim : 2 * w->emb_dim; }
long bah_ld_ih(const ac_bah_weights* w) { return w->variant == BAH_SPEC ? bah_xw(w) : 3L * w->emb_dim; }

size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }   // every carved array starts 16-byte aligned

// Y[M][N] = X[M][K] W[N][K]^T + bias on the exact-f32 MFMA GEMM of csrc/train.hip
int gemm(const float* X, long ldx, const float* W, long ldw, const float* bias, float* Y, long ldy, int M, int N, int K,
         void* stream) {
  return ac_gemm(X, ldx, 1, W, 1, ldw, Y, ldy, M, N, K, bias, 0, 0.0f, 1, 0.0f, 0ull, nullptr, 0, nullptr, 0, stream);
}

// ---- the condition's part of the input gates (BAH_COND / BAH_SPEC), once per batch ---------------------------------
// cond_emb[b] = (1 - c_b) W[0] + c_b W[1]   (torch.matmul([[1 - c, c]], condition_embedding.weight), rnn_decoder.py:311-312)
__global__ __launch_bounds__(256) void bah_cond_emb_kernel(const float* cond, const float* cw, float* out, int B, int E) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)B * E) return;
  const float c = cond[i / E];
  const int e = (int)(i % E);
  out[i] = (1.0f - c) * cw[e] + c * cw[E + e];
}

// gf[b] = c_b W_ih[:, E + A] + b_ih   (the raw condition is the last input column, rnn_decoder.py:563-565)
__global__ __launch_bounds__(256) void bah_cond_col_kernel(const float* cond, const float* col, const float* b_ih, float* gf,
                                                           int B, int n) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)B * n) return;
  const int j = (int)(i % n);
  gf[i] = fmaf(cond[i / n], col[j], b_ih[j]);
}

// gf [B][3d] of a conditional variant from cond [B]; pfc [B][E] receives cond_emb (BAH_COND)
int bah_cond_gates(const ac_bah_weights* w, const float* cond, float* pfc, float* gf, int B, void* stream) {
  const int E = w->emb_dim, d = w->d_model;
  if (w->variant == BAH_SPEC) {
    hipLaunchKernelGGL(bah_cond_col_kernel, dim3((unsigned)((3L * B * d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cond,
                       w->fc_w, w->b_ih, gf, B, 3 * d);
    return ac_check_launch();
  }
  hipLaunchKernelGGL(bah_cond_emb_kernel, dim3((unsigned)(((long)B * E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cond,
                     w->fc_w, pfc, B, E);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  return gemm(pfc, E, w->w_ih + 2 * E, 3L * E, w->b_ih, gf, 3L * d, B, 3 * d, E, stream);
}

}  // namespace
