// Training of the Bahdanau-attention GRU caption decoder (csrc/attn_gru.hip is its inference side): the scheduled-sampling
// forward that keeps what the backward needs, and the backward through time of the GRU cell and the additive attention
// (reference rnn_decoder.py:183-215, hf_wrapper.py:1377-1414,1513-1554, driven by base.py:152-208, attn_model.py:34-65).
//
// Forward, step t over the B clips - bah_step's chain and arithmetic, every buffer indexed [step][clip]:
//   hg[t]  = h_t [W_h ; W_hh]^T + [0 ; b_hh]                    two GEMMs
//   bah_train_attn_kernel    the step's input word (cap[:, t], <start>, or the arg-max of step t - 1), its embedding (the
//                            tag's at t == 0 of a temporal decoder) times the in_dropout mask, scores, softmax, context
//   xin[t][:, E:2E] = ctx[t] ctx_proj^T + b ;  gi = xin[t] W_ih[:, :2E]^T        two GEMMs
//   bah_train_gate_kernel    GRU cell; keeps r, z, n and h_{t+1}
//   logit[:, t] = h_{t+1} classifier^T + b                        GEMM
//   bah_train_pick_kernel    seq[:, t] = arg-max (first index on ties), its log-probability
// The SCST rollout (ac_bah_train_rollout) is the same chain with no caption: the pick is ac_scst_pick (the sampled or forced
// word under the finished-row rule, into an int32 buffer) and step t > 0 feeds the word that step t - 1 stored there.
// Kept per (step, clip): h_t, h_{t+1}, hg (the query projection W_h h and W_hh h + b_hh), the attention weights, the
// context, xin, the gates, the input word.  tanh(q + ek) is NOT kept (B T Tm S floats): the backward recomputes it.
//
// Backward, t = T-1 .. 0, per step:
//   bah_train_gate_bwd_kernel   dh_t (carry + classifier part) -> dgi[t], dgh[t], carry = z dh
//   dxin[t] = dgi[t] W_ih[:, :2E] ;  dctx = dxin[t][:, E:2E] ctx_w              two GEMMs
//   bah_train_attn_bwd_kernel   one workgroup per clip: dw = dctx . attn_emb[tm], softmax backward, tanh recomputed,
//                               dq[t], dv[t], d attn_emb[clip] += w dctx, dek[clip] += dscore v (1 - tanh^2)
//   carry += dq[t] W_h + dgh[t] W_hh                                              two GEMMs
// dek and d attn_emb of a clip are touched by that clip's workgroup only and the steps run in stream order, so the
// accumulation over the steps is a plain read-modify-write: no atomics, no waits across workgroups.  Everything off the
// recurrence (dlogit W_cls in front; every weight gradient, bias column sum and the embedding scatter behind) runs once
// over all B T rows.  The per-step products have M = B rows and run in exact f32 like bah_step's; the products over all
// rows go through ac_gemm_bf16x3, which keeps the small ones on the exact-f32 kernels.
//
// The condition-controlled variants (ac_bah.h; ac_bah_train_forward_cond / ac_bah_train_backward_cond, cond [B] in fc_emb's
// place) run the same chain with xin bah_xw(w) wide.  BAH_SPEC has no ctx_proj: the context is xin[:, E:E+A], dctx is that
// slice of dxin.  Their own gradients, all off the recurrence, from dgf = sum_t dgi[t]:
//   BAH_COND   d cond_emb = dgf W_ih[:, 2E:3E];  d condition_embedding.weight[k] += sum_b ([1 - c_b, c_b][k]) d cond_emb[b]
//   BAH_SPEC   d W_ih[:, E+A] += sum_b c_b dgf[b]
// Neither reads fc_emb (d_fc_emb is written as zeros) and cond is data (no gradient).  W_ih of BAH_SPEC is read from the
// host's aligned [3d][E+A] pack; its gradient goes into the parameter's real layout: g->w_ih [3d][E+A+1] with the odd pitch
// as ldc of the weight-gradient product, g->fc_w = g->w_ih + E + A the last column, pitch E+A+1.
#include "ac_bah.h"
#include "ac_drop.h"

namespace {

constexpr int BAH_KMAX = BAH_MAX_DIM / 64;   // attention columns a lane of a 64-lane wave owns

// The workspace, in floats: the once-per-batch part, what the forward keeps, what the backward fills.
struct TrainWs {
  float *ek, *pfc, *gf;                                   // [B*Tm][S], [B][E], [B][3d]
  float *hg, *w, *ctx, *xin, *gates, *h_all, *embed, *gi; // [T][B][S+3d], [T][B][Tm], [T][B][A], [T][B][xw], [T][B][3d],
                                                          // [T+1][B][d], [B][T][d], [B][3d]
  int* tok;                                               // [T][B]: the input word; -1 - tag at the tag step
  float *dhc, *dgi, *dgh, *dxin, *dq, *dv;                // [B][T][d], [T][B][3d] x 2, [T][B][xw], [T][B][S] x 2
  float *dctx, *dh, *dek, *dgf, *dpfc;                    // [B][A], [B][d], [B*Tm][S], [B][3d], [B][E]
  size_t total;
};

TrainWs train_carve(const ac_bah_weights* w, float* base, int B, int Tm, int T) {
  const size_t E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim;
  const size_t R = (size_t)T * B;
  TrainWs s;
  size_t o = 0;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += up4(n); return p; };
  s.ek = take((size_t)B * Tm * S);
  s.pfc = take((size_t)B * E);
  s.gf = take((size_t)B * 3 * d);
  s.hg = take(R * (S + 3 * d));
  s.w = take(R * Tm);
  s.ctx = take(R * A);
  s.xin = take(R * bah_xw(w));
  s.gates = take(R * 3 * d);
  s.h_all = take((R + B) * d);
  s.embed = take(R * d);
  s.gi = take((size_t)B * 3 * d);
  s.tok = (int*)take(R);
  s.dhc = take(R * d);
  s.dgi = take(R * 3 * d);
  s.dgh = take(R * 3 * d);
  s.dxin = take(R * bah_xw(w));
  s.dq = take(R * S);
  s.dv = take(R * S);
  s.dctx = take((size_t)B * A);
  s.dh = take((size_t)B * d);
  s.dek = take((size_t)B * Tm * S);
  s.dgf = take((size_t)B * 3 * d);
  s.dpfc = take((size_t)B * E);
  s.total = o;
  return s;
}

__device__ __forceinline__ int clamp_len(int len, int Tm) { return len < 0 ? 0 : (len > Tm ? Tm : len); }

// ---- forward ---------------------------------------------------------------------------------------------------
struct TAttnP {
  const float* hg; long ld_hg;           // clip b's W_h h_t at hg + b * ld_hg
  const float *ek, *attn_emb, *v;        // [B][Tm][S], [B][Tm][A], [S]
  const int* mem_len;
  const float *emb, *temb;
  const int* tags;                       // [B] at the tag step, null otherwise
  const long long* cap; long cap_ld;     // [B][cap_ld]
  const int64_t* seq;                    // [B][T]: the arg-max of the steps so far
  const int* words; long words_ld;       // rollout: [B][words_ld], the words ac_scst_pick stored; null otherwise
  int* tok;                              // this step's [B]
  float *ctx; long ld_ctx;               // this step's context of clip b at ctx + b * ld_ctx, A values
  float *xin; long ld_xin;               // this step's input embedding of clip b at xin + b * ld_xin, E values
  float* w;                              // this step's [B][Tm]
  float* attn_out;                       // weight of (clip b, frame tm) at attn_out + (b * Tm + tm) * T
  Drop drop;
  int use_cap, t, T, B, start_idx, Tm, S, A, E, V, n_tags;
};

// One workgroup per clip: bah_attn_kernel with the scheduled-sampling word choice and in_dropout in front.
__global__ __launch_bounds__(256) void bah_train_attn_kernel(TAttnP p) {
  __shared__ float s_q[BAH_MAX_DIM];
  __shared__ float s_v[BAH_MAX_DIM];
  __shared__ float s_w[BAH_MAX_TM];
  __shared__ float s_red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = clamp_len(p.mem_len[b], p.Tm);
  for (int a = tid; a < p.S; a += 256) {
    s_q[a] = p.hg[(size_t)b * p.ld_hg + a];
    s_v[a] = p.v[a];
  }
  {
    const float* src;
    int code;
    if (p.tags) {
      int g = p.tags[b];
      g = g < 0 ? 0 : (g >= p.n_tags ? p.n_tags - 1 : g);
      src = p.temb + (size_t)g * p.E;
      code = -1 - g;
    } else {
      long long wd;
      if (p.words) wd = p.t == 0 ? (long long)p.start_idx : (long long)p.words[(size_t)b * p.words_ld + p.t - 1];
      else wd = p.use_cap ? p.cap[(size_t)b * p.cap_ld + p.t]
                          : (p.t == 0 ? (long long)p.start_idx : (long long)p.seq[(size_t)b * p.T + p.t - 1]);
      wd = wd < 0 ? 0 : (wd >= p.V ? p.V - 1 : wd);
      src = p.emb + (size_t)wd * p.E;
      code = (int)wd;
    }
    if (tid == 0) p.tok[b] = code;
    const uint64_t i0 = ((uint64_t)p.t * p.B + b) * p.E;    // in_dropout's mask index: (step, clip, feature)
    for (int e = tid; e < p.E; e += 256) p.xin[(size_t)b * p.ld_xin + e] = src[e] * p.drop.mask(i0 + e);
  }
  __syncthreads();
  const float* ek = p.ek + (size_t)b * p.Tm * p.S;
  for (int t = wave; t < p.Tm; t += 4) {
    float sc = -1e10f;   // masked_fill(mask == 0, -1e10)
    if (t < len) {
      float acc = 0.f;
      for (int a = lane; a < p.S; a += 64) acc += s_v[a] * tanhf(s_q[a] + ek[(size_t)t * p.S + a]);
      sc = wave_sum(acc);
    }
    if (lane == 0) s_w[t] = sc;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = tid; t < p.Tm; t += 256) m = fmaxf(m, s_w[t]);
  m = block_max256(m, s_red);
  float sum = 0.f;
  for (int t = tid; t < p.Tm; t += 256) {
    const float e = expf(s_w[t] - m);
    s_w[t] = e;
    sum += e;
  }
  sum = block_sum256(sum, s_red);
  for (int t = tid; t < p.Tm; t += 256) {
    const float wgt = s_w[t] / sum;
    s_w[t] = wgt;
    p.w[(size_t)b * p.Tm + t] = wgt;
    p.attn_out[((size_t)b * p.Tm + t) * p.T] = wgt;
  }
  __syncthreads();
  const int nt = len > 0 ? len : p.Tm;
  const float* mem = p.attn_emb + (size_t)b * p.Tm * p.A;
  for (int a = tid; a < p.A; a += 256) {
    float acc = 0.f;
    for (int t = 0; t < nt; ++t) acc = fmaf(s_w[t], mem[(size_t)t * p.A + a], acc);
    p.ctx[(size_t)b * p.ld_ctx + a] = acc;
  }
}

struct TGateP {
  const float *gi, *gf, *hg; long ld_hg;    // gi, gf [B][3d]; clip b's W_hh h + b_hh at hg + b * ld_hg
  const float* h_in; float *h_out, *gates;  // [B][d], [B][d], [B][3d]
  float *embed_ws, *embed_out;              // [B][T][d] + t * d
  int B, d, T;
};

// bah_gate_kernel, keeping the gates
__global__ __launch_bounds__(256) void bah_train_gate_kernel(TGateP p) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)p.B * p.d) return;
  const int b = (int)(i / p.d), j = (int)(i % p.d), d = p.d;
  const float h = p.h_in[i];
  const float* gi = p.gi + (size_t)b * 3 * d;
  const float* gf = p.gf + (size_t)b * 3 * d;
  const float* gh = p.hg + (size_t)b * p.ld_hg;
  const float rg = ac_sigmoid_exact((gi[j] + gf[j]) + gh[j]);
  const float zg = ac_sigmoid_exact((gi[d + j] + gf[d + j]) + gh[d + j]);
  const float ng = tanhf((gi[2 * d + j] + gf[2 * d + j]) + rg * gh[2 * d + j]);
  const float hn = (1.0f - zg) * ng + zg * h;
  float* g = p.gates + (size_t)b * 3 * d;
  g[j] = rg;
  g[d + j] = zg;
  g[2 * d + j] = ng;
  p.h_out[i] = hn;
  p.embed_ws[(size_t)b * p.T * d + j] = hn;
  p.embed_out[(size_t)b * p.T * d + j] = hn;
}

// One workgroup per clip: seq = the first index of the largest logit, logprob = max(log_softmax(logit)).
__global__ __launch_bounds__(256) void bah_train_pick_kernel(const float* logit, long ldl, int V, int64_t* seq,
                                                             float* logprob, long ld_out) {
  __shared__ float s_red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* lg = logit + (size_t)b * ldl;
  float best = -INFINITY;
  int bi = V;
  for (int v = tid; v < V; v += 256) {
    const float x = lg[v];
    if (x > best) { best = x; bi = v; }
  }
  const float m = block_max256(best, s_red);
  // the smallest index that holds the maximum (indices below 2^24 are exact in f32)
  float c = (best == m && bi < V) ? -(float)bi : -INFINITY;
  c = block_max256(c, s_red);
  float sum = 0.f;
  for (int v = tid; v < V; v += 256) sum += expf(lg[v] - m);
  sum = block_sum256(sum, s_red);
  if (tid == 0) {
    seq[(size_t)b * ld_out] = c > -INFINITY ? (int64_t)(-c) : 0;
    logprob[(size_t)b * ld_out] = -logf(sum);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
struct TGateBP {
  const float *dhc; long ld_dhc;        // clip b's d(loss)/d(h_{t+1}) through the classifier at dhc + b * ld_dhc
  const float *gates, *hn; long ld_hn;  // [B][3d]; clip b's W_hn h + b_hn at hn + b * ld_hn
  const float* h_in;                    // [B][d]
  float *dh, *dgi, *dgh;                // [B][d] (in: the carry, out: z dh), [B][3d] x 2
  int B, d;
};

// h' = (1 - z) n + z h, n = tanh(i_n + r hn), r = sigmoid(i_r + h_r), z = sigmoid(i_z + h_z)
__global__ __launch_bounds__(256) void bah_train_gate_bwd_kernel(TGateBP p) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)p.B * p.d) return;
  const int b = (int)(i / p.d), j = (int)(i % p.d), d = p.d;
  const float* g = p.gates + (size_t)b * 3 * d;
  const float r = g[j], z = g[d + j], n = g[2 * d + j];
  const float hn = p.hn[(size_t)b * p.ld_hn + j];
  const float h = p.h_in[i];
  const float dh = p.dh[i] + p.dhc[(size_t)b * p.ld_dhc + j];
  const float dn_pre = dh * (1.0f - z) * (1.0f - n * n);
  const float dz_pre = dh * (h - n) * z * (1.0f - z);
  const float dr_pre = dn_pre * hn * r * (1.0f - r);
  float* dgi = p.dgi + (size_t)b * 3 * d;
  float* dgh = p.dgh + (size_t)b * 3 * d;
  dgi[j] = dr_pre;
  dgi[d + j] = dz_pre;
  dgi[2 * d + j] = dn_pre;
  dgh[j] = dr_pre;
  dgh[d + j] = dz_pre;
  dgh[2 * d + j] = dn_pre * r;
  p.dh[i] = dh * z;
}

struct TAttnBP {
  const float* hg; long ld_hg;                   // clip b's W_h h_t
  const float *ek, *attn_emb, *v, *w;            // [B][Tm][S], [B][Tm][A], [S], the step's [B][Tm]
  const float* dctx; long ld_dctx;               // clip b's d(loss)/d(context) at dctx + b * ld_dctx, A values
  const int* mem_len;
  float *dq, *dv;                                // the step's [B][S]
  float *d_attn_emb, *dek;                       // [B][Tm][A], [B][Tm][S]: accumulated over the steps
  int Tm, S, A;
};

// One workgroup per clip.  Frames at or beyond the clip's length are never touched: their gradients stay the zeros the
// buffers were cleared to.  (A clip of length 0 attends uniformly to all Tm frames through the -1e10 fill, which passes no
// gradient to the scores: only d attn_emb gets its share.)
__global__ __launch_bounds__(256) void bah_train_attn_bwd_kernel(TAttnBP p) {
  __shared__ float s_q[BAH_MAX_DIM];
  __shared__ float s_v[BAH_MAX_DIM];
  __shared__ float s_dc[BAH_MAX_DIM];
  __shared__ float s_ds[BAH_MAX_TM];
  __shared__ float s_acc[4][BAH_MAX_DIM];
  __shared__ float s_red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = clamp_len(p.mem_len[b], p.Tm);
  const int nt = len > 0 ? len : p.Tm;
  for (int a = tid; a < p.S; a += 256) {
    s_q[a] = p.hg[(size_t)b * p.ld_hg + a];
    s_v[a] = p.v[a];
  }
  for (int c = tid; c < p.A; c += 256) s_dc[c] = p.dctx[(size_t)b * p.ld_dctx + c];
  __syncthreads();
  const float* wrow = p.w + (size_t)b * p.Tm;
  const float* mem = p.attn_emb + (size_t)b * p.Tm * p.A;
  float* dmem = p.d_attn_emb + (size_t)b * p.Tm * p.A;
  // c = sum_tm w_tm attn_emb[tm]:  dw_tm = dctx . attn_emb[tm],  d attn_emb[tm] += w_tm dctx
  for (int tm = wave; tm < nt; tm += 4) {
    const float wt = wrow[tm];
    float acc = 0.f;
    for (int c = lane; c < p.A; c += 64) {
      const size_t o = (size_t)tm * p.A + c;
      acc = fmaf(s_dc[c], mem[o], acc);
      dmem[o] = fmaf(wt, s_dc[c], dmem[o]);
    }
    acc = wave_sum(acc);
    if (lane == 0) s_ds[tm] = acc;
  }
  __syncthreads();
  // softmax backward over the valid frames: dscore_tm = w_tm (dw_tm - sum_k w_k dw_k)
  float part = 0.f;
  for (int tm = tid; tm < nt; tm += 256) part = fmaf(wrow[tm], s_ds[tm], part);
  const float dot = block_sum256(part, s_red);
  for (int tm = tid; tm < nt; tm += 256) s_ds[tm] = len > 0 ? wrow[tm] * (s_ds[tm] - dot) : 0.f;
  __syncthreads();
  // score_tm = sum_a v_a tanh(q_a + ek[tm][a]), tanh recomputed; a lane owns columns lane, lane + 64, ...
  float u[BAH_KMAX], dvv[BAH_KMAX];
#pragma unroll
  for (int k = 0; k < BAH_KMAX; ++k) u[k] = dvv[k] = 0.f;
  const float* ek = p.ek + (size_t)b * p.Tm * p.S;
  float* dek = p.dek + (size_t)b * p.Tm * p.S;
  for (int tm = wave; tm < len; tm += 4) {
    const float ds = s_ds[tm];
#pragma unroll
    for (int k = 0; k < BAH_KMAX; ++k) {
      const int a = lane + 64 * k;
      if (a < p.S) {
        const size_t o = (size_t)tm * p.S + a;
        const float th = tanhf(s_q[a] + ek[o]);
        const float g = ds * (1.0f - th * th);
        u[k] += g;
        dvv[k] = fmaf(ds, th, dvv[k]);
        dek[o] = fmaf(g, s_v[a], dek[o]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < BAH_KMAX; ++k) {
    const int a = lane + 64 * k;
    if (a < p.S) s_acc[wave][a] = u[k];
  }
  __syncthreads();
  for (int a = tid; a < p.S; a += 256)
    p.dq[(size_t)b * p.S + a] = s_v[a] * ((s_acc[0][a] + s_acc[1][a]) + (s_acc[2][a] + s_acc[3][a]));
  __syncthreads();
#pragma unroll
  for (int k = 0; k < BAH_KMAX; ++k) {
    const int a = lane + 64 * k;
    if (a < p.S) s_acc[wave][a] = dvv[k];
  }
  __syncthreads();
  for (int a = tid; a < p.S; a += 256)
    p.dv[(size_t)b * p.S + a] = (s_acc[0][a] + s_acc[1][a]) + (s_acc[2][a] + s_acc[3][a]);
}

// d(word_embedding) / d(temporal_embedding) += dxin[:, :E] * in_dropout's mask, row (step, clip) into the row of its input
__global__ __launch_bounds__(256) void bah_train_embed_bwd_kernel(const float* dxin, const int* tok, float* demb, float* dtemb,
                                                                  long rows, int E, long ld_dxin, Drop drop) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= rows * E) return;
  const long row = i / E;
  const int e = (int)(i % E);
  const int code = tok[row];
  float* dst = code < 0 ? dtemb + (size_t)(-1 - code) * E : demb + (size_t)code * E;
  atomicAdd(dst + e, dxin[(size_t)row * ld_dxin + e] * drop.mask((uint64_t)i));
}

// backward of fc_emb = mean over the valid frames of attn_emb[:, :, :F]
__global__ __launch_bounds__(256) void bah_mean_lens_bwd_kernel(const float* d_fc, const int* lens, float* d_attn, int B,
                                                                int Tm, int A, int F) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)B * Tm * F) return;
  const int c = (int)(i % F);
  const int tm = (int)((i / F) % Tm);
  const int b = (int)(i / ((long)F * Tm));
  const int len = clamp_len(lens[b], Tm);
  if (tm < len) d_attn[((size_t)b * Tm + tm) * A + c] += d_fc[(size_t)b * F + c] / (float)len;
}

// dX[M][K] (beta: +)= dY[M][N] W[N][K], exact f32 (the per-step products)
int dx_step(const float* dY, long lddy, const float* W, long ldw, float* dX, long lddx, int M, int N, int K, float beta,
            void* stream) {
  return ac_gemm(dY, lddy, 1, W, ldw, 1, dX, lddx, M, K, N, nullptr, 0, beta, 1, 0.0f, 0ull, nullptr, 0, nullptr, 0, stream);
}

// The same over all rows: slices of a long reduction on separate workgroups when the output has few tiles
int dx_rows(const float* dY, long lddy, const float* W, long ldw, float* dX, long lddx, int M, int N, int K, float beta,
            void* stream) {
  const long tiles = (long)((M + 63) / 64) * ((K + 63) / 64);
  long sk = 1;
  if (tiles < 200) {
    sk = (255 + tiles) / tiles;
    if (sk > N / 256) sk = N / 256;
    if (sk < 1) sk = 1;
  }
  return ac_gemm_bf16x3(dY, lddy, 1, W, ldw, 1, dX, lddx, M, K, N, nullptr, 0, beta, (int)sk, 0.0f, 0ull, nullptr, 0, nullptr,
                        0, stream);
}

// dW[N][K] += dY[rows][N]^T X[rows][K] (split over the rows when the output has few tiles)
int dw_rows(const float* dY, long lddy, const float* X, long ldx, float* dW, long lddw, long rows, int N, int K,
            void* stream) {
  const long blocks = (long)((N + 63) / 64) * ((K + 63) / 64);
  long sk = 512 / (blocks > 0 ? blocks : 1);
  if (sk > rows / 128) sk = rows / 128;
  if (sk < 1) sk = 1;
  return ac_gemm_bf16x3(dY, 1, lddy, X, ldx, 1, dW, lddw, N, K, (int)rows, nullptr, 0, 1.0f, (int)sk, 0.0f, 0ull, nullptr, 0,
                        nullptr, 0, stream);
}

bool train_dims_ok(const ac_bah_weights* w, int B, int Tm, int T, float drop_p) {
  return bah_shape_ok(w) && B > 0 && Tm > 0 && Tm <= BAH_MAX_TM && T > 0 && (long)B * T <= (1L << 24) && drop_p >= 0.f &&
         drop_p < 1.f;
}

bool grads_ok(const ac_bah_weights* w, const ac_bah_grads* g) {
  if (!g || !g->emb || !g->w_ih || !g->w_hh || !g->b_ih || !g->b_hh || !g->attn_w || !g->attn_b || !g->attn_v || !g->fc_w ||
      !g->cls_w || !g->cls_b || (w->n_tags && !g->temb))
    return false;
  // a slot the variant does not use is NULL in the gradient struct as it is in the weight struct
  if (w->variant == BAH_CATFC) return g->fc_b && g->ctx_w && g->ctx_b;
  if (w->variant == BAH_COND) return !g->fc_b && g->ctx_w && g->ctx_b && !g->temb;
  return !g->fc_b && !g->ctx_w && !g->ctx_b && !g->temb;
}

// d condition_embedding.weight [2][E] += [1 - c, c]^T-weighted sum over the clips of d cond_emb [B][E]
__global__ __launch_bounds__(256) void bah_cond_emb_bwd_kernel(const float* cond, const float* dpfc, float* dcw, int B, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float a0 = 0.f, a1 = 0.f;
  for (int b = 0; b < B; ++b) {
    const float c = cond[b], g = dpfc[(size_t)b * E + e];
    a0 = fmaf(1.0f - c, g, a0);
    a1 = fmaf(c, g, a1);
  }
  dcw[e] += a0;
  dcw[E + e] += a1;
}

// d W_ih[:, E + A] (element j at dcol + j * ld) += sum_b c_b dgf[b][j]
__global__ __launch_bounds__(256) void bah_cond_col_bwd_kernel(const float* cond, const float* dgf, float* dcol, long ld,
                                                               int B, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float a = 0.f;
  for (int b = 0; b < B; ++b) a = fmaf(cond[b], dgf[(size_t)b * n + j], a);
  dcol[(size_t)j * ld] += a;
}

#define BAH_TRY(call) do { if ((call) != AC_OK) return AC_ERR_LAUNCH; } while (0)

// What the SCST rollout has in place of the caption and the arg-max pick
struct Rollout {
  int* seq;                          // [B][T] int32: the stored words (ac_scst_pick writes, the next step's word feed reads)
  int* scratch;                      // [2 B]: ac_scst_pick's done and drawn
  const int* forced; long forced_ld; // the caller's words instead of the draws, or null
  const uint64_t* sample_seed_dev;
  float temp;
  int end_idx;
};

// The forward chain of T steps; the arguments have been checked.  ro == null: scheduled sampling on cap / the arg-max.
// `side` is fc_emb [B][F] (BAH_CATFC) or cond [B] (the conditional variants).
int train_forward_steps(const ac_bah_weights* w, const float* attn_emb, const float* side, const int* mem_len,
                        const long long* cap, long cap_ld, const int* use_cap, const int* tags, int B, int Tm, int T,
                        int start_idx, float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev,
                        const int64_t* seq_in, int64_t* seq, const Rollout* ro, float* logit, float* logprob, float* embed,
                        float* attn_weight, float* state, float* ws, void* stream) {
  const int E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim, F = w->fc_emb_dim, V = w->vocab;
  hipStream_t s = (hipStream_t)stream;
  const TrainWs c = train_carve(w, ws, B, Tm, T);
  const long ld_hg = S + 3L * d, xw = bah_xw(w);
  const bool spec = w->variant == BAH_SPEC;
  // once per batch, as ac_bah_memory / ac_bah_memory_cond: the key projection and the fc or condition part of the input gates
  BAH_TRY(gemm(attn_emb, A, w->attn_w + d, d + A, w->attn_b, c.ek, S, B * Tm, S, A, stream));
  if (w->variant == BAH_CATFC) {
    BAH_TRY(gemm(side, F, w->fc_w, F, w->fc_b, c.pfc, E, B, E, F, stream));
    BAH_TRY(gemm(c.pfc, E, w->w_ih + 2 * E, 3L * E, w->b_ih, c.gf, 3L * d, B, 3 * d, E, stream));
  } else {
    BAH_TRY(bah_cond_gates(w, side, c.pfc, c.gf, B, stream));
  }
  if (hipMemsetAsync(c.h_all, 0, (size_t)B * d * sizeof(float), s) != hipSuccess) return AC_ERR_LAUNCH;
  const Drop drop = make_drop(drop_p, drop_seed, seed_dev);
  for (int t = 0; t < T; ++t) {
    const size_t r0 = (size_t)t * B;
    const float* h_in = c.h_all + r0 * d;
    float* h_out = c.h_all + (r0 + B) * d;
    float* hg = c.hg + r0 * ld_hg;
    float* xin = c.xin + r0 * xw;
    float* ctx = spec ? xin + E : c.ctx + r0 * A;
    const long ld_ctx = spec ? xw : A;
    BAH_TRY(gemm(h_in, d, w->attn_w, d + A, nullptr, hg, ld_hg, B, S, d, stream));
    BAH_TRY(gemm(h_in, d, w->w_hh, d, w->b_hh, hg + S, ld_hg, B, 3 * d, d, stream));
    TAttnP a;
    a.hg = hg; a.ld_hg = ld_hg; a.ek = c.ek; a.attn_emb = attn_emb; a.v = w->attn_v; a.mem_len = mem_len;
    a.emb = w->emb; a.temb = w->temb; a.tags = (t == 0 && w->n_tags) ? tags : nullptr;
    a.cap = cap; a.cap_ld = cap_ld; a.seq = seq_in; a.tok = c.tok + r0;
    a.words = ro ? ro->seq : nullptr; a.words_ld = T;
    a.ctx = ctx; a.ld_ctx = ld_ctx; a.xin = xin; a.ld_xin = xw; a.w = c.w + r0 * Tm; a.attn_out = attn_weight + t; a.drop = drop;
    a.use_cap = ro ? 0 : use_cap[t] != 0; a.t = t; a.T = T; a.B = B; a.start_idx = start_idx;
    a.Tm = Tm; a.S = S; a.A = A; a.E = E; a.V = V; a.n_tags = w->n_tags;
    hipLaunchKernelGGL(bah_train_attn_kernel, dim3(B), dim3(256), 0, s, a);
    BAH_TRY(ac_check_launch());
    if (!spec) BAH_TRY(gemm(ctx, A, w->ctx_w, A, w->ctx_b, xin + E, xw, B, E, A, stream));
    BAH_TRY(gemm(xin, xw, w->w_ih, bah_ld_ih(w), nullptr, c.gi, 3L * d, B, 3 * d, (int)xw, stream));
    TGateP g;
    g.gi = c.gi; g.gf = c.gf; g.hg = hg + S; g.ld_hg = ld_hg; g.h_in = h_in; g.h_out = h_out;
    g.gates = c.gates + r0 * 3 * d; g.embed_ws = c.embed + (size_t)t * d; g.embed_out = embed + (size_t)t * d;
    g.B = B; g.d = d; g.T = T;
    hipLaunchKernelGGL(bah_train_gate_kernel, dim3((unsigned)(((long)B * d + 255) / 256)), dim3(256), 0, s, g);
    BAH_TRY(ac_check_launch());
    BAH_TRY(gemm(h_out, d, w->cls_w, d, w->cls_b, logit + (size_t)t * V, (long)T * V, B, V, d, stream));
    if (ro) {
      BAH_TRY(ac_scst_pick(logit + (size_t)t * V, (long)T * V, B, V, ro->temp, ro->sample_seed_dev, t, ro->end_idx, ro->forced,
                           ro->forced_ld, ro->scratch, ro->scratch + B, ro->seq, T, logprob, T, stream));
    } else {
      hipLaunchKernelGGL(bah_train_pick_kernel, dim3(B), dim3(256), 0, s, logit + (size_t)t * V, (long)T * V, V, seq + t,
                         logprob + t, (long)T);
      BAH_TRY(ac_check_launch());
    }
  }
  if (hipMemcpyAsync(state, c.h_all + (size_t)T * B * d, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, s) !=
      hipSuccess)
    return AC_ERR_LAUNCH;
  return AC_OK;
}

// The backward through time; `side` as in train_forward_steps.
int train_backward_steps(const ac_bah_weights* w, const ac_bah_grads* g, const float* attn_emb, const float* side,
                         const int* mem_len, const float* dlogit, int B, int Tm, int T, float drop_p,
                         unsigned long long drop_seed, const unsigned long long* seed_dev, float* d_attn_emb,
                         float* d_fc_emb, float* ws, void* stream) {
  if (!train_dims_ok(w, B, Tm, T, drop_p) || !grads_ok(w, g) || !attn_emb || !side || !mem_len || !dlogit ||
      !d_attn_emb || !d_fc_emb || !ws)
    return AC_ERR_ARG;
  const int E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim, F = w->fc_emb_dim, V = w->vocab;
  hipStream_t s = (hipStream_t)stream;
  const TrainWs c = train_carve(w, ws, B, Tm, T);
  const long ld_hg = S + 3L * d, R = (long)T * B, xw = bah_xw(w), ld_ih = bah_ld_ih(w);
  const bool spec = w->variant == BAH_SPEC;
  const long ld_gih = spec ? xw + 1 : ld_ih;     // the row pitch of the weight_ih_l0 gradient: the parameter's own
  // the classifier's input gradient for every (clip, step) at once, in dlogit's (clip, step) row order
  BAH_TRY(dx_rows(dlogit, V, w->cls_w, d, c.dhc, d, (int)R, V, d, 0.0f, stream));
  if (hipMemsetAsync(c.dh, 0, (size_t)B * d * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(c.dek, 0, (size_t)B * Tm * S * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(d_attn_emb, 0, (size_t)B * Tm * A * sizeof(float), s) != hipSuccess)
    return AC_ERR_LAUNCH;
  for (int t = T - 1; t >= 0; --t) {
    const size_t r0 = (size_t)t * B;
    const float* hg = c.hg + r0 * ld_hg;
    float* dgi = c.dgi + r0 * 3 * d;
    float* dgh = c.dgh + r0 * 3 * d;
    float* dxin = c.dxin + r0 * xw;
    float* dq = c.dq + r0 * S;
    TGateBP gb;
    gb.dhc = c.dhc + (size_t)t * d; gb.ld_dhc = (long)T * d; gb.gates = c.gates + r0 * 3 * d;
    gb.hn = hg + S + 2 * d; gb.ld_hn = ld_hg; gb.h_in = c.h_all + r0 * d; gb.dh = c.dh; gb.dgi = dgi; gb.dgh = dgh;
    gb.B = B; gb.d = d;
    hipLaunchKernelGGL(bah_train_gate_bwd_kernel, dim3((unsigned)(((long)B * d + 255) / 256)), dim3(256), 0, s, gb);
    BAH_TRY(ac_check_launch());
    BAH_TRY(dx_step(dgi, 3L * d, w->w_ih, ld_ih, dxin, xw, B, 3 * d, (int)xw, 0.0f, stream));
    if (!spec) BAH_TRY(dx_step(dxin + E, xw, w->ctx_w, A, c.dctx, A, B, E, A, 0.0f, stream));
    TAttnBP ab;
    ab.hg = hg; ab.ld_hg = ld_hg; ab.ek = c.ek; ab.attn_emb = attn_emb; ab.v = w->attn_v; ab.w = c.w + r0 * Tm;
    ab.dctx = spec ? dxin + E : c.dctx; ab.ld_dctx = spec ? xw : A; ab.mem_len = mem_len; ab.dq = dq; ab.dv = c.dv + r0 * S; ab.d_attn_emb = d_attn_emb; ab.dek = c.dek;
    ab.Tm = Tm; ab.S = S; ab.A = A;
    hipLaunchKernelGGL(bah_train_attn_bwd_kernel, dim3(B), dim3(256), 0, s, ab);
    BAH_TRY(ac_check_launch());
    if (t > 0) {   // h_0 is the constant zero state
      BAH_TRY(dx_step(dq, S, w->attn_w, d + A, c.dh, d, B, S, d, 1.0f, stream));
      BAH_TRY(dx_step(dgh, 3L * d, w->w_hh, d, c.dh, d, B, 3 * d, d, 1.0f, stream));
    }
  }
  // ---- everything off the recurrence, over all T B rows ----
  // classifier
  BAH_TRY(dw_rows(dlogit, V, c.embed, d, g->cls_w, d, R, V, d, stream));
  BAH_TRY(ac_colsum(dlogit, V, g->cls_b, R, V, stream));
  // GRU: W_hh, b_hh; the embedding and context columns of W_ih
  BAH_TRY(dw_rows(c.dgh, 3L * d, c.h_all, d, g->w_hh, d, R, 3 * d, d, stream));
  BAH_TRY(ac_colsum(c.dgh, 3L * d, g->b_hh, R, 3 * d, stream));
  BAH_TRY(dw_rows(c.dgi, 3L * d, c.xin, xw, g->w_ih, ld_gih, R, 3 * d, (int)xw, stream));
  if (!spec) {   // ctx_proj
    BAH_TRY(dw_rows(c.dxin + E, xw, c.ctx, A, g->ctx_w, A, R, E, A, stream));
    BAH_TRY(ac_colsum(c.dxin + E, xw, g->ctx_b, R, E, stream));
  }
  // attention: the decoder-state columns of h2attn, v
  BAH_TRY(dw_rows(c.dq, S, c.h_all, d, g->attn_w, d + A, R, S, d, stream));
  BAH_TRY(ac_colsum(c.dv, S, g->attn_v, R, S, stream));
  // the key projection: the encoder columns of h2attn, its bias, d attn_emb += dek W_enc
  BAH_TRY(dw_rows(c.dek, S, attn_emb, A, g->attn_w + d, d + A, (long)B * Tm, S, A, stream));
  BAH_TRY(ac_colsum(c.dek, S, g->attn_b, (long)B * Tm, S, stream));
  BAH_TRY(dx_rows(c.dek, S, w->attn_w + d, d + A, d_attn_emb, A, B * Tm, S, A, 1.0f, stream));
  // gf (the fc or condition part of the input gates, + b_ih) is shared by the steps: dgf = sum_t dgi[t]
  BAH_TRY(ac_sum_replicas(c.dgi, c.dgf, (long)B * 3 * d, T, stream));
  BAH_TRY(ac_colsum(c.dgf, 3L * d, g->b_ih, B, 3 * d, stream));
  if (spec) {
    hipLaunchKernelGGL(bah_cond_col_bwd_kernel, dim3((3 * d + 255) / 256), dim3(256), 0, s, side, c.dgf, g->fc_w, ld_gih, B,
                       3 * d);
    BAH_TRY(ac_check_launch());
  } else {
    BAH_TRY(dw_rows(c.dgf, 3L * d, c.pfc, E, g->w_ih + 2 * E, 3L * E, B, 3 * d, E, stream));
    BAH_TRY(dx_step(c.dgf, 3L * d, w->w_ih + 2 * E, 3L * E, c.dpfc, E, B, 3 * d, E, 0.0f, stream));
  }
  if (w->variant == BAH_CATFC) {
    BAH_TRY(dw_rows(c.dpfc, E, side, F, g->fc_w, F, B, E, F, stream));
    BAH_TRY(ac_colsum(c.dpfc, E, g->fc_b, B, E, stream));
    BAH_TRY(dx_step(c.dpfc, E, w->fc_w, F, d_fc_emb, F, B, E, F, 0.0f, stream));
  } else {
    if (w->variant == BAH_COND) {
      hipLaunchKernelGGL(bah_cond_emb_bwd_kernel, dim3((E + 255) / 256), dim3(256), 0, s, side, c.dpfc, g->fc_w, B, E);
      BAH_TRY(ac_check_launch());
    }
    if (hipMemsetAsync(d_fc_emb, 0, (size_t)B * F * sizeof(float), s) != hipSuccess) return AC_ERR_LAUNCH;   // never read
  }
  // the embedding tables
  hipLaunchKernelGGL(bah_train_embed_bwd_kernel, dim3((unsigned)((R * E + 255) / 256)), dim3(256), 0, s, c.dxin, c.tok,
                     g->emb, g->temb, R, E, xw, make_drop(drop_p, drop_seed, seed_dev));
  return ac_check_launch();
}

}  // namespace

extern "C" {

long ac_bah_train_workspace_floats(const ac_bah_weights* w, int B, int Tm, int T) {
  if (!train_dims_ok(w, B, Tm, T, 0.f)) return -1;
  return (long)train_carve(w, nullptr, B, Tm, T).total;
}

int ac_bah_train_forward(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, const int* mem_len,
                         const long long* cap, long cap_ld, const int* use_cap, const int* tags, int B, int Tm, int T,
                         int start_idx, float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev,
                         int64_t* seq, float* logit, float* logprob, float* embed, float* attn_weight, float* state,
                         float* ws, void* stream) {
  if (!train_dims_ok(w, B, Tm, T, drop_p) || w->variant != BAH_CATFC || !attn_emb || !fc_emb || !mem_len || !cap ||
      cap_ld < T || !use_cap || !seq || !logit || !logprob || !embed || !attn_weight || !state || !ws ||
      (w->n_tags == 0) != (tags == nullptr))
    return AC_ERR_ARG;
  return train_forward_steps(w, attn_emb, fc_emb, mem_len, cap, cap_ld, use_cap, tags, B, Tm, T, start_idx, drop_p, drop_seed,
                             seed_dev, seq, seq, nullptr, logit, logprob, embed, attn_weight, state, ws, stream);
}

int ac_bah_train_forward_cond(const ac_bah_weights* w, const float* attn_emb, const float* cond, const int* mem_len,
                              const long long* cap, long cap_ld, const int* use_cap, int B, int Tm, int T, int start_idx,
                              float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev, int64_t* seq,
                              float* logit, float* logprob, float* embed, float* attn_weight, float* state, float* ws,
                              void* stream) {
  if (!train_dims_ok(w, B, Tm, T, drop_p) || w->variant == BAH_CATFC || !attn_emb || !cond || !mem_len || !cap ||
      cap_ld < T || !use_cap || !seq || !logit || !logprob || !embed || !attn_weight || !state || !ws)
    return AC_ERR_ARG;
  return train_forward_steps(w, attn_emb, cond, mem_len, cap, cap_ld, use_cap, nullptr, B, Tm, T, start_idx, drop_p, drop_seed,
                             seed_dev, seq, seq, nullptr, logit, logprob, embed, attn_weight, state, ws, stream);
}

int ac_bah_train_rollout(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, const int* mem_len,
                         const int* tags, int B, int Tm, int T, int start_idx, int end_idx, float temp,
                         const uint64_t* sample_seed_dev, const int* forced, long forced_ld, float drop_p,
                         unsigned long long drop_seed, const unsigned long long* seed_dev, int* seq, int* scratch,
                         float* logit, float* logprob, float* embed, float* attn_weight, float* state, float* ws,
                         void* stream) {
  if (T < 1 || !train_dims_ok(w, B, Tm, T, drop_p) || w->variant != BAH_CATFC || !attn_emb || !fc_emb || !mem_len ||
      !sample_seed_dev || !seq || !scratch || !logit || !logprob || !embed || !attn_weight || !state || !ws || !isfinite(temp) || !(temp > 0.f) ||
      (forced && forced_ld < T) || (w->n_tags == 0) != (tags == nullptr) ||
      ac_sample_check(w->vocab, AC_SAMPLE_PLAIN, 0, 1.0f, temp) != AC_OK)
    return AC_ERR_ARG;
  Rollout ro;
  ro.seq = seq; ro.scratch = scratch; ro.forced = forced; ro.forced_ld = forced_ld; ro.sample_seed_dev = sample_seed_dev;
  ro.temp = temp; ro.end_idx = end_idx;
  return train_forward_steps(w, attn_emb, fc_emb, mem_len, nullptr, 0, nullptr, tags, B, Tm, T, start_idx, drop_p, drop_seed,
                             seed_dev, nullptr, nullptr, &ro, logit, logprob, embed, attn_weight, state, ws, stream);
}

int ac_bah_train_backward(const ac_bah_weights* w, const ac_bah_grads* g, const float* attn_emb, const float* fc_emb,
                          const int* mem_len, const float* dlogit, int B, int Tm, int T, float drop_p,
                          unsigned long long drop_seed, const unsigned long long* seed_dev, float* d_attn_emb,
                          float* d_fc_emb, float* ws, void* stream) {
  if (!w || w->variant != BAH_CATFC) return AC_ERR_ARG;
  return train_backward_steps(w, g, attn_emb, fc_emb, mem_len, dlogit, B, Tm, T, drop_p, drop_seed, seed_dev, d_attn_emb,
                              d_fc_emb, ws, stream);
}

int ac_bah_train_backward_cond(const ac_bah_weights* w, const ac_bah_grads* g, const float* attn_emb, const float* cond,
                               const int* mem_len, const float* dlogit, int B, int Tm, int T, float drop_p,
                               unsigned long long drop_seed, const unsigned long long* seed_dev, float* d_attn_emb,
                               float* d_fc_emb, float* ws, void* stream) {
  if (!w || w->variant == BAH_CATFC) return AC_ERR_ARG;
  return train_backward_steps(w, g, attn_emb, cond, mem_len, dlogit, B, Tm, T, drop_p, drop_seed, seed_dev, d_attn_emb,
                              d_fc_emb, ws, stream);
}

int ac_bah_mean_lens_bwd(const float* d_fc_emb, const int* lens, float* d_attn_emb, int B, int Tm, int A, int F,
                         void* stream) {
  if (!d_fc_emb || !lens || !d_attn_emb || B <= 0 || Tm <= 0 || A <= 0 || F <= 0 || F > A) return AC_ERR_ARG;
  hipLaunchKernelGGL(bah_mean_lens_bwd_kernel, dim3((unsigned)(((long)B * Tm * F + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, d_fc_emb, lens, d_attn_emb, B, Tm, A, F);
  return ac_check_launch();
}

}  // extern "C"
