// Bahdanau-attention GRU caption decoder (reference captioning/models/rnn_decoder.py BahAttnCatFcDecoder,
// hf_wrapper.py:1377-1554 Seq2SeqAttention / TemporalBahAttnDecoder) for inference on gfx950.
//
// One decoder step over R rows is a short chain of ordinary launches.  Every projection runs on 64-row tiles through the
// exact-f32 MFMA GEMM of csrc/train.hip (ac_gemm: v_mfma_f32_32x32x2_f32, each weight read once per tile of rows); the
// per-row work is fused around them:
//
//   hg  = h [W_h ; W_hh]^T + [0 ; b_hh]         two GEMMs into one [R][S + 3d] buffer (they share their input rows)
//   bah_attn_kernel   row r: score_t = v . tanh(hg[r][:S] + ek[clip][t]), -1e10 at t >= len, softmax, the context
//                     c = sum_t w_t attn_emb[clip][t], and the row's input embedding (word, or the tag at t == 0)
//   xin[:, E:2E] = c ctx_proj^T + b             GEMM
//   gi  = xin W_ih[:, :2E]^T                    GEMM
//   bah_gate_kernel   GRU cell (gates r, z, n) on gi + gf[clip] and hg[r][S:]: the new state, the `embed` row
//   logit = h' classifier^T + b                 GEMM
//
// ek (the key projection W_enc attn_emb + b_attn) and gf (the fc part of the input gates, W_ih[:, 2E:3E] fc_proj(fc_emb) +
// b_ih) do not depend on the step: ac_bah_memory computes them once per batch.  No other algebraic fold is used.
// tanhf / expf are the accurate library forms; no cross-workgroup waits anywhere.
//
// The condition-controlled decoders (ConditionalBahAttnDecoder rnn_decoder.py:276-336, SpecificityBahAttnDecoder :519-575)
// are the same chain under ac_bah_weights.variant (ac_bah.h); one float per clip, cond, takes fc_emb's place and
// ac_bah_memory_cond computes their gf:
//   BAH_COND   gf = W_ih[:, 2E:3E] ((1 - cond) W_c[0] + cond W_c[1]) + b_ih; the step is unchanged
//   BAH_SPEC   xin = [embed | c] is [R][E + A]: the attention kernel writes the context straight into it, there is no
//              ctx_proj product, gi = xin W_ih[:, :E+A]^T, and gf = cond W_ih[:, E+A] + b_ih.
// weight_ih_l0 of BAH_SPEC has the odd row pitch E + A + 1, which would put the gi product on ac_gemm's unaligned general
// kernel.  The host therefore repacks it whenever it rebuilds the struct (rnn_decoder.py weights()): w_ih is an aligned
// [3d][E + A] block and fc_w the [3d] last column.  The training backward writes the gradient into the parameter's real
// layout (ac_gemm's C stores are scalar, any ldc).
#include "ac_bah.h"

namespace {

// The workspace, in floats: the once-per-batch part (ek, gf), the per-step buffers, the buffers of a whole search.
struct BahWs {
  float *ek, *pfc, *gf;          // [B*Tm][S], [B][E], [B][3d]
  float *hg, *ctx, *xin, *gi;    // [R][S + 3d], [R][A], [R][bah_xw], [R][3d]
  float* state[2];               // [R][d] each
  int *tok, *unfinished;         // [R][max_len + 1], [R]
  unsigned char* mask;           // [R][max_len + 1]
  size_t total;
};

BahWs bah_carve(const ac_bah_weights* w, float* base, int B, int R, int Tm, int max_len) {
  const size_t E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim;
  BahWs s;
  size_t o = 0;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += up4(n); return p; };
  s.ek = take((size_t)B * Tm * S);
  s.pfc = take((size_t)B * E);
  s.gf = take((size_t)B * 3 * d);
  s.hg = take((size_t)R * (S + 3 * d));
  s.ctx = take((size_t)R * A);
  s.xin = take((size_t)R * bah_xw(w));
  s.gi = take((size_t)R * 3 * d);
  s.state[0] = take((size_t)R * d);
  s.state[1] = take((size_t)R * d);
  s.tok = (int*)take((size_t)R * (max_len + 1));
  s.unfinished = (int*)take((size_t)R);
  s.mask = (unsigned char*)take(((size_t)R * (max_len + 1) + 3) / 4);
  s.total = o;
  return s;
}

struct AttnP {
  const float *hg; long ld_hg;       // row r's W_h h at hg + r * ld_hg, S values
  const float *ek, *attn_emb, *v;    // [B][Tm][S], [B][Tm][A], [S]
  const int* mem_len;                // [B]
  const float *emb, *temb;           // [V][E], [n_tags][E]
  const int* words; long word_stride;
  const int* tags;                   // [B] or null
  const int* stop;                   // null, or a word that reads 0 once the search is over
  float *ctx; long ld_ctx;           // row r's context at ctx + r * ld_ctx, A values
  float *xin; long ld_xin;           // row r's input embedding at xin + r * ld_xin, E values
  float* attn_out; long attn_row, attn_frame;   // weight of (row r, frame t) at attn_out + r * attn_row + t * attn_frame
  int row_div, Tm, S, A, E, V, n_tags;
};

// One workgroup per row: scores, mask, softmax, context, and the row's input embedding.
__global__ __launch_bounds__(256) void bah_attn_kernel(AttnP p) {
  __shared__ float s_q[BAH_MAX_DIM];
  __shared__ float s_v[BAH_MAX_DIM];
  __shared__ float s_w[BAH_MAX_TM];
  __shared__ float s_red[4];
  if (p.stop && *p.stop == 0) return;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int clip = r / p.row_div;
  int len = p.mem_len[clip];
  len = len < 0 ? 0 : (len > p.Tm ? p.Tm : len);
  for (int a = tid; a < p.S; a += 256) {
    s_q[a] = p.hg[(size_t)r * p.ld_hg + a];
    s_v[a] = p.v[a];
  }
  // the input embedding of the step: the tag's at t == 0 of a temporal decoder, the previous word's otherwise
  {
    const float* src;
    if (p.tags) {
      int g = p.tags[clip];
      g = g < 0 ? 0 : (g >= p.n_tags ? p.n_tags - 1 : g);
      src = p.temb + (size_t)g * p.E;
    } else {
      int wd = p.words[(size_t)r * p.word_stride];
      wd = wd < 0 ? 0 : (wd >= p.V ? p.V - 1 : wd);
      src = p.emb + (size_t)wd * p.E;
    }
    for (int e = tid; e < p.E; e += 256) p.xin[(size_t)r * p.ld_xin + e] = src[e];
  }
  __syncthreads();
  const float* ek = p.ek + (size_t)clip * p.Tm * p.S;
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
    if (p.attn_out) p.attn_out[(size_t)r * p.attn_row + (size_t)t * p.attn_frame] = wgt;
  }
  __syncthreads();
  // masked frames weigh exactly 0 whenever one frame is valid; with none (len 0) the reference's uniform weights remain
  const int nt = len > 0 ? len : p.Tm;
  const float* mem = p.attn_emb + (size_t)clip * p.Tm * p.A;
  for (int a = tid; a < p.A; a += 256) {
    float acc = 0.f;
    for (int t = 0; t < nt; ++t) acc = fmaf(s_w[t], mem[(size_t)t * p.A + a], acc);
    p.ctx[(size_t)r * p.ld_ctx + a] = acc;
  }
}

struct GateP {
  const float *gi, *gf, *hg; long ld_hg;   // gi [R][3d]; gf [B][3d]; row r's W_hh h + b_hh at hg + r * ld_hg
  const float* h_in; float* h_out;         // [R][d]
  float* embed; long ld_embed;             // may be null
  const int* stop;
  int R, d, row_div;
};

// torch.nn.GRU's cell, gate order r, z, n:  n = tanh(i_n + r * h_n),  h' = (1 - z) n + z h
__global__ __launch_bounds__(256) void bah_gate_kernel(GateP p) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)p.R * p.d) return;
  const int r = (int)(i / p.d), j = (int)(i % p.d);
  const float h = p.h_in[i];
  if (p.stop && *p.stop == 0) {   // the search is over: the state stays what the last executed step left
    p.h_out[i] = h;
    return;
  }
  const float* gi = p.gi + (size_t)r * 3 * p.d;
  const float* gf = p.gf + (size_t)(r / p.row_div) * 3 * p.d;
  const float* gh = p.hg + (size_t)r * p.ld_hg;
  const float rg = ac_sigmoid_exact((gi[j] + gf[j]) + gh[j]);
  const float zg = ac_sigmoid_exact((gi[p.d + j] + gf[p.d + j]) + gh[p.d + j]);
  const float ng = tanhf((gi[2 * p.d + j] + gf[2 * p.d + j]) + rg * gh[2 * p.d + j]);
  const float hn = (1.0f - zg) * ng + zg * h;
  p.h_out[i] = hn;
  if (p.embed) p.embed[(size_t)r * p.ld_embed + j] = hn;
}

struct StepIo {
  const float* state_in; float* state_out;
  const int* words; long word_stride; const int* tags; const int* stop;
  float* embed; long ld_embed; float* logit; long ldl;
  float* attn_out; long attn_row, attn_frame;
};

int bah_step(const ac_bah_weights* w, const BahWs& s, const float* attn_emb, const int* mem_len, int R, int row_div, int Tm,
             const StepIo& io, void* stream) {
  const int E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim, V = w->vocab;
  const long ld_hg = S + 3L * d, xw = bah_xw(w);
  const bool spec = w->variant == BAH_SPEC;
  // W_h h (the decoder-state columns of h2attn come first, hf_wrapper.py:1401) and W_hh h + b_hh
  if (gemm(io.state_in, d, w->attn_w, d + A, nullptr, s.hg, ld_hg, R, S, d, stream) != AC_OK) return AC_ERR_LAUNCH;
  if (gemm(io.state_in, d, w->w_hh, d, w->b_hh, s.hg + S, ld_hg, R, 3 * d, d, stream) != AC_OK) return AC_ERR_LAUNCH;
  AttnP a;
  a.hg = s.hg; a.ld_hg = ld_hg; a.ek = s.ek; a.attn_emb = attn_emb; a.v = w->attn_v; a.mem_len = mem_len;
  a.emb = w->emb; a.temb = w->temb; a.words = io.words; a.word_stride = io.word_stride; a.tags = io.tags; a.stop = io.stop;
  a.ctx = spec ? s.xin + E : s.ctx; a.ld_ctx = spec ? xw : A; a.xin = s.xin; a.ld_xin = xw; a.attn_out = io.attn_out; a.attn_row = io.attn_row; a.attn_frame = io.attn_frame;
  a.row_div = row_div; a.Tm = Tm; a.S = S; a.A = A; a.E = E; a.V = V; a.n_tags = w->n_tags;
  hipLaunchKernelGGL(bah_attn_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  if (!spec && gemm(s.ctx, A, w->ctx_w, A, w->ctx_b, s.xin + E, xw, R, E, A, stream) != AC_OK) return AC_ERR_LAUNCH;
  if (gemm(s.xin, xw, w->w_ih, bah_ld_ih(w), nullptr, s.gi, 3L * d, R, 3 * d, (int)xw, stream) != AC_OK) return AC_ERR_LAUNCH;
  GateP g;
  g.gi = s.gi; g.gf = s.gf; g.hg = s.hg + S; g.ld_hg = ld_hg; g.h_in = io.state_in; g.h_out = io.state_out;
  g.embed = io.embed; g.ld_embed = io.ld_embed; g.stop = io.stop; g.R = R; g.d = d; g.row_div = row_div;
  hipLaunchKernelGGL(bah_gate_kernel, dim3((unsigned)(((long)R * d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  return gemm(io.state_out, d, w->cls_w, d, w->cls_b, io.logit, io.ldl, R, V, d, stream);
}

// The start of a search: every row unfinished on <start> with a zero state, the outputs at the values the columns of
// steps that never run keep (seq <end>, everything else 0).
__global__ void bah_init_kernel(int64_t* seq, float* logprob, int* cnt, int* tok, unsigned char* mask, int* unfinished,
                                float* state0, int B, int max_len, int d, int start_idx, int end_idx, int pad_idx) {
  const long n = (long)B * (max_len > d ? max_len : d);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i % B);
    const long c = i / B;
    if (c < max_len) {
      seq[(size_t)b * max_len + c] = end_idx;
      logprob[(size_t)b * max_len + c] = 0.f;
      if (b == 0) cnt[c] = 0;
    }
    if (c < d) state0[(size_t)b * d + c] = 0.f;
    if (c == 0) {
      tok[(size_t)b * (max_len + 1)] = start_idx;
      mask[(size_t)b * (max_len + 1)] = start_idx == pad_idx ? 1 : 0;
      unfinished[b] = 1;
    }
  }
}

// The end of a search: position (b, t) is dead when row b emitted <end> before step t (all rows have once the search has
// stopped) - its logit, embed and attention columns and its stored value read 0.  Block (b, t).
__global__ __launch_bounds__(256) void bah_finish_kernel(const int64_t* seq, float* logit, float* logprob, float* embed,
                                                         float* attn, const float* state_last, float* state, int max_len,
                                                         int V, int d, int Tm, int end_idx) {
  const int b = blockIdx.x / max_len, t = blockIdx.x % max_len, tid = threadIdx.x;
  if (t == 0)
    for (int j = tid; j < d; j += 256) state[(size_t)b * d + j] = state_last[(size_t)b * d + j];
  bool dead = false;
  for (int c = 0; c < t; ++c) dead |= seq[(size_t)b * max_len + c] == end_idx;
  if (!dead) return;
  float* lg = logit + ((size_t)b * max_len + t) * V;
  for (int j = tid; j < V; j += 256) lg[j] = 0.f;
  for (int j = tid; j < d; j += 256) embed[((size_t)b * max_len + t) * d + j] = 0.f;
  for (int j = tid; j < Tm; j += 256) attn[((size_t)b * Tm + j) * max_len + t] = 0.f;
  if (tid == 0) logprob[(size_t)b * max_len + t] = 0.f;
}

// Beam rows after the selection of step t (hf_wrapper.py:1661,1665-1669): row r takes the state, and the attention history
// with this step's weights as column t, of row src_row[r].  A clip that had retired before the step keeps its history.
__global__ __launch_bounds__(256) void bah_beam_gather_kernel(const int* src_row, const int* active_before,
                                                              const float* state_new, float* state_next,
                                                              const float* step_w, const float* hist_in, float* hist_out,
                                                              int beam, int d, int Tm, int max_len, int t) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool act = active_before[r / beam] != 0;
  const int sr = act ? src_row[r] : r;
  for (int j = tid; j < d; j += 256) state_next[(size_t)r * d + j] = state_new[(size_t)sr * d + j];
  const size_t hs = (size_t)max_len * Tm;
  const float* hin = hist_in + (size_t)sr * hs;
  float* ho = hist_out + (size_t)r * hs;
  for (int i = tid; i < t * Tm; i += 256) ho[i] = hin[i];
  for (int j = tid; j < Tm; j += 256) ho[(size_t)t * Tm + j] = act ? step_w[(size_t)sr * Tm + j] : 0.f;
}

bool search_args_ok(const ac_bah_weights* w, const void* attn_emb, const void* mem_len, const int* tags, int B, int Tm,
                    int max_len, const void* ws) {
  return bah_shape_ok(w) && attn_emb && mem_len && ws && B > 0 && Tm > 0 && Tm <= BAH_MAX_TM && max_len > 0 &&
         (w->n_tags == 0) == (tags == nullptr);
}

// greedy (method < 0) or sampled search of B rows
int bah_search(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, const int* tags, int B, int Tm,
               int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
               float* embed, float* attn_weight, float* state, int* unfinished_cnt, float* ws, int method, int k,
               float top_p, float temp, const uint64_t* seed_dev, void* stream) {
  if (!search_args_ok(w, attn_emb, mem_len, tags, B, Tm, max_len, ws) || !seq || !logit || !logprob || !embed ||
      !attn_weight || !state || !unfinished_cnt)
    return AC_ERR_ARG;
  if (method >= 0 && (ac_sample_check(w->vocab, method, k, top_p, temp) != AC_OK || !seed_dev)) return AC_ERR_ARG;
  const int d = w->d_model, V = w->vocab;
  hipStream_t s = (hipStream_t)stream;
  const BahWs c = bah_carve(w, ws, B, B, Tm, max_len);
  if (hipMemsetAsync(logit, 0, (size_t)B * max_len * V * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(embed, 0, (size_t)B * max_len * d * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(attn_weight, 0, (size_t)B * Tm * max_len * sizeof(float), s) != hipSuccess)
    return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(bah_init_kernel, dim3(64), dim3(256), 0, s, seq, logprob, unfinished_cnt, c.tok, c.mask, c.unfinished,
                     c.state[0], B, max_len, d, start_idx, end_idx, pad_idx);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  const long ld = max_len + 1, ldl = (long)max_len * V;
  for (int t = 0; t < max_len; ++t) {
    StepIo io;
    io.state_in = c.state[t & 1]; io.state_out = c.state[(t + 1) & 1];
    io.words = c.tok + t; io.word_stride = ld; io.tags = t == 0 ? tags : nullptr;
    io.stop = t == 0 ? nullptr : unfinished_cnt + t - 1;
    io.embed = embed + (size_t)t * d; io.ld_embed = (long)max_len * d;
    io.logit = logit + (size_t)t * V; io.ldl = ldl;
    io.attn_out = attn_weight + t; io.attn_row = (long)Tm * max_len; io.attn_frame = max_len;
    int rc = bah_step(w, c, attn_emb, mem_len, B, 1, Tm, io, stream);
    if (rc != AC_OK) return rc;
    if (method < 0) {
      const float* plane[1] = {io.logit};
      rc = ac_ens_greedy_pick(plane, 1, ldl, B, V, t, max_len, end_idx, pad_idx, seq, logprob, c.tok, c.mask, c.unfinished,
                              unfinished_cnt, stream);
    } else {
      SampleParams p = {};
      p.logit = io.logit; p.ldl = ldl; p.rows = B; p.V = V; p.method = method; p.k = k; p.top_p = top_p; p.temp = temp;
      p.seed = seed_dev; p.t = t; p.logprob = logprob + t; p.ld_lp = max_len;
      p.seq = seq; p.max_len = max_len; p.end_idx = end_idx; p.pad_idx = pad_idx;
      p.tok = c.tok; p.mask = c.mask; p.unfinished = c.unfinished; p.cnt = unfinished_cnt;
      rc = ac_sample_launch(p, s);
    }
    if (rc != AC_OK) return rc;
  }
  hipLaunchKernelGGL(bah_finish_kernel, dim3(B * max_len), dim3(256), 0, s, seq, logit, logprob, embed, attn_weight,
                     c.state[max_len & 1], state, max_len, V, d, Tm, end_idx);
  return ac_check_launch();
}

}  // namespace

extern "C" {

long ac_bah_workspace_floats(const ac_bah_weights* w, int B, int R, int Tm, int max_len) {
  if (!bah_shape_ok(w) || B <= 0 || R < B || Tm <= 0 || Tm > BAH_MAX_TM || max_len <= 0) return -1;
  return (long)bah_carve(w, nullptr, B, R, Tm, max_len).total;
}

int ac_bah_memory(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, int B, int R, int Tm, int max_len,
                  float* ws, void* stream) {
  if (!bah_shape_ok(w) || w->variant != BAH_CATFC || !attn_emb || !fc_emb || !ws || B <= 0 || R < B || Tm <= 0 ||
      Tm > BAH_MAX_TM || max_len <= 0)
    return AC_ERR_ARG;
  const int E = w->emb_dim, d = w->d_model, S = w->attn_size, A = w->attn_emb_dim, F = w->fc_emb_dim;
  const BahWs c = bah_carve(w, ws, B, R, Tm, max_len);
  // the encoder-frame columns of h2attn follow the d_model decoder-state columns (hf_wrapper.py:1401)
  if (gemm(attn_emb, A, w->attn_w + d, d + A, w->attn_b, c.ek, S, B * Tm, S, A, stream) != AC_OK) return AC_ERR_LAUNCH;
  if (gemm(fc_emb, F, w->fc_w, F, w->fc_b, c.pfc, E, B, E, F, stream) != AC_OK) return AC_ERR_LAUNCH;
  return gemm(c.pfc, E, w->w_ih + 2 * E, 3L * E, w->b_ih, c.gf, 3L * d, B, 3 * d, E, stream);
}

int ac_bah_memory_cond(const ac_bah_weights* w, const float* attn_emb, const float* cond, int B, int R, int Tm, int max_len,
                       float* ws, void* stream) {
  if (!bah_shape_ok(w) || w->variant == BAH_CATFC || !attn_emb || !cond || !ws || B <= 0 || R < B || Tm <= 0 ||
      Tm > BAH_MAX_TM || max_len <= 0)
    return AC_ERR_ARG;
  const int d = w->d_model, S = w->attn_size, A = w->attn_emb_dim;
  const BahWs c = bah_carve(w, ws, B, R, Tm, max_len);
  if (gemm(attn_emb, A, w->attn_w + d, d + A, w->attn_b, c.ek, S, B * Tm, S, A, stream) != AC_OK) return AC_ERR_LAUNCH;
  return bah_cond_gates(w, cond, c.pfc, c.gf, B, stream);
}

int ac_bah_step_logits(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, int B, int R, int row_div,
                       int Tm, int max_len, const float* state_in, const int* words, long word_stride, const int* tags,
                       float* state_out, float* embed, long ld_embed, float* logit, long ldl, float* attn_weight,
                       long attn_row_stride, long attn_frame_stride, float* ws, void* stream) {
  if (!bah_shape_ok(w) || !attn_emb || !mem_len || !ws || B <= 0 || row_div <= 0 || R != B * row_div || Tm <= 0 ||
      Tm > BAH_MAX_TM || max_len <= 0 || !state_in || !state_out || state_in == state_out || !logit || ldl < w->vocab ||
      (!words && !tags) || (tags && !w->n_tags) || (embed && ld_embed < w->d_model))
    return AC_ERR_ARG;
  StepIo io;
  io.state_in = state_in; io.state_out = state_out; io.words = words; io.word_stride = word_stride; io.tags = tags;
  io.stop = nullptr; io.embed = embed; io.ld_embed = ld_embed; io.logit = logit; io.ldl = ldl;
  io.attn_out = attn_weight; io.attn_row = attn_row_stride; io.attn_frame = attn_frame_stride;
  return bah_step(w, bah_carve(w, ws, B, R, Tm, max_len), attn_emb, mem_len, R, row_div, Tm, io, stream);
}

int ac_bah_greedy(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, const int* tags, int B, int Tm,
                  int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, float* attn_weight, float* state, int* unfinished_cnt, float* ws, void* stream) {
  return bah_search(w, attn_emb, mem_len, tags, B, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    attn_weight, state, unfinished_cnt, ws, -1, 0, 0.f, 1.f, nullptr, stream);
}

int ac_bah_sample(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, const int* tags, int B, int Tm,
                  int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, float* attn_weight, float* state, int* unfinished_cnt, float* ws, int method, int k,
                  float top_p, float temp, const uint64_t* seed_dev, void* stream) {
  if (method < 0) return AC_ERR_ARG;
  return bah_search(w, attn_emb, mem_len, tags, B, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    attn_weight, state, unfinished_cnt, ws, method, k, top_p, temp, seed_dev, stream);
}

int ac_bah_beam_gather(const int* src_row, const int* active_before, const float* state_new, float* state_next,
                       const float* step_weight, const float* hist_in, float* hist_out, int B, int beam, int d, int Tm,
                       int max_len, int t, void* stream) {
  if (!src_row || !active_before || !state_new || !state_next || state_new == state_next || !step_weight || !hist_in ||
      !hist_out || hist_in == hist_out || B <= 0 || beam <= 0 || d <= 0 || Tm <= 0 || max_len <= 0 || t < 0 || t >= max_len)
    return AC_ERR_ARG;
  hipLaunchKernelGGL(bah_beam_gather_kernel, dim3(B * beam), dim3(256), 0, (hipStream_t)stream, src_row, active_before,
                     state_new, state_next, step_weight, hist_in, hist_out, beam, d, Tm, max_len, t);
  return ac_check_launch();
}

}  // extern "C"
