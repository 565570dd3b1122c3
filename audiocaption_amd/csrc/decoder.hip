// Autoregressive Transformer decoder on gfx950: memory preparation, the per-position decoder step with
// a self-attention KV cache, on-device greedy search and the device half of beam search.
//
// Replaces reference TransformerDecoder.forward (transformer_decoder.py:80-103), the decode loops
// CaptionModel.stepwise_forward / sample_next_word / beam_search (base.py:152-325) and
// TransformerModel.prepare_decoder_input (transformer_model.py:34-86).
//
// What is different from the reference's schedule (results are the same function of the inputs):
//  * the reference re-runs the decoder on the WHOLE prefix every step and recomputes attn_proj and
//    the cross-attention K/V projections of the audio memory on every call; here the memory side is
//    computed once per batch (ac_trm_memory) and each step processes only the new position against
//    cached self-attention K/V (the causal mask makes position t independent of later tokens);
//  * the greedy loop never returns to the host: argmax, log-prob, <end> bookkeeping and the
//    "every clip finished" test live in one kernel per step, so a whole decode is a fixed launch
//    sequence on one stream.  The reference leaves its loop once every clip of the batch has finished;
//    here the launches of the remaining steps stay in the sequence and their workgroups return at once
//    (struct Live), per batch when several batches share the chain.
// Projections run on the f32 matrix cores through ac_linear; softmax / LayerNorm reductions are
// 64-lane wavefront shuffles.
#include "ac_common.h"
#include "ac_logit_rules.h"
#include "ac_sample.h"
#include "ac_beam.h"
#include "../../include/audiocaption_hip.h"
#include <stdlib.h>
#include <string.h>

extern "C" int ac_linear(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K,
                         long ldx, long ldw, long ldy, int relu, void* stream);
// csrc/decoder_wide.hip: the projections of a step over >= AUDIOCAPTION_DEC_WIDE_MIN rows
extern "C" long ac_dec_wide_packed_floats(int N, int K);
extern "C" int ac_dec_wide_pack(const float* W, long ldw, int N, int K, float* out, void* stream);
extern "C" int ac_dec_wide_gemm(int producer, const float* X, long ldx, const float* Y2, long ldy2, const float* ln_w,
                                const float* ln_b, const int* tok, long tok_stride, int t, const float* emb, const float* pe,
                                float emb_scale, float* xout, long ldxo, const float* Wp, const float* bias, float* Y, long ldy,
                                int M, int N, int K, int relu, int ntb, int split_out, void* stream);

// DEC_REGCAP: registers per lane the decode chain's kernels may use (development switch: -DDEC_REGCAP=64 builds them to fit
// beside a one-wave-per-SIMD conv workgroup, which leaves 64 of a SIMD's 512 registers - tools/tax_probe.py)
#ifndef DEC_REGCAP
#define DEC_REGCAP 0
#endif
#if DEC_REGCAP
#define DEC_CAP __attribute__((amdgpu_waves_per_eu(512 / DEC_REGCAP, 8)))
#define DEC_ROW_BOUNDS __launch_bounds__(256) DEC_CAP
#else
#define DEC_CAP
#define DEC_ROW_BOUNDS __launch_bounds__(256, 2)
#endif

namespace {

// Which rows of a step of the on-device search still run.  The rows of a chain are `segments` of seg_rows rows each (the
// batches that share it; a lone batch is one segment), and the reference stops a batch's loop once every row of that batch
// has emitted <end> (base.py:167): row r runs step t iff t == 0 or cnt[r / seg_rows][t - 1] > 0, the number of rows of its
// segment still unfinished after step t - 1 (written by that step's pick, a kernel earlier on the stream).  Per segment,
// never per row: a finished row keeps decoding while its batch runs, as in the reference.  cnt null: every row runs (beam
// search, teacher forcing).
struct Live {
  const int* cnt = nullptr;   // [segments][max_len]
  int seg_rows = 1, max_len = 0, t = 0;
};
__device__ __forceinline__ bool row_live(const Live& L, int r) {
  return !L.cnt || L.t == 0 || L.cnt[(size_t)(r / L.seg_rows) * L.max_len + L.t - 1] > 0;
}
// any of the rows r0 .. r1 - 1: the same answer in every thread of a workgroup that asks about the same rows
__device__ __forceinline__ bool rows_live(const Live& L, int r0, int r1) {
  if (!L.cnt || L.t == 0) return true;
  for (int sg = r0 / L.seg_rows; sg <= (r1 - 1) / L.seg_rows; ++sg)
    if (L.cnt[(size_t)sg * L.max_len + L.t - 1] > 0) return true;
  return false;
}

// ---------------------------------------------------------------------------------------------
// out = LayerNorm(x + y) * w + b, one wave per row
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_layernorm_kernel(const float* x, const float* y, const float* w,
                                                            const float* b, float* out, int rows, int d,
                                                            long ldx, long ldy, long ldo, Live live) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows || !row_live(live, row)) return;   // per wave: the kernel has no barrier
  const float* xr = x + (size_t)row * ldx;
  const float* yr = y ? y + (size_t)row * ldy : nullptr;
  float v[16];  // d <= 1024
  float s = 0.f;
  int n = 0;
  for (int c = lane; c < d; c += 64, ++n) {
    v[n] = xr[c] + (yr ? yr[c] : 0.f);
    s += v[n];
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int i = 0; i < n; ++i) {
    const float dlt = v[i] - mean;
    q = fmaf(dlt, dlt, q);
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)d + 1e-5f);
  n = 0;
  for (int c = lane; c < d; c += 64, ++n) out[(size_t)row * ldo + c] = (v[n] - mean) * rstd * w[c] + b[c];
}

// ---------------------------------------------------------------------------------------------
// Single-query multi-head attention for one decode position.  grid (rows, heads), one wave each.
//   self  : keys 0..t from the KV cache (the new k/v row is appended here), key j masked when
//           key_mask[r][j] != 0                      (tgt_key_padding_mask, transformer_model.py:55)
//   cross : keys 0..Tm-1 of the projected audio memory, key j masked when j >= key_len[r / row_div]
//           (memory_key_padding_mask, transformer_decoder.py:94)
// ---------------------------------------------------------------------------------------------
constexpr int MAX_KEYS = 1024;

struct AttnParams {
  const float* q; long ldq;
  const float* K; const float* V;        // key j of kv-row R at K + R*row_stride + j*key_stride
  long row_stride, key_stride;
  int row_div, nkeys;
  const int* key_len;                     // per kv-row valid length or null
  const unsigned char* key_mask; long mask_stride;  // per row or null
  const float* new_k; const float* new_v; long ld_new;  // appended at key index nkeys-1 when non-null
  float* Kw; float* Vw;                   // writable cache base (same geometry as K/V) for the append
  float* out; long ldo;
  int hd; float scale;
  // wide route (csrc/decoder_wide.hip): the context rows leave as three bf16 planes in MFMA fragment order instead, the A
  // operand of the out-projection launch: pack[row / 32][k step of 16][plane][lane = row % 32 + 32 * (k % 16 / 8)][k % 8]
  unsigned char* out_pk = nullptr; int pk_kst = 0;
  Live live;                              // rows of a finished segment are skipped (dec_row*_kernel take it from here too)
};

__global__ __launch_bounds__(64) DEC_CAP void attn_step_kernel(AttnParams p) {
  __shared__ float sc[MAX_KEYS];
  const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  if (!row_live(p.live, r)) return;   // one row per workgroup: uniform, before any load or barrier
  const int kr = r / p.row_div;
  const bool act = lane < p.hd;
  const size_t hoff = (size_t)h * p.hd;
  // (A skipped step leaves its cache slot unwritten.  No later step reads it: a segment's count stays 0 once it is 0 - no
  // pick of that segment runs again to raise it - so the rows of a skipped step are skipped at every later step too.)
  if (p.new_k && act) {
    const size_t dst = (size_t)kr * p.row_stride + (size_t)(p.nkeys - 1) * p.key_stride + hoff + lane;
    p.Kw[dst] = p.new_k[(size_t)r * p.ld_new + hoff + lane];
    p.Vw[dst] = p.new_v[(size_t)r * p.ld_new + hoff + lane];
  }
  __syncthreads();
  const float* qp = p.q + (size_t)r * p.ldq + hoff;
  const float* Kb = p.K + (size_t)kr * p.row_stride + hoff;
  const float* Vb = p.V + (size_t)kr * p.row_stride + hoff;
  const int klen = p.key_len ? p.key_len[kr] : p.nkeys;
  if (lane < 32 && lane >= p.nkeys) sc[lane] = 0.f;  // the unrolled value loop reads sc[0..31]
  // scores: a wave-instruction covers FOUR keys (16 lanes x 16 bytes = one 256-byte K row each), so a
  // fragment costs 8 cache-line requests; the 4-element partial dots are reduced over the 16-lane groups
  if (p.hd == 64) {
    const int ks = lane >> 4, d4 = lane & 15;
    const f32x4 q4 = *(const f32x4*)(qp + 4 * d4);
#pragma unroll 4
    for (int j0 = 0; j0 < p.nkeys; j0 += 4) {
      const int j = j0 + ks;
      float s = 0.f;
      if (j < p.nkeys) {
        const f32x4 kv = *(const f32x4*)(Kb + (size_t)j * p.key_stride + 4 * d4);
        s = (q4[0] * kv[0] + q4[1] * kv[1]) + (q4[2] * kv[2] + q4[3] * kv[3]);
      }
      s = row16_sum(s);
      if (d4 == 0 && j < p.nkeys) {
        const bool masked = (j >= klen) || (p.key_mask && p.key_mask[(size_t)r * p.mask_stride + j]);
        sc[j] = masked ? -INFINITY : s * p.scale;
      }
    }
  } else {
    for (int j = lane; j < p.nkeys; j += 64) {
      const float* kp = Kb + (size_t)j * p.key_stride;
      float s = 0.f;
      for (int c = 0; c < p.hd; ++c) s = fmaf(qp[c], kp[c], s);
      const bool masked = (j >= klen) || (p.key_mask && p.key_mask[(size_t)r * p.mask_stride + j]);
      sc[j] = masked ? -INFINITY : s * p.scale;
    }
  }
  // the value rows do not depend on the softmax: request them now (coalesced, one row per instruction) so
  // their latency overlaps the score reductions
  constexpr int VPRE = 32;
  float vpre[VPRE];
#pragma unroll
  for (int j = 0; j < VPRE; ++j) vpre[j] = (act && j < p.nkeys) ? Vb[(size_t)j * p.key_stride + lane] : 0.f;
  __syncthreads();
  float m = -INFINITY;
  for (int j = lane; j < p.nkeys; j += 64) m = fmaxf(m, sc[j]);
  m = wave_max(m);
  float den = 0.f;
  for (int j = lane; j < p.nkeys; j += 64) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    den += e;
  }
  den = wave_sum(den);
  __syncthreads();
  if (act) {
    // lane d owns output channel d
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll
    for (int j = 0; j < VPRE; j += 4) {
      o0 = fmaf(sc[j], vpre[j], o0);  // sc[j] = 0 and vpre[j] = 0 beyond nkeys
      o1 = fmaf(sc[j + 1], vpre[j + 1], o1);
      o2 = fmaf(sc[j + 2], vpre[j + 2], o2);
      o3 = fmaf(sc[j + 3], vpre[j + 3], o3);
    }
    for (int j = VPRE; j < p.nkeys; ++j) o0 = fmaf(sc[j], Vb[(size_t)j * p.key_stride + lane], o0);
    const float val = ((o0 + o1) + (o2 + o3)) / den;
    if (p.out_pk) {
      const int c = (int)hoff + lane;
      unsigned short* d = (unsigned short*)(p.out_pk + ((size_t)(r >> 5) * p.pk_kst + (c >> 4)) * 3072 +
                                            (size_t)((r & 31) + 32 * ((c >> 3) & 1)) * 16 + (c & 7) * 2);
      // RNE to bf16, three times over the exact remainders (the split of csrc/decoder_wide.hip, one value at a time)
      auto rne = [](float x) { const unsigned u = __builtin_bit_cast(unsigned, x); return (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u; };
      const unsigned h0 = rne(val);
      const float r1 = val - __builtin_bit_cast(float, h0);
      const unsigned h1 = rne(r1);
      const float r2 = r1 - __builtin_bit_cast(float, h1);
      const unsigned h2 = rne(r2);
      d[0] = (unsigned short)(h0 >> 16);
      d[512] = (unsigned short)(h1 >> 16);
      d[1024] = (unsigned short)(h2 >> 16);
    } else {
      p.out[(size_t)r * p.ldo + hoff + lane] = val;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// One attention sub-layer of a decode step for ONE row per workgroup (d_model 256, 4 heads of 64): everything after the
// QKV projection is row-local, so the four launches attention -> out-projection -> residual + LayerNorm -> next
// projection become one.  Wave h runs head h of the single-query attention (the same code path as attn_step_kernel);
// the 256-float context then stays in LDS; the out-projection is a matrix-vector product against a TRANSPOSED copy of
// the weights (WoT[k][n]: wave w takes k in [64 w, 64 w + 64), lane l the four outputs 4 l .. 4 l + 3, so a wave
// instruction reads one contiguous 1 KiB row and 16 such loads are in flight per lane), reduced over the waves in LDS;
// then the residual join + LayerNorm, and for the self-attention sub-layer the cross-attention query projection of the
// fresh row.  A workgroup streams 256 KiB per projection from L2 (64 workgroups: 16 MB per launch, ~2 us), which
// replaces two 5.5-7 us launches whose cost was launch boundary + first-touch latency, not arithmetic.
// ---------------------------------------------------------------------------------------------
constexpr int ROW_D = 256, ROW_H = 4;

struct RowParams {
  AttnParams a;                          // attention geometry; a.out is unused
  const float* res; long ldres;          // residual input rows
  const float* WoT; const float* bo;     // out-projection, transposed [k][n]
  const float* ln_w; const float* ln_b;
  float* xout; long ldxo;                // LayerNorm(res + attention output)
  const float* WqT; const float* bq;     // optional next projection of the normalised row (self: the cross query)
  float* qout; long ldqo;
};

constexpr int ATT_KPRE = 8, ATT_VPRE = 32;
struct AttnLoads {            // what a wave has requested for one attention phase (one head of one row)
  f32x4 kpre[ATT_KPRE];       // key rows of the first 32 keys: lane (ks = l / 16, d4 = l % 16) holds dims 4 d4 .. + 3 of key 4 i + ks
  float vpre[ATT_VPRE];       // value column `lane` of the first 32 keys
  unsigned char mpre[ATT_KPRE];   // key_mask of those keys (0 without a mask)
  int klen;                   // keys of this row that exist (key_len, or all)
};

// Request everything head h of row r reads from memory - NOT the query: it may not exist yet.  The newest key / value
// (this step's projection, which also goes into the cache for the steps to come) is read from where the projection left it
// instead of being stored, fenced and read back.
__device__ __forceinline__ void attn_issue_k(const AttnParams& p, int r, int h, int lane, f32x4 (&kpre)[ATT_KPRE]) {
  const int kr = r / p.row_div;
  const size_t hoff = (size_t)h * 64;
  const float* Kb = p.K + (size_t)kr * p.row_stride + hoff;
  const float* nk = p.new_k ? p.new_k + (size_t)r * p.ld_new + hoff : nullptr;
  const int newest = p.new_k ? p.nkeys - 1 : -1;
  const int ks = lane >> 4, d4 = lane & 15;
  // branch-free: a key beyond the last one re-reads the last one (its score is never used), so that the number of loads in
  // flight is known to the compiler and a later wait can leave the younger ones in flight
  const int last = p.nkeys - 1;
#pragma unroll
  for (int i = 0; i < ATT_KPRE; ++i) {
    const int j = 4 * i + ks < last ? 4 * i + ks : last;
    const float* src = j == newest ? nk + 4 * d4 : Kb + (size_t)j * p.key_stride + 4 * d4;
    kpre[i] = *(const f32x4*)src;
  }
}

__device__ __forceinline__ void attn_issue_v(const AttnParams& p, int r, int h, int lane, float (&vpre)[ATT_VPRE]) {
  const int kr = r / p.row_div;
  const size_t hoff = (size_t)h * 64;
  const float* Vb = p.V + (size_t)kr * p.row_stride + hoff;
  const float* nk = p.new_k ? p.new_k + (size_t)r * p.ld_new + hoff : nullptr;
  const float* nv = p.new_k ? p.new_v + (size_t)r * p.ld_new + hoff : nullptr;
  const int newest = p.new_k ? p.nkeys - 1 : -1;
  const int last = p.nkeys - 1;
#pragma unroll
  for (int j = 0; j < ATT_VPRE; ++j) {   // branch-free like the keys; columns beyond the last key are zeroed below
    const int jj = j < last ? j : last;
    const float* src = jj == newest ? nv + lane : Vb + (size_t)jj * p.key_stride + lane;
    vpre[j] = *src;
  }
#pragma unroll
  for (int j = 0; j < ATT_VPRE; ++j) vpre[j] = j < p.nkeys ? vpre[j] : 0.f;
  // the cache rows of this step, for the steps to come (nobody in this launch reads them back).  A step skipped for a
  // finished segment (Live) writes none - and none is missed: the segment's count stays 0 from then on, so every later
  // step of these rows is skipped as well and never reads the slots a skipped step left unwritten.
  if (p.new_k) {
    const size_t dst = (size_t)kr * p.row_stride + (size_t)newest * p.key_stride + hoff + lane;
    p.Kw[dst] = nk[lane];
    p.Vw[dst] = nv[lane];
  }
}

__device__ __forceinline__ void attn_issue(const AttnParams& p, int r, int h, int lane, AttnLoads& L) {
  attn_issue_k(p, r, h, lane, L.kpre);
  {   // the mask bytes and the row's key count travel with the keys (they used to be a second round trip inside the score loop)
    const int ks = lane >> 4, last = p.nkeys - 1;
#pragma unroll
    for (int i = 0; i < ATT_KPRE; ++i) {
      const int j = 4 * i + ks < last ? 4 * i + ks : last;
      L.mpre[i] = p.key_mask ? p.key_mask[(size_t)r * p.mask_stride + j] : (unsigned char)0;
    }
    L.klen = p.key_len ? p.key_len[r / p.row_div] : p.nkeys;
  }
  attn_issue_v(p, r, h, lane, L.vpre);
}

// Head h of row r, one wave, from the requested rows; returns output channel `lane` (< 64) of the head.  The arithmetic
// of attn_step_kernel.
__device__ __forceinline__ float attn_compute(const AttnParams& p, int r, int h, int lane, float* sc, const AttnLoads& L) {
  const int kr = r / p.row_div;
  const size_t hoff = (size_t)h * 64;
  const float* qp = p.q + (size_t)r * p.ldq + hoff;
  const float* Kb = p.K + (size_t)kr * p.row_stride + hoff;
  const float* Vb = p.V + (size_t)kr * p.row_stride + hoff;
  const float* nk = p.new_k ? p.new_k + (size_t)r * p.ld_new + hoff : nullptr;
  const float* nv = p.new_k ? p.new_v + (size_t)r * p.ld_new + hoff : nullptr;
  const int newest = p.new_k ? p.nkeys - 1 : -1;
  const int klen = L.klen;
  const int ks = lane >> 4, d4 = lane & 15;
  const f32x4 q4 = *(const f32x4*)(qp + 4 * d4);
  if (lane < 32 && lane >= p.nkeys) sc[lane] = 0.f;
#pragma unroll 4
  for (int j0 = 0; j0 < p.nkeys; j0 += 4) {
    const int j = j0 + ks;
    float s = 0.f;
    unsigned char mk = 0;
    if (j < p.nkeys) {
      f32x4 kv;
      if (j0 < 4 * ATT_KPRE) {
#pragma unroll
        for (int i = 0; i < ATT_KPRE; ++i)
          if (j0 == 4 * i) { kv = L.kpre[i]; mk = L.mpre[i]; }
      } else {
        kv = *(const f32x4*)(j == newest ? nk + 4 * d4 : Kb + (size_t)j * p.key_stride + 4 * d4);
        mk = p.key_mask ? p.key_mask[(size_t)r * p.mask_stride + j] : (unsigned char)0;
      }
      s = (q4[0] * kv[0] + q4[1] * kv[1]) + (q4[2] * kv[2] + q4[3] * kv[3]);
    }
    s = row16_sum(s);
    if (d4 == 0 && j < p.nkeys) {
      const bool masked = (j >= klen) || mk;
      sc[j] = masked ? -INFINITY : s * p.scale;
    }
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = lane; j < p.nkeys; j += 64) m = fmaxf(m, sc[j]);
  m = wave_max(m);
  float den = 0.f;
  for (int j = lane; j < p.nkeys; j += 64) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    den += e;
  }
  den = wave_sum(den);
  __syncthreads();
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll
  for (int j = 0; j < ATT_VPRE; j += 4) {
    o0 = fmaf(sc[j], L.vpre[j], o0);
    o1 = fmaf(sc[j + 1], L.vpre[j + 1], o1);
    o2 = fmaf(sc[j + 2], L.vpre[j + 2], o2);
    o3 = fmaf(sc[j + 3], L.vpre[j + 3], o3);
  }
  for (int j = ATT_VPRE; j < p.nkeys; ++j) o0 = fmaf(sc[j], j == newest ? nv[lane] : Vb[(size_t)j * p.key_stride + lane], o0);
  return ((o0 + o1) + (o2 + o3)) / den;
}

__device__ __forceinline__ float attn_head_row(const AttnParams& p, int r, int h, int lane, float* sc, bool active) {
  (void)active;
  AttnLoads L;
  attn_issue(p, r, h, lane, L);
  return attn_compute(p, r, h, lane, sc, L);
}

// Matrix-vector product against a transposed 256 x 256 matrix, split over the 4 waves of the workgroup: wave w owns
// k in [64 w, 64 w + 64), lane l the outputs 4 l .. 4 l + 3, so a wave instruction reads one contiguous 1 KiB row; 16 rows
// are in flight per lane.  Every thread gets y[tid] = bias[tid] + sum_k WT[k][tid] x[k]; x in LDS, part = [4][256] scratch.
// (Register budget on purpose: in the throughput schedule this kernel has to fit into the slot ONE finished conv
// workgroup leaves on a CU - 4 waves of <= 240 VGPRs.  Variants with 32 + 32 rows in flight over 8 waves, or with the
// rows requested before the attention (256 VGPRs), were ~1 us faster alone and cost the overlapped pipeline 0.7-0.8 ms
// per step, because their workgroups waited for whole CUs.)
__device__ __forceinline__ float row_gemv256(const float* WT, const float* bias, const float* x, float* part, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const f32x4* wp = (const f32x4*)(WT + (size_t)(wave * 64) * ROW_D) + lane;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#if defined(DEC_PK_PROBE)
  // Development (tools/pk_rootcause.py, packed-f32 builds only): the same product with every weight row of a 16-row batch
  // LANDED before the first multiply-add touches it.  DEC_PK_PROBE >= 1: explicit s_waitcnt vmcnt(0) lgkmcnt(0) between the
  // loads and the arithmetic (inline asm: invisible to the compiler's own wait-count pass, which keeps its partial
  // vmcnt(N) waits as well); 2: a workgroup-scope fence on top.
  for (int k0 = 0; k0 < 64; k0 += 16) {
    f32x4 wv[16];
    float xv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      wv[k] = wp[(size_t)(k0 + k) * (ROW_D / 4)];
      xv[k] = x[wave * 64 + k0 + k];
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#if DEC_PK_PROBE == 2
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#endif
#if DEC_PK_PROBE == 3   // 3: sixteen idle issue slots between the landed loads and the first packed multiply-add
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
#endif
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#if DEC_PK_PROBE == 4   // 4: the packed instructions never read a register a LOAD wrote: every row goes through a plain v_mov first
#pragma unroll
      for (int e = 0; e < 4; ++e) asm volatile("v_mov_b32 %0, %1" : "=v"(wv[k][e]) : "v"(wv[k][e]));
      asm volatile("v_mov_b32 %0, %1" : "=v"(xv[k]) : "v"(xv[k]));
#endif
      asm volatile("" : "+v"(wv[k]));   // the arithmetic below cannot be hoisted above the wait
      acc[0] = fmaf(wv[k][0], xv[k], acc[0]);
      acc[1] = fmaf(wv[k][1], xv[k], acc[1]);
      acc[2] = fmaf(wv[k][2], xv[k], acc[2]);
      acc[3] = fmaf(wv[k][3], xv[k], acc[3]);
    }
  }
#else
#pragma unroll 16
  for (int k = 0; k < 64; ++k) {
    const f32x4 wv = wp[(size_t)k * (ROW_D / 4)];
    const float xv = x[wave * 64 + k];
    acc[0] = fmaf(wv[0], xv, acc[0]);
    acc[1] = fmaf(wv[1], xv, acc[1]);
    acc[2] = fmaf(wv[2], xv, acc[2]);
    acc[3] = fmaf(wv[3], xv, acc[3]);
  }
#endif
  *(f32x4*)(part + wave * ROW_D + 4 * lane) = acc;
  __syncthreads();
  const float y = ((part[tid] + part[ROW_D + tid]) + (part[2 * ROW_D + tid] + part[3 * ROW_D + tid])) + (bias ? bias[tid] : 0.f);
  __syncthreads();   // part is reused by the next projection
  return y;
}

#ifdef AC_ROW_STAMPS   // development (tools/row_stamps.py): phase timestamps (100 MHz) of workgroup 0 of dec_row2_kernel
__device__ unsigned long long g_row_stamps[16];
#define ROW_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_row_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int ac_row_stamps_read(unsigned long long* out16) {
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_row_stamps), sizeof(g_row_stamps)) == hipSuccess ? 0 : -2;
}
#else
#define ROW_STAMP(k) do { } while (0)
#endif

__global__ DEC_ROW_BOUNDS void dec_row_kernel(RowParams p) {
  __shared__ float sc[ROW_H][MAX_KEYS];
  __shared__ __attribute__((aligned(16))) float sx[ROW_D];
  __shared__ __attribute__((aligned(16))) float part[4 * ROW_D];
  __shared__ float red[8];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!row_live(p.a.live, r)) return;   // one row per workgroup: uniform, before any load or barrier
  const float resv = p.res[(size_t)r * p.ldres + tid];
  sx[tid] = attn_head_row(p.a, r, wave, lane, sc[wave], true);
  __syncthreads();
  const float v = resv + row_gemv256(p.WoT, p.bo, sx, part, tid);
  // LayerNorm over the 256 values (one per thread)
  const float s1 = wave_sum(v);
  if (lane == 0) red[wave] = s1;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.0f / ROW_D);
  const float dl = v - mean;
  const float s2 = wave_sum(dl * dl);
  if (lane == 0) red[4 + wave] = s2;
  __syncthreads();
  const float rstd = rsqrtf(((red[4] + red[5]) + (red[6] + red[7])) * (1.0f / ROW_D) + 1e-5f);
  const float xn = dl * rstd * p.ln_w[tid] + p.ln_b[tid];
  p.xout[(size_t)r * p.ldxo + tid] = xn;
  if (p.WqT) {
    sx[tid] = xn;
    __syncthreads();
    p.qout[(size_t)r * p.ldqo + tid] = row_gemv256(p.WqT, p.bq, sx, part, tid);
  }
}

// Both attention sub-layers of a decoder layer for one row in ONE launch: self attention -> out-projection -> LN1 -> cross
// query projection (dec_row_kernel with WqT) and then, with the query still in LDS, cross attention -> out-projection ->
// LN2 (dec_row_kernel on the audio memory).  Everything after the QKV projection is row-local, so the second launch only
// bought a kernel boundary and a global round trip of the 256-float query.  The same functions in the same order: the
// same bits as the two launches.
__global__ DEC_ROW_BOUNDS void dec_row2_kernel(RowParams p1, RowParams p2) {
  __shared__ float sc[ROW_H][MAX_KEYS];
  __shared__ __attribute__((aligned(16))) float sx[ROW_D];
  __shared__ __attribute__((aligned(16))) float sq[ROW_D];
  __shared__ __attribute__((aligned(16))) float part[4 * ROW_D];
  __shared__ float red[8];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float xn;
  if (!row_live(p1.a.live, r)) return;   // one row per workgroup: uniform, before any load or barrier
  ROW_STAMP(0);
  const float resv = p1.res[(size_t)r * p1.ldres + tid];
  sx[tid] = attn_head_row(p1.a, r, wave, lane, sc[wave], true);
  // (Requesting the cross attention's rows up here as well - they depend on nothing computed in this kernel - was tried:
  // held in registers they make the compiler serialise the matrix-vector products' loads (2.3 -> 14 us each); parked in
  // LDS the cross phase drops from 4.2 to 1.9 us and the self phase grows by as much, waiting for them to land.)
  {
    __syncthreads();
    ROW_STAMP(1);
    const float v = resv + row_gemv256(p1.WoT, p1.bo, sx, part, tid);
    ROW_STAMP(2);
    const float s1 = wave_sum(v);
    if (lane == 0) red[wave] = s1;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.0f / ROW_D);
    const float dl = v - mean;
    const float s2 = wave_sum(dl * dl);
    if (lane == 0) red[4 + wave] = s2;
    __syncthreads();
    const float rstd = rsqrtf(((red[4] + red[5]) + (red[6] + red[7])) * (1.0f / ROW_D) + 1e-5f);
    xn = dl * rstd * p1.ln_w[tid] + p1.ln_b[tid];
    p1.xout[(size_t)r * p1.ldxo + tid] = xn;
    sx[tid] = xn;
    __syncthreads();
    ROW_STAMP(3);
    sq[tid] = row_gemv256(p1.WqT, p1.bq, sx, part, tid);
    __syncthreads();
    ROW_STAMP(4);
  }
  AttnParams a2 = p2.a;
  a2.q = sq;            // the cross query of this row, still in LDS
  a2.ldq = 0;
  sx[tid] = attn_head_row(a2, r, wave, lane, sc[wave], true);
  __syncthreads();
  ROW_STAMP(5);
  const float v = xn + row_gemv256(p2.WoT, p2.bo, sx, part, tid);
  ROW_STAMP(6);
  const float s1 = wave_sum(v);
  __syncthreads();      // red[] of the first half has been read by every thread
  if (lane == 0) red[wave] = s1;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.0f / ROW_D);
  const float dl = v - mean;
  const float s2 = wave_sum(dl * dl);
  if (lane == 0) red[4 + wave] = s2;
  __syncthreads();
  const float rstd = rsqrtf(((red[4] + red[5]) + (red[6] + red[7])) * (1.0f / ROW_D) + 1e-5f);
  p2.xout[(size_t)r * p2.ldxo + tid] = dl * rstd * p2.ln_w[tid] + p2.ln_b[tid];
  ROW_STAMP(7);
}

// WT[k][n] = W[n][k] for a d x d matrix (rows n of W may be a slice of a taller matrix: ldw)
__global__ void transpose_sq_kernel(const float* W, long ldw, int d, float* WT) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) tile[i][threadIdx.x] = W[(size_t)(by + i) * ldw + bx + threadIdx.x];
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) WT[(size_t)(bx + i) * d + by + threadIdx.x] = tile[threadIdx.x][i];
}

// ---------------------------------------------------------------------------------------------
// Decode-step projection  Y[R, N] = act(A[R, K] W[N, K]^T + bias)  with the producer of A fused in:
//   PRO_PLAIN : A = X                                   (rows of a previous kernel's output)
//   PRO_EMBED : A = E[tok[r][t]] * sqrt(d) + pe[t]       (transformer_decoder.py:89-91)
//   PRO_ADDLN : A = LayerNorm(X + Y2) * g + b            (the post-LN residual join of the previous sub-layer)
//   PRO_EMBED_KW : A = LayerNorm(E[tok[r][t]] * sqrt(d) + kwp[r / kw_div]) * g + b + pe[t]
//                  (KeywordProbTransformerDecoder, transformer_decoder.py:196-202; kwp = keyword_proj(keyword), once per batch)
// For the fused producers the 32-row A tile is built once per block in LDS (K = d_model) and the blocks of
// column tile 0 also write it out (xout): it is the residual stream for the next join / the `embed` output.
// Tile 32 x 32, the four waves split K and reduce through LDS: the step is latency-, not throughput-bound.
// ---------------------------------------------------------------------------------------------
enum { PRO_PLAIN = 0, PRO_EMBED = 1, PRO_ADDLN = 2, PRO_EMBED_KW = 3 };
constexpr int DEC_MAX_D = 512;

struct DecGemmParams {
  const float* X; long ldx;          // PLAIN: A rows; ADDLN: residual input; EMBED_KW: the projected keyword rows kwp
  const float* Y2; long ldy2;        // ADDLN: sub-layer output to add
  const float* ln_w; const float* ln_b;   // ADDLN: the join's norm; EMBED_KW: word_keyword_norm
  int kw_div;                        // EMBED_KW: decoder row r reads kwp row r / kw_div (beam search: B * beam rows over B clips)
  const int* tok; long tok_stride; int t;  // EMBED
  const float* emb; const float* pe; float emb_scale;
  float* xout; long ldxo;            // where column-tile-0 blocks store the produced A rows (may be null)
  const float* Wp; const float* bias;  // Wp: fragment-packed weights [ceil(N/16)][K/16][64][4]
  float* Y; long ldy;
  int M, N, K, relu;
  int ntb;  // consecutive 16-column tiles per block (1 unless K fits one chunk)
  Live live;  // a block whose 16 rows all belong to finished segments returns at once; a tile across a segment boundary
              // computes all its rows and stores the live ones
};

#ifdef AC_DEC_STAMPS  // development probe only (tools/dec_probe.hip): phase timestamps of block (0,0), wave 0
__device__ long long g_dec_stamps[16];
#define DEC_STAMP(k) do { if (blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 0) g_dec_stamps[k] = clock64(); } while (0)
#else
#define DEC_STAMP(k) do { } while (0)
#endif

constexpr int DEC_WAVES = 4;   // waves per block: they split K (and the 16 producer rows)
constexpr int DEC_KC = 512;    // K chunk staged in LDS at a time
constexpr int DEC_T = 16;      // output tile: 16 rows x 16 columns (v_mfma_f32_16x16x4_f32)

// A decode step is ~0.36 GFLOP spread over 18 dependent launches: what matters is how many CUs each
// launch reaches and how few cache-line requests each block issues, not MFMA efficiency.  Hence small
// 16 x 16 tiles (64 ... 1092 blocks per projection) and weights pre-packed in MFMA fragment order
// (ac_trm_pack_step_weights):
//   Wp[n_tile][k_group][lane][4],  16 columns x 16 k per group, lane = (n % 16) + 16 * ((k % 16) / 4),
//   element = k % 4: a wave's B fragment is ONE contiguous 1 KiB read.
__global__ void pack_frag_kernel(const float* W, long ldw, int N, int K, float* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one float4 of the packed matrix
  const int kgs = K >> 4;
  const size_t total = (size_t)((N + DEC_T - 1) / DEC_T) * kgs * 64;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  const size_t g = i >> 6;
  const int kg = (int)(g % kgs), nt = (int)(g / kgs);
  const int n = nt * DEC_T + (lane & 15), k = kg * 16 + (lane >> 4) * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (n < N) v = *(const f32x4*)(W + (size_t)n * ldw + k);
  *(f32x4*)(out + i * 4) = v;
}

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  // lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; result reg r: D[(l >> 4) * 4 + r][l & 15]
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int PRO>
__global__ __launch_bounds__(64 * DEC_WAVES) DEC_CAP void dec_gemm_kernel(DecGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  float* sX = dsm;   // [16][KC + 4] A tile: the fused producer's rows, or a coalesced copy of X
  float* red = dsm + DEC_T * ((p.K < DEC_KC ? p.K : DEC_KC) + 4);  // [DEC_WAVES][16*17] split-K partials
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4;           // which 4 of the 16 k of a group this lane feeds
  const int m0 = blockIdx.y * DEC_T;
  if (!rows_live(p.live, m0, m0 + DEC_T < p.M ? m0 + DEC_T : p.M)) return;   // block-uniform, before any load or barrier
  const int nt0 = blockIdx.x * p.ntb;  // first of the ntb consecutive column tiles of this block
  const int KC = p.K < DEC_KC ? p.K : DEC_KC;
  const int ldsx = KC + 4;
  const int kwc = KC / DEC_WAVES;     // k range of one wave inside a chunk (multiple of 16)
  const int nsteps = kwc >> 4;        // MFMA groups of 16 k per wave per chunk (<= 8)
  const size_t wtile = (size_t)(p.K >> 4) * 64;  // float4 per packed column tile
  const f32x4* wp0 = (const f32x4*)p.Wp + (size_t)nt0 * wtile + (size_t)wave * nsteps * 64 + lane;
  DEC_STAMP(0);
  // the weight fragments of the first chunk do not depend on the producer: request them first
  f32x4 b0[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) b0[u] = wp0[(size_t)(u < nsteps ? u : 0) * 64];

  if (PRO != PRO_PLAIN) {
    // Fused producer of the 16 A rows.  A wave owns 4 rows, ONE ROW PER 16-LANE GROUP: lane (g = lane >> 4,
    // s = lane & 15) holds the row's float4 columns s, s + 16, ... so that loads are 16-byte, a group reads
    // 256 contiguous bytes, and the LayerNorm reductions are 4 DPP steps inside the group (no cross-row
    // traffic, all four rows of the wave advance together).
    constexpr int NF = DEC_MAX_D / 64;  // float4 per lane: K = d_model <= 512 -> up to 8
    const int nf = p.K >> 6;
    const int grp = lane >> 4, sub = lane & 15;
    const int row = wave * 4 + grp, r = m0 + row;
    const bool ok = r < p.M;
    const bool keep = ok && row_live(p.live, r);
    f32x4 v[NF], gw[NF], gb[NF];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (PRO == PRO_EMBED) {
      const int w = ok ? p.tok[(size_t)r * p.tok_stride + p.t] : 0;
      const f32x4* e4 = (const f32x4*)(p.emb + (size_t)w * p.K);
      const f32x4* p4 = (const f32x4*)(p.pe + (size_t)p.t * p.K);
#pragma unroll
      for (int i = 0; i < NF; ++i)
        v[i] = (ok && i < nf) ? e4[sub + 16 * i] * p.emb_scale + p4[sub + 16 * i] : zero4;
    } else {
      if (PRO == PRO_EMBED_KW) {
        // the embedding with the clip's keyword row added, then normalised like a join; pe[t] is added after the norm
        const int w = ok ? p.tok[(size_t)r * p.tok_stride + p.t] : 0;
        const f32x4* e4 = (const f32x4*)(p.emb + (size_t)w * p.K);
        const f32x4* k4 = (const f32x4*)(p.X + (size_t)(ok ? r / p.kw_div : 0) * p.ldx);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          gw[i] = i < nf ? ((const f32x4*)p.ln_w)[sub + 16 * i] : zero4;
          gb[i] = i < nf ? ((const f32x4*)p.ln_b)[sub + 16 * i] : zero4;
          v[i] = (ok && i < nf) ? e4[sub + 16 * i] * p.emb_scale + k4[sub + 16 * i] : zero4;
        }
      } else {
        const f32x4* x4 = (const f32x4*)(p.X + (size_t)(ok ? r : 0) * p.ldx);
        const f32x4* y4 = (const f32x4*)(p.Y2 + (size_t)(ok ? r : 0) * p.ldy2);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          gw[i] = i < nf ? ((const f32x4*)p.ln_w)[sub + 16 * i] : zero4;
          gb[i] = i < nf ? ((const f32x4*)p.ln_b)[sub + 16 * i] : zero4;
          v[i] = (ok && i < nf) ? x4[sub + 16 * i] + y4[sub + 16 * i] : zero4;
        }
      }
      DEC_STAMP(1);
      float sm = 0.f;
#pragma unroll
      for (int i = 0; i < NF; ++i) sm += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      const float mean = row16_sum(sm) / (float)p.K;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < NF; ++i)
        if (i < nf) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float dl = v[i][e] - mean; q = fmaf(dl, dl, q); }
        }
      const float rstd = rsqrtf(row16_sum(q) / (float)p.K + 1e-5f);
#pragma unroll
      for (int i = 0; i < NF; ++i) v[i] = (v[i] - mean) * rstd * gw[i] + gb[i];
      if (PRO == PRO_EMBED_KW) {
        const f32x4* p4 = (const f32x4*)(p.pe + (size_t)p.t * p.K);
#pragma unroll
        for (int i = 0; i < NF; ++i)
          if (i < nf) v[i] = v[i] + p4[sub + 16 * i];
      }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i)
      if (i < nf) {
        *(f32x4*)(sX + row * ldsx + (sub + 16 * i) * 4) = ok ? v[i] : zero4;
        if (blockIdx.x == 0 && p.xout && keep) *(f32x4*)(p.xout + (size_t)r * p.ldxo + (sub + 16 * i) * 4) = v[i];
      }
  }
  DEC_STAMP(2);
  const float* xa = sX + (lane & 15) * ldsx + wave * kwc + kq * 4;
  // PRO_PLAIN: the X chunk is copied into the LDS tile with coalesced 16-byte loads (row = 4*KC bytes);
  // chunk c+1 is requested into registers before the MFMAs of chunk c
  constexpr int XLD = DEC_T * (DEC_KC / 4) / (64 * DEC_WAVES);  // float4 per thread per chunk (8)
  const int c4n = KC >> 2;
  f32x4 xr[XLD];
  auto x_load = [&](int c0) {
#pragma unroll
    for (int u = 0; u < XLD; ++u) {
      const int idx = tid + u * 64 * DEC_WAVES;
      const int row = idx / (DEC_KC / 4), c4 = idx % (DEC_KC / 4);  // constants: shifts
      const bool okr = c4 < c4n && m0 + row < p.M;
      xr[u] = okr ? *(const f32x4*)(p.X + (size_t)(m0 + row) * p.ldx + c0 + c4 * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  auto x_store = [&]() {
#pragma unroll
    for (int u = 0; u < XLD; ++u) {
      const int idx = tid + u * 64 * DEC_WAVES;
      const int row = idx / (DEC_KC / 4), c4 = idx % (DEC_KC / 4);
      if (c4 < c4n) *(f32x4*)(sX + row * ldsx + c4 * 4) = xr[u];
    }
  };
  if (PRO == PRO_PLAIN) x_load(0);
  // ntb consecutive column tiles re-use the A tile (single-chunk K only; the launcher enforces it)
  for (int nt = 0; nt < p.ntb; ++nt) {
    const int n0 = (nt0 + nt) * DEC_T;
    if (n0 >= p.N) break;
    const f32x4* wp = wp0 + (size_t)nt * wtile;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < p.K; c0 += KC) {
      f32x4 b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        b[u] = (c0 == 0 && nt == 0) ? b0[u] : wp[((size_t)(c0 >> 4) + (u < nsteps ? u : 0)) * 64];
      if (PRO == PRO_PLAIN) {
        if (c0 > 0) __syncthreads();
        if (nt == 0) {
          x_store();
          if (c0 + KC < p.K) x_load(c0 + KC);
        }
      }
      if (nt == 0) __syncthreads();
      DEC_STAMP(3);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (u < nsteps) {
          const f32x4 a = *(const f32x4*)(xa + 16 * u);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = mfma16(a[s], b[u][s], acc);
        }
      }
    }
    DEC_STAMP(4);
    if (nt > 0) __syncthreads();  // the previous tile's partials have been consumed
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave * (DEC_T * 17) + (kq * 4 + r) * 17 + (lane & 15)] = acc[r];
    __syncthreads();
    {
      const int i = tid >> 4, jn = tid & 15;  // 256 threads = the 16 x 16 outputs
      const int gm = m0 + i, gn = n0 + jn;
      if (gm < p.M && gn < p.N && row_live(p.live, gm)) {
        const int o = i * 17 + jn;
        float y = (red[o] + red[DEC_T * 17 + o]) + (red[2 * DEC_T * 17 + o] + red[3 * DEC_T * 17 + o]);
        if (p.bias) y += p.bias[gn];
        if (p.relu) y = fmaxf(y, 0.f);
        p.Y[(size_t)gm * p.ldy + gn] = y;
      }
    }
  }
  DEC_STAMP(5);
}

template <int PRO>
int launch_dec_gemm(const DecGemmParams& p_in, hipStream_t s) {
  DecGemmParams p = p_in;
  if (p.K % 64 || (PRO != PRO_PLAIN && p.K > DEC_MAX_D) || (p.K > DEC_KC && p.K % DEC_KC)) return AC_ERR_ARG;
  const int KC = p.K < DEC_KC ? p.K : DEC_KC;
  if (p.ntb < 1) return AC_ERR_ARG;
  if (p.K > DEC_KC) p.ntb = 1;   // several column tiles per block re-use ONE staged A tile: single-chunk K only
  // the A tile is [16][KC + 4]: sized by the launch's K chunk, so that the K = 256 projections fit 7 workgroups to a CU
  const size_t lds = ((size_t)DEC_T * (KC + 4) + (size_t)DEC_WAVES * DEC_T * 17) * sizeof(float);
  const int ntiles = (p.N + DEC_T - 1) / DEC_T;
  dim3 grid((ntiles + p.ntb - 1) / p.ntb, (p.M + DEC_T - 1) / DEC_T);
  hipLaunchKernelGGL((dec_gemm_kernel<PRO>), grid, dim3(64 * DEC_WAVES), lds, s, p);
  return ac_check_launch();
}

// ---------------------------------------------------------------------------------------------
// greedy pick for step t (base.py:214-218 log_softmax + max, :161-167, :202-208)
// ---------------------------------------------------------------------------------------------
struct PickParams {
  const float* logit; long ldl;  // row b at logit + b*ldl (already offset to step t)
  int V, t, max_len, end_idx, pad_idx;
  int64_t* seq; float* logprob;
  int* tok; unsigned char* mask;  // [B][max_len+1]
  int* unfinished;                // [B]
  int* cnt;                       // [segments][max_len], zeroed by greedy_init_kernel
  int seg_rows;                   // rows per segment (struct Live)
};

__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

constexpr int PICK_MAXV = 16384;  // logits of a row are held in registers: <= 64 per thread

__global__ __launch_bounds__(256) DEC_CAP void greedy_pick_kernel(PickParams p) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ float ssum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* const cnt = p.cnt + (size_t)(b / p.seg_rows) * p.max_len;   // of this row's segment
  if (p.t > 0 && cnt[p.t - 1] == 0) return;  // the reference loop of this batch has already stopped (base.py:167)
  const float* row = p.logit + (size_t)b * p.ldl;
  // one pass over memory: all loads in flight at once, max / arg-max / exp-sum from registers
  float x[PICK_MAXV / 256];
#pragma unroll
  for (int i = 0; i < PICK_MAXV / 256; ++i) {
    const int c = tid + 256 * i;
    x[i] = c < p.V ? row[c] : -INFINITY;
  }
  float v = -INFINITY;
  int idx = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < PICK_MAXV / 256; ++i) argmax_merge(v, idx, x[i], tid + 256 * i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    argmax_merge(v, idx, ov, oi);
  }
  if (lane == 0) { sv[wave] = v; si[wave] = idx; }
  __syncthreads();
  v = sv[0]; idx = si[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) argmax_merge(v, idx, sv[k], si[k]);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PICK_MAXV / 256; ++i)
    if (tid + 256 * i < p.V) s += expf(x[i] - v);
  s = wave_sum(s);
  if (lane == 0) ssum[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const float tot = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    const int prev = p.t == 0 ? 1 : p.unfinished[b];
    const int unf = prev && (idx != p.end_idx);
    const int w = unf ? idx : p.end_idx;
    p.unfinished[b] = unf;
    p.seq[(size_t)b * p.max_len + p.t] = w;
    p.logprob[(size_t)b * p.max_len + p.t] = -logf(tot);
    p.tok[(size_t)b * (p.max_len + 1) + p.t + 1] = w;
    p.mask[(size_t)b * (p.max_len + 1) + p.t + 1] = (w == p.pad_idx) ? 1 : 0;
    if (unf) atomicAdd(&cnt[p.t], 1);
  }
}

__global__ void greedy_init_kernel(int64_t* seq, float* logprob, int* tok, unsigned char* mask, int* unfinished,
                                   int* cnt, int n_cnt, int B, int max_len, int start_idx, int end_idx, int pad_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * max_len) { seq[i] = end_idx; logprob[i] = 0.f; }
  if (i < B * (max_len + 1)) {
    const int c = i % (max_len + 1);
    tok[i] = c == 0 ? start_idx : end_idx;
    mask[i] = c == 0 ? (start_idx == pad_idx) : 0;
  }
  if (i < B) unfinished[i] = 1;
  if (i < n_cnt) cnt[i] = 0;   // n_cnt = segments * max_len <= B * max_len: inside the grid
}

// The columns of the steps a segment did not run read as the reference leaves them - it never allocates them: logit and
// embed 0 (seq = <end> and log-probability 0 are what greedy_init_kernel wrote and no pick touched).  The search works in
// static buffers that still hold an earlier, longer search; one launch at the end of the chain, grid (rows, max_len - 1),
// clears exactly the columns not run, also for the routes whose kernels do not skip (the generic-GEMM classifier, the wide
// and hybrid routes).  It writes what the skipped steps would have written, at the memory system's speed, once.
__global__ __launch_bounds__(256) void search_finalize_kernel(float* logit, float* embed, Live live, int V, int d) {
  const int r = blockIdx.x;
  live.t = blockIdx.y + 1;
  if (row_live(live, r)) return;
  float* lg = logit + ((size_t)r * live.max_len + live.t) * V;
  float* em = embed + ((size_t)r * live.max_len + live.t) * d;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  if (V % 4 == 0 && !((uintptr_t)logit & 15)) {
    for (int c = threadIdx.x; c < V / 4; c += 256) ((f32x4*)lg)[c] = zero4;
  } else {
    for (int c = threadIdx.x; c < V; c += 256) lg[c] = 0.f;
  }
  if (d % 4 == 0 && !((uintptr_t)embed & 15)) {
    for (int c = threadIdx.x; c < d / 4; c += 256) ((f32x4*)em)[c] = zero4;
  } else {
    for (int c = threadIdx.x; c < d; c += 256) em[c] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// beam search, device half (base.py:282-289)
// ---------------------------------------------------------------------------------------------
// lp[r][:] = log_softmax(log_softmax(logit[r]) / temp) + cum[r]
__global__ __launch_bounds__(256) void beam_logprob_kernel(const float* logit, const float* cum, float temp,
                                                           float* lp, int V) {
  __shared__ float sh[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = logit + (size_t)r * V;
  float m = -INFINITY;
  for (int c = tid; c < V; c += 256) m = fmaxf(m, row[c]);
  m = block_max256(m, sh);
  float s = 0.f;
  for (int c = tid; c < V; c += 256) s += expf(row[c] - m);
  s = block_sum256(s, sh);
  const float lse1 = m + logf(s);
  const float inv_t = 1.0f / temp;
  float m2 = -INFINITY;
  for (int c = tid; c < V; c += 256) m2 = fmaxf(m2, (row[c] - lse1) * inv_t);
  m2 = block_max256(m2, sh);
  float s2 = 0.f;
  for (int c = tid; c < V; c += 256) s2 += expf((row[c] - lse1) * inv_t - m2);
  s2 = block_sum256(s2, sh);
  const float lse2 = m2 + logf(s2);
  const float cr = cum[r];
  for (int c = tid; c < V; c += 256) lp[(size_t)r * V + c] = cr + ((row[c] - lse1) * inv_t - lse2);
}

// per clip: the `beam` largest entries of lp[clip*beam .. +nrows][V] flattened (lowest index wins ties).
// One pass over the scores: every thread keeps its own best TOPK_LOCAL candidates in registers; the workgroup then
// picks the winners from the 256 x TOPK_LOCAL survivors in LDS (the global top `beam` is contained in them because each
// thread's list holds its own best `beam`).  beam > TOPK_LOCAL falls back to one full scan per winner.
constexpr int TOPK_LOCAL = 4;
__device__ __forceinline__ bool cand_better(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

__global__ __launch_bounds__(256) void beam_topk_kernel(const float* lp, int beam, int nrows, int V,
                                                        float* top_val, int* top_idx) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int chosen[64];
  __shared__ float cv[256 * TOPK_LOCAL];
  __shared__ int ci[256 * TOPK_LOCAL];
  const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = lp + (size_t)clip * beam * V;
  const int n = nrows * V;
  const bool local = beam <= TOPK_LOCAL;
  if (local) {
    float bv[TOPK_LOCAL];
    int bi[TOPK_LOCAL];
#pragma unroll
    for (int j = 0; j < TOPK_LOCAL; ++j) { bv[j] = -INFINITY; bi[j] = 0x7fffffff; }
    for (int c = tid; c < n; c += 256) {
      float v = base[c];
      int idx = c;
      if (cand_better(v, idx, bv[TOPK_LOCAL - 1], bi[TOPK_LOCAL - 1])) {
#pragma unroll
        for (int j = 0; j < TOPK_LOCAL; ++j)   // insertion into the sorted list (best first)
          if (cand_better(v, idx, bv[j], bi[j])) {
            const float tv = bv[j]; const int ti = bi[j];
            bv[j] = v; bi[j] = idx; v = tv; idx = ti;
          }
      }
    }
#pragma unroll
    for (int j = 0; j < TOPK_LOCAL; ++j) { cv[tid * TOPK_LOCAL + j] = bv[j]; ci[tid * TOPK_LOCAL + j] = bi[j]; }
    __syncthreads();
  }
  const int ncand = local ? 256 * TOPK_LOCAL : n;
  for (int k = 0; k < beam; ++k) {
    float v = -INFINITY;
    int idx = 0x7fffffff;
    for (int c = tid; c < ncand; c += 256) {
      const float x = local ? cv[c] : base[c];
      const int xi = local ? ci[c] : c;
      bool skip = false;
      for (int j = 0; j < k; ++j) skip |= (chosen[j] == xi);
      if (!skip) argmax_merge(v, idx, x, xi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      argmax_merge(v, idx, ov, oi);
    }
    __syncthreads();
    if (lane == 0) { sv[wave] = v; si[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
      v = sv[0]; idx = si[0];
      for (int w = 1; w < 4; ++w) argmax_merge(v, idx, sv[w], si[w]);
      chosen[k] = idx;
      top_val[clip * beam + k] = v;
      top_idx[clip * beam + k] = idx;
    }
    __syncthreads();
  }
}

// The two kernels above as ONE pass per row (beam <= 8, V <= 256 NV): the logits of a row live in registers (one global
// read instead of five sweeps), lp = log_softmax(log_softmax(x) / temp) + cum is never written - the row only publishes
// its own best `beam` candidates (the clip's best `beam` are among the per-row best `beam`), picked by `beam` rounds of a
// workgroup arg-max over the registers.  Same arithmetic in the same order as beam_logprob_kernel (the second maximum
// is the image of the first: the map is increasing), same tie rule as beam_topk_kernel: identical results.
template <int NV>
__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* logit, const float* cum, float temp, int beam, int V,
                                                            float* cand_val, int* cand_idx) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int s_win;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logit + (size_t)r * V;
  float x[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) x[k] = tid + 256 * k < V ? row[tid + 256 * k] : -INFINITY;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NV; ++k) m = fmaxf(m, x[k]);
  m = block_max256(m, sh);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (tid + 256 * k < V) s += expf(x[k] - m);
  s = block_sum256(s, sh);
  const float lse1 = m + logf(s);
  const float inv_t = 1.0f / temp;
  const float m2 = (m - lse1) * inv_t;
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (tid + 256 * k < V) s2 += expf((x[k] - lse1) * inv_t - m2);
  s2 = block_sum256(s2, sh);
  const float lse2 = m2 + logf(s2);
  const float cr = cum[r];
#pragma unroll
  for (int k = 0; k < NV; ++k) x[k] = tid + 256 * k < V ? cr + ((x[k] - lse1) * inv_t - lse2) : -INFINITY;
  unsigned taken = 0u;
  const int flat0 = (r % beam) * V;           // index of the row's first entry in the clip's flattened scores
  for (int j = 0; j < beam; ++j) {
    float v = -INFINITY;
    int idx = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (!((taken >> k) & 1u) && tid + 256 * k < V) argmax_merge(v, idx, x[k], tid + 256 * k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      argmax_merge(v, idx, ov, oi);
    }
    __syncthreads();
    if (lane == 0) { sv[wave] = v; si[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
      v = sv[0]; idx = si[0];
      for (int w = 1; w < 4; ++w) argmax_merge(v, idx, sv[w], si[w]);
      s_win = idx;
      cand_val[(size_t)r * beam + j] = v;
      cand_idx[(size_t)r * beam + j] = flat0 + idx;
    }
    __syncthreads();
    const int win = s_win;
    if ((win & 255) == tid) taken |= 1u << (win >> 8);
  }
}

// per clip: the `beam` best of the nrows x beam row candidates (<= 64: one per lane), lowest flattened index wins ties
__global__ __launch_bounds__(64) void beam_merge_kernel(const float* cand_val, const int* cand_idx, int beam, int nrows,
                                                       float* top_val, int* top_idx) {
  const int clip = blockIdx.x, lane = threadIdx.x;
  const int n = nrows * beam;
  float v = lane < n ? cand_val[(size_t)clip * beam * beam + lane] : -INFINITY;
  int idx = lane < n ? cand_idx[(size_t)clip * beam * beam + lane] : 0x7fffffff;
  for (int j = 0; j < beam; ++j) {
    float bv = v;
    int bi = idx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      argmax_merge(bv, bi, ov, oi);
    }
    if (lane == 0) {
      top_val[clip * beam + j] = bv;
      top_idx[clip * beam + j] = bi;
    }
    if (idx == bi) { v = -INFINITY; idx = 0x7fffffff; }
  }
}

// Per-clip beam bookkeeping of base.py:290-323 on the device (one workgroup per clip, thread 0 does the serial part):
// re-gather the token rows by the chosen previous beams, append the new words, record the beams that END this step
// (in beam order, score = logprob / (t + 1)), apply the -1000 trick to their cumulative scores and retire the clip
// when its number of finished beams EQUALS the beam size (the reference's '==').  A retired clip keeps its rows.
// retire == 0 (ac_trm_beam_update_all): the ensemble search of ensemble.py:195-261 has no such break - every clip searches to
// max_len and collects every finished beam (at most beam * max_len of them).
__global__ __launch_bounds__(64) void beam_update_kernel(const float* top_val, const int* top_idx, const int* tok_in,
                                                        int* tok_out, unsigned char* mask_out, float* cum, int* active,
                                                        int* done_cnt, int* done_seq, float* done_score, int* src_row,
                                                        int* n_active, int beam, int V, int max_len, int t, int end_idx,
                                                        int pad_idx, int cap, int retire) {
  __shared__ int s_src[64];
  __shared__ int s_word[64];
  const int clip = blockIdx.x, tid = threadIdx.x;
  const int ld = max_len + 1;
  const bool act = active[clip] != 0;
  if (tid < beam) {
    const int flat = top_idx[clip * beam + tid];
    s_src[tid] = act ? clip * beam + flat / V : clip * beam + tid;
    s_word[tid] = flat % V;
    src_row[clip * beam + tid] = s_src[tid];
  }
  __syncthreads();
  // token rows (and the key-padding mask the decoder step reads)
  for (int e = tid; e < beam * ld; e += 64) {
    const int k = e / ld, c = e % ld;
    int v = tok_in[(size_t)s_src[k] * ld + c];
    if (act && c == t + 1) v = s_word[k];
    tok_out[(size_t)(clip * beam + k) * ld + c] = v;
    mask_out[(size_t)(clip * beam + k) * ld + c] = v == pad_idx ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0 && act) {
    int cnt = done_cnt[clip];
    for (int k = 0; k < beam; ++k) {
      const float v = top_val[clip * beam + k];
      const bool is_end = s_word[k] == end_idx || t == max_len - 1;
      if (is_end) {
        if (cnt < cap) {
          int* dst = done_seq + ((size_t)clip * cap + cnt) * max_len;
          const int* row = tok_out + (size_t)(clip * beam + k) * ld;
          for (int c = 0; c < max_len; ++c) dst[c] = c <= t ? row[c + 1] : end_idx;
          done_score[(size_t)clip * cap + cnt] = v / (float)(t + 1);
        }
        ++cnt;
      }
      cum[clip * beam + k] = v - (is_end ? 1000.0f : 0.0f);
    }
    done_cnt[clip] = cnt;
    if (retire && cnt == beam) {
      active[clip] = 0;
      atomicSub(n_active, 1);
    }
  }
}

// dst[l][r][0..t][:] = src[l][src_row[r]][0..t][:] for both K and V caches
__global__ void cache_gather_kernel(const float* src, float* dst, const int* src_row, int R, int max_len, int t,
                                    int d, size_t set_stride /* floats between K and V sets and layers */, int nsets) {
  const int r = blockIdx.x, set = blockIdx.y;
  const int sr = src_row[r];
  const size_t n = (size_t)(t + 1) * d;
  const float* s = src + set * set_stride + (size_t)sr * max_len * d;
  float* o = dst + set * set_stride + (size_t)r * max_len * d;
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) o[i] = s[i];
}

// ---------------------------------------------------------------------------------------------
// workspace carving
// ---------------------------------------------------------------------------------------------
// The wide route (steps over many rows, csrc/decoder_wide.hip) covers the reference's decoder width: d_model 256 (its fused
// producers stage a 256-wide row; heads of <= 64) and a feed-forward width of 256, 512 or 1024.
inline bool wide_shape_ok(const ac_trm_weights* w) {
  return w->d_model == 256 && (w->dim_ff == 256 || w->dim_ff == 512 || w->dim_ff == 1024);
}

struct Ws {
  float *x, *x2, *qkv, *att, *tmp, *ff, *q2, *lg;
  float *attp, *ffp;        // wide route: fragment packs of the attention context rows / the feed-forward hidden rows
  float* cache[2];  // [2 (K,V)][nlayers][R][max_len][d] each
  int *tok, *unfinished;
  unsigned char* mask;
  size_t cache_set_stride;  // R*max_len*d
  size_t total;
};

inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

Ws carve(const ac_trm_weights* w, int R, int max_len, float* base) {
  Ws s;
  const size_t d = w->d_model;
  size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += align4(n); return p; };
  s.x = take(R * d);
  s.x2 = take(R * d);
  s.qkv = take(R * 3 * d);
  s.att = take(R * d);
  s.tmp = take(R * d);
  s.ff = take((size_t)R * w->dim_ff);
  s.q2 = take(R * d);
  s.lg = take((size_t)R * w->vocab);
  const size_t r32 = (size_t)(R + 31) / 32 * 32;
  s.attp = take(wide_shape_ok(w) ? r32 * d * 3 / 2 : 0);
  s.ffp = take(wide_shape_ok(w) ? r32 * (size_t)w->dim_ff * 3 / 2 : 0);
  s.cache_set_stride = (size_t)R * max_len * d;
  for (int i = 0; i < 2; ++i) s.cache[i] = take(2 * (size_t)w->nlayers * s.cache_set_stride);
  s.tok = (int*)take((size_t)R * (max_len + 1));
  s.unfinished = (int*)take(R);
  s.mask = (unsigned char*)take(((size_t)R * (max_len + 1) + 3) / 4);
  s.total = off;
  return s;
}

#define AC_TRY(expr)            \
  do {                          \
    int _e = (expr);            \
    if (_e != AC_OK) return _e; \
  } while (0)

// The shapes a decoder step runs (decoder_step, launch_dec_gemm, attn_step_kernel), in one place: the A tile of a projection
// with a fused producer holds a whole d_model row (64 | d_model <= DEC_MAX_D), the four waves of dec_gemm_kernel split a K
// chunk into groups of 16 (64 | K) and a K beyond one chunk runs whole chunks (dim_ff <= DEC_KC or DEC_KC | dim_ff), a head
// is one wave with a lane per channel (head width <= 64).
inline bool step_shape_ok(int d_model, int nhead, int dim_ff) {
  if (d_model < 64 || d_model % 64 || d_model > DEC_MAX_D) return false;
  if (dim_ff < 64 || dim_ff % 64 || (dim_ff > DEC_KC && dim_ff % DEC_KC)) return false;
  return nhead >= 1 && d_model % nhead == 0 && d_model / nhead <= 64;
}

// Every entry point that takes an ac_trm_weights asks this first - the size queries, the weight pack, the memory projection
// and the searches refuse the same set, before anything is launched.
int check_weights(const ac_trm_weights* w) {
  if (!w || w->nlayers < 1 || w->nlayers > AC_MAX_LAYERS) return AC_ERR_ARG;
  if (!step_shape_ok(w->d_model, w->nhead, w->dim_ff)) return AC_ERR_ARG;
  if (w->attn_emb_dim < 32 || w->attn_emb_dim % 32) return AC_ERR_ARG;
  return AC_OK;
}

int launch_ln(const float* x, const float* y, const float* w, const float* b, float* out, int rows, int d,
              long ldx, long ldy, long ldo, hipStream_t s, const Live& live = Live()) {
  hipLaunchKernelGGL(add_layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, y, w, b, out, rows, d, ldx,
                     ldy, ldo, live);
  return ac_check_launch();
}

// Offsets (in floats) of the fragment-packed step weights inside ac_trm_weights::step_pk, fixed order: per layer the six
// projections, three transposed copies, the six wide packs; then the classifier and its wide pack.
struct ProjOffsets { size_t sa_in, sa_out, ca_q, ca_out, l1, l2; };
struct PackLayout {
  ProjOffsets n;                    // dec_gemm_kernel's fragment order
  size_t sa_outT, ca_qT, ca_outT;   // transposed [k][n] copies for the fused per-row sub-layer kernel
  ProjOffsets w;                    // three-plane bf16 packs of the wide route (csrc/decoder_wide.hip)
};
struct PackOffsets { PackLayout layer[AC_MAX_LAYERS]; size_t cls, wcls, total; };   // cls / wcls: the classifier's two packs
inline size_t packed_floats(int N, int K) { return (size_t)((N + DEC_T - 1) / DEC_T) * DEC_T * K; }
inline PackOffsets pack_layout(const ac_trm_weights* w) {
  const int d = w->d_model, ff = w->dim_ff;
  const bool wide = wide_shape_ok(w);
  auto wf = [&](int N, int K) { return wide ? (size_t)ac_dec_wide_packed_floats(N, K) : (size_t)0; };
  PackOffsets po = {};
  size_t off = 0;
  for (int l = 0; l < w->nlayers; ++l) {
    PackLayout& t = po.layer[l];
    t.n.sa_in = off; off += packed_floats(3 * d, d);
    t.n.sa_out = off; off += packed_floats(d, d);
    t.n.ca_q = off; off += packed_floats(d, d);
    t.n.ca_out = off; off += packed_floats(d, d);
    t.n.l1 = off; off += packed_floats(ff, d);
    t.n.l2 = off; off += packed_floats(d, ff);
    t.sa_outT = off; off += (size_t)d * d;
    t.ca_qT = off; off += (size_t)d * d;
    t.ca_outT = off; off += (size_t)d * d;
    t.w.sa_in = off; off += wf(3 * d, d);
    t.w.sa_out = off; off += wf(d, d);
    t.w.ca_q = off; off += wf(d, d);
    t.w.ca_out = off; off += wf(d, d);
    t.w.l1 = off; off += wf(ff, d);
    t.w.l2 = off; off += wf(d, ff);
  }
  po.cls = off; off += packed_floats(w->vocab, d);
  po.wcls = off; off += wf(w->vocab, d);
  po.total = off;
  return po;
}

// Which launches make up a decode position over R rows: decided ONCE per step (decoder_step) and handed to classifier_step
// with the step's result.  Every AUDIOCAPTION_DEC_* switch of this file is read here, and not all at the same time:
//   on every call (tests switch them; a captured graph keeps what it was captured with):
//     AUDIOCAPTION_DEC_WIDE_MIN, AUDIOCAPTION_DEC_HYBRID, AUDIOCAPTION_DEC_ROW=gemm, AUDIOCAPTION_DEC_WIDE_CLS_NTB
//   latched by the first step of the process (development switches; so is AUDIOCAPTION_BEAM_TOPK in ac_trm_beam_step):
//     AUDIOCAPTION_DEC_ROW=split, AUDIOCAPTION_DEC_NTB, AUDIOCAPTION_DEC_CLS_GEMM, AUDIOCAPTION_DEC_CLS_NTB
struct Route {
  bool wide = false;                       // the wide route; else the fused per-row route (rows) or the general one
  bool rows = false, rows_split = false;   // rows_split: the two per-row sub-layers as a launch each
  bool hybrid = false;                     // narrow, but the joined QKV projections and the classifier on their wide twins
  int ntb = 1;                             // column tiles per block of the single-chunk projections
  bool cls_ln_gemm = false;                // the classifier as LayerNorm + ac_gemm (where it has room for the normalised rows)
  int cls_ntb = 4, wide_cls_ntb = 2;       // column tiles per block of the classifier projection / of its wide twin
};

Route resolve_route(const ac_trm_weights* w, int R, int Tm, int t, bool keyword = false) {
  auto is = [](const char* v, const char* want) { return v && !strcmp(v, want); };
  Route rt;
  // AUDIOCAPTION_DEC_WIDE_MIN=n (default 0 = never): a step over n rows or more takes the wide route.  Opt-in, because it does
  // not pay on this part: stand-alone it is 145 / 202 us per step at 256 / 768 rows against 115 / 193 for the narrow route
  // (22 launches per step instead of 10, each ~3 us of launch overhead + a 3-5 us critical path, although a projection
  // occupies 32-128 workgroups for 3-5 us instead of every CU for 7-18), and beside the next batches' encoders the step
  // costs what its DURATION is, not its CU time: headline 13.85 k vs 14.10 k clips/s, EffB2-Trm 20.65 k vs 20.55 k
  // (EXPERIMENTS.md, round 6).
  const char* e = getenv("AUDIOCAPTION_DEC_WIDE_MIN");
  const int wide_min = e ? atoi(e) : 0;
  // (a keyword decoder stays on the general / rows routes: the wide kernels have no keyword producer)
  rt.wide = !keyword && wide_min > 0 && R >= wide_min && wide_shape_ok(w) && w->d_model / w->nhead <= 64 && w->d_model % w->nhead == 0;
  // AUDIOCAPTION_DEC_HYBRID=1 (default off): from 512 rows on (a beam search over grouped batches) the QKV projection with the
  // residual join in its prologue and the classifier take their wide twins (csrc/decoder_wide.hip).  Stand-alone those are the
  // two launches of the narrow route furthest from their arithmetic (20 and 30 + 5 us at 768 rows against 11 and 27); inside the
  // EffB2-Trm pipeline the wide classifier's one-workgroup-per-CU blocks take 43 us beside the encoder and the step does not move
  // (20.41 vs 20.41 k clips/s, 30 s / beam 4: 7.70 vs 7.70 k): opt-in, kept for the record.
  rt.hybrid = !keyword && !rt.wide && is(getenv("AUDIOCAPTION_DEC_HYBRID"), "1") && R >= 512 && wide_shape_ok(w);
  // the reference's decoder shape (d_model 256 = 4 heads of 64) takes the fused per-row sub-layer kernel: 4 launches per
  // layer instead of 8; any other shape the general 8-launch sequence
  // AUDIOCAPTION_DEC_ROW=gemm: the general 18-launch sequence (attn_step_kernel + dec_gemm_kernel) instead of the per-row
  // kernels.  (The row kernels once gave co-runner-dependent results: built with packed-f32 VALU instructions their
  // matrix-vector products broke beside MFMA-heavy kernels of another stream - see audiocaption_amd/build.py; every mode is
  // now held to tests/test_gpu_model.py::test_decode_is_bit_stable_beside_matrix_heavy_kernels.)
  // AUDIOCAPTION_DEC_ROW=split: dec_row_kernel per sub-layer (5 launches per layer) instead of one dec_row2_kernel.
  static const bool split = is(getenv("AUDIOCAPTION_DEC_ROW"), "split");
  rt.rows = !rt.wide && w->d_model == ROW_D && w->nhead == ROW_H && t + 1 <= MAX_KEYS && Tm <= MAX_KEYS &&
            !is(getenv("AUDIOCAPTION_DEC_ROW"), "gemm");
  rt.rows_split = rt.rows && split;
  // column tiles per block of the single-chunk projections: two from 512 rows on (beam search over grouped batches: 768
  // rows - the A tile is staged once for both, EffB2-Trm 19.15 -> 19.40 k clips/s; at 256 rows and below no difference).  The
  // arithmetic of an output does not depend on it.  AUDIOCAPTION_DEC_NTB overrides (development).
  static const int dev_ntb = getenv("AUDIOCAPTION_DEC_NTB") ? atoi(getenv("AUDIOCAPTION_DEC_NTB")) : 0;
  rt.ntb = dev_ntb > 0 ? dev_ntb : (R >= 512 ? 2 : 1);
  // From 512 rows on (beam search over grouped batches: 768 rows x 4368 words) the 16 x 16-tile projection re-reads the
  // classifier once per 16 rows: 47 us per step; the residual join as its own launch + the tiled exact-f32 GEMM (ac_gemm)
  // take 4 + 30.  Another summation order than the projection's (last bits of the logits; not a precision change).
  // AUDIOCAPTION_DEC_CLS_GEMM=0: the projection at every row count.
  static const bool cls_gemm = !is(getenv("AUDIOCAPTION_DEC_CLS_GEMM"), "0");
  rt.cls_ln_gemm = cls_gemm && R >= 512;
  // 1092 column tiles: four per block keep the grid near one resident wave of blocks.  AUDIOCAPTION_DEC_CLS_NTB: development
  static const int dev_cls_ntb = getenv("AUDIOCAPTION_DEC_CLS_NTB") ? atoi(getenv("AUDIOCAPTION_DEC_CLS_NTB")) : 4;
  rt.cls_ntb = dev_cls_ntb;
  // 64-column groups per workgroup of the wide classifier: the LayerNorm of a 32-row tile is redone once per group block
  e = getenv("AUDIOCAPTION_DEC_WIDE_CLS_NTB");
  rt.wide_cls_ntb = e ? atoi(e) : (R >= 512 ? 4 : 2);
  if (rt.wide_cls_ntb < 1) rt.wide_cls_ntb = 1;
  return rt;
}

// A residual join that has not run: LayerNorm(x + y) * ln_w + ln_b is produced in the prologue of the next projection
// (the residual joins and the embedding never run alone).  x null: none pending - the next projection embeds the tokens.
struct Join { const float *x, *y, *ln_w, *ln_b; };

// What decoder_step hands to classifier_step: the LAST join (embed = LayerNorm(x + y) with the last layer's norm3) and the route
struct StepOut { Join join; Route route; };

// One decode position over R rows, as the descriptor builders read it.  `shared`: what the dec_gemm_kernel projections of a
// step have in common, filled once (decoder_step): M, ntb, live and the embedding's tok / tok_stride / t / emb / pe / emb_scale.
struct Step {
  const ac_trm_weights* w; const Ws* ws;
  const float* memkv; const int* mem_len;        // cross-attention K | V of every layer: R / row_div memory rows of Tm keys
  float* cache; const unsigned char* mask;       // the active KV cache set; key mask [R][shared.tok_stride]
  int R, row_div, Tm, max_len, t;
  DecGemmParams shared;
};

// What the attentions of a route share: head geometry, where the context rows go, which rows run.  On the wide route they
// leave as the fragment pack of the out-projection and the launch skips nothing (live stays Live(): the search clears what
// it wrote for ended segments, search_finalize_kernel); on the others they go to ws.att (the per-row kernels keep them in
// LDS and ignore it) and the rows of ended segments are skipped.
void attn_output(const Step& c, bool wide, AttnParams& a) {
  const int d = c.w->d_model;
  a.hd = d / c.w->nhead; a.scale = 1.0f / sqrtf((float)a.hd);
  if (wide) { a.out_pk = (unsigned char*)c.ws->attp; a.pk_kst = d / 16; }
  else { a.out = c.ws->att; a.ldo = d; a.live = c.shared.live; }
}

// self attention of layer l: the query and the new key / value row are the thirds of ws.qkv; keys 0 .. t of the cache
AttnParams self_attn_params(const Step& c, int l, bool wide) {
  const long d = c.w->d_model;
  AttnParams a{};
  a.K = a.Kw = c.cache + (size_t)(2 * l) * c.ws->cache_set_stride;
  a.V = a.Vw = c.cache + (size_t)(2 * l + 1) * c.ws->cache_set_stride;
  a.row_stride = (long)c.max_len * d; a.key_stride = d; a.row_div = 1; a.nkeys = c.t + 1;
  a.q = c.ws->qkv; a.ldq = 3 * d; a.key_mask = c.mask; a.mask_stride = c.shared.tok_stride;
  a.new_k = c.ws->qkv + d; a.new_v = c.ws->qkv + 2 * d; a.ld_new = 3 * d;
  attn_output(c, wide, a);
  return a;
}

// cross attention of layer l: the query is ws.q2; the first mem_len keys of memory row r / row_div, nothing appended
AttnParams cross_attn_params(const Step& c, int l, bool wide) {
  const long d = c.w->d_model;
  const float* mk = c.memkv + (size_t)l * ((size_t)(c.R / c.row_div) * c.Tm) * 2 * d;
  AttnParams a{};
  a.q = c.ws->q2; a.ldq = d; a.K = mk; a.V = mk + d; a.key_len = c.mem_len;
  a.row_stride = (long)c.Tm * 2 * d; a.key_stride = 2 * d; a.row_div = c.row_div; a.nkeys = c.Tm;
  attn_output(c, wide, a);
  return a;
}

// dec_gemm_kernel<PRO_PLAIN>: Y[M, N] = act(X W^T + bias).  g: the fields the launches of a step share (Step::shared)
DecGemmParams plain_proj(DecGemmParams g, const float* X, long ldx, const float* Wp, const float* bias, float* Y, long ldy,
                         int N, int K, int relu) {
  g.X = X; g.ldx = ldx; g.Wp = Wp; g.bias = bias; g.Y = Y; g.ldy = ldy; g.N = N; g.K = K; g.relu = relu;
  return g;
}

// The same over rows a producer makes in the prologue (K = d_model): the pending join j (PRO_ADDLN) or the embedding of the
// step's tokens (PRO_EMBED: from g, j is not read).  The produced rows are also stored to xout unless it is null.
DecGemmParams produced_proj(DecGemmParams g, const Join& j, int d, float* xout, long ldxo, const float* Wp, const float* bias,
                            float* Y, long ldy, int N, int relu) {
  g = plain_proj(g, j.x, d, Wp, bias, Y, ldy, N, d, relu);
  g.Y2 = j.y; g.ldy2 = d; g.ln_w = j.ln_w; g.ln_b = j.ln_b; g.xout = xout; g.ldxo = ldxo;
  return g;
}

// A produced_proj launch with no join pending, for a keyword decoder: the embedding's descriptor plus the keyword operands
DecGemmParams keyword_embed(DecGemmParams p, const ac_trm_keyword* kw, int d) {
  p.X = kw->kwp; p.ldx = d; p.ln_w = kw->ln_w; p.ln_b = kw->ln_b; p.kw_div = kw->row_div;
  return p;
}

// Null or misaligned keyword operands (the producer reads them with 16-byte loads), or a row_div other than the search's
int check_keyword(const ac_trm_keyword* kw, int row_div) {
  if (!kw || !kw->kwp || !kw->ln_w || !kw->ln_b || kw->row_div != row_div) return AC_ERR_ARG;
  if (((uintptr_t)kw->kwp | (uintptr_t)kw->ln_w | (uintptr_t)kw->ln_b) & 15) return AC_ERR_ARG;
  return AC_OK;
}

// The wide twin of a produced_proj launch (csrc/decoder_wide.hip) over the same descriptor: producer 2 = the join, 1 = the
// embedding.  ntb: 64-column groups per workgroup; split_out: Y leaves as a fragment pack
int wide_produced(const DecGemmParams& p, int producer, int ntb, int split_out, hipStream_t s) {
  return ac_dec_wide_gemm(producer, p.X, p.ldx, p.Y2, p.ldy2, p.ln_w, p.ln_b, p.tok, p.tok_stride, p.t, p.emb, p.pe, p.emb_scale,
                          p.xout, p.ldxo, p.Wp, p.bias, p.Y, p.ldy, p.M, p.N, p.K, p.relu, ntb, split_out, (void*)s);
}

// One per-row sub-layer (dec_row_kernel / dec_row2_kernel): xout = LayerNorm(res + out-projection of attention a), rows of d
// floats (j.y: the kernel computes it).  The self-attention one also projects its row to the cross query: the caller names those.
RowParams row_params(const AttnParams& a, const Join& j, const float* WoT, const float* bo, float* xout, long d) {
  RowParams r{};
  r.a = a; r.res = j.x; r.ldres = d; r.WoT = WoT; r.bo = bo; r.ln_w = j.ln_w; r.ln_b = j.ln_b; r.xout = xout; r.ldxo = d;
  return r;
}

// One decoder position for R rows.  tokens/mask: [R][tok_stride]; the input token is column t.  cache: active KV cache set.
// Returns through `fin` the operands of the LAST residual join, which the caller fuses into the classifier projection
// (classifier_step), and the route.  `live` (struct Live): the rows of finished segments of an on-device search are skipped
// by every kernel of the step (Live() = every row runs; the wide route's attention does not skip, see attn_output).
//
// One layer loop for every route (struct Route); a route only chooses the kernel behind a sub-layer:
//   general  attn_step_kernel and dec_gemm_kernel, 8 launches per layer, any supported shape
//   wide     the same 8 with every projection on the bf16 matrix cores in 32-row workgroups (csrc/decoder_wide.hip); rows that
//            feed a projection without a join in front (attention contexts, feed-forward hidden rows) travel as bf16-plane
//            fragment packs (ws.attp, ws.ffp)
//   rows     self attention .. norm2 one row per workgroup in ONE launch (rows_split: one per attention); the feed forward
//            reads the materialised x2: 4 launches per layer (5)
//   hybrid   general or rows with the joined QKV projection (layer 1 on; the embedding one stays narrow) on its wide twin
// kw (may be null): the keyword operands of a KeywordProbTransformerDecoder, checked by the caller (check_keyword) - the first
// projection then embeds through PRO_EMBED_KW with kwp row r / row_div; nothing else of the step changes.
int decoder_step(const ac_trm_weights* w, const float* memkv, const int* mem_len, int R, int row_div, int Tm,
                 int max_len, int t, const int* tok, const unsigned char* mask, long tok_stride, float* cache,
                 const Ws& ws, StepOut* fin, hipStream_t s, const Live& live, const ac_trm_keyword* kw = nullptr) {
  if (t >= w->max_pos || !w->step_pk) return AC_ERR_ARG;
  const int d = w->d_model, ff = w->dim_ff;
  const float* pk = w->step_pk;
  const Route rt = resolve_route(w, R, Tm, t, kw != nullptr);
  const PackOffsets po = pack_layout(w);
  Step c{};
  c.w = w; c.ws = &ws; c.memkv = memkv; c.mem_len = mem_len; c.cache = cache; c.mask = mask;
  c.R = R; c.row_div = row_div; c.Tm = Tm; c.max_len = max_len; c.t = t;
  DecGemmParams& g = c.shared;
  g.tok = tok; g.tok_stride = tok_stride; g.t = t; g.emb = w->emb; g.pe = w->pe; g.emb_scale = sqrtf((float)d);
  g.M = R; g.ntb = rt.ntb; g.live = live;
  // a projection of rows a launch wrote: X[R, K] (wide: their fragment pack) -> Y[R, N]
  auto plain = [&](const float* X, size_t wp, const float* bias, float* Y, int N, int K, int relu) {
    if (rt.wide)
      return ac_dec_wide_gemm(0, X, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0.f, nullptr, 0, pk + wp,
                              bias, Y, N, R, N, K, relu, 1, 0, (void*)s);
    return launch_dec_gemm<PRO_PLAIN>(plain_proj(g, X, K, pk + wp, bias, Y, N, N, K, relu), s);   // K beyond one chunk: the launcher takes one tile per block
  };
  // a projection with a producer: the join j, or with none pending the embedding; the produced rows go to xout as well.
  // wide_twin: on the wide kernel (out & PACK_OUT: Y leaves as a fragment pack); the hybrid's carries no embedding operands
  enum { RELU = 1, PACK_OUT = 2 };
  DecGemmParams rows_only{}; rows_only.M = R;
  auto produced = [&](const Join& j, bool wide_twin, float* xout, size_t wp, const float* bias, float* Y, int N, int out) {
    const bool pack_out = out & PACK_OUT;
    const DecGemmParams p = produced_proj(wide_twin && !rt.wide ? rows_only : g, j, d, xout, d, pk + wp, bias, Y,
                                          pack_out ? 0 : N, N, out & RELU);
    if (wide_twin) return wide_produced(p, j.x ? 2 : 1, 1, pack_out, s);
    if (j.x) return launch_dec_gemm<PRO_ADDLN>(p, s);
    return kw ? launch_dec_gemm<PRO_EMBED_KW>(keyword_embed(p, kw, d), s) : launch_dec_gemm<PRO_EMBED>(p, s);
  };
  auto attention = [&](const AttnParams& a) {
    hipLaunchKernelGGL(attn_step_kernel, dim3(R, w->nhead), dim3(64), 0, s, a);
    return ac_check_launch();
  };
  float *xa = ws.x, *xb = ws.x2;   // residual stream, ping-pong: a join reads one and writes the other
  // attention context rows / feed-forward hidden rows, as the route's projections read them
  float *ctx = rt.wide ? ws.attp : ws.att, *hid = rt.wide ? ws.ffp : ws.ff;
  Join j{};
  for (int l = 0; l < w->nlayers; ++l) {
    const ac_trm_layer& L = w->layer[l];
    const PackLayout& P = po.layer[l];
    const ProjOffsets& W = rt.wide ? P.w : P.n;
    const AttnParams self = self_attn_params(c, l, rt.wide), cross = cross_attn_params(c, l, rt.wide);
    const bool qkv_twin = rt.wide || (rt.hybrid && l > 0);
    AC_TRY(produced(j, qkv_twin, xa, qkv_twin ? P.w.sa_in : P.n.sa_in, L.sa_in_b, ws.qkv, 3 * d, 0));
    if (rt.rows) {
      RowParams r1 = row_params(self, {xa, nullptr, L.n1_w, L.n1_b}, pk + P.sa_outT, L.sa_out_b, xb, d);    // x1 -> xb
      r1.WqT = pk + P.ca_qT; r1.bq = L.ca_in_b; r1.qout = ws.q2; r1.ldqo = d;
      const RowParams r2 = row_params(cross, {xb, nullptr, L.n2_w, L.n2_b}, pk + P.ca_outT, L.ca_out_b, xa, d);   // x2 -> xa
      if (rt.rows_split) {
        hipLaunchKernelGGL(dec_row_kernel, dim3(R), dim3(256), 0, s, r1);
        AC_TRY(ac_check_launch());
        hipLaunchKernelGGL(dec_row_kernel, dim3(R), dim3(256), 0, s, r2);
      } else {
        hipLaunchKernelGGL(dec_row2_kernel, dim3(R), dim3(256), 0, s, r1, r2);
      }
      AC_TRY(ac_check_launch());
      AC_TRY(plain(xa, W.l1, L.l1_b, hid, ff, d, 1));
    } else {
      AC_TRY(attention(self));
      AC_TRY(plain(ctx, W.sa_out, L.sa_out_b, ws.tmp, d, d, 0));
      AC_TRY(produced({xa, ws.tmp, L.n1_w, L.n1_b}, rt.wide, xb, W.ca_q, L.ca_in_b, ws.q2, d, 0));   // x1 -> xb
      AC_TRY(attention(cross));
      AC_TRY(plain(ctx, W.ca_out, L.ca_out_b, ws.tmp, d, d, 0));
      AC_TRY(produced({xb, ws.tmp, L.n2_w, L.n2_b}, rt.wide, xa, W.l1, L.l1_b, hid, ff, RELU | (rt.wide ? PACK_OUT : 0)));   // x2 -> xa
    }
    AC_TRY(plain(hid, W.l2, L.l2_b, ws.tmp, d, ff, 0));
    // x3 = LN3(x2 + ff) is produced by the next consumer (next layer's QKV or the caller's projection)
    j = {xa, ws.tmp, L.n3_w, L.n3_b};
    float* tswap = xa; xa = xb; xb = tswap;  // next layer writes its input into the other buffer
  }
  fin->join = j; fin->route = rt;
  return AC_OK;
}

// logits[R, V] = LayerNorm(fin.join) W_cls^T, the normalised rows also stored to xout (= `embed`).  scratch: R x d_model
// floats for the normalised rows of the LayerNorm + ac_gemm form when xout is null
int classifier_step(const ac_trm_weights* w, const StepOut& fin, int R, float* xout, long ldxo, float* logit,
                    long ldl, hipStream_t s, const Live& live, float* scratch = nullptr) {
  const Route& rt = fin.route;
  const Join& j = fin.join;
  const int d = w->d_model;
  const PackOffsets po = pack_layout(w);
  DecGemmParams g{}; g.M = R;
  if ((rt.wide || rt.hybrid) && (!xout || (ldxo % 4 == 0 && !((uintptr_t)xout & 15))))
    return wide_produced(produced_proj(g, j, d, xout, ldxo, w->step_pk + po.wcls, nullptr, logit, ldl, w->vocab, 0), 2,
                         rt.wide_cls_ntb, 0, s);
  if (rt.cls_ln_gemm && (xout || scratch) && w->cls_w) {
    float* nx = xout ? xout : scratch;
    const long ldn = xout ? ldxo : (long)d;
    AC_TRY(launch_ln(j.x, j.y, j.ln_w, j.ln_b, nx, R, d, d, d, ldn, s, live));
    return ac_gemm(nx, ldn, 1, w->cls_w, 1, d, logit, ldl, R, w->vocab, d, nullptr, 0, 0.f, 1, 0.f, 0, nullptr, 0, nullptr, 0,
                   (void*)s);
  }
  g.ntb = rt.cls_ntb; g.live = live;
  return launch_dec_gemm<PRO_ADDLN>(produced_proj(g, j, d, xout, ldxo, w->step_pk + po.cls, nullptr, logit, ldl, w->vocab, 0), s);
}

}  // namespace

extern "C" int ac_abi_version(void) { return AC_ABI_VERSION; }

extern "C" int ac_add_layernorm(const float* x, const float* y, const float* w, const float* b, float* out,
                                int rows, int d, long ldx, long ldy, long ldo, void* stream) {
  if (!x || !w || !b || !out || rows <= 0 || d <= 0 || d > 1024) return AC_ERR_ARG;
  return launch_ln(x, y, w, b, out, rows, d, ldx, ldy, ldo, (hipStream_t)stream);
}

extern "C" int ac_trm_memory(const ac_trm_weights* w, const float* attn_emb, int R, int Tm, float* memkv,
                             float* tmp, void* stream) {
  AC_TRY(check_weights(w));
  if (!attn_emb || !memkv || !tmp || R <= 0 || Tm <= 0 || Tm > MAX_KEYS) return AC_ERR_ARG;
  const int d = w->d_model, rows = R * Tm;
  hipStream_t s = (hipStream_t)stream;
  // attn_proj: Linear -> ReLU -> (Dropout: identity in eval) -> LayerNorm
  AC_TRY(ac_linear(attn_emb, w->proj_w, w->proj_b, tmp, rows, d, w->attn_emb_dim, w->attn_emb_dim,
                   w->attn_emb_dim, d, 1, stream));
  AC_TRY(launch_ln(tmp, nullptr, w->proj_ln_w, w->proj_ln_b, tmp, rows, d, d, 0, d, s));
  // cross-attention K and V of every layer: rows d..3d-1 of multihead_attn.in_proj
  for (int l = 0; l < w->nlayers; ++l) {
    const ac_trm_layer& L = w->layer[l];
    AC_TRY(ac_linear(tmp, L.ca_in_w + (size_t)d * d, L.ca_in_b + d, memkv + (size_t)l * rows * 2 * d, rows,
                     2 * d, d, d, d, 2 * d, 0, stream));
  }
  return AC_OK;
}

extern "C" long ac_trm_step_pack_floats(const ac_trm_weights* w) {
  if (check_weights(w) != AC_OK) return -1;
  return (long)pack_layout(w).total;
}

extern "C" int ac_trm_pack_step_weights(const ac_trm_weights* w, float* out, void* stream) {
  AC_TRY(check_weights(w));
  if (!out) return AC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int d = w->d_model, ff = w->dim_ff;
  const PackOffsets po = pack_layout(w);
  const bool wide = wide_shape_ok(w);
  auto wpack = [&](const float* W, int N, int K, float* dst) {
    return wide ? ac_dec_wide_pack(W, (long)K, N, K, dst, stream) : AC_OK;
  };
  auto pack = [&](const float* W, int N, int K, float* dst) {
    const size_t n4 = packed_floats(N, K) / 4;
    hipLaunchKernelGGL(pack_frag_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, W, (long)K, N, K, dst);
    return ac_check_launch();
  };
  for (int l = 0; l < w->nlayers; ++l) {
    const ac_trm_layer& L = w->layer[l];
    const PackLayout& P = po.layer[l];
    AC_TRY(pack(L.sa_in_w, 3 * d, d, out + P.n.sa_in));
    AC_TRY(pack(L.sa_out_w, d, d, out + P.n.sa_out));
    AC_TRY(pack(L.ca_in_w, d, d, out + P.n.ca_q));  // rows 0..d-1 of in_proj = the query projection
    AC_TRY(pack(L.ca_out_w, d, d, out + P.n.ca_out));
    AC_TRY(pack(L.l1_w, ff, d, out + P.n.l1));
    AC_TRY(pack(L.l2_w, d, ff, out + P.n.l2));
    AC_TRY(wpack(L.sa_in_w, 3 * d, d, out + P.w.sa_in));
    AC_TRY(wpack(L.sa_out_w, d, d, out + P.w.sa_out));
    AC_TRY(wpack(L.ca_in_w, d, d, out + P.w.ca_q));
    AC_TRY(wpack(L.ca_out_w, d, d, out + P.w.ca_out));
    AC_TRY(wpack(L.l1_w, ff, d, out + P.w.l1));
    AC_TRY(wpack(L.l2_w, d, ff, out + P.w.l2));
    const float* src[3] = {L.sa_out_w, L.ca_in_w, L.ca_out_w};
    const size_t dst[3] = {P.sa_outT, P.ca_qT, P.ca_outT};
    for (int i = 0; i < 3; ++i) {
      hipLaunchKernelGGL(transpose_sq_kernel, dim3(d / 32, d / 32), dim3(32, 8), 0, s, src[i], (long)d, d, out + dst[i]);
      AC_TRY(ac_check_launch());
    }
  }
  AC_TRY(pack(w->cls_w, w->vocab, d, out + po.cls));
  return wpack(w->cls_w, w->vocab, d, out + po.wcls);
}

extern "C" long ac_trm_workspace_floats(const ac_trm_weights* w, int rows, int max_len) {
  if (check_weights(w) != AC_OK || rows <= 0 || max_len <= 0) return -1;
  return (long)carve(w, rows, max_len, nullptr).total;
}

// The on-device search of ac_trm_greedy / ac_trm_sample: `sp` null = the argmax pick, else the sampler with these
// method parameters (its row / bookkeeping fields are filled per step here).
// The B rows are `segments` batches of B / segments rows, each searched as the reference searches a batch of its own: its
// loop ends when every row of THAT batch has emitted <end> (base.py:167, :206-211).  The launch sequence is fixed - it is
// captured into a graph - so the end is data: from then on every workgroup of every launch that holds only rows of ended
// segments returns before its first load (struct Live), and a last launch clears the columns of the steps not run.
// row_div: rows per clip - row r reads the memory K / V and the length of clip r / row_div (memkv and mem_len hold
// B / row_div clips), as the rows of a beam do; 1 = a clip per row.
static int trm_search(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int segments, int Tm,
                      int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                      float* embed, int* unfinished_cnt, float* ws_base, const SampleParams* sp, void* stream,
                      const ac_trm_keyword* kw = nullptr, int row_div = 1, const ac_logit_rules* rules = nullptr,
                      float* plane = nullptr, long ld_plane = 0) {
  AC_TRY(check_weights(w));
  // rules: every step's pick reads the constrained copy of the step's logits in `plane` (csrc/logit_rules.hip)
  if (rules && (ac_logit_rules_check(rules, w->vocab) != AC_OK || !plane || ld_plane < w->vocab)) return AC_ERR_ARG;
  if (!memkv || !mem_len || !seq || !logit || !logprob || !embed || !unfinished_cnt || !ws_base) return AC_ERR_ARG;
  if (B <= 0 || Tm <= 0 || Tm > MAX_KEYS || max_len <= 0 || max_len > w->max_pos) return AC_ERR_ARG;
  if (segments <= 0 || B % segments || row_div <= 0 || B % row_div) return AC_ERR_ARG;
  if (w->vocab > PICK_MAXV) return AC_ERR_ARG;
  if (sp && (ac_sample_check(w->vocab, sp->method, sp->k, sp->top_p, sp->temp) != AC_OK || !sp->seed)) return AC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const Ws ws = carve(w, B, max_len, ws_base);
  const int d = w->d_model, V = w->vocab;
  const int n_init = B * (max_len + 1);
  hipLaunchKernelGGL(greedy_init_kernel, dim3((n_init + 255) / 256), dim3(256), 0, s, seq, logprob, ws.tok,
                     ws.mask, ws.unfinished, unfinished_cnt, segments * max_len, B, max_len, start_idx, end_idx, pad_idx);
  AC_TRY(ac_check_launch());
  Live live;
  live.cnt = unfinished_cnt; live.seg_rows = B / segments; live.max_len = max_len;
  for (int t = 0; t < max_len; ++t) {
    StepOut fin;
    live.t = t;
    AC_TRY(decoder_step(w, memkv, mem_len, B, row_div, Tm, max_len, t, ws.tok, ws.mask, max_len + 1, ws.cache[0], ws,
                        &fin, s, live, kw));
    AC_TRY(classifier_step(w, fin, B, embed + (size_t)t * d, (long)max_len * d, logit + (size_t)t * V,
                           (long)max_len * V, s, live));
    const float* picked = logit + (size_t)t * V;   // what the pick reads: the step's logits, or their constrained copy
    long ld_picked = (long)max_len * V;
    if (rules) {
      AC_TRY(ac_logit_rules_launch(picked, ld_picked, plane, ld_plane, B, V, ws.tok, max_len + 1, t, rules, unfinished_cnt,
                                   live.seg_rows, max_len, s));
      picked = plane; ld_picked = ld_plane;
    }
    if (sp) {
      SampleParams q = *sp;
      q.logit = picked; q.ldl = ld_picked; q.rows = B; q.V = V; q.t = t; q.word = nullptr;
      q.logprob = logprob + t; q.ld_lp = max_len;
      q.seq = seq; q.max_len = max_len; q.end_idx = end_idx; q.pad_idx = pad_idx;
      q.tok = ws.tok; q.mask = ws.mask; q.unfinished = ws.unfinished; q.cnt = unfinished_cnt; q.seg_rows = live.seg_rows;
      AC_TRY(ac_sample_launch(q, s));
      continue;
    }
    PickParams p;
    p.logit = picked; p.ldl = ld_picked;
    p.V = V; p.t = t; p.max_len = max_len; p.end_idx = end_idx; p.pad_idx = pad_idx;
    p.seq = seq; p.logprob = logprob; p.tok = ws.tok; p.mask = ws.mask; p.unfinished = ws.unfinished;
    p.cnt = unfinished_cnt; p.seg_rows = live.seg_rows;
    hipLaunchKernelGGL(greedy_pick_kernel, dim3(B), dim3(256), 0, s, p);
    AC_TRY(ac_check_launch());
  }
  if (max_len > 1) {
    hipLaunchKernelGGL(search_finalize_kernel, dim3(B, max_len - 1), dim3(256), 0, s, logit, embed, live, V, d);
    AC_TRY(ac_check_launch());
  }
  return AC_OK;
}

extern "C" int ac_trm_greedy(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int Tm,
                             int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit,
                             float* logprob, float* embed, int* unfinished_cnt, float* ws_base, void* stream) {
  return trm_search(w, memkv, mem_len, B, 1, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, nullptr, stream);
}

extern "C" int ac_trm_greedy_segments(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int segments,
                                      int Tm, int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq,
                                      float* logit, float* logprob, float* embed, int* unfinished_cnt, float* ws_base,
                                      void* stream) {
  return trm_search(w, memkv, mem_len, B, segments, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, nullptr, stream);
}

extern "C" int ac_trm_sample(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int Tm, int max_len,
                             int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                             float* embed, int* unfinished_cnt, float* ws_base, int method, int k, float top_p, float temp,
                             const uint64_t* seed_dev, void* stream) {
  SampleParams sp = {};
  sp.method = method; sp.k = k; sp.top_p = top_p; sp.temp = temp; sp.seed = seed_dev;
  return trm_search(w, memkv, mem_len, B, 1, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, &sp, stream);
}

extern "C" int ac_trm_sample_multi(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B,
                                   int samples_per_clip, int Tm, int max_len, int start_idx, int end_idx, int pad_idx,
                                   int64_t* seq, float* logit, float* logprob, float* embed, int* unfinished_cnt,
                                   float* ws_base, int method, int k, float top_p, float temp, const uint64_t* seed_dev,
                                   void* stream) {
  // the row indices of the search (tokens, masks, the initialisation) are ints
  if (B <= 0 || samples_per_clip < 1 || max_len <= 0 || (long)B * samples_per_clip * ((long)max_len + 1) > 0x7fffffffL)
    return AC_ERR_ARG;
  SampleParams sp = {};
  sp.method = method; sp.k = k; sp.top_p = top_p; sp.temp = temp; sp.seed = seed_dev;
  return trm_search(w, memkv, mem_len, B * samples_per_clip, 1, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob,
                    embed, unfinished_cnt, ws_base, &sp, stream, nullptr, samples_per_clip);
}

static int forward_tokens(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len, int N,
                          int Tm, const int* tokens, const unsigned char* key_mask, int T, float* embed, float* logit,
                          float* ws_base, void* stream) {
  AC_TRY(check_weights(w));
  if (!memkv || !mem_len || !tokens || !embed || !logit || !ws_base) return AC_ERR_ARG;
  if (N <= 0 || Tm <= 0 || Tm > MAX_KEYS || T <= 0 || T > w->max_pos) return AC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const Ws ws = carve(w, N, T, ws_base);
  const int d = w->d_model, V = w->vocab;
  for (int t = 0; t < T; ++t) {
    StepOut fin;
    AC_TRY(decoder_step(w, memkv, mem_len, N, 1, Tm, T, t, tokens, key_mask, T, ws.cache[0], ws, &fin, s, Live(), kw));
    AC_TRY(classifier_step(w, fin, N, embed + (size_t)t * d, (long)T * d, logit + (size_t)t * V, (long)T * V, s, Live()));
  }
  return AC_OK;
}

extern "C" int ac_trm_forward_tokens(const ac_trm_weights* w, const float* memkv, const int* mem_len, int N,
                                     int Tm, const int* tokens, const unsigned char* key_mask, int T,
                                     float* embed, float* logit, float* ws_base, void* stream) {
  return forward_tokens(w, nullptr, memkv, mem_len, N, Tm, tokens, key_mask, T, embed, logit, ws_base, stream);
}

extern "C" int ac_trm_step_logits(const ac_trm_weights* w, const float* memkv, const int* mem_len, int R, int row_div,
                                  int Tm, int max_len, int t, const int* tokens, const unsigned char* key_mask,
                                  int cache_set, float* logit, long ldl, float* embed, long ld_embed, float* ws_base,
                                  void* stream) {
  AC_TRY(check_weights(w));
  if (!memkv || !mem_len || !tokens || !key_mask || !logit || !ws_base) return AC_ERR_ARG;
  if (R <= 0 || row_div <= 0 || R % row_div || Tm <= 0 || Tm > MAX_KEYS || t < 0 || t >= max_len) return AC_ERR_ARG;
  if (max_len > w->max_pos || ldl < w->vocab || (cache_set != 0 && cache_set != 1)) return AC_ERR_ARG;
  if (embed && ld_embed < w->d_model) return AC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const Ws ws = carve(w, R, max_len, ws_base);
  StepOut fin;
  AC_TRY(decoder_step(w, memkv, mem_len, R, row_div, Tm, max_len, t, tokens, key_mask, max_len + 1,
                      ws.cache[cache_set], ws, &fin, s, Live()));
  return classifier_step(w, fin, R, embed, ld_embed, logit, ldl, s, Live(), ws.att);   // ws.att: dead once the last layer has consumed it
}

static int beam_step(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len, int B,
                     int beam, int Tm, int max_len, int t, float temp, const int* tokens, const unsigned char* key_mask,
                     const float* cum_logprob, float* top_val, int* top_idx, float* ws_base, void* stream,
                     const ac_logit_rules* rules = nullptr, float* plane = nullptr) {
  AC_TRY(check_weights(w));
  if (!memkv || !mem_len || !tokens || !cum_logprob || !top_val || !top_idx || !ws_base) return AC_ERR_ARG;
  if (rules && (ac_logit_rules_check(rules, w->vocab) != AC_OK || !plane)) return AC_ERR_ARG;
  if (B <= 0 || beam <= 0 || beam > 64 || Tm <= 0 || Tm > MAX_KEYS || t < 0 || t >= max_len) return AC_ERR_ARG;
  if (max_len > w->max_pos || !(temp > 0.f)) return AC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int R = B * beam, V = w->vocab;
  const Ws ws = carve(w, R, max_len, ws_base);
  StepOut fin;
  AC_TRY(decoder_step(w, memkv, mem_len, R, beam, Tm, max_len, t, tokens, key_mask, max_len + 1,
                      ws.cache[t & 1], ws, &fin, s, Live(), kw));
  AC_TRY(classifier_step(w, fin, R, nullptr, 0, ws.lg, V, s, Live(), ws.att));   // ws.att: dead once the last layer has consumed it
  float* lg = ws.lg;   // the rows the scores are formed from: the step's logits, or their constrained copy
  if (rules) {
    AC_TRY(ac_logit_rules_launch(ws.lg, V, plane, V, R, V, tokens, max_len + 1, t, rules, nullptr, 1, 0, s));
    lg = plane;
  }
  static const bool two_kernels = getenv("AUDIOCAPTION_BEAM_TOPK") && !strcmp(getenv("AUDIOCAPTION_BEAM_TOPK"), "scan");
  if (beam <= 8 && V <= 8192 && !two_kernels) {
    // scores + per-row candidates in one pass over registers, then a one-wave merge per clip; the candidates (2 x R x
    // beam words) go into the QKV scratch of the decoder step, which is dead until the next step starts
    float* cand_val = ws.qkv;
    int* cand_idx = (int*)(cand_val + (size_t)R * beam);
    if (V <= 5120) hipLaunchKernelGGL(beam_row_topk_kernel<20>, dim3(R), dim3(256), 0, s, lg, cum_logprob, temp, beam, V, cand_val, cand_idx);
    else hipLaunchKernelGGL(beam_row_topk_kernel<32>, dim3(R), dim3(256), 0, s, lg, cum_logprob, temp, beam, V, cand_val, cand_idx);
    AC_TRY(ac_check_launch());
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), 0, s, cand_val, cand_idx, beam, t == 0 ? 1 : beam, top_val, top_idx);
    return ac_check_launch();
  }
  float* lp = lg;  // in place: every element is read before it is written by the same thread
  hipLaunchKernelGGL(beam_logprob_kernel, dim3(R), dim3(256), 0, s, lg, cum_logprob, temp, lp, V);
  AC_TRY(ac_check_launch());
  hipLaunchKernelGGL(beam_topk_kernel, dim3(B), dim3(256), 0, s, lp, beam, t == 0 ? 1 : beam, V, top_val,
                     top_idx);
  return ac_check_launch();
}

extern "C" int ac_trm_beam_step(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int beam,
                                int Tm, int max_len, int t, float temp, const int* tokens,
                                const unsigned char* key_mask, const float* cum_logprob, float* top_val,
                                int* top_idx, float* ws_base, void* stream) {
  return beam_step(w, nullptr, memkv, mem_len, B, beam, Tm, max_len, t, temp, tokens, key_mask, cum_logprob, top_val, top_idx,
                   ws_base, stream);
}

// ---- the same searches with the rules of csrc/logit_rules.hip between a step's logits and its pick -------------------------
extern "C" int ac_trm_search_rules(const ac_trm_weights* w, const float* memkv, const int* mem_len, int R, int row_div, int Tm,
                                   int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit,
                                   float* logprob, float* embed, int* unfinished_cnt, float* ws_base, int method, int k,
                                   float top_p, float temp, const uint64_t* seed_dev, const ac_logit_rules* rules,
                                   float* plane, long ld_plane, void* stream) {
  // the row indices of the search (tokens, masks, the initialisation) are ints
  if (!rules || R <= 0 || max_len <= 0 || (long)R * ((long)max_len + 1) > 0x7fffffffL) return AC_ERR_ARG;
  if (rules->end_idx != end_idx) return AC_ERR_ARG;
  SampleParams sp = {};
  sp.method = method; sp.k = k; sp.top_p = top_p; sp.temp = temp; sp.seed = seed_dev;
  return trm_search(w, memkv, mem_len, R, 1, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, method == AC_SEARCH_GREEDY ? nullptr : &sp, stream, nullptr, row_div, rules, plane,
                    ld_plane);
}

extern "C" int ac_trm_beam_step_rules(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int beam, int Tm,
                                      int max_len, int t, float temp, const int* tokens, const unsigned char* key_mask,
                                      const float* cum_logprob, float* top_val, int* top_idx, float* ws_base,
                                      const ac_logit_rules* rules, float* plane, void* stream) {
  if (!rules) return AC_ERR_ARG;
  return beam_step(w, nullptr, memkv, mem_len, B, beam, Tm, max_len, t, temp, tokens, key_mask, cum_logprob, top_val, top_idx,
                   ws_base, stream, rules, plane);
}

// ---- keyword-conditioned decoder (KeywordProbTransformerDecoder): the same searches with the keyword operands --------------
extern "C" int ac_trm_kw_greedy_segments(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv,
                                         const int* mem_len, int B, int segments, int Tm, int max_len, int start_idx,
                                         int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob, float* embed,
                                         int* unfinished_cnt, float* ws_base, void* stream) {
  AC_TRY(check_keyword(kw, 1));
  return trm_search(w, memkv, mem_len, B, segments, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, nullptr, stream, kw);
}

extern "C" int ac_trm_kw_sample(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len,
                                int B, int Tm, int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq,
                                float* logit, float* logprob, float* embed, int* unfinished_cnt, float* ws_base, int method,
                                int k, float top_p, float temp, const uint64_t* seed_dev, void* stream) {
  AC_TRY(check_keyword(kw, 1));
  SampleParams sp = {};
  sp.method = method; sp.k = k; sp.top_p = top_p; sp.temp = temp; sp.seed = seed_dev;
  return trm_search(w, memkv, mem_len, B, 1, Tm, max_len, start_idx, end_idx, pad_idx, seq, logit, logprob, embed,
                    unfinished_cnt, ws_base, &sp, stream, kw);
}

extern "C" int ac_trm_kw_forward_tokens(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv,
                                        const int* mem_len, int N, int Tm, const int* tokens,
                                        const unsigned char* key_mask, int T, float* embed, float* logit, float* ws_base,
                                        void* stream) {
  AC_TRY(check_keyword(kw, 1));
  return forward_tokens(w, kw, memkv, mem_len, N, Tm, tokens, key_mask, T, embed, logit, ws_base, stream);
}

extern "C" int ac_trm_kw_beam_step(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len,
                                   int B, int beam, int Tm, int max_len, int t, float temp, const int* tokens,
                                   const unsigned char* key_mask, const float* cum_logprob, float* top_val, int* top_idx,
                                   float* ws_base, void* stream) {
  AC_TRY(check_keyword(kw, beam));
  return beam_step(w, kw, memkv, mem_len, B, beam, Tm, max_len, t, temp, tokens, key_mask, cum_logprob, top_val, top_idx,
                   ws_base, stream);
}

// The first launch of a keyword decoder's step alone: xout [R][d] = the produced embedding rows, qkv [R][3 d] = layer 0's
// self-attention in-projection of them (what decoder_step writes to its workspace before anything overwrites it)
extern "C" int ac_trm_kw_embed_qkv(const ac_trm_weights* w, const ac_trm_keyword* kw, int R, int row_div, int t,
                                   const int* tokens, long tok_stride, float* xout, float* qkv, void* stream) {
  AC_TRY(check_weights(w));
  if (row_div <= 0) return AC_ERR_ARG;
  AC_TRY(check_keyword(kw, row_div));
  if (!tokens || !xout || !qkv || !w->step_pk || R <= 0 || R % row_div || t < 0 || t >= w->max_pos || tok_stride <= t)
    return AC_ERR_ARG;
  if (((uintptr_t)xout | (uintptr_t)qkv) & 15) return AC_ERR_ARG;
  const int d = w->d_model;
  DecGemmParams g{};
  g.tok = tokens; g.tok_stride = tok_stride; g.t = t; g.emb = w->emb; g.pe = w->pe; g.emb_scale = sqrtf((float)d);
  g.M = R; g.ntb = 1;
  const ac_trm_layer& L = w->layer[0];
  const DecGemmParams p = produced_proj(g, Join{}, d, xout, d, w->step_pk + pack_layout(w).layer[0].n.sa_in, L.sa_in_b, qkv,
                                        3 * d, 3 * d, 0);
  return launch_dec_gemm<PRO_EMBED_KW>(keyword_embed(p, kw, d), (hipStream_t)stream);
}

static int beam_update(const float* top_val, const int* top_idx, const int* tokens_in, int* tokens_out,
                       unsigned char* key_mask_out, float* cum_logprob, int* active, int* done_count, int* done_seq,
                       float* done_score, int* src_row, int* n_active, int B, int beam, int V, int max_len, int t,
                       int end_idx, int pad_idx, int done_capacity, int retire, void* stream) {
  if (!top_val || !top_idx || !tokens_in || !tokens_out || !key_mask_out || !cum_logprob || !active || !done_count ||
      !done_seq || !done_score || !src_row || !n_active || B <= 0 || beam <= 0 || beam > 64 || V <= 0 || max_len <= 0 ||
      t < 0 || t >= max_len || done_capacity <= 0)
    return AC_ERR_ARG;
  hipLaunchKernelGGL(beam_update_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, top_val, top_idx, tokens_in, tokens_out,
                     key_mask_out, cum_logprob, active, done_count, done_seq, done_score, src_row, n_active, beam, V,
                     max_len, t, end_idx, pad_idx, done_capacity, retire);
  return ac_check_launch();
}

extern "C" int ac_trm_beam_update(const float* top_val, const int* top_idx, const int* tokens_in, int* tokens_out,
                                  unsigned char* key_mask_out, float* cum_logprob, int* active, int* done_count,
                                  int* done_seq, float* done_score, int* src_row, int* n_active, int B, int beam, int V,
                                  int max_len, int t, int end_idx, int pad_idx, int done_capacity, void* stream) {
  return beam_update(top_val, top_idx, tokens_in, tokens_out, key_mask_out, cum_logprob, active, done_count, done_seq,
                     done_score, src_row, n_active, B, beam, V, max_len, t, end_idx, pad_idx, done_capacity, 1, stream);
}

extern "C" int ac_trm_beam_update_all(const float* top_val, const int* top_idx, const int* tokens_in, int* tokens_out,
                                      unsigned char* key_mask_out, float* cum_logprob, int* active, int* done_count,
                                      int* done_seq, float* done_score, int* src_row, int* n_active, int B, int beam,
                                      int V, int max_len, int t, int end_idx, int pad_idx, int done_capacity,
                                      void* stream) {
  return beam_update(top_val, top_idx, tokens_in, tokens_out, key_mask_out, cum_logprob, active, done_count, done_seq,
                     done_score, src_row, n_active, B, beam, V, max_len, t, end_idx, pad_idx, done_capacity, 0, stream);
}

// csrc/ensemble.hip merges its per-row candidates with the single-model search's kernel (ac_beam.h)
int ac_beam_merge_launch(const float* cand_val, const int* cand_idx, int B, int beam, int nrows, float* top_val,
                         int* top_idx, hipStream_t s) {
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), 0, s, cand_val, cand_idx, beam, nrows, top_val, top_idx);
  return ac_check_launch();
}

extern "C" int ac_trm_beam_reorder(const ac_trm_weights* w, int R, int max_len, int t, const int* src_row,
                                   float* ws_base, void* stream) {
  AC_TRY(check_weights(w));
  if (!src_row || !ws_base || R <= 0 || t < 0 || t >= max_len) return AC_ERR_ARG;
  const Ws ws = carve(w, R, max_len, ws_base);
  hipLaunchKernelGGL(cache_gather_kernel, dim3(R, 2 * w->nlayers), dim3(256), 0, (hipStream_t)stream,
                     ws.cache[t & 1], ws.cache[(t + 1) & 1], src_row, R, max_len, t, w->d_model,
                     ws.cache_set_stride, 2 * w->nlayers);
  return ac_check_launch();
}
