// HTS-AT audio encoder (a Swin Transformer over the folded log-mel) on gfx950: the kernels that are not GEMMs.
//
//   ac_htsat_patch_embed   bicubic stretch of the time axis + fold into the 256 x 256 image + 4x4 patch product + LayerNorm
//   ac_swin_window_attn    (shifted-)window attention: gather by addressing, scores and P V on v_mfma_f32_16x16x4_f32
//   ac_swin_patch_merge    2x2 gather in the reference's channel order + LayerNorm(4C)
//   ac_htsat_pool          mean over the frequency bins of a time frame -> attn_emb, mean over the frames -> fc_emb
//   ac_htsat_token_mean    mean over the tokens of a stage output (layer_i embeddings)
//   ac_gelu                exact (erf) GELU
//
// The linear layers (qkv, proj, fc1, fc2, the merge reduction) run on ac_gemm_bf16x3 (csrc/train.hip), the
// pre-norm LayerNorms on ac_add_layernorm (csrc/decoder.hip).  Replaces transformer_encoder.py:182-221 (PatchEmbed),
// :364-442 (WindowAttention), :525-556 (shift, partition, reverse), :568-604 (PatchMerging), :899-919 (tail), :933-951
// (reshape_wav2img) of the reference.
#include "ac_common.h"

namespace {

constexpr int HT_FRAMES = 1024;   // time frames of the folded image (spec_size * freq_ratio)
constexpr int HT_GRID = 64;       // tokens per image side (256 / 4)
constexpr int HT_TOKENS = HT_GRID * HT_GRID;

// torch's cubic convolution (upsample_bicubic2d, A = -0.75)
__device__ __forceinline__ float cubic_near(float t) { return ((1.25f * t - 2.25f) * t) * t + 1.0f; }                // |t| <= 1
__device__ __forceinline__ float cubic_far(float t) { return ((-0.75f * t + 3.75f) * t - 6.0f) * t + 3.0f; }         // 1 < |t| < 2

// One wave per token.  Pixel (i, j) of the token's 4x4 patch is image row 4r + i, column 4c + j; image row R is mel bin
// R % 64 of time chunk R / 64, so the pixel is frame (R / 64) * 256 + 4c + j of the stretched log-mel.  The stretch is
// torch's bicubic with align_corners: source position f (T - 1) / 1023, formed from the integer quotient and remainder, so
// the taps' fraction is exact to one rounding whatever T is.
__global__ __launch_bounds__(256) void htsat_patch_embed_kernel(const float* __restrict__ x, int T,
                                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                                const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                                float* __restrict__ out, int C, long ntok) {
  const int lane = threadIdx.x & 63;
  const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= ntok) return;   // per wave: the kernel has no barrier
  const int b = (int)(tok / HT_TOKENS), t = (int)(tok % HT_TOKENS);
  const int r = t / HT_GRID, c = t % HT_GRID;
  const int p = lane & 15, R = 4 * r + (p >> 2);
  const int mel = R & 63, frame = (R >> 6) * 256 + 4 * c + (p & 3);
  const float* xc = x + (long)b * T * 64 + mel;
  float v;
  if (T == HT_FRAMES) {
    v = xc[(long)frame * 64];
  } else {
    const int num = frame * (T - 1);
    const int i0 = num / (HT_FRAMES - 1);
    const float tt = (float)(num % (HT_FRAMES - 1)) / (float)(HT_FRAMES - 1);
    const float c0 = cubic_far(tt + 1.0f), c1 = cubic_near(tt), c2 = cubic_near(1.0f - tt), c3 = cubic_far(2.0f - tt);
    const float x0 = xc[(long)max(i0 - 1, 0) * 64], x1 = xc[(long)i0 * 64];
    const float x2 = xc[(long)min(i0 + 1, T - 1) * 64], x3 = xc[(long)min(i0 + 2, T - 1) * 64];
    v = x0 * c0 + x1 * c1 + x2 * c2 + x3 * c3;
  }
  float px[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) px[q] = lane_read(v, q);
  float y[4];   // C <= 256
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int ch = lane + 64 * n;
    y[n] = 0.f;
    if (ch < C) {
      float a = bias[ch];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 wv = *(const f32x4*)(w + (long)ch * 16 + q4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaf(wv[e], px[q4 * 4 + e], a);
      }
      y[n] = a;
      s += a;
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (lane + 64 * n < C) {
      const float d = y[n] - mean;
      q = fmaf(d, d, q);
    }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + 1e-5f);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int ch = lane + 64 * n;
    if (ch < C) out[tok * C + ch] = (y[n] - mean) * rstd * lnw[ch] + lnb[ch];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Window attention.  One workgroup per (window, head, clip): the window's 64 tokens are gathered from their un-shifted
// positions (shifted coordinate hs is row (hs + shift) % H of the input), q (scaled), k and v of the head staged in LDS,
// S = q k^T (64 x 64 x 24) and P v (64 x 24 x 64) on the exact-f32 16x16x4 MFMA: wave w owns rows 16w .. 16w + 15.
// v_mfma_f32_16x16x4_f32: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register r of lane l is
// D[4 * (l >> 4) + r][l & 15] - a score row lives in one 16-lane row, so the softmax reductions are DPP row reductions.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SW_WIN = 8, SW_N = 64, SW_HD = 24;
constexpr int SW_QP = 25, SW_VP = 33, SW_PP = 65;   // odd LDS pitches: the 16 rows a fragment read touches fall in 16 banks

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void swin_window_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                               float* __restrict__ out, int H, int W, int C, int shift) {
  __shared__ float qs[SW_N * SW_QP];
  __shared__ float ks[SW_N * SW_QP];
  __shared__ float vs[SW_N * SW_VP];
  __shared__ float ps[4][16 * SW_PP];
  __shared__ int tok_of[SW_N];
  __shared__ int region_of[SW_N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nww = W / SW_WIN;
  const int wi = blockIdx.x / nww, wj = blockIdx.x % nww, head = blockIdx.y, b = blockIdx.z;
  if (tid < SW_N) {
    const int hs = wi * SW_WIN + (tid >> 3), ws = wj * SW_WIN + (tid & 7);
    tok_of[tid] = ((hs + shift) % H) * W + (ws + shift) % W;
    // the regions of the shifted image that hold tokens which were not neighbours before the roll
    const int rh = shift == 0 ? 0 : (hs < H - SW_WIN ? 0 : (hs < H - shift ? 1 : 2));
    const int rw = shift == 0 ? 0 : (ws < W - SW_WIN ? 0 : (ws < W - shift ? 1 : 2));
    region_of[tid] = rh * 3 + rw;
  }
  for (int e = tid; e < SW_N * 8; e += 256) vs[(e >> 3) * SW_VP + SW_HD + (e & 7)] = 0.f;   // v padded to 32 columns
  __syncthreads();
  const float* base = qkv + (long)b * H * W * 3 * C + head * SW_HD;
  const float scale = 0.2041241452319315f;   // 24 ** -0.5
  for (int e = tid; e < SW_N * 18; e += 256) {
    const int token = e / 18, quad = e % 18, which = quad / 6, d4 = (quad % 6) * 4;
    const f32x4 val = *(const f32x4*)(base + (long)tok_of[token] * 3 * C + which * C + d4);
    float* dst = which == 0 ? qs + token * SW_QP + d4 : which == 1 ? ks + token * SW_QP + d4 : vs + token * SW_VP + d4;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = which == 0 ? val[i] * scale : val[i];
  }
  __syncthreads();
  const int r0 = wave * 16, li = lane & 15, lk = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < SW_HD / 4; ++kk) {
    const float a = qs[(r0 + li) * SW_QP + kk * 4 + lk];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = mfma16(a, ks[(t * 16 + li) * SW_QP + kk * 4 + lk], acc[t]);
  }
  const float* hb = bias + (long)head * SW_N * SW_N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * lk + r;
    const int reg = region_of[row];
    float s[4];
    float m = -3.0e38f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = t * 16 + li;
      s[t] = acc[t][r] + hb[row * SW_N + col] + (region_of[col] != reg ? -100.0f : 0.0f);
      m = fmaxf(m, s[t]);
    }
    m = row16_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = expf(s[t] - m);
      sum += s[t];
    }
    sum = row16_sum(sum);
#pragma unroll
    for (int t = 0; t < 4; ++t) ps[wave][(4 * lk + r) * SW_PP + t * 16 + li] = s[t] / sum;
  }
  __syncthreads();
  f32x4 o[2];
  o[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < SW_N / 4; ++kk) {
    const float a = ps[wave][li * SW_PP + kk * 4 + lk];
#pragma unroll
    for (int n = 0; n < 2; ++n) o[n] = mfma16(a, vs[(kk * 4 + lk) * SW_VP + n * 16 + li], o[n]);
  }
  float* ob = out + (long)b * H * W * C + head * SW_HD;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int col = n * 16 + li;
    if (col < SW_HD) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ob[(long)tok_of[r0 + 4 * lk + r] * C + col] = o[n][r];
    }
  }
}

// One wave per merged token: channel q * C + c is channel c of x(2i + (q & 1), 2j + (q >> 1)).
constexpr int PM_MAX = 24;   // 4C <= 1536
__global__ __launch_bounds__(256) void swin_patch_merge_kernel(const float* __restrict__ x, const float* __restrict__ lnw,
                                                               const float* __restrict__ lnb, float* __restrict__ out,
                                                               int H, int W, int C, long ntok) {
  const int lane = threadIdx.x & 63;
  const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= ntok) return;   // per wave: the kernel has no barrier
  const int H2 = H / 2, W2 = W / 2, C4 = 4 * C;
  const int b = (int)(tok / (H2 * W2)), t = (int)(tok % (H2 * W2));
  const int i = t / W2, j = t % W2;
  const float* xb = x + (long)b * H * W * C;
  float v[PM_MAX];
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < PM_MAX; ++n) {
    const int idx = lane + 64 * n;
    v[n] = 0.f;
    if (idx < C4) {
      const int q = idx / C, c = idx % C;
      v[n] = xb[((long)(2 * i + (q & 1)) * W + 2 * j + (q >> 1)) * C + c];
      s += v[n];
    }
  }
  const float mean = wave_sum(s) / (float)C4;
  float qq = 0.f;
#pragma unroll
  for (int n = 0; n < PM_MAX; ++n)
    if (lane + 64 * n < C4) {
      const float d = v[n] - mean;
      qq = fmaf(d, d, qq);
    }
  const float rstd = rsqrtf(wave_sum(qq) / (float)C4 + 1e-5f);
#pragma unroll
  for (int n = 0; n < PM_MAX; ++n) {
    const int idx = lane + 64 * n;
    if (idx < C4) out[tok * C4 + idx] = (v[n] - mean) * rstd * lnw[idx] + lnb[idx];
  }
}

// One thread per (clip, channel): frame (chunk, w) is the mean of the fbins token rows of the chunk at column w.
__global__ __launch_bounds__(256) void htsat_pool_kernel(const float* __restrict__ x, float* __restrict__ attn,
                                                         float* __restrict__ fc, int Hh, int Ww, int C, int fbins) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  const int chunks = Hh / fbins;
  const float* xb = x + (long)b * Hh * Ww * C + c;
  float* ab = attn + (long)b * chunks * Ww * C + c;
  float tot = 0.f;
  for (int k = 0; k < chunks; ++k)
    for (int w = 0; w < Ww; ++w) {
      float s = 0.f;
      for (int f = 0; f < fbins; ++f) s += xb[((long)(k * fbins + f) * Ww + w) * C];
      s /= (float)fbins;
      ab[(long)(k * Ww + w) * C] = s;
      tot += s;
    }
  fc[(long)b * C + c] = tot / (float)(chunks * Ww);
}

// grid (C / 64, B): lane = channel, each wave a quarter of the tokens; fixed order of additions.
__global__ __launch_bounds__(256) void htsat_token_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int N,
                                                               int C) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
  float s = 0.f;
  if (c < C) {
    const float* xb = x + (long)b * N * C + c;
    for (int t = wave; t < N; t += 4) s += xb[(long)t * C];
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C) out[(long)b * C + c] = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / (float)N;
}

__global__ __launch_bounds__(256) void gelu_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = x[i];
    y[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
  }
}

}  // namespace

extern "C" {

int ac_htsat_patch_embed(const float* x, int B, int T, const float* w, const float* bias,
                         const float* ln_w, const float* ln_b, float* out, int C, void* stream) {
  if (!x || !w || !bias || !ln_w || !ln_b || !out || B <= 0 || T < 1 || T > HT_FRAMES || C <= 0 || C > 256 ||
      ((uintptr_t)w & 15) != 0)
    return AC_ERR_ARG;
  const long ntok = (long)B * HT_TOKENS;
  if (ntok / 4 > 0x7fffffffL) return AC_ERR_ARG;
  hipLaunchKernelGGL(htsat_patch_embed_kernel, dim3((unsigned)(ntok / 4)), dim3(256), 0, (hipStream_t)stream, x, T, w, bias, ln_w, ln_b, out, C, ntok);
  return ac_check_launch();
}

int ac_swin_window_attn(const float* qkv, const float* bias, float* out, int B, int H, int W, int C, int heads, int shift,
                        void* stream) {
  if (!qkv || !bias || !out || B <= 0 || B > 65535 || H <= 0 || W <= 0 || heads <= 0 || heads > 65535 || C != heads * SW_HD ||
      H % SW_WIN != 0 || W % SW_WIN != 0 || shift < 0 || shift >= SW_WIN || (shift > 0 && (H <= SW_WIN || W <= SW_WIN)) ||
      ((uintptr_t)qkv & 15) != 0)
    return AC_ERR_ARG;
  hipLaunchKernelGGL(swin_window_attn_kernel, dim3((H / SW_WIN) * (W / SW_WIN), heads, B), dim3(256), 0, (hipStream_t)stream,
                     qkv, bias, out, H, W, C, shift);
  return ac_check_launch();
}

int ac_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float* out, int B, int H, int W, int C,
                        void* stream) {
  if (!x || !ln_w || !ln_b || !out || B <= 0 || H <= 0 || W <= 0 || H % 2 != 0 || W % 2 != 0 || C <= 0 || 4 * C > 64 * PM_MAX)
    return AC_ERR_ARG;
  const long ntok = (long)B * (H / 2) * (W / 2);
  if ((ntok + 3) / 4 > 0x7fffffffL) return AC_ERR_ARG;
  hipLaunchKernelGGL(swin_patch_merge_kernel, dim3((unsigned)((ntok + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ln_w,
                     ln_b, out, H, W, C, ntok);
  return ac_check_launch();
}

int ac_htsat_pool(const float* x, float* attn, float* fc, int B, int Hh, int Ww, int C, int fbins, void* stream) {
  if (!x || !attn || !fc || B <= 0 || B > 65535 || Hh <= 0 || Ww <= 0 || C <= 0 || fbins <= 0 || Hh % fbins != 0)
    return AC_ERR_ARG;
  hipLaunchKernelGGL(htsat_pool_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, x, attn, fc, Hh, Ww, C,
                     fbins);
  return ac_check_launch();
}

int ac_htsat_token_mean(const float* x, float* out, int B, int N, int C, void* stream) {
  if (!x || !out || B <= 0 || B > 65535 || N <= 0 || C <= 0) return AC_ERR_ARG;
  hipLaunchKernelGGL(htsat_token_mean_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, x, out, N, C);
  return ac_check_launch();
}

int ac_gelu(const float* x, float* y, long n, void* stream) {
  if (!x || !y || n <= 0) return AC_ERR_ARG;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return ac_check_launch();
}

}  // extern "C"
