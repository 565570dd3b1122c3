// Encoder-level knowledge distillation (kd_wrapper.py:56-226: MseEncoderKdWrapper, ContraEncoderKdWrapper,
// ContraMseEncoderKdWrapper; hf_wrapper.py:1095-1111): the loss head between a student's projected clip embedding s [B][D]
// and a teacher's t [B][D], with its gradient with respect to both and to logit_scale, in at most four launches.
//
//   n(x)    = x / max(||x||_2, 1e-12)                                                         (F.normalize)
//   L       = logit_scale * n(s) n(t)^T                                                       (not exponentiated)
//   loss_c  = 0.5 * (mean_i CE(L_i., i) + mean_j CE(L_.j, j))
//   loss_m  = mean over B*D of (a - b)^2,  (a, b) = (n(s), n(t)) with L2NORM, (s, t) without
//   G       = (softmax_rows(L) + softmax_cols(L) - 2 I) / (2 B)
//   d n(s)  = logit_scale * G n(t),  d n(t) = logit_scale * G^T n(s),  d logit_scale = sum_ij G_ij cos_ij
//   dx      = (dy - y (y . dy)) / ||x||  through y = n(x), dy / 1e-12 where the clamp holds
//
//   launch 1  enc_kd_norm   one workgroup per clip: both norms, n(s) and n(t) into the workspace, the clip's MSE sum
//   launch 2  enc_kd_cos    cos = n(s) n(t)^T in 16 x 16 tiles staged through LDS            (contrastive kinds only)
//   launch 3  enc_kd_stats  one workgroup per row and per column of L: max, sum of exp(L - max), its cross-entropy term
//                           and sum_j softmax_j cos_j (the row's share of d logit_scale)        (contrastive kinds only)
//   launch 4  enc_kd_grad   one workgroup per row of ds and of dt (G against the other side's normalised rows, then the
//                           normalisation's backward), plus one that adds up the loss terms and d logit_scale
//
// Every sum has a fixed order and nothing is accumulated atomically: two calls on the same inputs give the same bits.  Sums
// over D and over B run in double (the head is a few microseconds of latency-bound work; the f64 FMAs are free), every
// exponential is taken of (L - max) <= 0, so a learnt logit_scale of 100 stays finite.  All loads are 4-byte scalar: rows
// may start at any float.
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

namespace {

constexpr int EK_MAXB = 512;
constexpr int EK_MAXD = 4096;
constexpr float EK_EPS = 1e-12f;
constexpr int EK_TILE = 16;
constexpr int EK_KC = 64;     // columns of a staged tile; rows are padded by one word against bank conflicts

// L_ij, rounded once: every kernel must see the SAME float for a logit.  This file is built with -ffp-contract=off
// (build.py EXTRA_FLAGS): fused into the subtraction of the maximum the product would be rounded in one place and not in
// another, and one clip's contrastive loss would be the product's rounding error (5.7e-8) instead of exactly 0.  The
// long sums below ask for their FMAs by name.
__device__ __forceinline__ float ek_logit(float scale, float cos) { return scale * cos; }

// workspace (floats): ns [B][D] | nt [B][D] | cos [B][B] | nrm_s [B] | nrm_t [B] | mse_row [B] | rstat [B][4] | cstat [B][4]
// nrm = max(||x||, eps), stored NEGATED where the clamp holds; stat = (max, sum exp(L - max), CE term, sum_j softmax_j cos_j)
struct EkWs {
  float *ns, *nt, *cos, *nrm_s, *nrm_t, *mse_row, *rstat, *cstat;
};
__host__ __device__ inline EkWs ek_ws(float* ws, int B, int D) {
  EkWs w;
  w.ns = ws;
  w.nt = w.ns + (long)B * D;
  w.cos = w.nt + (long)B * D;
  w.nrm_s = w.cos + (long)B * B;
  w.nrm_t = w.nrm_s + B;
  w.mse_row = w.nrm_t + B;
  w.rstat = w.mse_row + B;
  w.cstat = w.rstat + 4 * B;
  return w;
}

__global__ __launch_bounds__(256) void enc_kd_norm_kernel(const float* __restrict__ s, long ld_s, const float* __restrict__ t,
                                                          long ld_t, int B, int D, int kind, float* ws) {
  __shared__ double red[2][4];
  const EkWs w = ek_ws(ws, B, D);
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* sp = s + (long)i * ld_s;
  const float* tp = t + (long)i * ld_t;
  double acc[2] = {0.0, 0.0};
  for (int k = tid; k < D; k += 256) {
    const double a = sp[k], b = tp[k];
    acc[0] += a * a;
    acc[1] += b * b;
  }
  block_sums256(acc, red);
  const double ls = sqrt(acc[0]), lt = sqrt(acc[1]);
  const double ds_ = fmax(ls, (double)EK_EPS), dt_ = fmax(lt, (double)EK_EPS);
  if (tid == 0) {
    w.nrm_s[i] = ls < (double)EK_EPS ? -(float)ds_ : (float)ds_;
    w.nrm_t[i] = lt < (double)EK_EPS ? -(float)dt_ : (float)dt_;
  }
  const bool l2 = (kind & AC_ENC_KD_L2NORM) != 0;
  double m[1] = {0.0};
  for (int k = tid; k < D; k += 256) {
    const double a = sp[k], b = tp[k];
    const double ya = a / ds_, yb = b / dt_;
    w.ns[(long)i * D + k] = (float)ya;
    w.nt[(long)i * D + k] = (float)yb;
    const double d = l2 ? ya - yb : a - b;
    m[0] += d * d;
  }
  block_sums256(m, red);
  if (tid == 0) w.mse_row[i] = (float)m[0];
}

// cos[i][j] = ns[i] . nt[j]; thread (ty, tx) of a 16 x 16 tile, the two operand tiles staged EK_KC columns at a time
__global__ __launch_bounds__(256) void enc_kd_cos_kernel(int B, int D, float* ws) {
  __shared__ float As[EK_TILE][EK_KC + 1];
  __shared__ float Bs[EK_TILE][EK_KC + 1];
  const EkWs w = ek_ws(ws, B, D);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * EK_TILE, j0 = blockIdx.x * EK_TILE;
  double acc = 0.0;
  for (int k0 = 0; k0 < D; k0 += EK_KC) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EK_TILE * EK_KC / 256; ++e) {
      const int idx = e * 256 + tid, r = idx / EK_KC, c = idx % EK_KC;
      const bool ok = k0 + c < D;
      As[r][c] = ok && i0 + r < B ? w.ns[(long)(i0 + r) * D + k0 + c] : 0.f;
      Bs[r][c] = ok && j0 + r < B ? w.nt[(long)(j0 + r) * D + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 16
    for (int c = 0; c < EK_KC; ++c) acc = fma((double)As[ty][c], (double)Bs[tx][c], acc);
  }
  if (i0 + ty < B && j0 + tx < B) w.cos[(long)(i0 + ty) * B + j0 + tx] = (float)acc;
}

// workgroup r < B: row r of L; workgroup B + c: column c
__global__ __launch_bounds__(256) void enc_kd_stats_kernel(int B, int D, const float* __restrict__ logit_scale, float* ws) {
  __shared__ float redf[4];
  __shared__ double red[2][4];
  const EkWs w = ek_ws(ws, B, D);
  const int tid = threadIdx.x;
  const bool col = (int)blockIdx.x >= B;
  const int r = col ? blockIdx.x - B : blockIdx.x;
  const float scale = logit_scale[0];
  const long base = col ? r : (long)r * B, step = col ? B : 1;
  float c[EK_MAXB / 256], l[EK_MAXB / 256];
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < EK_MAXB / 256; ++e) {
    const int j = e * 256 + tid;
    c[e] = j < B ? w.cos[base + j * step] : 0.f;
    l[e] = j < B ? ek_logit(scale, c[e]) : -INFINITY;
    mx = fmaxf(mx, l[e]);
  }
  mx = block_max256(mx, redf);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < EK_MAXB / 256; ++e) {
    const float p = expf(l[e] - mx);      // 0 beyond B
    acc[0] += (double)p;
    acc[1] += (double)p * (double)c[e];
  }
  block_sums256(acc, red);
  if (tid == 0) {
    float* st = (col ? w.cstat : w.rstat) + 4 * r;
    const float diag = ek_logit(scale, w.cos[(long)r * B + r]);
    st[0] = mx;
    st[1] = (float)acc[0];
    st[2] = (float)((double)(mx - diag) + log(acc[0]));
    st[3] = (float)(acc[1] / acc[0]);
  }
}

// workgroup r < B: ds[r]; B <= r < 2B: dt[r - B]; 2B: the loss terms and d logit_scale.  NE = ceil(D / 256) rounded up to a
// built size: the row's gradient stays in registers between the product with G and the normalisation's backward.
template <int NE>
__global__ __launch_bounds__(256) void enc_kd_grad_kernel(const float* __restrict__ s, long ld_s, const float* __restrict__ t,
                                                          long ld_t, int B, int D, int kind,
                                                          const float* __restrict__ logit_scale, float* loss, float* ds,
                                                          float* dt, float* dscale, float gscale, const float* gscale_dev,
                                                          float* ws) {
  __shared__ float Gs[EK_MAXB];
  __shared__ double red[4][4];
  const EkWs w = ek_ws(ws, B, D);
  const int tid = threadIdx.x;
  const bool contra = (kind & AC_ENC_KD_CONTRA) != 0, mse = (kind & AC_ENC_KD_MSE) != 0, l2 = (kind & AC_ENC_KD_L2NORM) != 0;
  const float gs = gscale * (gscale_dev ? gscale_dev[0] : 1.0f);
  const float scale = contra ? logit_scale[0] : 0.f;

  if ((int)blockIdx.x == 2 * B) {
    // [0] sum of the rows' CE terms, [1] of the columns', [2] sum_r E_r + sum_c E_c - 2 sum_i cos_ii, [3] the MSE sum
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < B; i += 256) {
      if (contra) {
        a[0] += (double)w.rstat[4 * i + 2];
        a[1] += (double)w.cstat[4 * i + 2];
        a[2] += ((double)w.rstat[4 * i + 3] - (double)w.cos[(long)i * B + i]) +
                ((double)w.cstat[4 * i + 3] - (double)w.cos[(long)i * B + i]);
      }
      if (mse) a[3] += (double)w.mse_row[i];
    }
    block_sums256(a, red);
    if (tid == 0) {
      const float lc = contra ? (float)(0.5 * (a[0] + a[1]) / (double)B) : 0.f;
      const float lm = mse ? (float)(a[3] / ((double)B * (double)D)) : 0.f;
      loss[0] = lc + lm;
      loss[1] = lc;
      loss[2] = lm;
      if (dscale) dscale[0] = contra ? gs * (float)(a[2] / (2.0 * (double)B)) : 0.f;
    }
    return;
  }

  const bool teacher = (int)blockIdx.x >= B;
  const int r = teacher ? blockIdx.x - B : blockIdx.x;
  float* out = teacher ? dt : ds;
  if (!out) return;
  const float* mine = teacher ? w.nt : w.ns;        // y = n(x) of the side this row belongs to
  const float* other = teacher ? w.ns : w.nt;
  const float nrm = teacher ? w.nrm_t[r] : w.nrm_s[r];

  double g[NE];      // d loss / d y
#pragma unroll
  for (int e = 0; e < NE; ++e) g[e] = 0.0;
  if (contra) {
    // G over this row (student) or this column (teacher) of L
    const float* my = (teacher ? w.cstat : w.rstat) + 4 * r;
    const float* th = teacher ? w.rstat : w.cstat;
    const float mmax = my[0], minv = 1.0f / my[1];
    for (int j = tid; j < B; j += 256) {
      const float lij = ek_logit(scale, teacher ? w.cos[(long)j * B + r] : w.cos[(long)r * B + j]);
      const float p = expf(lij - mmax) * minv + expf(lij - th[4 * j]) / th[4 * j + 1];
      Gs[j] = (p - (j == r ? 2.0f : 0.0f)) / (2.0f * (float)B);
    }
    __syncthreads();
    for (int j = 0; j < B; ++j) {
      const double gj = (double)Gs[j];
      const float* o = other + (long)j * D;
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int k = e * 256 + tid;
        if (k < D) g[e] = fma(gj, (double)o[k], g[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) g[e] *= (double)scale;
  }
  const double inv_bd = 2.0 / ((double)B * (double)D);
  const float* yp = mine + (long)r * D;
  const float* op = other + (long)r * D;
  if (mse && l2) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int k = e * 256 + tid;
      if (k < D) g[e] += inv_bd * ((double)yp[k] - (double)op[k]);     // d/da (a - b)^2 and d/db (b - a)^2 alike
    }
  }
  const bool through_norm = contra || (mse && l2);
  double dot[1] = {0.0};
  if (through_norm && nrm > 0.f) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int k = e * 256 + tid;
      if (k < D) dot[0] += g[e] * (double)yp[k];
    }
    block_sums256(dot, red);
  }
  const float* xs = s + (long)r * ld_s;
  const float* xt = t + (long)r * ld_t;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int k = e * 256 + tid;
    if (k < D) {
      double v = 0.0;
      if (through_norm) v = nrm > 0.f ? (g[e] - (double)yp[k] * dot[0]) / (double)nrm : g[e] / (double)EK_EPS;
      if (mse && !l2) v += inv_bd * (teacher ? (double)xt[k] - (double)xs[k] : (double)xs[k] - (double)xt[k]);
      out[(long)r * D + k] = gs * (float)v;
    }
  }
}

}  // namespace

extern "C" long ac_enc_kd_workspace_floats(int B, int D) {
  if (B < 1 || B > EK_MAXB || D < 1 || D > EK_MAXD) return -1;
  return 2L * B * D + (long)B * B + 11L * B;
}

extern "C" int ac_enc_kd_loss(const float* s, long ld_s, const float* t, long ld_t, int B, int D, int kind,
                              const float* logit_scale, float* loss, float* ds, float* dt, float* dscale, float gscale,
                              const float* gscale_dev, float* ws, void* stream) {
  const bool contra = (kind & AC_ENC_KD_CONTRA) != 0;
  if (!s || !t || !loss || !ws || B < 1 || B > EK_MAXB || D < 1 || D > EK_MAXD || ld_s < D || ld_t < D ||
      (kind & ~(AC_ENC_KD_CONTRA | AC_ENC_KD_MSE | AC_ENC_KD_L2NORM)) != 0 || !(kind & (AC_ENC_KD_CONTRA | AC_ENC_KD_MSE)) ||
      (contra && !logit_scale) || !isfinite(gscale))
    return AC_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(enc_kd_norm_kernel, dim3(B), dim3(256), 0, st, s, ld_s, t, ld_t, B, D, kind, ws);
  if (contra) {
    const int tiles = (B + EK_TILE - 1) / EK_TILE;
    hipLaunchKernelGGL(enc_kd_cos_kernel, dim3(tiles, tiles), dim3(256), 0, st, B, D, ws);
    hipLaunchKernelGGL(enc_kd_stats_kernel, dim3(2 * B), dim3(256), 0, st, B, D, logit_scale, ws);
  }
  const dim3 grid(2 * B + 1);
#define EK_GO(NE)                                                                                                          \
  hipLaunchKernelGGL((enc_kd_grad_kernel<NE>), grid, dim3(256), 0, st, s, ld_s, t, ld_t, B, D, kind, logit_scale, loss, ds, \
                     dt, dscale, gscale, gscale_dev, ws)
  const int ne = (D + 255) / 256;
  if (ne <= 1) EK_GO(1);
  else if (ne <= 4) EK_GO(4);
  else if (ne <= 8) EK_GO(8);
  else EK_GO(16);
#undef EK_GO
  return ac_check_launch();
}
