// Cnn6 conv stack on gfx950: 5x5 / stride 1 / pad 2 convolution + eval-mode BatchNorm + ReLU (+ 2x2 average pooling).
//
// Replaces reference ConvBlock5x5.forward (cnn_encoder.py:96-111) and the pooling glue of Cnn6Encoder.forward
// (cnn_encoder.py:192-199).
//
// Data layout: the project's channels-last rows [B * Hp][W][C] f32 (csrc/conv3x3.hip), with a STRONGER zero-row invariant:
// a 5x5 conv reads two rows beyond a clip, so every clip owns Hp >= H + 2 physical rows (the entry points refuse less) and
// rows h >= H are zero.  The kernels do not rely on the producer for that: staging tests every row against the clip's own H
// and reads rows at or beyond it as zeros, and the epilogues write rows at or beyond H (H >> 1 of a pooled output) as zeros.
// Hp is even, so a pooling pair never straddles two clips.
//
//   ac_conv5x5_first            Cin = 1, 25 taps, Cout = 64: f32 FMAs, BN + ReLU + the 2x2 pool fused - the full-resolution
//                               64-channel map never reaches HBM.
//   ac_conv5x5_bn_relu_bf16x3   implicit GEMM, M = pixels, N = Cout, K = 25 * Cin, on split-bf16 operands
//                               (csrc/ac_split_bf16.h): the arithmetic of the "bf16x3" 3x3 tier.  A 256-thread block owns
//                               128 pixels (TR rows x TC columns, TC = min(W, 16)) by 128 channels; per 32-channel K chunk it
//                               stages the (TR+4) x (TC+4) halo patch in LDS once, already split, and all 25 taps read it.
//                               Weights come straight from L2 in MFMA fragment order, one tap ahead in registers.
//   ac_pack_conv5x5_weight_bf16x3   OIHW f32 -> that fragment order, on the device.
#include "ac_common.h"
#include "ac_split_bf16.h"

namespace {

constexpr int TAPS = 25;
constexpr int BROW = 40;            // bf16 elements per staged pixel: 32 channels + 8 pad (80 bytes = 5 slots of 16 bytes)
constexpr int BM = 128, BN = 128;   // pixels and channels per block
constexpr int PLANE_BYTES = 23040;  // largest patch plane: TC = 8 -> 20 rows of 72 slots

struct Conv5Params {
  const float* in;
  const void* wfrag;
  const float* scale;
  const float* shift;
  float* out;
  int rows_total, Hp, H, W, Cin, Cout;
  int tc_log2, mt_cols, NT;
  int Hp_out, H_out, W_out;
};

// slots of 16 bytes per patch row: PW pixels of 5 slots, padded to 8 mod 16 - the 2 rows x 8 columns that a 16-lane group
// of a fragment read covers then fall into 16 different slots
__device__ __host__ inline int patch_pitch_slots(int TC) {
  const int s = (TC + 4) * 5;
  return s + ((8 - s) & 15);
}

template <int MODE>   // 0: full output; 1: 2x2 average pool (ReLU before the pool)
__global__ __launch_bounds__(256, 2) void conv5x5_bf16x3_kernel(Conv5Params p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * PLANE_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5;

  const int n_tile = blockIdx.x % p.NT, m_tile = blockIdx.x / p.NT;
  const int TC = 1 << p.tc_log2, TR = BM >> p.tc_log2;
  const int PW = TC + 4, PH = TR + 4;
  const int PITCH = patch_pitch_slots(TC) * 8;   // bf16 elements per patch row
  const int row0 = (m_tile / p.mt_cols) * TR, col0 = (m_tile % p.mt_cols) * TC;
  __bf16* sAh = (__bf16*)smem;
  __bf16* sAl = sAh + PH * PITCH;

  // MFMA row i of a 32-pixel tile = 4 * window + 2 * dy + dx: the four pixels of a pooling window are four consecutive
  // accumulator registers of one lane.  Windows run along the columns first.
  const int QR2 = 32 >> p.tc_log2;   // rows of a 32-pixel tile
  int pbase[2];
  {
    const int i = lane & 31;
    const int win = i >> 2, dy = (i >> 1) & 1, dx = i & 1;
    const int qc = win & ((TC >> 1) - 1), qr = win >> (p.tc_log2 - 1);
#pragma unroll
    for (int m = 0; m < 2; ++m) pbase[m] = ((2 * wm + m) * QR2 + 2 * qr + dy) * PITCH + (2 * qc + dx) * BROW + half * 8;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  const int rc0 = row0 % p.Hp;
  const bool all_pad = rc0 >= p.H && rc0 + TR <= p.Hp;   // a tile of padding rows only: zeros, no arithmetic
  if (!all_pad) {
    const int nchunk = p.Cin >> 5, total = nchunk * TAPS;
    const int NT32 = p.Cout >> 5;
    // fragments of one (chunk, tap): [2 ks][Cout/32][2 (hi, lo)][64 lanes][8] bf16
    const size_t it_stride = (size_t)2 * NT32 * 2 * 512;
    const __bf16* wsrc = (const __bf16*)p.wfrag + ((size_t)(n_tile * 4 + wn * 2) * 2) * 512 + lane * 8;
    auto w_load = [&](int it, bf16x8 (&b)[2][2][2]) {   // [ks][n][plane]
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            b[ks][n][pl] = *(const bf16x8*)(wsrc + (size_t)it * it_stride + ((size_t)(ks * NT32 + n) * 2 + pl) * 512);
    };
    auto stage_patch = [&](int c) {
      for (int idx = tid; idx < PW * PH * 8; idx += 256) {
        const int pix = idx >> 3, c4 = idx & 7;
        const int pr = pix / PW, pc = pix - pr * PW;
        const int gr = row0 - 2 + pr, gc = col0 - 2 + pc;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gr >= 0 && gr < p.rows_total && gc >= 0 && gc < p.W && (gr % p.Hp) < p.H)
          v = *(const f32x4*)(p.in + ((size_t)gr * p.W + gc) * p.Cin + c * 32 + c4 * 4);
        u32x2 hi, lo;
        split_bf16x4(v, hi, lo);
        *(u32x2*)(sAh + pr * PITCH + pc * BROW + c4 * 4) = hi;
        *(u32x2*)(sAl + pr * PITCH + pc * BROW + c4 * 4) = lo;
      }
    };
    bf16x8 bcur[2][2][2], bnext[2][2][2];
    w_load(0, bcur);
    int it = 0;
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
      __syncthreads();   // every wave is done with the previous chunk's patch
      stage_patch(c);
      __syncthreads();
#pragma unroll 1
      for (int tap = 0; tap < TAPS; ++tap, ++it) {
        w_load(it + 1 < total ? it + 1 : it, bnext);
        const int ky = tap / 5, kx = tap - 5 * ky;
        const int aoff = ky * PITCH + kx * BROW;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {   // two K = 16 steps per 32-channel chunk
          bf16x8 ah[2], al[2];
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            ah[m] = *(const bf16x8*)(sAh + aoff + pbase[m] + ks * 16);
            al[m] = *(const bf16x8*)(sAl + aoff + pbase[m] + ks * 16);
          }
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = mfma_bf16x3(ah[m], al[m], bcur[ks][n][0], bcur[ks][n][1], acc[m][n]);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) bcur[ks][n][pl] = bnext[ks][n][pl];
      }
    }
  }

  // ---- epilogue: BN scale / shift, ReLU, pool, zero rows; lanes 0..31 store 32 consecutive channels ----
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int ch = n_tile * BN + (wn * 2 + n) * 32 + (lane & 31);
    const float sc = p.scale[ch], sh = p.shift[ch];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int win = 2 * rq + half;   // registers 4 * rq + (2 * dy + dx)
        const int qc = win & ((TC >> 1) - 1), qr = win >> (p.tc_log2 - 1);
        const int wy = row0 + (2 * wm + m) * QR2 + 2 * qr;   // physical row of the window's dy = 0 (even)
        const int wx = col0 + 2 * qc;
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaxf(fmaf(acc[m][n][4 * rq + e], sc, sh), 0.f);
        if (MODE == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int gr = wy + (e >> 1), gc = wx + (e & 1);
            if (gr < p.rows_total) p.out[((size_t)gr * p.W + gc) * p.Cout + ch] = (gr % p.Hp) < p.H ? y[e] : 0.f;
          }
        } else if (wy < p.rows_total) {   // (rows_total is even: the pair wy, wy + 1 is inside or outside as one)
          const int orow = wy >> 1, ocol = wx >> 1;
          const float o = 0.25f * ((y[0] + y[1]) + (y[2] + y[3]));
          p.out[((size_t)orow * p.W_out + ocol) * p.Cout + ch] = (orow % p.Hp_out) < p.H_out ? o : 0.f;
        }
      }
    }
  }
}

// ---- block 1 of Cnn6: Cin = 1, 25 taps, 64 channels out, BN + ReLU + 2x2 average pool ----
// A block owns 4 conv rows (2 pooled rows) of all 64 mel columns; 16 lanes cover the 64 channels of a pooled pixel (float4
// each), so a wave stores 1 KiB contiguous.
struct Conv5FirstParams {
  const float* in;   // [rows_total][64]
  const float* w;    // [64][25] (OIHW with I = 1)
  const float* scale;
  const float* shift;
  float* out;        // [rows_total / 2][32][64]
  int rows_total, Hp, H;
};

__global__ __launch_bounds__(256) void conv5x5_first_kernel(Conv5FirstParams p) {
  constexpr int RT = 4, W = 64;
  __shared__ float patch[RT + 4][W + 4];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * RT;
  for (int idx = tid; idx < (RT + 4) * (W + 4); idx += 256) {
    const int pr = idx / (W + 4), pc = idx - pr * (W + 4);
    const int gr = row0 - 2 + pr, gc = pc - 2;
    float v = 0.f;
    if (gr >= 0 && gr < p.rows_total && gc >= 0 && gc < W && (gr % p.Hp) < p.H) v = p.in[(size_t)gr * W + gc];
    patch[pr][pc] = v;
  }
  const int cg = tid & 15, ps = tid >> 4;
  float w[4][TAPS], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sc[j] = p.scale[cg * 4 + j];
    sh[j] = p.shift[cg * 4 + j];
#pragma unroll
    for (int t = 0; t < TAPS; ++t) w[j][t] = p.w[(cg * 4 + j) * TAPS + t];
  }
  __syncthreads();
  const int Hp_out = p.Hp >> 1, H_out = p.H >> 1;
  for (int px = ps; px < (RT / 2) * (W / 2); px += 16) {
    const int r = px / (W / 2), c = px - r * (W / 2);   // pooled row (of this block) and column
    const int orow = (row0 >> 1) + r;
    if (2 * orow >= p.rows_total) break;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((orow % Hp_out) < H_out) {   // both conv rows of the pair are valid rows of the clip
      float x[6][6];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) x[a][b] = patch[2 * r + a][2 * c + b];
      float a4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pool = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) s = fmaf(x[(e >> 1) + t / 5][(e & 1) + t % 5], w[j][t], s);
          pool += fmaxf(fmaf(s, sc[j], sh[j]), 0.f);
        }
        a4[j] = 0.25f * pool;
      }
      o = make_float4(a4[0], a4[1], a4[2], a4[3]);
    }
    *(float4*)(p.out + ((size_t)orow * (W / 2) + c) * 64 + cg * 4) = o;
  }
}

// one thread per 16-byte unit of the pack: [Cin/32][25][2 ks][Cout/32][2 (hi, lo)][64 lanes][8]
__global__ __launch_bounds__(256) void pack5x5_kernel(const float* w, u32x4* out, int Cin, int Cout, long units) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int NT32 = Cout >> 5;
  long q = u;
  const int lane = (int)(q & 63); q >>= 6;
  const int plane = (int)(q & 1); q >>= 1;
  const int nt = (int)(q % NT32); q /= NT32;
  const int ks = (int)(q & 1); q >>= 1;
  const int tap = (int)(q % TAPS);
  const int c = (int)(q / TAPS);
  const int co = nt * 32 + (lane & 31);
  const int ci0 = c * 32 + ks * 16 + (lane >> 5) * 8;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = w[((size_t)co * Cin + ci0 + e) * TAPS + tap];
  u32x4 hi, lo;
  split_bf16_pairs<4>(x, hi, lo);
  out[u] = plane == 0 ? hi : lo;
}

}  // namespace

extern "C" int ac_conv5x5_first(const float* in, const float* w, const float* scale, const float* shift, float* out,
                                int B, int Hp, int H, void* stream) {
  if (!in || !w || !scale || !shift || !out || B <= 0 || H < 1 || Hp < H + 2 || (Hp & 1)) return AC_ERR_ARG;
  if ((long)B * Hp >= (1l << 24)) return AC_ERR_ARG;
  Conv5FirstParams p;
  p.in = in; p.w = w; p.scale = scale; p.shift = shift; p.out = out;
  p.rows_total = B * Hp; p.Hp = Hp; p.H = H;
  const unsigned grid = (unsigned)((p.rows_total + 3) / 4);
  hipLaunchKernelGGL(conv5x5_first_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return ac_check_launch();
}

extern "C" int ac_conv5x5_bn_relu_bf16x3(const float* in, const void* wfrag, const float* scale, const float* shift,
                                         float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                                         void* stream) {
  if (!in || !wfrag || !scale || !shift || !out || B <= 0 || H < 1 || Hp < H + 2 || (Hp & 1)) return AC_ERR_ARG;
  if ((W != 8 && W != 16 && W != 32) || Cin <= 0 || Cin % 32 != 0 || Cout <= 0 || Cout % BN != 0) return AC_ERR_ARG;
  if (mode != 0 && mode != 1) return AC_ERR_ARG;
  if ((long)B * Hp * W >= (1l << 30)) return AC_ERR_ARG;
  Conv5Params p;
  p.in = in; p.wfrag = wfrag; p.scale = scale; p.shift = shift; p.out = out;
  p.rows_total = B * Hp; p.Hp = Hp; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  const int TC = W < 16 ? W : 16;
  p.tc_log2 = TC == 16 ? 4 : 3;
  const int TR = BM / TC;
  p.mt_cols = W / TC;
  p.NT = Cout / BN;
  p.Hp_out = Hp / 2; p.H_out = H / 2; p.W_out = W / 2;
  const unsigned grid = (unsigned)(((p.rows_total + TR - 1) / TR) * p.mt_cols * p.NT);
  if (mode == 0) hipLaunchKernelGGL(conv5x5_bf16x3_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(conv5x5_bf16x3_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return ac_check_launch();
}

extern "C" int ac_pack_conv5x5_weight_bf16x3(const float* w, void* wfrag, int Cin, int Cout, void* stream) {
  if (!w || !wfrag || Cin <= 0 || Cin % 32 != 0 || Cout <= 0 || Cout % 32 != 0) return AC_ERR_ARG;
  const long units = (long)(Cin / 32) * TAPS * 2 * (Cout / 32) * 2 * 64;
  hipLaunchKernelGGL(pack5x5_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (u32x4*)wfrag, Cin, Cout, units);
  return ac_check_launch();
}
