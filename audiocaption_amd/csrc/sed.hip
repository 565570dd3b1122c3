// Sound-event tagger (Cnn8rnnSedModel, hf_wrapper.py:1791-1859) - the parts the Cnn14 kernels do not have:
//   * avg_pool + max_pool over (2,2) / (1,2) windows on the conv stack's row-padded channels-last layout (ConvBlock.forward
//     with pool_type "avg+max", hf_wrapper.py:1212-1215), and the (1,2) pool fused with the mean over the remaining mel
//     columns (hf_wrapper.py:1840-1842);
//   * the head clamp(sigmoid(x + b), 1e-7, 1) (hf_wrapper.py:1848);
//   * double_threshold + decode_with_timestamps (hf_wrapper.py:89-216) on the SEGMENT-wise probabilities: the frame-wise
//     array (every segment repeated `ratio` times, the last one stretched to frames_num) is never materialised.
// The 3x3 convolutions, the linear layers and the GRU run on the existing kernels in mode 0; nothing here changes them.
#include "ac_common.h"

// ---- avg + max pooling --------------------------------------------------------------------------------------------------
// One thread per 4 channels of one output pixel; 16-byte loads and stores along C.
struct PoolParams {
  const float* in;   // [B*Hp][W][C]
  float* out;        // [B*Hp_out][W/2][C], or dense [B][H][C] (MEANW)
  int B, Hp, H, W, C, ph, Hp_out, H_out, W_out;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }

// avg + max of a window of PH x 2 pixels whose top-left pixel is `p` (row stride `rs`, pixel stride `C` floats)
template <int PH>
__device__ __forceinline__ f32x4 window_avgmax(const float* p, size_t rs, int C) {
  const f32x4 a = ld4(p), b = ld4(p + C);
  f32x4 r;
  if (PH == 2) {
    const f32x4 c = ld4(p + rs), d = ld4(p + rs + C);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = ((a[j] + b[j]) + (c[j] + d[j])) * 0.25f + fmaxf(fmaxf(a[j], b[j]), fmaxf(c[j], d[j]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (a[j] + b[j]) * 0.5f + fmaxf(a[j], b[j]);
  }
  return r;
}

template <int PH>
__global__ __launch_bounds__(256) void pool_avgmax_kernel(PoolParams p) {
  const int c4n = p.C / 4;
  const long n = (long)p.B * p.Hp_out * p.W_out * c4n;
  const size_t rs = (size_t)p.W * p.C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    long e = i / c4n;
    const int wo = (int)(e % p.W_out);
    e /= p.W_out;
    const int ho = (int)(e % p.Hp_out);
    const int b = (int)(e / p.Hp_out);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    // rows at or beyond H_out are the next conv's zero padding: an odd last input row never reaches row H_out
    if (ho < p.H_out) r = window_avgmax<PH>(p.in + ((size_t)b * p.Hp + (size_t)ho * PH) * rs + (size_t)(2 * wo) * p.C + c, rs, p.C);
    *(f32x4*)(p.out + (size_t)i * 4) = r;
  }
}

// (1,2) pool + mean over the W/2 pooled columns -> dense [B][H][C]
__global__ __launch_bounds__(256) void pool_avgmax_meanw_kernel(PoolParams p) {
  const int c4n = p.C / 4;
  const long n = (long)p.B * p.H * c4n;
  const size_t rs = (size_t)p.W * p.C;
  const float inv = 1.0f / (float)p.W_out;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    const long e = i / c4n;
    const int h = (int)(e % p.H);
    const int b = (int)(e / p.H);
    const float* row = p.in + ((size_t)b * p.Hp + h) * rs + c;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int wo = 0; wo < p.W_out; ++wo) {
      const f32x4 r = window_avgmax<1>(row + (size_t)(2 * wo) * p.C, rs, p.C);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += r[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] *= inv;
    *(f32x4*)(p.out + (size_t)i * 4) = s;
  }
}

static unsigned grid_for(long n) {
  const long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

extern "C" int ac_pool_avgmax(const float* in, float* out, int B, int Hp, int H, int W, int C, int ph, int Hp_out,
                              int mean_w, void* stream) {
  if (!in || !out || B <= 0 || H <= 0 || Hp < H || W < 2 || (W & 1) || C <= 0 || (C & 3)) return AC_ERR_ARG;
  if (ph != 1 && ph != 2) return AC_ERR_ARG;
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return AC_ERR_ARG;
  PoolParams p;
  p.in = in; p.out = out; p.B = B; p.Hp = Hp; p.H = H; p.W = W; p.C = C; p.ph = ph;
  p.H_out = H / ph; p.W_out = W / 2; p.Hp_out = Hp_out;
  hipStream_t s = (hipStream_t)stream;
  if (mean_w) {
    if (ph != 1) return AC_ERR_ARG;
    hipLaunchKernelGGL(pool_avgmax_meanw_kernel, dim3(grid_for((long)B * H * (C / 4))), dim3(256), 0, s, p);
    return ac_check_launch();
  }
  if (Hp_out < p.H_out || Hp_out <= 0) return AC_ERR_ARG;
  const long n = (long)B * Hp_out * p.W_out * (C / 4);
  if (ph == 2) hipLaunchKernelGGL(pool_avgmax_kernel<2>, dim3(grid_for(n)), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(pool_avgmax_kernel<1>, dim3(grid_for(n)), dim3(256), 0, s, p);
  return ac_check_launch();
}

// ---- head -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sed_head_kernel(const float* x, const float* bias, float* pre, float* prob, long n, int C) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i] + (bias ? bias[i % C] : 0.f);
    if (pre) pre[i] = v;
    prob[i] = fminf(fmaxf(ac_sigmoid_exact(v), 1e-7f), 1.0f);
  }
}

extern "C" int ac_sed_head(const float* x, const float* bias, float* pre, float* prob, long rows, int C, void* stream) {
  if (!x || !prob || rows <= 0 || C <= 0) return AC_ERR_ARG;
  const long n = rows * C;
  hipLaunchKernelGGL(sed_head_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, bias, pre, prob, n, C);
  return ac_check_launch();
}

// ---- temporal tag ---------------------------------------------------------------------------------------------------------
// workspace: [header: B segment counts + 1 overflow word, padded to 16 bytes][B][cap] segments of 16 bytes
// (class, onset frame, offset frame, 0), cap = C * ceil(S / 2): a class cannot have more runs than that.
static long tag_cap(int S, int C) { return (long)C * ((S + 1) / 2); }
static long tag_header_bytes(int B) { return (((long)B + 1) * 4 + 15) & ~15L; }

extern "C" long ac_sed_tag_workspace_bytes(int B, int S, int C) {
  if (B <= 0 || S <= 0 || C <= 0) return AC_ERR_ARG;
  return tag_header_bytes(B) + (long)B * tag_cap(S, C) * 16;
}

struct TagParams {
  const float* prob;   // [B][S][C]
  int* counts;         // [B] + overflow word at [B]
  int4* segs;          // [B][cap]
  int* tags;           // [B]
  long cap;
  int B, S, C, frames_num, ratio, n_connect;
  float high, low;
  double res, thre;
};

// The segment counters and the overflow word are cleared by a kernel, not a memset node (memset nodes
// in captured work were not reliably ordered before the kernel that follows).
__global__ void sed_tag_reset_kernel(int* counts, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) counts[i] = 0;
}

// Pass 1, one thread per (clip, class): runs of p > low that contain a p > high, merged when the gap between two of them
// is <= n_connect FRAMES (connect_, hf_wrapper.py:170-189), as (class, onset frame, offset frame); a run that reaches the
// last segment ends at frames_num (pad_framewise_output repeats the last segment).
__global__ __launch_bounds__(256) void sed_tag_runs_kernel(TagParams p) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)p.B * p.C) return;
  const int b = (int)(i / p.C), c = (int)(i % p.C);
  const float* x = p.prob + (size_t)b * p.S * p.C + c;
  int4* segs = p.segs + (size_t)b * p.cap;
  int cur_on = -1, cur_off = 0;     // the merged segment not yet emitted
  int run_on = -1;                  // first segment of the open run, -1: none
  bool run_high = false;
  auto emit = [&](int on, int off) {
    const int idx = atomicAdd(&p.counts[b], 1);
    if (idx < p.cap) segs[idx] = make_int4(c, on, off, 0);
    else atomicOr(&p.counts[p.B], 1);   // cannot happen (cap is the worst case); never dropped silently
  };
  auto close_run = [&](int s_end) {
    if (run_high) {
      const int on = run_on * p.ratio;
      const int off = s_end == p.S ? p.frames_num : s_end * p.ratio;
      if (cur_on >= 0 && on - cur_off <= p.n_connect) cur_off = off;
      else {
        if (cur_on >= 0) emit(cur_on, cur_off);
        cur_on = on; cur_off = off;
      }
    }
    run_on = -1; run_high = false;
  };
  for (int s = 0; s < p.S; ++s) {
    const float v = x[(size_t)s * p.C];
    if (v > p.low) {
      if (run_on < 0) run_on = s;
      run_high = run_high || v > p.high;
    } else if (run_on >= 0) close_run(s);
  }
  if (run_on >= 0) close_run(p.S);
  if (cur_on >= 0) emit(cur_on, cur_off);
}

// Pass 2, one workgroup per clip: segments_to_temporal_tag (hf_wrapper.py:191-203) over all ordered pairs of segments of
// different classes, in the reference's float64 arithmetic: t = frame * res, overlap = e_j - s_k against
// thre * min(e_j - s_j, e_k - s_k).  Exact ties are common (durations are multiples of `ratio` frames) and fall as the
// rounding of frame * 0.01 decides, so no product may be contracted into the subtraction that follows it: this file is
// built with -ffp-contract=off (audiocaption_amd/build.py EXTRA_FLAGS - HIP's __dmul_rn / __dsub_rn are plain operators
// in a header compiled under the default contraction and fuse after inlining), and the pragma below says so again.
__global__ __launch_bounds__(256) void sed_tag_pairs_kernel(TagParams p) {
#pragma clang fp contract(off)
  __shared__ int t_cls[256];
  __shared__ double t_s[256], t_e[256], t_d[256];
  __shared__ int flags;   // 2: after, 1: while = the tag
  const int b = blockIdx.x, tid = threadIdx.x;
  const long cnt = p.counts[b];
  const int n = (int)(cnt < p.cap ? cnt : p.cap);
  const int4* segs = p.segs + (size_t)b * p.cap;
  if (tid == 0) flags = 0;
  bool done = false;
  for (int j0 = 0; j0 < n && !done; j0 += 256) {
    const int j = j0 + tid;
    const bool have = j < n;
    int cj = -1;
    double sj = 0.0, ej = 0.0, dj = 0.0;
    if (have) {
      const int4 t = segs[j];
      cj = t.x;
      sj = ((double)t.y * p.res);
      ej = ((double)t.z * p.res);
      dj = (ej - sj);
    }
    for (int k0 = 0; k0 < n; k0 += 256) {
      __syncthreads();                 // the tile is free; flag writes of the previous tile are visible
      const int f = flags;
      if (f == 3) { done = true; break; }   // both set: nothing can change (uniform: every thread reads between two barriers)
      if (k0 + tid < n) {
        const int4 t = segs[k0 + tid];
        const double s = ((double)t.y * p.res), e = ((double)t.z * p.res);
        t_cls[tid] = t.x; t_s[tid] = s; t_e[tid] = e; t_d[tid] = (e - s);
      }
      __syncthreads();
      if (have) {
        const int m = n - k0 < 256 ? n - k0 : 256;
        int local = 0;
        for (int kk = 0; kk < m; ++kk) {
          if (t_cls[kk] == cj) continue;
          const double sk = t_s[kk];
          const double lim = (p.thre * fmin(dj, t_d[kk]));
          const double ov = (ej - sk);
          if (ov < lim) local |= 2;
          if (sj < sk && ov > lim) local |= 1;
        }
        if (local & ~f) atomicOr(&flags, local);
      }
    }
  }
  __syncthreads();
  if (tid == 0) p.tags[b] = p.counts[p.B] ? -1 : flags;
}

extern "C" int ac_sed_temporal_tag(const float* prob, int B, int S, int C, int frames_num, int ratio, float high, float low,
                                   int n_connect, const double* rule, void* workspace, long workspace_bytes, int* tags,
                                   void* stream) {
  if (!prob || !rule || !workspace || !tags || B <= 0 || S <= 0 || C <= 0 || ratio <= 0 || n_connect < 0) return AC_ERR_ARG;
  if ((long)S * ratio > frames_num || (long)S * ratio >= (1L << 30)) return AC_ERR_ARG;   // the pad only ever stretches
  if (!(high >= low)) return AC_ERR_ARG;   // a run's high point lies inside the run
  if (((uintptr_t)workspace & 15) || workspace_bytes < ac_sed_tag_workspace_bytes(B, S, C)) return AC_ERR_ARG;
  TagParams p;
  p.prob = prob; p.counts = (int*)workspace; p.segs = (int4*)((char*)workspace + tag_header_bytes(B)); p.tags = tags;
  p.cap = tag_cap(S, C); p.B = B; p.S = S; p.C = C; p.frames_num = frames_num; p.ratio = ratio; p.n_connect = n_connect;
  p.high = high; p.low = low; p.res = rule[0]; p.thre = rule[1];   // host doubles: {time resolution, thre}
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sed_tag_reset_kernel, dim3((unsigned)((B + 1 + 255) / 256)), dim3(256), 0, s, p.counts, B + 1);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(sed_tag_runs_kernel, dim3((unsigned)(((long)B * C + 255) / 256)), dim3(256), 0, s, p);
  if (ac_check_launch() != AC_OK) return AC_ERR_LAUNCH;
  hipLaunchKernelGGL(sed_tag_pairs_kernel, dim3(B), dim3(256), 0, s, p);
  return ac_check_launch();
}
