// Bookkeeping shared by the conv kernels over channels-last rows [B * Hp][W][C] (csrc/conv3x3*.hip): the epilogue modes,
// the row-inside-the-clip division and the dead-block test.
#pragma once
#include "ac_common.h"

namespace {

// MEANW: W == 2, mean over the two mel columns, dense (B, H, Cout) output
enum { MODE_FULL = 0, MODE_POOL = 1, MODE_MEANW = 2 };

// x mod d (and x / d) for 0 <= x < 2^23 with a reciprocal computed once per wave: the epilogues need the row inside the
// clip for every stored row, and an integer division by the run-time Hp costs ~25 instructions each.
struct FastDiv {
  int d;
  float inv;
  __device__ __forceinline__ explicit FastDiv(int d_) : d(d_), inv(1.0f / (float)d_) {}
  __device__ __forceinline__ int div(int x, int& rem) const {
    int q = (int)((float)x * inv);
    int r = x - q * d;
    if (r < 0) { r += d; --q; }
    if (r >= d) { r -= d; ++q; }
    rem = r;
    return q;
  }
  __device__ __forceinline__ int mod(int x) const { int r; div(x, r); return r; }
};

// Dead block: every one of its `nrows` rows from `row0` lies in the padding of its clip(s) - beyond the geometry's H valid
// rows, or (ragged batches) beyond the need_mul * clip_frames[b] + need_add rows the clip's own length can bring to an
// output frame.  Such a block convolves nothing and stores zeros.
__device__ __forceinline__ bool rows_live(int row0, int nrows, int rows_total, int Hp, int H, const int* clip_frames,
                                          int need_mul, int need_add) {
  bool live = false;
  if (row0 < rows_total) {
    const int r_end = row0 + nrows < rows_total ? row0 + nrows : rows_total;
    int b = row0 / Hp;
    for (int base = b * Hp; base < r_end; base += Hp, ++b) {
      const int lo = (row0 > base ? row0 : base) - base;
      int lim = H;
      if (clip_frames) {
        const int need = need_mul * clip_frames[b] + need_add;
        lim = need < lim ? need : lim;
      }
      live = live || lo < lim;
    }
  }
  return live;
}

}  // namespace
