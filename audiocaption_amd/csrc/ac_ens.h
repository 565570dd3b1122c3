// Front end of the ensemble pick kernels (csrc/ensemble.hip, and the sampler of csrc/sample.hip when it is handed member
// planes): one 256-thread workgroup per row reads the row of every member's logit plane ONCE into registers and leaves
//   m = (1 / M) sum_n log_softmax(logit_n)          (ensemble.py:133-136, :212-216; f32, members added in order)
// in registers.  No member's log-softmax is written to memory; m is NOT renormalised (logsumexp(m) <= 0).
#pragma once
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

#include <math.h>

struct EnsPlanes {
  const float* p[AC_ENS_MAX];   // member n's row r at p[n] + r * ld
  long ld;
  int n;                        // members, 1 .. AC_ENS_MAX (0: not an ensemble call)
  int vec;                      // every plane 16-byte aligned and ld % 4 == 0: 16-byte loads
};

// Column held by register i of thread tid.  NPT % 4 == 0 and registers come in groups of four consecutive columns, so a
// group is one 16-byte load.  STRIDED: consecutive lanes hold consecutive groups (coalesced: a wave reads 1 KiB per load);
// otherwise thread tid holds the NPT consecutive columns from tid * NPT (the sampler's scans are in vocabulary order).
template <int NPT, bool STRIDED>
__device__ __forceinline__ int ens_col(int tid, int i) {
  return STRIDED ? (tid + 256 * (i >> 2)) * 4 + (i & 3) : tid * NPT + i;
}

// x[i] = m[ens_col(tid, i)], -inf beyond V.  sh: 4 words of LDS.  All 256 threads must call it.
template <int NPT, bool STRIDED>
__device__ __forceinline__ void ens_mean(const EnsPlanes& e, int r, int V, float (&x)[NPT], float* sh) {
  static_assert(NPT % 4 == 0, "registers are loaded in groups of four columns");
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NPT; ++i) x[i] = 0.f;
#pragma unroll
  for (int n = 0; n < AC_ENS_MAX; ++n) {
    if (n >= e.n) break;
    const float* row = e.p[n] + (size_t)r * e.ld;
    float y[NPT];
#pragma unroll
    for (int g = 0; g < NPT / 4; ++g) {
      const int c = ens_col<NPT, STRIDED>(tid, 4 * g);
      if (e.vec && c + 3 < V) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(row + c);
        y[4 * g] = q[0]; y[4 * g + 1] = q[1]; y[4 * g + 2] = q[2]; y[4 * g + 3] = q[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[4 * g + j] = c + j < V ? row[c + j] : -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPT; ++i) mx = fmaxf(mx, y[i]);
    mx = block_max256(mx, sh);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NPT; ++i) s += expf(y[i] - mx);   // exp(-inf) = 0 beyond V
    const float lse = mx + logf(block_sum256(s, sh));
#pragma unroll
    for (int i = 0; i < NPT; ++i) x[i] += y[i] - lse;
  }
  const float cnt = (float)e.n;   // a division, as torch's mean: the same f32 value for every member count
#pragma unroll
  for (int i = 0; i < NPT; ++i) x[i] = ens_col<NPT, STRIDED>(tid, i) < V ? x[i] / cnt : -INFINITY;
}

// host side: fill EnsPlanes from the ABI's pointer list; AC_ERR_ARG for a bad count or a null plane
static inline int ens_planes(const float* const* logits, int n_models, long ld, int V, EnsPlanes* e) {
  if (!logits || n_models < 1 || n_models > AC_ENS_MAX || ld < V) return AC_ERR_ARG;
  e->ld = ld; e->n = n_models; e->vec = (ld % 4 == 0);
  for (int n = 0; n < AC_ENS_MAX; ++n) {
    e->p[n] = n < n_models ? logits[n] : nullptr;
    if (n < n_models && !logits[n]) return AC_ERR_ARG;
    if (n < n_models && ((uintptr_t)logits[n] & 15)) e->vec = 0;
  }
  return AC_OK;
}
