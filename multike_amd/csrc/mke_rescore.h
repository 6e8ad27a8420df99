// mke_rescore.h — what the evaluator's sweeps share (mke_csls.hip, mke_stable.hip): the metric / CSLS epilogue of one
// similarity, the order-preserving integer image of a float, and the bounds of the whole-row rounds.
#pragma once
#include "mke_common.h"

#include <math.h>

namespace mke {

template <int MET>
__device__ __forceinline__ float metric_value(float dot, float sqi, float sqj) {
  if (MET == MKE_METRIC_EUCLIDEAN) return 1.0f - sqrtf(fmaxf(sqi + sqj - 2.0f * dot, 0.0f));
  return dot;
}

template <int MET, bool CSLS>
__device__ __forceinline__ float rescore(float dot, float sqi, float sqj, float rt, float rs) {
  float v = metric_value<MET>(dot, sqi, sqj);
  if (CSLS) v = (2.0f * v - rt) - rs;
  return v;
}

__device__ __forceinline__ unsigned csls_key(float v) {  // order-preserving integer image (+0 and -0 one key)
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float csls_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

static inline bool kpad_ok(int kpad) {
  switch (kpad) {
    case 16: case 32: case 48: case 64: case 80: case 96: case 112: case 128: case 160: case 192: case 208: case 256: case 320:
      return true;
    default:
      return false;
  }
}

// rows of a whole-row round: the similarity rows of one round stay under 2^26 floats (256 MB)
static inline int64_t fallback_rows(int64_t n_a, int64_t n_b) {
  int64_t r = ((int64_t)1 << 26) / n_b;
  r = r / 128 * 128;  // SIMT_BM
  if (r < 128) r = 128;
  return r < n_a ? r : n_a;
}

static inline int64_t pow2_at_least(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

}  // namespace mke
