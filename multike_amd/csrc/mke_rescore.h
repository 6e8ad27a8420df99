// mke_rescore.h — what the evaluator's re-scoring sweeps share (k_align_rank_ex and k_topk_partial of mke_csls.hip,
// k_stable_select of mke_stable.hip): the metric / CSLS epilogue of one similarity, its dispatch on the host, and the bounds
// of the whole-row rounds.
#pragma once
#include "mke_select.h"
#include "mke_simtile.h"

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

// (euclidean, CSLS) as compile-time constants: f(std::integral_constant<int, MKE_METRIC_*>{}, std::bool_constant<CSLS>{})
template <class F>
static inline void for_rescore(bool euc, bool csls, F&& f) {
  using Euc = std::integral_constant<int, MKE_METRIC_EUCLIDEAN>;
  using Inner = std::integral_constant<int, MKE_METRIC_INNER>;
  if (euc && csls) f(Euc{}, std::true_type{});
  else if (euc) f(Euc{}, std::false_type{});
  else if (csls) f(Inner{}, std::true_type{});
  else f(Inner{}, std::false_type{});
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
