// mke_rescore.h — what the evaluator's sweeps share (k_align_rank of mke_eval.hip, k_topk_partial of mke_csls.hip,
// k_lse_partial of mke_sinkhorn.hip, k_stable_select of mke_stable.hip, k_align_mutual of mke_mutual.hip): the metric / CSLS epilogue of one similarity, its
// dispatch on the host, the one check of a sweep client's operands, the column split of the partial sweeps, and the bounds of
// the whole-row rounds.
#pragma once
#include "mke_select.h"
#include "mke_simtile.h"

#include <math.h>

#include <initializer_list>

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

// ------------------------------------------------------------------------------------------------ operands of a sweep client
// Operands a [n_a][ld_a] / b [n_b][ld_b] of an evaluator entry point and what all five entry points (and their *_temp_bytes
// queries, which fill in the counts and kpad only) check about them.  `who` is the prefix of the error texts ("mke_align_lse: ";
// empty for mke_align_rank: its texts of these checks carry none).  `gold`: the two rank entry points name their
// operands 1 / 2 and refuse kpad and ld with one text; the others name them a / b and have a text for each.
struct SweepOperands {
  const char* who;
  bool gold;
  int64_t n_a, n_b;
  int kpad, ld_a, ld_b;
  int metric;
  const float *sq_a, *sq_b;          // euclidean: squared row norms
  const float *term_row, *term_col;  // re-scoring terms: both or neither
};

enum OperandCheck { OP_ROWS, OP_KPAD, OP_LD, OP_METRIC, OP_NORMS, OP_TERMS, OP_WIDTH };

// The checks named by `order`, in that order; the first that fails sets the error text and returns its code.  The order is the
// caller's: the entry points grew apart in it (mke_align_rank_ex refuses an unknown metric before it looks for n1 == 0,
// mke_align_rank takes the width last, after its own n2 >= n1), and which of two wrong arguments is reported is part of the ABI.
static inline int check_operands(const SweepOperands& o, std::initializer_list<OperandCheck> order) {
  for (const OperandCheck c : order) {
    switch (c) {
      case OP_ROWS:
        if (o.n_a < 0 || o.n_b < 0 || o.n_a > 0x7FFFFF00LL || o.n_b > 0x7FFFFF00LL) {
          set_error(o.gold ? "%sbad n1/n2" : "%sbad n_a / n_b", o.who);
          return MKE_E_SHAPE;
        }
        break;
      case OP_KPAD:
      case OP_LD:
        if (c == OP_KPAD ? (o.kpad <= 0 || o.kpad % 16 != 0 || o.kpad > MKE_MAX_STRIDE)
                         : (o.ld_a < o.kpad || o.ld_b < o.kpad || o.ld_a % 4 != 0 || o.ld_b % 4 != 0)) {
          if (o.gold) set_error("%skpad must be a multiple of 16 <= %d and <= ld1, ld2 (both multiples of 4)", o.who, MKE_MAX_STRIDE);
          else if (c == OP_KPAD) set_error("%skpad must be a multiple of 16 <= %d", o.who, MKE_MAX_STRIDE);
          else set_error("%slda, ldb must be multiples of 4 >= kpad", o.who);
          return MKE_E_SHAPE;
        }
        break;
      case OP_METRIC:
        if (o.metric != MKE_METRIC_INNER && o.metric != MKE_METRIC_EUCLIDEAN) {
          set_error("%sunknown metric %d", o.who, o.metric);
          return MKE_E_UNSUPPORTED;
        }
        break;
      case OP_NORMS:
        if (o.metric == MKE_METRIC_EUCLIDEAN && (!o.sq_a || !o.sq_b)) {
          set_error(o.gold ? "%seuclidean needs sq1 and sq2" : "%seuclidean needs sq_a and sq_b", o.who);
          return MKE_E_NULL;
        }
        break;
      case OP_TERMS:
        if ((o.term_row == nullptr) != (o.term_col == nullptr)) {
          set_error("%scsls_row and csls_col are both NULL or both set", o.who);
          return MKE_E_NULL;
        }
        break;
      case OP_WIDTH:
        if (!simt_kpad_ok(o.kpad)) {
          set_error("%sunsupported kpad %d", o.who, o.kpad);
          return MKE_E_UNSUPPORTED;
        }
        break;
    }
  }
  return MKE_OK;
}

// Column chunks of a sweep that leaves one partial per (row, chunk) in the caller's scratch (k_topk_partial, k_lse_partial): at
// most 64, so that the scratch stays bounded; the scratch query and the launch agree on them.
#define SWEEP_MAX_PARTIALS 64
static inline SimtSplit partial_split(int64_t n_a, int64_t n_b, int kpad) { return simt_split(n_a, n_b, kpad, 6144, 16, SWEEP_MAX_PARTIALS); }

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
