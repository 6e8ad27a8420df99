// mke_sampler_o32.h — which instantiation of the sampler a launch takes (plain C++, no HIP: the host test of
// tests/test_sampler_exact_gpu.py compiles it by itself).
#pragma once
#include <stdint.h>

namespace mke {

// The sampler's O32 instantiation forms byte offsets in 32 bits (on scalar bases) for the epoch's positives, the output arrays, a side's
// entity list and the filter.  That is legal when every such offset stays below 2^32:
//   outputs       n_pos * neg_per_pos int32 words  -> n_pos * neg_per_pos <= 2^30 (the positives, n_pos words, are fewer)
//   entity lists  n_ent int32 words per side       -> n_ent <= 2^30
//   filters       at most 4 MB by construction (FILTER_MAX_BITS_LOG2)
// The candidate table and the exact probe of the known-triple table keep 64-bit arithmetic in both forms.
constexpr int64_t MKE_SAMPLER_O32_MAX_WORDS = (int64_t)1 << 30;
inline bool sampler_o32_fits(int64_t n_pos, int neg_per_pos, int64_t n_ent0, int64_t n_ent1) {
  if (n_pos < 0 || neg_per_pos < 1) return false;
  if (n_pos > MKE_SAMPLER_O32_MAX_WORDS / neg_per_pos) return false;   // n_pos * neg_per_pos without overflow
  return n_ent0 <= MKE_SAMPLER_O32_MAX_WORDS && n_ent1 <= MKE_SAMPLER_O32_MAX_WORDS;
}

}  // namespace mke
