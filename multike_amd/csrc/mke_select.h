// mke_select.h — the selection primitives of the per-row kernels behind the sweep's clients (k_topk_rows and k_topk_long of
// mke_knn.hip, k_topk_mean of mke_csls.hip, k_stable_pick and k_stable_gather of mke_stable.hip): the order-preserving integer
// image of a float, the radix select of the k-th largest key, and the block bitonic sort.
#pragma once
#include "mke_common.h"

namespace mke {

// larger float <=> larger unsigned, on the raw bits
__device__ __forceinline__ unsigned ordered_bits(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// order-preserving integer image of a float; -0 and +0 compare equal as floats: one key.  NaN: the positive ones order above
// +inf, the negative ones below -inf.
__device__ __forceinline__ unsigned float_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return ordered_bits(u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The `best` word of the rank kernel (k_align_rank of mke_eval.hip), for a 64-bit atomicMax: similarity in the high word, the
// lowest column wins a tie.  Deliberately NOT float_key: -0 stays below +0 here, as it always has in the published keys.
// Which (value, column) a row of NaN or -inf publishes differs between the kernel's two entry points on purpose; the rule
// and its constants are RankBest in mke_eval.hip.
__device__ __forceinline__ unsigned long long best_key(float v, int col) {
  return ((unsigned long long)ordered_bits(__float_as_uint(v)) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)col);
}

// The LDS of a radix select is declared by the kernel, which may use s_wave for scans of its own between selects: s_hist, a
// private histogram per wavefront (4x fewer collisions than one); s_wave, the wavefronts' scan totals; s_prefix, the key bits
// decided so far; s_need, the rank still wanted among the keys that share them.

// One digit, most significant first.  In: the histograms of the digit at `shift` over the keys that match the prefix `pre`,
// complete (barrier passed); `need` = rank of the wanted key among them, from the top.  Thread t owns digit 255 - t: the
// bins are summed and scanned from the largest digit down by all 256 threads, and the one thread whose digit takes the
// count from the top to `need` extends the prefix.  Ends in a barrier.
__device__ __forceinline__ void radix_digit_step(int (&s_hist)[MKE_BLOCK / 64][256], int* s_wave, unsigned* s_prefix, int* s_need,
                                                 unsigned pre, int need, int shift) {
  static_assert(MKE_BLOCK == 256, "one histogram bin per thread");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int dgt = 255 - tid;
  const int h = s_hist[0][dgt] + s_hist[1][dgt] + s_hist[2][dgt] + s_hist[3][dgt];
  int incl = h;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  for (int q = 0; q < wv; ++q) incl += s_wave[q];
  if (incl >= need && incl - h < need) {
    *s_prefix = pre | ((unsigned)dgt << shift);
    *s_need = need - (incl - h);
  }
  __syncthreads();
}

// The k-th largest of the n keys key_of(0 .. n-1) by the whole block, in four byte-wise passes.  *ties = how many of the keys
// equal to it belong to the top k.
template <class KeyOf>
__device__ __forceinline__ unsigned radix_select_kth(int (&s_hist)[MKE_BLOCK / 64][256], int* s_wave, unsigned* s_prefix, int* s_need,
                                                     int n, int k, int* ties, KeyOf&& key_of) {
  const int tid = threadIdx.x, wv = tid >> 6;
  if (tid == 0) { *s_prefix = 0u; *s_need = k; }
  __syncthreads();
  for (int hi = 32; hi > 0; hi -= 8) {
    const int shift = hi - 8;
#pragma unroll
    for (int q = 0; q < MKE_BLOCK / 64; ++q) s_hist[q][tid] = 0;
    __syncthreads();
    const unsigned pre = *s_prefix;
    const int need = *s_need;
    for (int i = tid; i < n; i += MKE_BLOCK) {
      const unsigned kx = key_of(i);
      if (hi >= 32 || (kx >> hi) == (pre >> hi)) atomicAdd(&s_hist[wv][(kx >> shift) & 255u], 1);
    }
    __syncthreads();
    radix_digit_step(s_hist, s_wave, s_prefix, s_need, pre, need, shift);
  }
  *ties = *s_need;
  return *s_prefix;
}

// bitonic sort of np2 (a power of two) 32- or 64-bit keys, descending, by the whole block
template <class T>
__device__ __forceinline__ void sort_desc(T* buf, int np2) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < np2 / 2; i += MKE_BLOCK) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const T x = buf[lo], y = buf[hi];
        if ((x < y) == desc) { buf[lo] = y; buf[hi] = x; }
      }
      __syncthreads();
    }
  }
}

}  // namespace mke
