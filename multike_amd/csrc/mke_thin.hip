// mke_thin.hip — libmultike_thin.so (include/multike_thin.h): capped neighbour tables of the truncated sampler, a keyed
// uniform m-subset of every row of an id list, in list order.  A library of its own: libmultike_hip.so and its C-ABI stay as
// they are; this file shares only device helpers (mke_common.h, mke_select.h) with it and keeps its own error message.
//
// One workgroup per row.  A position's 64-bit key is a function of (seed, the row's entity id, the id at the position), so
// it is RECOMPUTED wherever it is needed and never stored: the row (k ids, up to ~10^5) is streamed from global memory / L2
// once per radix pass, eight byte-wise passes fix the m-th smallest key and how many of its ties belong to the kept set, and
// a ninth pass compacts the kept positions in list order (wave ballots + one running offset per row, as k_topk_long of
// mke_knn.hip).  The only atomics are the integer LDS histogram counts; no atomic decides an output position, so the output
// is a function of the arguments alone.
#include <cstdarg>
#include <cstdio>

#include "../../include/multike_thin.h"
#include "mke_select.h"

namespace {
thread_local char g_thin_err[256] = "";
void thin_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_thin_err, sizeof(g_thin_err), fmt, ap);
  va_end(ap);
}
}  // namespace

namespace mke {

struct ThinParams {
  const int32_t* __restrict__ ids;      // [rows][ld]
  int64_t ld, row0;                     // this launch covers rows row0 + blockIdx.x
  const int32_t* __restrict__ row_ids;  // nullable: the row number keys the row
  int k, m;
  uint64_t seed;
  int32_t* __restrict__ out;            // [rows][m]
};

// The selection works on the COMPLEMENT of the key: the m smallest keys are the m largest complements, which is the form
// radix_digit_step (mke_select.h) resolves, first ties in list order included.
__device__ __forceinline__ uint64_t thin_ckey(uint64_t row_key, int32_t id) { return ~mix64(row_key ^ (uint64_t)(uint32_t)id); }

__global__ __launch_bounds__(MKE_BLOCK) void k_idlist_thin(const ThinParams p) {
  __shared__ int s_hist[MKE_BLOCK / 64][256];
  __shared__ int s_wave[MKE_BLOCK / 64];
  __shared__ unsigned s_prefix;
  __shared__ int s_need;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = p.row0 + (int64_t)blockIdx.x;
  const int32_t* __restrict__ v = p.ids + row * p.ld;
  int32_t* __restrict__ o = p.out + row * (int64_t)p.m;
  if (p.m == p.k) {                                  // the whole list (block-uniform)
    for (int i = tid; i < p.k; i += MKE_BLOCK) o[i] = v[i];
    return;
  }
  const uint64_t rid = p.row_ids ? (uint64_t)(uint32_t)p.row_ids[row] : (uint64_t)row;
  const uint64_t row_key = mix64(p.seed + 0x9E3779B97F4A7C15ull * (rid + 1ull));
  // radix select of the m-th largest complement: the high word's four digits, then the low word's among the keys that share
  // the high word
  unsigned kth_hi = 0u;
  for (int word = 0; word < 2; ++word) {
    if (tid == 0) { s_prefix = 0u; if (word == 0) s_need = p.m; }
    __syncthreads();
    for (int hi = 32; hi > 0; hi -= 8) {
      const int shift = hi - 8;
#pragma unroll
      for (int q = 0; q < MKE_BLOCK / 64; ++q) s_hist[q][tid] = 0;
      __syncthreads();
      const unsigned pre = s_prefix;
      const int need = s_need;
      for (int i = tid; i < p.k; i += MKE_BLOCK) {
        const uint64_t c = thin_ckey(row_key, v[i]);
        const unsigned kx = word == 0 ? (unsigned)(c >> 32) : (unsigned)c;
        const bool in = (word == 0 || (unsigned)(c >> 32) == kth_hi) && (hi >= 32 || (kx >> hi) == (pre >> hi));
        if (in) atomicAdd(&s_hist[wv][(kx >> shift) & 255u], 1);
      }
      __syncthreads();
      radix_digit_step(s_hist, s_wave, &s_prefix, &s_need, pre, need, shift);
    }
    if (word == 0) kth_hi = s_prefix;
    __syncthreads();                                 // everyone has read s_prefix before it is reset
  }
  const uint64_t kth = ((uint64_t)kth_hi << 32) | (uint64_t)s_prefix;
  const int ties = s_need;                           // how many of the keys equal to kth are kept: the first in list order
  int gt_run = 0, eq_run = 0;                        // block-uniform running counts of the chunks before this one
  for (int base = 0; base < p.k; base += MKE_BLOCK) {
    const int i = base + tid;
    const int32_t id = i < p.k ? v[i] : 0;
    const uint64_t c = thin_ckey(row_key, id);
    const bool is_gt = i < p.k && c > kth, is_eq = i < p.k && c == kth;
    const uint64_t mg = __ballot(is_gt), me = __ballot(is_eq);
    const uint64_t lt = (1ull << lane) - 1ull;
    if (lane == 0) s_wave[wv] = __popcll(mg) | (__popcll(me) << 16);
    __syncthreads();
    int gt = gt_run + __popcll(mg & lt), eq = eq_run + __popcll(me & lt), tot = 0;
    for (int q = 0; q < MKE_BLOCK / 64; ++q) {
      const int cnt = s_wave[q];
      if (q < wv) { gt += cnt & 0xFFFF; eq += cnt >> 16; }
      tot += cnt;                                    // packed sums: <= 256 per half, no carry between the halves
    }
    const int at = gt + min(eq, ties);               // < m by construction: exactly m positions pass
    if ((is_gt || (is_eq && eq < ties)) && at < p.m) o[at] = id;
    gt_run += tot & 0xFFFF;
    eq_run += tot >> 16;
    __syncthreads();
  }
}

}  // namespace mke

extern "C" const char* mke_thin_last_error(void) { return g_thin_err; }

extern "C" int mke_idlist_thin(const int32_t* ids, int64_t rows, int k, int64_t ld_ids, const int32_t* row_ids, int m, uint64_t seed,
                               int32_t* out, void* stream) {
  using namespace mke;
  if (rows < 0 || k < 1 || m < 1 || m > k || ld_ids < k) { thin_error("mke_idlist_thin: need rows >= 0, 1 <= m <= k <= ld_ids"); return MKE_E_SHAPE; }
  if (rows == 0) return MKE_OK;
  if (!ids || !out) { thin_error("mke_idlist_thin: NULL pointer"); return MKE_E_NULL; }
  ThinParams p;
  p.ids = ids; p.ld = ld_ids; p.row_ids = row_ids; p.k = k; p.m = m; p.seed = seed; p.out = out;
  const int64_t chunk = 1ll << 22;                   // rows per launch: 2^30 threads, inside every grid limit
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    p.row0 = r0;
    const int64_t nr = rows - r0 < chunk ? rows - r0 : chunk;
    hipLaunchKernelGGL(k_idlist_thin, dim3((unsigned)nr), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { thin_error("k_idlist_thin: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  }
  return MKE_OK;
}
