// mke_keyed.hip — libmultike_keyed.so (include/multike_keyed.h): matrix-free exact neighbour selection for capped tables at
// large k.  A library of its own: libmultike_hip.so, libmultike_thin.so and their C-ABIs stay as they are; this file shares
// only device helpers (mke_common.h, mke_select.h, mke_simtile.h) with them and keeps its own error message.
//
//   k_sim_select_keyed  simt_sweep with a keyed epilogue.  As in k_sim_select (mke_knn.hip) the similarities never leave the
//                       registers and a ballot per accumulator register gives every stored hit its slot.  A hit above the row's
//                       upper threshold is certainly in the top k; it is counted, and kept only if its key — a function of
//                       (seed, row id, column id), not of the similarity — is below key_below, i.e. with probability ~ m / k.
//                       A hit between the two thresholds may or may not be in the top k and is always kept.  The key is computed
//                       on the lanes above the upper threshold only; the row's half of it and the upper threshold sit in LDS
//                       (128 rows a block), the column's id is fetched one 32-column group ahead.
//   k_keyed_finish      one workgroup per row.  The list stays in global memory / L2 and is streamed in passes (as k_idlist_thin
//                       streams its ids): four byte-wise radix passes fix the (k - sure)-th largest band value, one ordered pass
//                       its last tie, eight fix the m-th smallest key among the members (keys are recomputed, never stored), and
//                       the last compacts the kept members in list order.  The only atomics are the integer LDS histogram counts.
#include <cstdarg>
#include <cstdio>

#include "../../include/multike_keyed.h"
#include "mke_select.h"
#include "mke_simtile.h"

namespace {
thread_local char g_keyed_err[256] = "";
void keyed_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_keyed_err, sizeof(g_keyed_err), fmt, ap);
  va_end(ap);
}
}  // namespace

namespace mke {

#define KEYED_GOLD 0x9E3779B97F4A7C15ull

__host__ __device__ __forceinline__ uint64_t keyed_row_key(uint64_t seed, int32_t row_id) {
  return mix64(seed + KEYED_GOLD * ((uint64_t)(uint32_t)row_id + 1ull));
}
__host__ __device__ __forceinline__ uint64_t keyed_key(uint64_t row_key, int32_t col_id) { return mix64(row_key ^ (uint64_t)(uint32_t)col_id); }

struct KeyedSelectParams {
  const float* __restrict__ emb;  // [n][ld], columns >= dim zero up to kpad
  int ld;
  int n_cols;
  int row_lo, row_hi;
  const float* __restrict__ tau_lo;     // [row_hi - row_lo]
  const float* __restrict__ tau_hi;     // [row_hi - row_lo]
  const int32_t* __restrict__ col_ids;  // [n_cols]
  uint64_t seed, key_below;
  int n_seg, seg_cap, tiles_per_seg;
  mke_keyed_candidate* __restrict__ cand;  // [rows][n_seg][seg_cap]
  int32_t* __restrict__ seg_count;         // [rows][n_seg]
  int32_t* __restrict__ seg_sure;          // [rows][n_seg]
};

// Launch bounds as k_sim_select: three blocks per CU up to kpad 80, the compiler's own choice above.
template <int KS>  // kpad / 16
__global__ __launch_bounds__(MKE_BLOCK, KS <= 5 ? 3 : 1) void k_sim_select_keyed(const KeyedSelectParams p) {
  __shared__ uint64_t s_rowkey[SIMT_BM];
  __shared__ float s_tauhi[SIMT_BM];
  __shared__ int s_sure[SIMT_BM];  // per row, added to by lane 0 of the half-wave that owns the row: 16 registers fewer than a count per accumulator
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int block0 = p.row_lo + blockIdx.x * SIMT_BM;
  const int strip0 = block0 + wv * 32;
  if (threadIdx.x < SIMT_BM) {
    const int r = block0 + (int)threadIdx.x;
    const bool ok = r < p.row_hi;
    s_rowkey[threadIdx.x] = ok ? keyed_row_key(p.seed, p.col_ids[r]) : 0ull;
    s_tauhi[threadIdx.x] = ok ? p.tau_hi[r - p.row_lo] : 3.0e38f;
    s_sure[threadIdx.x] = 0;
  }
  float a[KS * 8];
  {
    const int r = strip0 + l31;
    const bool ok = r < p.row_hi;
    simt_load_fragment<KS>(p.emb + (int64_t)(ok ? r : p.row_lo) * p.ld, ok, half, a);
  }
  float tauL[16];
  int cnt[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    tauL[reg] = r < p.row_hi ? p.tau_lo[r - p.row_lo] : 3.0e38f;
    cnt[reg] = 0;
  }
  const int seg = blockIdx.y;
  const int ntiles = (p.n_cols + SIMT_BN_FOR(KS) - 1) / SIMT_BN_FOR(KS);
  const int t0 = seg * p.tiles_per_seg;
  const int t1 = min(ntiles, t0 + p.tiles_per_seg);
  const unsigned lt = (1u << l31) - 1u;
  // slot of (row of accumulator register reg, position) as a 32-bit BYTE offset from p.cand: the launcher bounds a launch to
  // 2^29 slots
  const unsigned row_stride_b = (unsigned)(p.n_seg * p.seg_cap) * 8u;
  const unsigned base0_b = (unsigned)(((strip0 - p.row_lo + 4 * half) * p.n_seg + seg) * p.seg_cap) * 8u;
  char* const cand_b = reinterpret_cast<char*>(p.cand);
  const int lrow0 = wv * 32 + 4 * half;  // this lane's first row inside the block (LDS index of register 0)
  // The id of the NEXT group's column is fetched while this one is worked on.  This leans on the ORDER in which simt_sweep
  // calls the epilogue, which its comment does not promise: tiles t0 .. t1-1 ascending and inside a tile the groups cg = 0 ..
  // BN/32 - 1 ascending (mke_simtile.h:129 and :157-161), i.e. column = t0 * BN + l31, then + 32 per call.  A sweep that
  // called in another order would key hits by the wrong column: tests/test_keyed_exact_gpu.py holds every stored entry and
  // every count to the oracle at both tile widths and fails on it; the remedy then is to load p.col_ids[col] in the epilogue.
  int32_t next_id = 0;
  {
    const int64_t c = (int64_t)t0 * SIMT_BN_FOR(KS) + l31;
    if (t0 < t1 && c < p.n_cols) next_id = p.col_ids[c];
  }
  __syncthreads();  // s_rowkey, s_tauhi, s_sure
  simt_sweep<KS>(a, p.emb, p.ld, p.n_cols, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    const int32_t col_id = next_id;
    next_id = (int64_t)col + 32 < p.n_cols ? p.col_ids[col + 32] : 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float v = acc[reg];
      const bool hit = col_ok && v > tauL[reg];
      const uint64_t mhit = __builtin_amdgcn_ballot_w64(hit);
      if (mhit == 0) continue;  // wave-uniform
      const int lr = lrow0 + simt_row(reg, 0);
      const bool is_sure = hit && v > s_tauhi[lr];
      const uint64_t msure = __builtin_amdgcn_ballot_w64(is_sure);
      bool store = hit;
      uint64_t mstore = mhit;
      if (msure != 0) {  // wave-uniform
        if (is_sure) store = keyed_key(s_rowkey[lr], col_id) < p.key_below;
        mstore = __builtin_amdgcn_ballot_w64(store);
        if (l31 == 0) s_sure[lr] += __popc(half ? (unsigned)(msure >> 32) : (unsigned)msure);
      }
      const unsigned mh = half ? (unsigned)(mstore >> 32) : (unsigned)mstore;  // the 32 lanes of a half hold 32 columns of ONE row
      const int pos = cnt[reg] + __popc(mh & lt);
      if (store && pos < p.seg_cap) {
        mke_keyed_candidate c;
        c.idx = col;
        c.sim = v;
        *reinterpret_cast<mke_keyed_candidate*>(cand_b + (base0_b + (unsigned)simt_row(reg, 0) * row_stride_b + (unsigned)pos * 8u)) = c;
      }
      cnt[reg] += __popc(mh);
    }
  });
  if (l31 == 0) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = simt_row(reg, half, strip0);
      if (r < p.row_hi) {
        p.seg_count[(int64_t)(r - p.row_lo) * p.n_seg + seg] = cnt[reg];
        p.seg_sure[(int64_t)(r - p.row_lo) * p.n_seg + seg] = s_sure[lrow0 + simt_row(reg, 0)];
      }
    }
  }
}

struct KeyedFinishParams {
  const mke_keyed_candidate* __restrict__ cand;  // [rows][n_seg][seg_cap]
  const int32_t* __restrict__ seg_count;         // [rows][n_seg]
  const int32_t* __restrict__ seg_sure;          // [rows][n_seg]
  int64_t row0;                                  // this launch covers rows row0 + blockIdx.x
  int n_seg, seg_cap;
  const float* __restrict__ tau_hi;              // [rows]
  const int32_t* __restrict__ row_ids;           // [rows]
  const int32_t* __restrict__ col_ids;
  int k, m;
  uint64_t seed, key_below;
  int32_t* __restrict__ out;                     // [rows][m]
  int32_t* __restrict__ status;                  // [rows]
};

// sum of one int per thread; every thread gets it.  Ends in a barrier (s_red may be reused at once).
__device__ __forceinline__ int keyed_block_sum(int v, int* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int q = 0; q < MKE_BLOCK / 64; ++q) tot += s_red[q];
  __syncthreads();
  return tot;
}

// One ordered pass over list positions [0, total) in chunks of MKE_BLOCK.  flags(j) -> bit 0: "greater", bit 1: "equal" (at most
// one of them) for position j < total; body(j, flags, gt, eq) gets the numbers of greater / equal positions before j.
template <class Flags, class Body>
__device__ __forceinline__ void keyed_ordered_pass(int total, int* s_wave, Flags&& flags, Body&& body) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int gt_run = 0, eq_run = 0;  // block-uniform running counts of the chunks before this one
  for (int base = 0; base < total; base += MKE_BLOCK) {
    const int j = base + tid;
    const int f = j < total ? flags(j) : 0;
    const uint64_t mg = __ballot((f & 1) != 0), me = __ballot((f & 2) != 0);
    const uint64_t lt = (1ull << lane) - 1ull;
    if (lane == 0) s_wave[wv] = __popcll(mg) | (__popcll(me) << 16);
    __syncthreads();
    int gt = gt_run + __popcll(mg & lt), eq = eq_run + __popcll(me & lt), tot = 0;
    for (int q = 0; q < MKE_BLOCK / 64; ++q) {
      const int c = s_wave[q];
      if (q < wv) { gt += c & 0xFFFF; eq += c >> 16; }
      tot += c;  // packed sums: <= 256 per half, no carry between the halves
    }
    if (f) body(j, f, gt, eq);
    gt_run += tot & 0xFFFF;
    eq_run += tot >> 16;
    __syncthreads();
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_keyed_finish(const KeyedFinishParams p) {
  __shared__ int s_hist[MKE_BLOCK / 64][256];
  __shared__ int s_wave[MKE_BLOCK / 64];
  __shared__ int s_red[MKE_BLOCK / 64];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_over, s_tie_last;
  __shared__ long long s_sure;
  __shared__ int s_off[MKE_KEYED_MAX_SEG + 1];
  const int tid = threadIdx.x, wv = tid >> 6;
  const int64_t row = p.row0 + (int64_t)blockIdx.x;
  if (tid == 0) {
    int tot = 0, over = 0;
    long long sure = 0;
    for (int s = 0; s < p.n_seg; ++s) {
      int c = p.seg_count[row * p.n_seg + s];
      if (c > p.seg_cap) { over = 1; c = p.seg_cap; }
      if (c < 0) c = 0;
      s_off[s] = tot;
      tot += c;
      sure += p.seg_sure[row * p.n_seg + s];
    }
    s_off[p.n_seg] = tot;
    s_over = over;
    s_sure = sure;
    s_tie_last = -1;
  }
  __syncthreads();
  // everything that decides a status below is block-uniform
  if (s_over) { if (tid == 0) p.status[row] = 2; return; }
  const long long need_ll = (long long)p.k - s_sure;
  if (need_ll < 0) { if (tid == 0) p.status[row] = 3; return; }
  const int total = s_off[p.n_seg];
  const float tau = p.tau_hi[row];
  const mke_keyed_candidate* __restrict__ list = p.cand + row * (int64_t)p.n_seg * p.seg_cap;
  // entry at list position j; `s` is the caller's segment cursor: a thread's positions only grow inside one pass
  auto entry = [&](int j, int& s) {
    while (j >= s_off[s + 1]) ++s;
    return list[(int64_t)s * p.seg_cap + (j - s_off[s])];
  };
  int band = 0;
  for (int j = tid, s = 0; j < total; j += MKE_BLOCK) band += entry(j, s).sim <= tau ? 1 : 0;
  band = keyed_block_sum(band, s_red);
  if (need_ll > (long long)band) { if (tid == 0) p.status[row] = 1; return; }
  const int need = (int)need_ll;
  // the need-th largest band value and how many of its ties are members
  unsigned kth = 0xFFFFFFFFu;  // need == 0: no float_key is above it and none of its ties is taken
  int ties = 0;
  if (need > 0) {
    if (tid == 0) { s_prefix = 0u; s_need = need; }
    __syncthreads();
    for (int hi = 32; hi > 0; hi -= 8) {
      const int shift = hi - 8;
#pragma unroll
      for (int q = 0; q < MKE_BLOCK / 64; ++q) s_hist[q][tid] = 0;
      __syncthreads();
      const unsigned pre = s_prefix;
      const int nd = s_need;
      for (int j = tid, s = 0; j < total; j += MKE_BLOCK) {
        const mke_keyed_candidate c = entry(j, s);
        const unsigned kx = float_key(c.sim);
        if (c.sim <= tau && (hi >= 32 || (kx >> hi) == (pre >> hi))) atomicAdd(&s_hist[wv][(kx >> shift) & 255u], 1);
      }
      __syncthreads();
      radix_digit_step(s_hist, s_wave, &s_prefix, &s_need, pre, nd, shift);
    }
    kth = s_prefix;
    ties = s_need;
    __syncthreads();  // everyone has read s_prefix / s_need before they are reset below
    int cur = 0;
    keyed_ordered_pass(total, s_wave,
                       [&](int j) { const mke_keyed_candidate c = entry(j, cur); return c.sim <= tau && float_key(c.sim) == kth ? 2 : 0; },
                       [&](int j, int, int, int eq) { if (eq == ties - 1) s_tie_last = j; });
  }
  const int tie_last = s_tie_last;  // keyed_ordered_pass ends in a barrier; -1 when need == 0
  const uint64_t row_key = keyed_row_key(p.seed, p.row_ids[row]);
  auto member = [&](int j, const mke_keyed_candidate& c) {
    if (c.sim > tau) return true;
    if (!(c.sim <= tau)) return false;
    const unsigned kx = float_key(c.sim);
    return kx > kth || (kx == kth && j <= tie_last);
  };
  int below = 0;
  for (int j = tid, s = 0; j < total; j += MKE_BLOCK) {
    const mke_keyed_candidate c = entry(j, s);
    below += member(j, c) && keyed_key(row_key, p.col_ids[c.idx]) < p.key_below ? 1 : 0;
  }
  below = keyed_block_sum(below, s_red);
  if (below < p.m) { if (tid == 0) p.status[row] = 4; return; }
  // radix select of the m-th largest COMPLEMENT of the key among the members (k_idlist_thin's selection): the high word's four
  // digits, then the low word's among the keys that share the high word
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
      const int nd = s_need;
      for (int j = tid, s = 0; j < total; j += MKE_BLOCK) {
        const mke_keyed_candidate c = entry(j, s);
        if (!member(j, c)) continue;
        const uint64_t ck = ~keyed_key(row_key, p.col_ids[c.idx]);
        const unsigned kx = word == 0 ? (unsigned)(ck >> 32) : (unsigned)ck;
        const bool in = (word == 0 || (unsigned)(ck >> 32) == kth_hi) && (hi >= 32 || (kx >> hi) == (pre >> hi));
        if (in) atomicAdd(&s_hist[wv][(kx >> shift) & 255u], 1);
      }
      __syncthreads();
      radix_digit_step(s_hist, s_wave, &s_prefix, &s_need, pre, nd, shift);
    }
    if (word == 0) kth_hi = s_prefix;
    __syncthreads();  // everyone has read s_prefix before it is reset
  }
  const uint64_t kth_key = ((uint64_t)kth_hi << 32) | (uint64_t)s_prefix;
  const int key_ties = s_need;  // how many of the keys equal to kth_key are kept: the first in list order
  int32_t* __restrict__ o = p.out + row * (int64_t)p.m;
  int cur = 0;
  int32_t my_id = 0;
  keyed_ordered_pass(total, s_wave,
                     [&](int j) {
                       const mke_keyed_candidate c = entry(j, cur);
                       if (!member(j, c)) return 0;
                       my_id = p.col_ids[c.idx];
                       const uint64_t ck = ~keyed_key(row_key, my_id);
                       return ck > kth_key ? 1 : (ck == kth_key ? 2 : 0);
                     },
                     [&](int, int f, int gt, int eq) {
                       const int at = gt + min(eq, key_ties);  // < m by construction: exactly m positions pass
                       if (((f & 1) || eq < key_ties) && at < p.m) o[at] = my_id;
                     });
  if (tid == 0) p.status[row] = 0;
}

// simt_for_kpad's widths and 224 (KS 14, the first width with 32-column tiles)
template <class F>
static inline bool keyed_for_kpad(int kpad, F&& f) {
  if (kpad == 224) { f(std::integral_constant<int, 14>{}); return true; }
  return simt_for_kpad(kpad, f);
}

}  // namespace mke

extern "C" const char* mke_keyed_last_error(void) { return g_keyed_err; }

static bool keyed_list_ok(int n_seg, int seg_cap) {
  return n_seg >= 1 && n_seg <= MKE_KEYED_MAX_SEG && seg_cap >= 1 && (int64_t)n_seg * seg_cap <= MKE_KEYED_MAX_LIST;
}

extern "C" int mke_sim_select_keyed(const float* emb, int ld, int kpad, int64_t n_cols, int64_t row_lo, int64_t row_hi, const float* tau_lo,
                                    const float* tau_hi, const int32_t* col_ids, uint64_t seed, uint64_t key_below, int n_seg, int seg_cap,
                                    mke_keyed_candidate* cand, int32_t* seg_count, int32_t* seg_sure, void* stream) {
  using namespace mke;
  if (n_cols < 0 || row_lo < 0 || row_hi < row_lo || row_hi > n_cols || n_cols > 0x7FFFFF00LL) { keyed_error("mke_sim_select_keyed: bad row/column range"); return MKE_KEYED_E_SHAPE; }
  if (row_hi == row_lo) return MKE_KEYED_OK;
  if (!emb || !tau_lo || !tau_hi || !col_ids || !cand || !seg_count || !seg_sure) { keyed_error("mke_sim_select_keyed: NULL pointer"); return MKE_KEYED_E_NULL; }
  if (kpad <= 0 || kpad % 16 != 0 || kpad > MKE_MAX_STRIDE || ld < kpad || ld % 4 != 0) { keyed_error("mke_sim_select_keyed: kpad must be a multiple of 16 <= %d and <= ld (ld a multiple of 4)", MKE_MAX_STRIDE); return MKE_KEYED_E_SHAPE; }
  if (!keyed_list_ok(n_seg, seg_cap)) { keyed_error("mke_sim_select_keyed: need 1 <= n_seg <= %d, seg_cap >= 1 and n_seg * seg_cap <= %d", MKE_KEYED_MAX_SEG, MKE_KEYED_MAX_LIST); return MKE_KEYED_E_SHAPE; }
  if ((row_hi - row_lo + SIMT_BM) * (int64_t)n_seg * seg_cap > 0x1FFFFFFFLL) { keyed_error("mke_sim_select_keyed: more than 2^29 candidate slots in one launch (split the row range)"); return MKE_KEYED_E_RANGE; }
  KeyedSelectParams p;
  p.emb = emb; p.ld = ld; p.n_cols = (int)n_cols; p.row_lo = (int)row_lo; p.row_hi = (int)row_hi; p.tau_lo = tau_lo; p.tau_hi = tau_hi;
  p.col_ids = col_ids; p.seed = seed; p.key_below = key_below; p.n_seg = n_seg; p.seg_cap = seg_cap;
  p.tiles_per_seg = simt_split_fixed(n_cols, kpad, n_seg).tiles_per_chunk;  // all n_seg segments are launched, empty ones too
  p.cand = cand; p.seg_count = seg_count; p.seg_sure = seg_sure;
  dim3 grid((unsigned)((row_hi - row_lo + SIMT_BM - 1) / SIMT_BM), (unsigned)n_seg);
  hipStream_t st = (hipStream_t)stream;
  const bool found = keyed_for_kpad(kpad, [&](auto ks) {
    hipLaunchKernelGGL((k_sim_select_keyed<decltype(ks)::value>), grid, dim3(MKE_BLOCK), 0, st, p);
  });
  if (!found) { keyed_error("mke_sim_select_keyed: unsupported kpad %d", kpad); return MKE_KEYED_E_UNSUPPORTED; }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { keyed_error("k_sim_select_keyed: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  return MKE_KEYED_OK;
}

extern "C" int mke_keyed_finish(const mke_keyed_candidate* cand, const int32_t* seg_count, const int32_t* seg_sure, int64_t rows, int n_seg,
                                int seg_cap, const float* tau_hi, const int32_t* row_ids, const int32_t* col_ids, int k, int m, uint64_t seed,
                                uint64_t key_below, int32_t* out, int32_t* status, void* stream) {
  using namespace mke;
  if (rows < 0 || rows > 0x7FFFFFFFLL || !keyed_list_ok(n_seg, seg_cap) || m < 1 || m >= k) {
    keyed_error("mke_keyed_finish: need 0 <= rows < 2^31, 1 <= n_seg <= %d, seg_cap >= 1, n_seg * seg_cap <= %d and 1 <= m < k", MKE_KEYED_MAX_SEG, MKE_KEYED_MAX_LIST);
    return MKE_KEYED_E_SHAPE;
  }
  if (rows == 0) return MKE_KEYED_OK;
  if (!cand || !seg_count || !seg_sure || !tau_hi || !row_ids || !col_ids || !out || !status) { keyed_error("mke_keyed_finish: NULL pointer"); return MKE_KEYED_E_NULL; }
  KeyedFinishParams p;
  p.cand = cand; p.seg_count = seg_count; p.seg_sure = seg_sure; p.n_seg = n_seg; p.seg_cap = seg_cap; p.tau_hi = tau_hi; p.row_ids = row_ids;
  p.col_ids = col_ids; p.k = k; p.m = m; p.seed = seed; p.key_below = key_below; p.out = out; p.status = status;
  const int64_t chunk = 1ll << 22;  // rows per launch: 2^30 threads, inside every grid limit
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    p.row0 = r0;
    const int64_t nr = rows - r0 < chunk ? rows - r0 : chunk;
    hipLaunchKernelGGL(k_keyed_finish, dim3((unsigned)nr), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { keyed_error("k_keyed_finish: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  }
  return MKE_KEYED_OK;
}
