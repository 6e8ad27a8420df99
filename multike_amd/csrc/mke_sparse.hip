// mke_sparse.hip — libmultike_sparse.so (include/multike_sparse.h): Sinkhorn re-scoring on the support of the candidate lists.
// A library of its own: libmultike_hip.so, libmultike_thin.so, libmultike_keyed.so, libmultike_links.so and their C-ABIs stay as
// they are; this file shares only mke_common.h with them and keeps its own error message.
//
// The support (mke_sparse_support), every step in slot or entry order, no atomic:
//   k_sp_emit     a 16-lane group per list; a slot's key is (row, column, list) packed into 64 bits, or the sentinel (row = n_a)
//                 for padding and for everything behind a list's first index out of range (one ballot per 16 slots finds it).
//   hipcub        radix sort of the keys over the bits in use, payload = the value's bits (stable: the row list's slot of a
//                 pair precedes the column list's, an earlier slot a later one).
//   k_sp_flag     flag = valid and not the pair of the predecessor; hipcub exclusive scan = the entry's position.
//   k_sp_compact  ent_col, ent_val, the entry's row (temp), the count.
//   k_sp_offsets  thread i: row_off[i] = lower bound of i in the compacted rows; the segment count of the row.
//   k_sp_colkeys / sort / k_sp_colwrite / k_sp_offsets: the same entries keyed (column, row), payload = the entry index.
// The half-iteration (mke_sparse_lse): k_sp_lse_short (16 lanes a list), k_sp_lse_seg (a wavefront a segment, the work-item
// list is `seg`, read on the device), k_sp_lse_merge (a thread a long list, float64, segment order).
#include <cstdarg>
#include <cstdio>
#include <math.h>
#include <type_traits>

#include <hipcub/hipcub.hpp>

#include "../../include/multike_sparse.h"
#include "mke_common.h"

static_assert(MKE_SPARSE_E_NULL == MKE_E_NULL && MKE_SPARSE_E_SHAPE == MKE_E_SHAPE && MKE_SPARSE_E_UNSUPPORTED == MKE_E_UNSUPPORTED &&
              MKE_SPARSE_E_RANGE == MKE_E_RANGE, "error codes of multike_hip.h");
static_assert(MKE_SPARSE_Q % 16 == 0 && MKE_SPARSE_SEG % 64 == 0 && MKE_SPARSE_SEG >= MKE_SPARSE_Q, "list classes");

namespace {
thread_local char g_sparse_err[256] = "";
void sparse_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_sparse_err, sizeof(g_sparse_err), fmt, ap);
  va_end(ap);
}
int bit_length(int64_t x) { return x <= 0 ? 0 : 64 - __builtin_clzll((unsigned long long)x); }
int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
}  // namespace

namespace mke {

struct SparseBuild {
  const float* __restrict__ val_r;
  const int32_t* __restrict__ col_r;
  const float* __restrict__ val_c;
  const int32_t* __restrict__ row_c;
  int64_t n_a, n_b;
  int cut_r, cut_c;
  int64_t slots;          // n_a * cut_r + n_b * cut_c
  int col_bits, row_bits;  // key = row << (col_bits + 1) | column << 1 | list
  uint64_t* keys;
  uint32_t* vals;
  int32_t* flags;         // [slots + 1]; the entries' columns once the flags are used up
  int32_t* pos;           // [slots + 1]
  int32_t* rows;          // [slots] the entries' rows
  int32_t* segcnt;        // [max(n_a, n_b) + 1]
  int32_t* ent_col;
  float* ent_val;
  int32_t* ent_row;
  int32_t* ent_idx;
  int64_t* count;
};

// lists [0, n_a) are the rows', [n_a, n_a + n_b) the columns'
__global__ __launch_bounds__(MKE_BLOCK) void k_sp_emit(const SparseBuild p) {
  const int l = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
  const int64_t list = (int64_t)blockIdx.x * MKE_SUBS_PER_BLOCK + (threadIdx.x >> 4);
  const bool live = list < p.n_a + p.n_b;
  const bool side = live && list >= p.n_a;   // a column's list
  const int64_t own = side ? list - p.n_a : list;
  const int cut = side ? p.cut_c : p.cut_r;
  const int64_t base = side ? p.n_a * p.cut_r + own * p.cut_c : own * p.cut_r;
  const int32_t* __restrict__ idx = (side ? p.row_c : p.col_r) + (side ? own * p.cut_c : own * p.cut_r);
  const float* __restrict__ val = (side ? p.val_c : p.val_r) + (side ? own * p.cut_c : own * p.cut_r);
  const int64_t other_n = side ? p.n_a : p.n_b;
  const uint64_t sentinel = (uint64_t)p.n_a << (p.col_bits + 1);
  const int longest = p.cut_r > p.cut_c ? p.cut_r : p.cut_c;   // every lane of a wavefront meets every ballot
  bool ended = false;
  for (int k0 = 0; k0 < longest; k0 += 16) {
    const int k = k0 + l;
    const bool slot = live && k < cut;
    const int j = slot ? idx[k] : 0;
    const bool bad = slot && !((uint64_t)(int64_t)j < (uint64_t)other_n);
    const unsigned m = (unsigned)(__ballot(bad) >> (16 * g)) & 0xFFFFu;
    const bool ok = slot && !ended && (m == 0 || l < __builtin_ctz(m));
    if (slot) {
      const uint64_t r = side ? (uint64_t)j : (uint64_t)own, c = side ? (uint64_t)own : (uint64_t)j;
      p.keys[base + k] = ok ? (r << (p.col_bits + 1) | c << 1 | (side ? 1u : 0u)) : sentinel;
      p.vals[base + k] = __float_as_uint(val[k]);
    }
    ended = ended || m != 0;
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sp_flag(const SparseBuild p, const uint64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (t > p.slots) return;
  int f = 0;
  if (t < p.slots) {
    const uint64_t k = keys[t];
    const bool valid = (k >> (p.col_bits + 1)) < (uint64_t)p.n_a;
    f = valid && (t == 0 || (keys[t - 1] >> 1) != (k >> 1));
  }
  p.flags[t] = f;
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sp_compact(const SparseBuild p, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (t > p.slots) return;
  if (t == p.slots) { p.count[0] = p.pos[t]; return; }
  if (!p.flags[t]) return;
  const int e = p.pos[t];
  const uint64_t k = keys[t];
  p.ent_col[e] = (int32_t)((k >> 1) & ((1ull << p.col_bits) - 1));
  p.ent_val[e] = __uint_as_float(vals[t]);
  p.rows[e] = (int32_t)(k >> (p.col_bits + 1));
}

__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ v, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// sorted [E] = the owner (row or column) of every entry, ascending; E = p.pos[p.slots]
__global__ __launch_bounds__(MKE_BLOCK) void k_sp_offsets(const SparseBuild p, const int32_t* __restrict__ sorted, int64_t n, int64_t* __restrict__ off) {
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i > n) return;
  const int64_t E = p.pos[p.slots];
  const int64_t lo = lower_bound_i32(sorted, E, i);
  off[i] = lo;
  int c = 0;
  if (i < n) {
    const int64_t len = lower_bound_i32(sorted, E, i + 1) - lo;
    c = len > MKE_SPARSE_Q ? (int)((len + MKE_SPARSE_SEG - 1) / MKE_SPARSE_SEG) : 0;
  }
  p.segcnt[i] = c;
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sp_colkeys(const SparseBuild p) {
  const int64_t t = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (t >= p.slots) return;
  const int64_t E = p.pos[p.slots];
  p.keys[t] = t < E ? ((uint64_t)p.ent_col[t] << p.row_bits | (uint64_t)p.rows[t]) : (uint64_t)p.n_b << p.row_bits;
  p.vals[t] = (uint32_t)t;
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sp_colwrite(const SparseBuild p, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (t >= p.pos[p.slots]) return;
  const uint64_t k = keys[t];
  p.ent_row[t] = (int32_t)(k & ((1ull << p.row_bits) - 1));
  p.ent_idx[t] = (int32_t)vals[t];
  p.flags[t] = (int32_t)(k >> p.row_bits);
}

struct SparseLse {
  int64_t n;
  const int64_t* __restrict__ off;
  const int32_t* __restrict__ seg;
  const int32_t* __restrict__ other;
  const float* __restrict__ val;
  const int32_t* __restrict__ idx;
  const float* __restrict__ sub;
  float scale;  // log2(e) / tau
  float tau;
  float* __restrict__ out;
  float2* __restrict__ part;
};

// (m, s) <- (m, s) + (om, os), both sums s 2^m; an empty side is (-inf, 0) and never meets inf - inf (mke_sinkhorn.hip)
__device__ __forceinline__ void sp_merge(float& m, float& s, float om, float os) {
  const float mn = fmaxf(m, om);
  const float e0 = m == mn ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
  const float e1 = om == mn ? 1.0f : __builtin_amdgcn_exp2f(om - mn);
  s = s * e0 + os * e1;
  m = mn;
}

// entries e0, e0 + step, ... below e1 into the lane's running (m, s)
template <bool IDX, bool SUB>
__device__ __forceinline__ void sp_accumulate(const SparseLse& p, int64_t e0, int64_t e1, int step, float& m, float& s) {
#pragma unroll 4
  for (int64_t e = e0; e < e1; e += step) {   // the loads of four entries are issued before the first dependent exp
    const int o = p.other[e];
    const float v = IDX ? p.val[p.idx[e]] : p.val[e];
    const float sb = SUB ? p.sub[o] : 0.f;
    const float x = (v - sb) * p.scale;
    if (x > -INFINITY) {                                     // an argument of -inf (or a NaN) adds nothing
      const float d = x - m;                                 // m = -inf (nothing seen yet): +inf
      const float ex = __builtin_amdgcn_exp2f(-fabsf(d));    // in (0, 1], 0 for d = +inf
      const bool up = d > 0.f;
      s = up ? fmaf(s, ex, 1.0f) : s + ex;
      m = up ? x : m;
    }
  }
}

__device__ __forceinline__ float sp_finish(float tau, double m, double s) {
  return (float)((double)tau * 0.69314718055994530942 * (m + log2(s)));
}

template <bool IDX, bool SUB>
__global__ __launch_bounds__(MKE_BLOCK) void k_sp_lse_short(const SparseLse p) {
  const int l = threadIdx.x & 15;
  const int64_t i = (int64_t)blockIdx.x * MKE_SUBS_PER_BLOCK + (threadIdx.x >> 4);
  const bool live = i < p.n;
  const int64_t o0 = live ? p.off[i] : 0, o1 = live ? p.off[i + 1] : 0;
  const bool mine = live && o1 - o0 <= MKE_SPARSE_Q;
  float m = -INFINITY, s = 0.f;
  if (mine) sp_accumulate<IDX, SUB>(p, o0 + l, o1, 16, m, s);
#pragma unroll
  for (int w = 1; w < 16; w <<= 1) {
    const float om = __shfl_xor(m, w, 16);
    const float os = __shfl_xor(s, w, 16);
    sp_merge(m, s, om, os);
  }
  if (mine && l == 0) p.out[i] = o1 == o0 ? 0.f : sp_finish(p.tau, (double)m, (double)s);
}

template <bool IDX, bool SUB>
__global__ __launch_bounds__(MKE_BLOCK) void k_sp_lse_seg(const SparseLse p) {
  const int lane = threadIdx.x & 63;
  const int items = p.seg[p.n];
  const int waves = gridDim.x * (MKE_BLOCK / 64);
  for (int w = blockIdx.x * (MKE_BLOCK / 64) + (threadIdx.x >> 6); w < items; w += waves) {   // wave-uniform
    int64_t lo = 0, hi = p.n;   // the last list i with seg[i] <= w: it owns the item (lists without items have seg[i] == seg[i + 1])
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (p.seg[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int64_t e0 = p.off[lo] + (int64_t)(w - p.seg[lo]) * MKE_SPARSE_SEG;
    const int64_t end = p.off[lo + 1];
    const int64_t e1 = e0 + MKE_SPARSE_SEG < end ? e0 + MKE_SPARSE_SEG : end;
    float m = -INFINITY, s = 0.f;
    sp_accumulate<IDX, SUB>(p, e0 + lane, e1, 64, m, s);
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
      const float om = __shfl_xor(m, x, 64);
      const float os = __shfl_xor(s, x, 64);
      sp_merge(m, s, om, os);
    }
    if (lane == 0) p.part[w] = make_float2(m, s);
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sp_lse_merge(const SparseLse p) {
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  const int w0 = p.seg[i], w1 = p.seg[i + 1];
  if (w0 == w1) return;   // a short list: k_sp_lse_short wrote it
  float top = -INFINITY;
  for (int w = w0; w < w1; ++w) top = fmaxf(top, p.part[w].x);
  double sum = 0.0;
  for (int w = w0; w < w1; ++w) {
    const float2 ms = p.part[w];
    if (ms.y > 0.f) sum += (double)ms.y * exp2((double)ms.x - (double)top);
  }
  p.out[i] = sp_finish(p.tau, (double)top, sum);
}

// the carving of mke_sparse_support's temp
struct SparseTemp {
  int64_t keys, keys_alt, vals, vals_alt, flags, pos, rows, segcnt, cub, total;
  size_t cub_bytes;
};

static SparseTemp sparse_temp(int64_t n_a, int64_t n_b, int64_t slots) {
  SparseTemp t;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += align256(bytes); return here; };
  t.keys = take(slots * 8); t.keys_alt = take(slots * 8);
  t.vals = take(slots * 4); t.vals_alt = take(slots * 4);
  t.flags = take((slots + 1) * 4); t.pos = take((slots + 1) * 4);
  t.rows = take(slots * 4);
  const int64_t longer = (n_a > n_b ? n_a : n_b) + 1;
  t.segcnt = take(longer * 4);
  size_t a = 0, b = 0, c = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)slots, 0, 64, (hipStream_t)0);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)(slots + 1), (hipStream_t)0);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const int32_t*)nullptr, (int32_t*)nullptr, (int)longer, (hipStream_t)0);
  t.cub_bytes = a > b ? a : b;
  if (c > t.cub_bytes) t.cub_bytes = c;
  t.cub = take((int64_t)t.cub_bytes);
  t.total = at;
  return t;
}

static int support_shape(int64_t n_a, int64_t n_b, int cut_r, int cut_c, int64_t* slots) {
  if (n_a < 0 || n_b < 0 || n_a > MKE_SPARSE_MAX_SLOTS || n_b > MKE_SPARSE_MAX_SLOTS) { sparse_error("mke_sparse_support: bad n_a / n_b"); return MKE_SPARSE_E_SHAPE; }
  if (cut_r < 1 || cut_c < 1) { sparse_error("mke_sparse_support: cut_r and cut_c must be >= 1 (got %d, %d)", cut_r, cut_c); return MKE_SPARSE_E_SHAPE; }
  const int64_t s = n_a * cut_r + n_b * cut_c;   // < 2^63: both products are below 2^62
  if (s > MKE_SPARSE_MAX_SLOTS) {
    sparse_error("mke_sparse_support: n_a * cut_r + n_b * cut_c = %lld list slots exceed what the sort counts (%d)", (long long)s, MKE_SPARSE_MAX_SLOTS);
    return MKE_SPARSE_E_RANGE;
  }
  *slots = s;
  return MKE_SPARSE_OK;
}

}  // namespace mke

extern "C" const char* mke_sparse_last_error(void) { return g_sparse_err; }

extern "C" int mke_sparse_version(void) { return MKE_SPARSE_VERSION; }

extern "C" int64_t mke_sparse_support_temp_bytes(int64_t n_a, int64_t n_b, int cut_r, int cut_c) {
  int64_t slots = 0;
  const int rc = mke::support_shape(n_a, n_b, cut_r, cut_c, &slots);
  if (rc != MKE_SPARSE_OK) return rc;
  return slots == 0 ? 0 : mke::sparse_temp(n_a, n_b, slots).total;
}

extern "C" int mke_sparse_support(const mke_sparse_support_args* args, void* stream) {
  using namespace mke;
  if (!args) { sparse_error("mke_sparse_support: NULL args"); return MKE_SPARSE_E_NULL; }
  const mke_sparse_support_args& g = *args;
  int64_t slots = 0;
  const int rc = support_shape(g.n_a, g.n_b, g.cut_r, g.cut_c, &slots);
  if (rc != MKE_SPARSE_OK) return rc;
  if (!g.row_off || !g.col_off || !g.row_seg || !g.col_seg || !g.count) { sparse_error("mke_sparse_support: NULL row_off, col_off, row_seg, col_seg or count"); return MKE_SPARSE_E_NULL; }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (slots == 0) {   // n_a == n_b == 0
    e = hipMemsetAsync(g.row_off, 0, sizeof(int64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g.col_off, 0, sizeof(int64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g.row_seg, 0, sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g.col_seg, 0, sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g.count, 0, sizeof(int64_t), st);
    if (e != hipSuccess) { sparse_error("mke_sparse_support: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    return MKE_SPARSE_OK;
  }
  if ((g.n_a > 0 && (!g.val_r || !g.col_r)) || (g.n_b > 0 && (!g.val_c || !g.row_c))) { sparse_error("mke_sparse_support: NULL list (val_r, col_r, val_c, row_c)"); return MKE_SPARSE_E_NULL; }
  if (!g.ent_col || !g.ent_val || !g.ent_row || !g.ent_idx) { sparse_error("mke_sparse_support: NULL ent_col, ent_val, ent_row or ent_idx"); return MKE_SPARSE_E_NULL; }
  if (!g.temp) { sparse_error("mke_sparse_support: NULL temp"); return MKE_SPARSE_E_NULL; }
  if (g.capacity < slots) { sparse_error("mke_sparse_support: capacity %lld below n_a * cut_r + n_b * cut_c = %lld", (long long)g.capacity, (long long)slots); return MKE_SPARSE_E_SHAPE; }
  const SparseTemp t = sparse_temp(g.n_a, g.n_b, slots);
  if (g.temp_bytes < t.total) { sparse_error("mke_sparse_support: temp_bytes below mke_sparse_support_temp_bytes (%lld)", (long long)t.total); return MKE_SPARSE_E_SHAPE; }
  char* base = (char*)g.temp;
  SparseBuild p;
  p.val_r = g.val_r; p.col_r = g.col_r; p.val_c = g.val_c; p.row_c = g.row_c; p.n_a = g.n_a; p.n_b = g.n_b; p.cut_r = g.cut_r; p.cut_c = g.cut_c;
  p.slots = slots; p.col_bits = bit_length(g.n_b); p.row_bits = bit_length(g.n_a);
  p.keys = (uint64_t*)(base + t.keys); p.vals = (uint32_t*)(base + t.vals);
  p.flags = (int32_t*)(base + t.flags); p.pos = (int32_t*)(base + t.pos); p.rows = (int32_t*)(base + t.rows); p.segcnt = (int32_t*)(base + t.segcnt);
  p.ent_col = g.ent_col; p.ent_val = g.ent_val; p.ent_row = g.ent_row; p.ent_idx = g.ent_idx; p.count = g.count;
  uint64_t* keys_alt = (uint64_t*)(base + t.keys_alt);
  uint32_t* vals_alt = (uint32_t*)(base + t.vals_alt);
  void* cub = base + t.cub;
  size_t tb = t.cub_bytes;
  auto blocks = [](int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
  auto launched = [&](const char* what) {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { sparse_error("%s: launch failed: %s", what, hipGetErrorString(le)); return (int)le; }
    return 0;
  };
  int le;
  hipLaunchKernelGGL(k_sp_emit, blocks(g.n_a + g.n_b, MKE_SUBS_PER_BLOCK), dim3(MKE_BLOCK), 0, st, p);
  if ((le = launched("k_sp_emit"))) return le;
  if ((e = hipcub::DeviceRadixSort::SortPairs(cub, tb, (const uint64_t*)p.keys, keys_alt, (const uint32_t*)p.vals, vals_alt, (int)slots, 0, p.col_bits + 1 + p.row_bits, st)) != hipSuccess) { sparse_error("mke_sparse_support: radix sort: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(k_sp_flag, blocks(slots + 1, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p, (const uint64_t*)keys_alt);
  if ((le = launched("k_sp_flag"))) return le;
  tb = t.cub_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(cub, tb, (const int32_t*)p.flags, p.pos, (int)(slots + 1), st)) != hipSuccess) { sparse_error("mke_sparse_support: scan: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(k_sp_compact, blocks(slots + 1, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p, (const uint64_t*)keys_alt, (const uint32_t*)vals_alt);
  if ((le = launched("k_sp_compact"))) return le;
  hipLaunchKernelGGL(k_sp_offsets, blocks(g.n_a + 1, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p, (const int32_t*)p.rows, g.n_a, g.row_off);
  if ((le = launched("k_sp_offsets"))) return le;
  tb = t.cub_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(cub, tb, (const int32_t*)p.segcnt, g.row_seg, (int)(g.n_a + 1), st)) != hipSuccess) { sparse_error("mke_sparse_support: scan: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(k_sp_colkeys, blocks(slots, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p);
  if ((le = launched("k_sp_colkeys"))) return le;
  tb = t.cub_bytes;
  if ((e = hipcub::DeviceRadixSort::SortPairs(cub, tb, (const uint64_t*)p.keys, keys_alt, (const uint32_t*)p.vals, vals_alt, (int)slots, 0, p.row_bits + p.col_bits, st)) != hipSuccess) { sparse_error("mke_sparse_support: radix sort: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(k_sp_colwrite, blocks(slots, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p, (const uint64_t*)keys_alt, (const uint32_t*)vals_alt);
  if ((le = launched("k_sp_colwrite"))) return le;
  hipLaunchKernelGGL(k_sp_offsets, blocks(g.n_b + 1, MKE_BLOCK), dim3(MKE_BLOCK), 0, st, p, (const int32_t*)p.flags, g.n_b, g.col_off);
  if ((le = launched("k_sp_offsets"))) return le;
  tb = t.cub_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(cub, tb, (const int32_t*)p.segcnt, g.col_seg, (int)(g.n_b + 1), st)) != hipSuccess) { sparse_error("mke_sparse_support: scan: %s", hipGetErrorString(e)); return (int)e; }
  return MKE_SPARSE_OK;
}

extern "C" int64_t mke_sparse_lse_temp_bytes(int64_t capacity) {
  if (capacity < 0) { sparse_error("mke_sparse_lse: capacity is negative"); return MKE_SPARSE_E_SHAPE; }
  return (capacity / MKE_SPARSE_Q + 1) * (int64_t)sizeof(float2);   // a list has segments only above Q entries: ceil(len / SEG) <= len / Q
}

extern "C" int mke_sparse_lse(const mke_sparse_lse_args* args, void* stream) {
  using namespace mke;
  if (!args) { sparse_error("mke_sparse_lse: NULL args"); return MKE_SPARSE_E_NULL; }
  const mke_sparse_lse_args& g = *args;
  if (g.n < 0 || g.n > MKE_SPARSE_MAX_SLOTS) { sparse_error("mke_sparse_lse: bad n"); return MKE_SPARSE_E_SHAPE; }
  if (g.capacity < 0) { sparse_error("mke_sparse_lse: capacity is negative"); return MKE_SPARSE_E_SHAPE; }
  if (!(g.tau > 0.f) || !isfinite(g.tau)) { sparse_error("mke_sparse_lse: tau must be positive and finite"); return MKE_SPARSE_E_RANGE; }
  if (g.n == 0) return MKE_SPARSE_OK;
  if (!g.off || !g.seg || !g.out) { sparse_error("mke_sparse_lse: NULL off, seg or out"); return MKE_SPARSE_E_NULL; }
  if (g.capacity > 0 && (!g.other || !g.val || !g.temp)) { sparse_error("mke_sparse_lse: NULL other, val or temp"); return MKE_SPARSE_E_NULL; }
  const int64_t need = mke_sparse_lse_temp_bytes(g.capacity);
  if (g.capacity > 0 && g.temp_bytes < need) { sparse_error("mke_sparse_lse: temp_bytes below mke_sparse_lse_temp_bytes (%lld)", (long long)need); return MKE_SPARSE_E_SHAPE; }
  hipStream_t st = (hipStream_t)stream;
  SparseLse p;
  p.n = g.n; p.off = g.off; p.seg = g.seg; p.other = g.other; p.val = g.val; p.idx = g.idx; p.sub = g.sub;
  p.scale = (float)(1.4426950408889634074 / (double)g.tau); p.tau = g.tau; p.out = g.out; p.part = (float2*)g.temp;
  const dim3 block(MKE_BLOCK);
  const dim3 short_grid((unsigned)((g.n + MKE_SUBS_PER_BLOCK - 1) / MKE_SUBS_PER_BLOCK));
  const int64_t max_items = g.capacity / MKE_SPARSE_Q;
  const int64_t seg_blocks = (max_items + MKE_BLOCK / 64 - 1) / (MKE_BLOCK / 64);
  const dim3 seg_grid((unsigned)(seg_blocks < 1024 ? seg_blocks : 1024));
  auto both = [&](auto idx, auto sub) {
    constexpr bool I = decltype(idx)::value, S = decltype(sub)::value;
    hipLaunchKernelGGL((k_sp_lse_short<I, S>), short_grid, block, 0, st, p);
    if (seg_grid.x > 0) hipLaunchKernelGGL((k_sp_lse_seg<I, S>), seg_grid, block, 0, st, p);
  };
  auto with_sub = [&](auto idx) {
    if (g.sub) both(idx, std::true_type{}); else both(idx, std::false_type{});
  };
  if (g.idx) with_sub(std::true_type{}); else with_sub(std::false_type{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sparse_error("k_sp_lse_short / k_sp_lse_seg: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  if (seg_grid.x > 0) {
    hipLaunchKernelGGL(k_sp_lse_merge, dim3((unsigned)((g.n + MKE_BLOCK - 1) / MKE_BLOCK)), block, 0, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) { sparse_error("k_sp_lse_merge: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  }
  return MKE_SPARSE_OK;
}
