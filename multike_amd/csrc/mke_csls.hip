// mke_csls.hip — CSLS re-scoring and the euclidean metric for the alignment evaluator (gfx950), without the n1 x n2 matrix.
//
// What it computes = code/base/similarity.py:9-81 as used by code/base/alignment.py:8-79 with metric / csls_k:
//   sim(i, j)  = METRIC(E1_i . E2_j):  inner: the dot product;  euclidean: 1 - sqrt(max(|E1_i|^2 + |E2_j|^2 - 2 dot, 0))
//   r_T(i)     = mean of the k largest sim(i, j) over the n2 columns     (calculate_nearest_k(sim_mat, k))
//   r_S(j)     = mean of the k largest sim(i, j) over the n1 rows        (calculate_nearest_k(sim_mat.T, k))
//   csls(i, j) = (2 sim(i, j) - r_T(i)) - r_S(j)                         (csls_sim, f32, in this order)
// This file makes r_T / r_S.  The reference builds the matrix (60K x 60K fp32 = 14 GB) and partitions it
// twice; here every similarity is made by the f32 MFMA sweep of mke_simtile.h and folded in registers / LDS:
//
//   k_topk_partial  the top-k of every row of A against one column chunk of B: a per-row LDS buffer of 64 floats takes the
//                   values above the row's running threshold tau (ballot per accumulator register, as k_sim_select); a full
//                   buffer is compacted to its k largest (rank by comparison inside the half-wave that owns the row) and
//                   tau rises to the k-th.  k values per (row, chunk) go out.  LDS: 32 KB of buffers + the sweep's tiles
//                   (43 KB at kpad 80: two blocks per CU on the 160 KB of gfx950).
//   k_topk_mean     per row of a list of values (the chunk partials, or a whole similarity row in the large-k path): exact
//                   k-th largest by radix_select_kth, the values above it sorted descending (sort_desc), summed in
//                   float64 in descending order with the ties of the k-th last, divided by k, rounded to f32 — a unique,
//                   run-to-run identical mean of the exact top-k multiset.
// The rank of the gold column under the re-scored similarity is k_align_rank of mke_eval.hip.
#include "mke_rescore.h"

#include <math.h>

namespace mke {

#define CSLS_BUF 64          // per-row LDS buffer of k_topk_partial
#define CSLS_FAST_K 32       // k <= CSLS_FAST_K: the partial sweep; above: whole rows through mke_sim_sample + k_topk_mean
#define CSLS_SORT_LDS 4096   // k_topk_mean sorts up to this many values in LDS, more in the caller's scratch

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------ top-k partials
struct TopkPartialParams {
  const float* __restrict__ a;  // [n_a][lda]
  int lda;
  const float* __restrict__ b;  // [n_b][ldb]
  int ldb;
  int n_a, n_b;
  const float* __restrict__ sq_a;  // euclidean: squared row norms
  const float* __restrict__ sq_b;
  int k, chunks, tiles_per_chunk;
  float* __restrict__ part;  // [n_a][chunks][k]
};

// The buffer of a row holds n values (n <= CSLS_BUF); the 32 lanes of the owning half-wave rank them (ties by position) and
// write the k largest, descending, to the front.  Returns the k-th largest.
__device__ __attribute__((noinline)) float csls_compact(float* buf, int n, int k, int l31) {
  const float x0 = l31 < n ? buf[l31] : 0.f;
  const float x1 = l31 + 32 < n ? buf[l31 + 32] : 0.f;
  int r0 = 0, r1 = 0;
  for (int j = 0; j < n; ++j) {
    const float y = buf[j];
    r0 += (y > x0 || (y == x0 && j < l31)) ? 1 : 0;
    r1 += (y > x1 || (y == x1 && j < l31 + 32)) ? 1 : 0;
  }
  wave_sync_lds();  // every read of the buffer is done before it is rewritten
  if (l31 < n && r0 < k) buf[r0] = x0;
  if (l31 + 32 < n && r1 < k) buf[r1] = x1;
  wave_sync_lds();
  return buf[k - 1];
}

template <int KS, int MET>
__global__ __launch_bounds__(MKE_BLOCK) void k_topk_partial(const TopkPartialParams p) {
  __shared__ float s_buf[SIMT_BM][CSLS_BUF];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int strip0 = blockIdx.x * SIMT_BM + wv * 32;
  float a[KS * 8];
  {
    const int r = strip0 + l31;
    const bool ok = r < p.n_a;
    simt_load_fragment<KS>(p.a + (int64_t)(ok ? r : 0) * p.lda, ok, half, a);
  }
  float tau[16], sqi[16];
  int cnt[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    tau[reg] = -INFINITY;
    cnt[reg] = 0;
    sqi[reg] = (MET == MKE_METRIC_EUCLIDEAN && r < p.n_a) ? p.sq_a[r] : 0.f;
  }
  const int ntiles = (p.n_b + SIMT_BN_FOR(KS) - 1) / SIMT_BN_FOR(KS);
  const int t0 = blockIdx.y * p.tiles_per_chunk;
  const int t1 = min(ntiles, t0 + p.tiles_per_chunk);
  const unsigned lt = (1u << l31) - 1u;
  const int k = p.k;
  simt_sweep<KS>(a, p.b, p.ldb, p.n_b, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    const float sqj = (MET == MKE_METRIC_EUCLIDEAN && col_ok) ? p.sq_b[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float v = col_ok ? metric_value<MET>(acc[reg], sqi[reg], sqj) : -INFINITY;
      const bool hit = v > tau[reg];
      const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
      if (m == 0) continue;  // wave-uniform
      const unsigned mh = half ? (unsigned)(m >> 32) : (unsigned)m;  // the 32 lanes of a half hold 32 columns of ONE row
      const int nh = __popc(mh);
      float* buf = s_buf[simt_row(reg, half, wv * 32)];
      if (cnt[reg] + nh > CSLS_BUF) {  // uniform in the half: cnt > CSLS_BUF - 32 >= k, keep the k largest
        tau[reg] = csls_compact(buf, cnt[reg], k, l31);
        cnt[reg] = k;  // k + nh <= 64: the hits still fit (they beat the old tau; extra ones go at the next compaction)
      }
      if (hit) buf[cnt[reg] + __popc(mh & lt)] = v;
      cnt[reg] += nh;
    }
  });
  wave_sync_lds();
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rr = simt_row(reg, half);
    float* buf = s_buf[wv * 32 + rr];
    if (cnt[reg] > k) csls_compact(buf, cnt[reg], k, l31);
    const int row = strip0 + rr;
    if (row < p.n_a && l31 < k) {  // k <= 32: one value per lane; a chunk with fewer than k columns pads with -inf
      const int64_t o = ((int64_t)row * p.chunks + blockIdx.y) * p.k + l31;
      p.part[o] = l31 < cnt[reg] ? buf[l31] : -INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------ exact top-k mean
struct TopkMeanParams {
  const float* __restrict__ vals;  // [rows][ld], m values per row
  int64_t ld;
  int m, k;
  int metric;                       // MKE_METRIC_EUCLIDEAN: vals are dot products, turned into similarities on the fly
  const float* __restrict__ sq_a;   // [rows] (offset to the launch's first row)
  const float* __restrict__ sq_b;   // [m]
  unsigned* __restrict__ sort_tmp;  // [rows][sort_ld] when k > CSLS_SORT_LDS
  int64_t sort_ld;
  float* __restrict__ out;  // [rows]
};

__device__ __forceinline__ float mean_value(const TopkMeanParams& p, const float* v, float sqi, int i) {
  return p.metric == MKE_METRIC_EUCLIDEAN ? metric_value<MKE_METRIC_EUCLIDEAN>(v[i], sqi, p.sq_b[i]) : v[i];
}

__global__ __launch_bounds__(MKE_BLOCK) void k_topk_mean(const TopkMeanParams p) {
  __shared__ int s_hist[MKE_BLOCK / 64][256];
  __shared__ int s_wave[MKE_BLOCK / 64];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_gt;
  __shared__ unsigned s_sort[CSLS_SORT_LDS];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* __restrict__ v = p.vals + row * p.ld;
  const float sqi = p.metric == MKE_METRIC_EUCLIDEAN ? p.sq_a[row] : 0.f;
  if (tid == 0) s_gt = 0;
  int ties;  // copies of the k-th value in the top k; the other k - ties values are above it
  const unsigned kth = radix_select_kth(s_hist, s_wave, &s_prefix, &s_need, p.m, p.k, &ties,
                                        [&](int i) { return float_key(mean_value(p, v, sqi, i)); });
  const int gt = p.k - ties;
  int np2 = 1;
  while (np2 < gt) np2 <<= 1;
  unsigned* buf = p.k <= CSLS_SORT_LDS ? s_sort : p.sort_tmp + row * p.sort_ld;
  for (int i = tid; i < p.m; i += MKE_BLOCK) {
    const unsigned kx = float_key(mean_value(p, v, sqi, i));
    if (kx > kth) buf[atomicAdd(&s_gt, 1)] = kx;
  }
  __syncthreads();
  for (int i = gt + tid; i < np2; i += MKE_BLOCK) buf[i] = 0u;  // below every float key: sorts last
  __syncthreads();
  sort_desc(buf, np2);
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < gt; ++i) s += (double)key_float(buf[i]);
    const double kv = (double)key_float(kth);
    for (int i = 0; i < ties; ++i) s += kv;
    p.out[row] = (float)(s / (double)p.k);
  }
}

}  // namespace mke

static int topk_mean_temp(const mke::SweepOperands& o, int k, int64_t* bytes) {
  using namespace mke;
  *bytes = 0;
  const int rc = check_operands(o, {OP_ROWS, OP_KPAD});
  if (rc != MKE_OK) return rc;
  const int64_t n_a = o.n_a, n_b = o.n_b;
  if (k < 1 || (int64_t)k > n_b - 2) { set_error("mke_align_topk_mean: need 1 <= k <= n_b - 2 (k = %d, n_b = %lld)", k, (long long)n_b); return MKE_E_SHAPE; }
  if (k > (1 << 30)) { set_error("mke_align_topk_mean: k above 2^30 (the sort of the large-k path counts with 32-bit ints)"); return MKE_E_RANGE; }
  if (n_a == 0) return MKE_OK;
  int64_t floats;
  if (k <= CSLS_FAST_K) {
    floats = n_a * partial_split(n_a, n_b, o.kpad).chunks * k;  // < 2^31 * 64 * 32: the kernels index it with int64 offsets
  } else {
    const int64_t r = fallback_rows(n_a, n_b);
    floats = r * n_b + (k > CSLS_SORT_LDS ? r * pow2_at_least(k) : 0);
  }
  if (floats > ((int64_t)1 << 40)) { set_error("mke_align_topk_mean: scratch beyond 2^40 floats"); return MKE_E_RANGE; }
  *bytes = floats * 4;
  return MKE_OK;
}

extern "C" int64_t mke_align_topk_mean_temp_bytes(int64_t n_a, int64_t n_b, int kpad, int k) {
  int64_t bytes = 0;
  const int rc = topk_mean_temp({"mke_align_topk_mean: ", false, n_a, n_b, kpad}, k, &bytes);
  return rc != MKE_OK ? rc : bytes;
}

extern "C" int mke_align_topk_mean(const mke_topk_mean_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_align_topk_mean: NULL args"); return MKE_E_NULL; }
  const mke_topk_mean_args& g = *args;
  const SweepOperands o = {"mke_align_topk_mean: ", false, g.n_a, g.n_b, g.kpad, g.lda, g.ldb, g.metric, g.sq_a, g.sq_b, nullptr, nullptr};
  int64_t need = 0;
  int rc = topk_mean_temp(o, g.k, &need);
  if (rc == MKE_OK) rc = check_operands(o, {OP_METRIC});
  if (rc != MKE_OK) return rc;
  if (g.n_a == 0) return MKE_OK;
  if (!g.a || !g.b || !g.out || (need > 0 && !g.temp)) { set_error("mke_align_topk_mean: NULL pointer"); return MKE_E_NULL; }
  rc = check_operands(o, {OP_NORMS, OP_LD, OP_WIDTH});
  if (rc != MKE_OK) return rc;
  if (g.temp_bytes < need) { set_error("mke_align_topk_mean: temp below mke_align_topk_mean_temp_bytes (%lld)", (long long)need); return MKE_E_SHAPE; }
  hipStream_t st = (hipStream_t)stream;
  TopkMeanParams mp;
  mp.k = g.k; mp.metric = g.metric; mp.sort_tmp = nullptr; mp.sort_ld = 0;
  if (g.k <= CSLS_FAST_K) {
    TopkPartialParams p;
    p.a = g.a; p.lda = g.lda; p.b = g.b; p.ldb = g.ldb; p.n_a = (int)g.n_a; p.n_b = (int)g.n_b; p.sq_a = g.sq_a; p.sq_b = g.sq_b;
    p.k = g.k;
    const SimtSplit sp = partial_split(g.n_a, g.n_b, g.kpad);
    p.chunks = sp.chunks; p.tiles_per_chunk = sp.tiles_per_chunk;
    p.part = (float*)g.temp;
    dim3 grid((unsigned)((g.n_a + SIMT_BM - 1) / SIMT_BM), (unsigned)p.chunks);
    simt_for_kpad(g.kpad, [&](auto ks) {
      for_rescore(g.metric == MKE_METRIC_EUCLIDEAN, false, [&](auto met, auto) {  // the partials take the metric only
        hipLaunchKernelGGL((k_topk_partial<decltype(ks)::value, decltype(met)::value>), grid, dim3(MKE_BLOCK), 0, st, p);
      });
    });
    const int e = check_launch("k_topk_partial");
    if (e) return e;
    mp.vals = p.part; mp.ld = (int64_t)p.chunks * g.k; mp.m = p.chunks * g.k;
    mp.metric = MKE_METRIC_INNER;  // the partials are similarities already
    mp.sq_a = nullptr; mp.sq_b = nullptr; mp.out = g.out;
    hipLaunchKernelGGL(k_topk_mean, dim3((unsigned)g.n_a), dim3(MKE_BLOCK), 0, st, mp);
    return check_launch("k_topk_mean");
  }
  // large k: whole similarity rows of a bounded round of rows (the f32 MFMA chains of mke_sim_sample), then the same mean
  const int64_t r = fallback_rows(g.n_a, g.n_b);
  float* simrows = (float*)g.temp;
  mp.ld = g.n_b; mp.m = (int)g.n_b; mp.sq_b = g.sq_b;
  if (g.k > CSLS_SORT_LDS) { mp.sort_tmp = (unsigned*)(simrows + r * g.n_b); mp.sort_ld = pow2_at_least(g.k); }
  for (int64_t lo = 0; lo < g.n_a; lo += r) {
    const int64_t hi = lo + r < g.n_a ? lo + r : g.n_a;
    int e = mke_sim_sample(g.a, g.lda, g.kpad, g.n_a, lo, hi, g.b, g.ldb, (int)g.n_b, simrows, stream);
    if (e) return e;
    mp.vals = simrows; mp.sq_a = g.sq_a ? g.sq_a + lo : nullptr; mp.out = g.out + lo;
    hipLaunchKernelGGL(k_topk_mean, dim3((unsigned)(hi - lo)), dim3(MKE_BLOCK), 0, st, mp);
    e = check_launch("k_topk_mean");
    if (e) return e;
  }
  return MKE_OK;
}
