// mke_sinkhorn.hip — Sinkhorn re-scoring for the alignment evaluator (gfx950), without the n1 x n2 matrix.
//
// S is the n1 x n2 matrix of METRIC(i, j) as the sweep of mke_simtile.h produces it (f32; inner or euclidean, (9b) of
// include/multike_hip.h).  Temperature tau > 0, iterations L >= 1.  Potentials are in similarity units: a^0 = 0 (n1) and
// b^0 = 0 (n2).  For l = 1..L, rows first and then columns:
//   a_i = tau log sum_j exp((s_ij - b_j) / tau)        (uses the b of the previous iteration)
//   b_j = tau log sum_i exp((s_ij - a_i) / tau)        (uses the a just computed)
// The re-scored similarity is s_ij - a_i - b_j = tau log of the Sinkhorn matrix after L iterations of row normalisation
// followed by column normalisation, starting from exp(S / tau).  The library hands it to the existing kernels as csls_row = 2a,
// csls_col = 2b: their (2 s - csls_row[i]) - csls_col[j] is 2 (s - a - b) in f32, the doubling is exact and the ranking the same.
//
// A half-iteration is one call of mke_align_lse: out[i] = tau log sum_{j < n_b} exp((METRIC(i, j) - sub_b[j]) / tau).
//   k_lse_partial  one simt_sweep; per accumulator register (one row, the columns = lane & 31 mod 32 of a column chunk) a running
//                  (m, s) with sum = s 2^m, m the largest argument seen in log2 units: x = (v - sub_b[j]) log2(e) / tau, and per
//                  similarity ONE v_exp_f32 of -|x - m| <= 0 (whichever of the old sum and the new term is the smaller gets
//                  scaled) — no exp of a raw argument, so neither +-200 / tau overflows.  A masked column is skipped, a lane
//                  that saw none stays (-inf, 0).  The 32 lanes of the half-wave that owns a row merge in a fixed butterfly and
//                  one (m, s) per (row, chunk) goes to temp.
//   k_lse_merge    one thread per row: the chunks in chunk order in float64, out = tau ln 2 (m + log2 s) rounded to f32.
// Every order is fixed: two runs give the same bits.
#include "mke_rescore.h"

#include <math.h>

namespace mke {

struct LsePartialParams {
  const float* __restrict__ a;  // [n_a][lda]
  int lda;
  const float* __restrict__ b;  // [n_b][ldb]
  int ldb;
  int n_a, n_b;
  const float* __restrict__ sq_a;  // euclidean: squared row norms
  const float* __restrict__ sq_b;
  const float* __restrict__ sub_b;  // [n_b] or NULL = zeros
  float scale;                      // log2(e) / tau
  int chunks, tiles_per_chunk;
  float2* __restrict__ part;  // [n_a][chunks] (m, s)
};

// (m, s) <- (m, s) + (om, os), both sums s 2^m; an empty side is (-inf, 0) and never meets inf - inf
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mn = fmaxf(m, om);
  const float e0 = m == mn ? 1.0f : __builtin_amdgcn_exp2f(m - mn);    // m < mn: mn is finite, m - mn is a number or -inf
  const float e1 = om == mn ? 1.0f : __builtin_amdgcn_exp2f(om - mn);
  s = s * e0 + os * e1;
  m = mn;
}

template <int KS, int MET>
__global__ __launch_bounds__(MKE_BLOCK) void k_lse_partial(const LsePartialParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int strip0 = blockIdx.x * SIMT_BM + wv * 32;
  float a[KS * 8];
  {
    const int r = strip0 + l31;
    const bool ok = r < p.n_a;
    simt_load_fragment<KS>(p.a + (int64_t)(ok ? r : 0) * p.lda, ok, half, a);
  }
  float m[16], s[16], sqi[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    m[reg] = -INFINITY;
    s[reg] = 0.f;
    sqi[reg] = (MET == MKE_METRIC_EUCLIDEAN && r < p.n_a) ? p.sq_a[r] : 0.f;
  }
  const int ntiles = (p.n_b + SIMT_BN_FOR(KS) - 1) / SIMT_BN_FOR(KS);
  const int t0 = blockIdx.y * p.tiles_per_chunk;
  const int t1 = min(ntiles, t0 + p.tiles_per_chunk);
  const float scale = p.scale;
  simt_sweep<KS>(a, p.b, p.ldb, p.n_b, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    if (!col_ok) return;  // a column past n_b (the ragged last tile) adds nothing to its lane
    const float sqj = MET == MKE_METRIC_EUCLIDEAN ? p.sq_b[col] : 0.f;
    const float bj = p.sub_b ? p.sub_b[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float x = (metric_value<MET>(acc[reg], sqi[reg], sqj) - bj) * scale;
      const float d = x - m[reg];                             // m = -inf (nothing seen yet): +inf
      const float e = __builtin_amdgcn_exp2f(-fabsf(d));      // in (0, 1], 0 for d = +inf
      const bool up = d > 0.f;
      s[reg] = up ? fmaf(s[reg], e, 1.0f) : s[reg] + e;       // the larger of (old maximum, x) is the new unit
      m[reg] = up ? x : m[reg];
    }
  });
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    float mm = m[reg], ss = s[reg];
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const float om = __shfl_xor(mm, off, 64);
      const float os = __shfl_xor(ss, off, 64);
      lse_merge(mm, ss, om, os);
    }
    const int row = simt_row(reg, half, strip0);
    if (l31 == 0 && row < p.n_a && t0 < t1) p.part[(int64_t)row * p.chunks + blockIdx.y] = make_float2(mm, ss);
  }
}

struct LseMergeParams {
  const float2* __restrict__ part;  // [n_a][chunks]
  int n_a, chunks;
  float tau;
  float* __restrict__ out;  // [n_a]
};

__global__ __launch_bounds__(MKE_BLOCK) void k_lse_merge(const LseMergeParams p) {
  const int64_t row = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (row >= p.n_a) return;
  const float2* __restrict__ v = p.part + row * p.chunks;
  float top = -INFINITY;
  for (int c = 0; c < p.chunks; ++c) top = fmaxf(top, v[c].x);
  double sum = 0.0;
  for (int c = 0; c < p.chunks; ++c) {
    const float2 ms = v[c];
    if (ms.y > 0.f) sum += (double)ms.y * exp2((double)ms.x - (double)top);  // a chunk always holds a column: s >= 1 there
  }
  p.out[row] = (float)((double)p.tau * 0.69314718055994530942 * ((double)top + log2(sum)));
}

}  // namespace mke

static int lse_temp(const mke::SweepOperands& o, int64_t* bytes) {
  using namespace mke;
  *bytes = 0;
  const int rc = check_operands(o, {OP_ROWS, OP_KPAD});
  if (rc != MKE_OK) return rc;
  const int64_t n_a = o.n_a, n_b = o.n_b;
  if (n_b < 1) { set_error("mke_align_lse: need n_b >= 1 (the sum over no column has no logarithm)"); return MKE_E_SHAPE; }
  if (n_a == 0) return MKE_OK;
  *bytes = n_a * partial_split(n_a, n_b, o.kpad).chunks * (int64_t)sizeof(float2);  // < 2^31 * 64 * 8: indexed with int64 offsets
  return MKE_OK;
}

extern "C" int64_t mke_align_lse_temp_bytes(int64_t n_a, int64_t n_b, int kpad) {
  int64_t bytes = 0;
  const int rc = lse_temp({"mke_align_lse: ", false, n_a, n_b, kpad}, &bytes);
  return rc != MKE_OK ? rc : bytes;
}

extern "C" int mke_align_lse(const mke_lse_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_align_lse: NULL args"); return MKE_E_NULL; }
  const mke_lse_args& g = *args;
  const SweepOperands o = {"mke_align_lse: ", false, g.n_a, g.n_b, g.kpad, g.lda, g.ldb, g.metric, g.sq_a, g.sq_b, nullptr, nullptr};
  int64_t need = 0;
  int rc = lse_temp(o, &need);
  if (rc == MKE_OK) rc = check_operands(o, {OP_METRIC});
  if (rc != MKE_OK) return rc;
  if (!(g.tau > 0.f) || !isfinite(g.tau)) { set_error("mke_align_lse: tau must be positive and finite"); return MKE_E_RANGE; }
  if (g.n_a == 0) return MKE_OK;
  if (!g.a || !g.b || !g.out || !g.temp) { set_error("mke_align_lse: NULL pointer"); return MKE_E_NULL; }
  rc = check_operands(o, {OP_NORMS, OP_LD, OP_WIDTH});
  if (rc != MKE_OK) return rc;
  if (g.temp_bytes < need) { set_error("mke_align_lse: temp below mke_align_lse_temp_bytes (%lld)", (long long)need); return MKE_E_SHAPE; }
  hipStream_t st = (hipStream_t)stream;
  LsePartialParams p;
  p.a = g.a; p.lda = g.lda; p.b = g.b; p.ldb = g.ldb; p.n_a = (int)g.n_a; p.n_b = (int)g.n_b; p.sq_a = g.sq_a; p.sq_b = g.sq_b;
  p.sub_b = g.sub_b;
  p.scale = (float)(1.4426950408889634074 / (double)g.tau);
  const SimtSplit sp = partial_split(g.n_a, g.n_b, g.kpad);
  p.chunks = sp.chunks; p.tiles_per_chunk = sp.tiles_per_chunk;
  p.part = (float2*)g.temp;
  dim3 grid((unsigned)((g.n_a + SIMT_BM - 1) / SIMT_BM), (unsigned)p.chunks);
  simt_for_kpad(g.kpad, [&](auto ks) {
    for_rescore(g.metric == MKE_METRIC_EUCLIDEAN, false, [&](auto met, auto) {  // the metric only
      hipLaunchKernelGGL((k_lse_partial<decltype(ks)::value, decltype(met)::value>), grid, dim3(MKE_BLOCK), 0, st, p);
    });
  });
  const int e = check_launch("k_lse_partial");
  if (e) return e;
  LseMergeParams mp;
  mp.part = p.part; mp.n_a = p.n_a; mp.chunks = p.chunks; mp.tau = g.tau; mp.out = g.out;
  hipLaunchKernelGGL(k_lse_merge, dim3((unsigned)((g.n_a + MKE_BLOCK - 1) / MKE_BLOCK)), dim3(MKE_BLOCK), 0, st, mp);
  return check_launch("k_lse_merge");
}
