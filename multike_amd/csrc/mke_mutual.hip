// mke_mutual.hip — mutual (bidirectional) nearest-neighbour alignment on the matrix cores (gfx950), WITHOUT the n_a x n_b
// similarity matrix: row i and column j are a predicted pair when j is i's best column AND i is j's best row.
//
//   mke_align_mutual  one sweep (mke_simtile.h) that folds every re-scored similarity s_ij — rescore<MET, CSLS> of
//                     mke_rescore.h, evaluated ONCE per pair — into BOTH directions: row_best[i] = max over j and
//                     col_best[j] = max over i of the packed word best_key(s_ij, other index).  Two sweeps with the operands
//                     swapped would round (2 s - r_T[i]) - r_S[j] and (2 s - r_S[j]) - r_T[i] differently; here "mutual" is
//                     decided on one f32 value.
//   mke_mutual_pairs  match[i] = the column j with row_best[i] -> j, col_best[j] -> i and value >= threshold, else -1; the
//                     counts.  Separate from the sweep: another threshold needs no second sweep.
//
// Row direction: k_align_rank's fold (mke_eval.hip, RankBest<true>) without its counters, one 64-bit atomic max per (row,
// column chunk).  Column direction: in the sweep's epilogue a lane holds ONE column and 16 rows of it; it folds the 16
// registers, then the wavefront's two halves (__shfl_xor 32), then the block's four wavefronts with an LDS 64-bit max into
// s_col[tile parity][column of the tile]; the NEXT tile's epilogue (a barrier of the sweep lies between) publishes the
// finished tile: BN consecutive threads, BN consecutive words of col_best = 512 / 256 contiguous bytes, one 64-bit atomic max
// per (column, row block).  Every fold is a maximum of one totally ordered key: the result does not depend on the order in
// which lanes, wavefronts or blocks arrive.  Two other forms stay selectable for measurements (mke_mutual_args.flags): without
// the LDS fold (four times the global atomics), and with a plain load of the word before the atomic that skips it when the word
// already holds more (it only grows, so a stale read is safe).  Neither is faster: the column fold costs its VALU work in the
// epilogue, not its atomics.  Measurements and the choice of this form: profiles/r19_mutual.md.
//
// NaN and -inf as mke_align_rank_ex: a NaN similarity is never anybody's best; a row or column of NaN leaves the caller's zeroed
// word; a row or column of -inf publishes (-inf, its lowest index).
#include "mke_rescore.h"

#include <math.h>

namespace mke {

struct MutualParams {
  const float* __restrict__ a;  // [n_a][lda]
  int lda;
  const float* __restrict__ b;  // [n_b][ldb]
  int ldb;
  int n_a, n_b;
  int tiles_per_chunk;
  const float* __restrict__ sq_a;  // euclidean: squared row norms
  const float* __restrict__ sq_b;
  const float* __restrict__ term_row;  // the re-scoring terms
  const float* __restrict__ term_col;
  unsigned long long* row_best;  // [n_a]
  unsigned long long* col_best;  // [n_b]
  int flags;                     // MKE_MUTUAL_*
};

#define MUTUAL_NO_INDEX 0x7FFFFFFF  // a running best that has no row / column yet

// (v, i) := the better of (v, i) and (ov, oi): the larger value, the lower index among equal values.  NaN loses every comparison.
__device__ __forceinline__ void mutual_take(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// one 64-bit atomic max on a word that only grows; `filter`: not when a plain load already shows at least the key
__device__ __forceinline__ void mutual_publish(unsigned long long* word, unsigned long long key, bool filter) {
  if (filter && *(volatile unsigned long long*)word >= key) return;
  atomicMax(word, key);
}

// KS = kpad / 16; MET, CSLS: the epilogue of mke_rescore.h
template <int KS, int MET, bool CSLS>
__global__ __launch_bounds__(MKE_BLOCK) void k_align_mutual(const MutualParams p) {
  constexpr bool EUC = MET == MKE_METRIC_EUCLIDEAN;
  constexpr int BN = SIMT_BN_FOR(KS);
  __shared__ unsigned long long s_col[2][BN];  // running column bests of the tile in flight / the tile being published
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int strip0 = blockIdx.x * SIMT_BM + wv * 32;
  const bool lds_fold = !(p.flags & MKE_MUTUAL_NO_LDS_FOLD), filter = (p.flags & MKE_MUTUAL_FILTER) != 0;
  float a[KS * 8];
  float sqi[16], rti[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    sqi[reg] = (EUC && r < p.n_a) ? p.sq_a[r] : 0.f;
    rti[reg] = (CSLS && r < p.n_a) ? p.term_row[r] : 0.f;
  }
  {
    const int r = strip0 + l31;
    const bool ok = r < p.n_a;
    simt_load_fragment<KS>(p.a + (int64_t)(ok ? r : 0) * p.lda, ok, half, a);
  }
  float bestv[16];
  int bestc[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    bestv[reg] = -INFINITY;
    bestc[reg] = MUTUAL_NO_INDEX;
  }
  for (int i = threadIdx.x; i < 2 * BN; i += MKE_BLOCK) s_col[i / BN][i % BN] = 0ull;  // the sweep's first barrier follows
  const int ntiles = (p.n_b + BN - 1) / BN;
  const int t0 = blockIdx.y * p.tiles_per_chunk;
  const int t1 = min(ntiles, t0 + p.tiles_per_chunk);
  // tile t is complete in s_col[t & 1] (a barrier of the sweep has passed since its last fold): publish it and clear the slots
  // for tile t + 2, whose folds lie behind the next barrier
  auto flush = [&](int t) {
    if (threadIdx.x < BN) {
      const unsigned long long key = s_col[t & 1][threadIdx.x];
      if (key != 0ull) {  // only a column < n_b that some row of this block reaches has a key
        s_col[t & 1][threadIdx.x] = 0ull;
        mutual_publish(&p.col_best[t * BN + threadIdx.x], key, filter);
      }
    }
  };
  simt_sweep<KS>(a, p.b, p.ldb, p.n_b, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    const int col0 = col - l31;  // the first column of this 32-column group
    const int t = col0 / BN;
    if (lds_fold && col0 % BN == 0 && t > t0) flush(t - 1);
    const float sqj = (EUC && col_ok) ? p.sq_b[col] : 0.f;
    const float rsj = (CSLS && col_ok) ? p.term_col[col] : 0.f;
    float cv = -INFINITY;  // this column over the lane's 16 rows
    int cr = MUTUAL_NO_INDEX;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float s = rescore<MET, CSLS>(acc[reg], sqi[reg], sqj, rti[reg], rsj);  // once: both folds see this value
      // columns ascend over the sweep, rows ascend with reg: the lowest index wins a tie, also against the start value -inf
      if (col_ok) mutual_take(bestv[reg], bestc[reg], s, col);
      const int row = simt_row(reg, half, strip0);
      if (row < p.n_a) mutual_take(cv, cr, s, row);
    }
    mutual_take(cv, cr, __shfl_xor(cv, 32, 64), __shfl_xor(cr, 32, 64));  // the other half: the same column, 16 other rows
    if (half == 0 && col_ok && cr != MUTUAL_NO_INDEX) {                    // else: all NaN, or no row of this strip exists
      const unsigned long long key = best_key(cv, cr);
      if (lds_fold) atomicMax(&s_col[t & 1][col - t * BN], key);
      else mutual_publish(&p.col_best[col], key, filter);
    }
  });
  if (lds_fold && t0 < t1) flush(t1 - 1);  // the sweep ends in a barrier
  // rows: fold the 32 lanes of each half (they hold different columns of the same 16 rows)
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    float bv = bestv[reg];
    int bc = bestc[reg];
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) mutual_take(bv, bc, __shfl_xor(bv, off, 64), __shfl_xor(bc, off, 64));
    const int row = simt_row(reg, half, strip0);
    if (l31 == 0 && row < p.n_a && t0 < t1 && bc != MUTUAL_NO_INDEX) atomicMax(&p.row_best[row], best_key(bv, bc));  // else: all NaN in this chunk
  }
}

struct MutualPairsParams {
  const unsigned long long* __restrict__ row_best;
  const unsigned long long* __restrict__ col_best;
  int n_a, n_b;
  float threshold;
  int32_t* __restrict__ match;
  int32_t* counts;
};

__device__ __forceinline__ int mutual_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

__global__ __launch_bounds__(MKE_BLOCK) void k_mutual_pairs(const MutualPairsParams p) {
  __shared__ int s_m[MKE_BLOCK / 64], s_g[MKE_BLOCK / 64];
  int matched = 0, gold = 0;
  for (int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; i < p.n_a; i += (int64_t)gridDim.x * MKE_BLOCK) {
    const unsigned long long key = p.row_best[i];
    int m = -1;
    if (key != 0ull) {
      const int j = mutual_index(key);
      // best_key keeps the raw bits' order: its inverse is that of ordered_bits
      const unsigned u = (unsigned)(key >> 32);
      const float v = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
      if (j >= 0 && j < p.n_b && v >= p.threshold) {
        const unsigned long long back = p.col_best[j];
        if (back != 0ull && mutual_index(back) == (int)i) m = j;
      }
    }
    p.match[i] = m;
    matched += m >= 0 ? 1 : 0;
    gold += m == (int)i ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    matched += __shfl_xor(matched, off, 64);
    gold += __shfl_xor(gold, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = matched; s_g[threadIdx.x >> 6] = gold; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int m = s_m[0] + s_m[1] + s_m[2] + s_m[3], g = s_g[0] + s_g[1] + s_g[2] + s_g[3];
    if (m) atomicAdd(&p.counts[0], m);
    if (g) atomicAdd(&p.counts[1], g);
  }
}

}  // namespace mke

extern "C" int mke_align_mutual(const mke_mutual_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_align_mutual: NULL args"); return MKE_E_NULL; }
  const mke_mutual_args& g = *args;
  const SweepOperands o = {"mke_align_mutual: ", false, g.n_a, g.n_b, g.kpad, g.lda, g.ldb, g.metric, g.sq_a, g.sq_b, g.csls_row, g.csls_col};
  int rc = check_operands(o, {OP_ROWS, OP_METRIC, OP_TERMS});
  if (rc != MKE_OK) return rc;
  if (g.flags & ~(MKE_MUTUAL_NO_LDS_FOLD | MKE_MUTUAL_FILTER)) { set_error("mke_align_mutual: unknown flags %d", g.flags); return MKE_E_UNSUPPORTED; }
  if (g.n_a == 0 || g.n_b == 0) return MKE_OK;  // no pair: both outputs stay as the caller zeroed them
  if (!g.a || !g.b || !g.row_best || !g.col_best) { set_error("mke_align_mutual: NULL pointer"); return MKE_E_NULL; }
  rc = check_operands(o, {OP_NORMS, OP_KPAD, OP_LD, OP_WIDTH});
  if (rc != MKE_OK) return rc;
  MutualParams p = {};
  p.a = g.a; p.lda = g.lda; p.b = g.b; p.ldb = g.ldb; p.n_a = (int)g.n_a; p.n_b = (int)g.n_b;
  p.sq_a = g.sq_a; p.sq_b = g.sq_b; p.term_row = g.csls_row; p.term_col = g.csls_col;
  p.row_best = (unsigned long long*)g.row_best; p.col_best = (unsigned long long*)g.col_best; p.flags = g.flags;
  // mke_align_rank_ex's column split (rank_grid of mke_eval.hip): the same chunk boundaries
  const SimtSplit sp = simt_split(p.n_a, p.n_b, g.kpad, 6144, 16, 6144);
  p.tiles_per_chunk = sp.tiles_per_chunk;
  const dim3 grid((unsigned)((p.n_a + SIMT_BM - 1) / SIMT_BM), (unsigned)sp.chunks);
  hipStream_t st = (hipStream_t)stream;
  (void)simt_for_kpad(g.kpad, [&](auto ks) {  // true: OP_WIDTH has passed
    for_rescore(g.metric == MKE_METRIC_EUCLIDEAN, g.csls_row != nullptr, [&](auto met, auto csls) {
      hipLaunchKernelGGL((k_align_mutual<decltype(ks)::value, decltype(met)::value, decltype(csls)::value>), grid, dim3(MKE_BLOCK), 0,
                         st, p);
    });
  });
  return check_launch("k_align_mutual");
}

extern "C" int mke_mutual_pairs(const uint64_t* row_best, const uint64_t* col_best, int64_t n_a, int64_t n_b, float threshold,
                                int32_t* match, int32_t* counts, void* stream) {
  using namespace mke;
  if (n_a < 0 || n_b < 0 || n_a > 0x7FFFFF00LL || n_b > 0x7FFFFF00LL) { set_error("mke_mutual_pairs: bad n_a / n_b"); return MKE_E_SHAPE; }
  if (threshold != threshold) { set_error("mke_mutual_pairs: the threshold is NaN (-INFINITY = none)"); return MKE_E_RANGE; }
  if (!counts || (n_a > 0 && (!row_best || !match)) || (n_a > 0 && n_b > 0 && !col_best)) {
    set_error("mke_mutual_pairs: NULL pointer");
    return MKE_E_NULL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st) != hipSuccess) return check_launch("mke_mutual_pairs: memset");
  if (n_a == 0) return MKE_OK;
  MutualPairsParams p = {(const unsigned long long*)row_best, (const unsigned long long*)col_best, (int)n_a, (int)n_b, threshold, match, counts};
  const int64_t blocks = (n_a + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_mutual_pairs, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_mutual_pairs");
}
