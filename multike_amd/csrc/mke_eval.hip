// mke_eval.hip — alignment evaluator on the matrix cores (gfx950): rank of the gold counterpart under a similarity, WITHOUT
// materialising the n1 x n2 similarity matrix.  One kernel, k_align_rank, behind both entry points.
//
// What it computes = what code/base/alignment.py:141-163 `calculate_rank` extracts from code/base/similarity.py:9-81 `sim`
// (gold column = row index): for row i,
//   rank_i  = #{ j : sim[i][j] > sim[i][i] }   (position of the gold in the descending order, ties aside)
//   best_i  = argmax_j sim[i][j]               (the `hits1_rest` pair)
// Hits@k = mean(rank < k), MR = mean(rank + 1), MRR = mean(1 / (rank + 1)).  The reference materialises a 60K x 60K
// fp32 matrix (14 GB) and argsorts its rows in 8 worker processes; here a wavefront keeps a 32-row strip of E1 in
// registers, the block streams 64-column tiles of E2 through LDS (mke_simtile.h), multiplies them with
// v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fma chain) and folds each tile of similarities into per-row counters.
//
//   mke_align_rank     sim = the inner product of the (already normalised) rows; the tie counter is optional.
//   mke_align_rank_ex  every similarity passed through METRIC (inner / euclidean) and, with csls_row / csls_col, the re-scoring
//                      (2 s - csls_row[i]) - csls_col[j] of mke_rescore.h (CSLS means, or twice the Sinkhorn potentials).
//
// The gold similarity is taken from the SAME MFMA computation (the diagonal tile) through the SAME epilogue, so `sim > gold`
// is an exact comparison of identically rounded numbers and a row never counts itself.
#include "mke_rescore.h"

#include <math.h>

namespace mke {

struct AlignRankParams {
  const float* __restrict__ emb1;  // [n1][ld1]
  int ld1;
  const float* __restrict__ emb2;  // [n2][ld2]
  int ld2;
  int n1, n2;
  int tiles_per_chunk;
  const float* __restrict__ sq1;  // euclidean: squared row norms
  const float* __restrict__ sq2;
  const float* __restrict__ csls_row;  // CSLS: the re-scoring terms
  const float* __restrict__ csls_col;
  int32_t* __restrict__ rank;
  int32_t* __restrict__ ties;  // #{ j : sim[i][j] == sim[i][i] } including j = i; unused without TIES
  unsigned long long* __restrict__ best;
};

// Where the two entry points differ on purpose: the running best of a (row, chunk).  What a row publishes follows from it —
//   mke_align_rank (EX = false): the best starts at (-3.0e38f, column 0) and is always published: a row none of whose
//     similarities exceeds -3.0e38f (all NaN, all -inf) publishes best_key(-3.0e38f, 0), a value no column has;
//   mke_align_rank_ex (EX = true): the best starts at (-inf, no column), an equal value at a lower column replaces it, and it
//     is published only once it has a column: a row of -inf publishes (-inf, its lowest column), a row of NaN leaves the
//     caller's zeroed word as it is.
// Everywhere else (any similarity above -3.0e38f) both publish (maximum, lowest column attaining it).
template <bool EX>
struct RankBest {
  static constexpr float kStart = EX ? -INFINITY : -3.0e38f;
  static constexpr int kStartCol = EX ? 0x7FFFFFFF : 0;  // EX: no column yet
  static constexpr bool kGuard = EX;                     // publish only a best that has a column
};

// KS = kpad / 16; MET, CSLS: the epilogue of mke_rescore.h; TIES: also count the columns that tie with the gold
template <int KS, int MET, bool CSLS, bool TIES, bool EX>
__global__ __launch_bounds__(MKE_BLOCK) void k_align_rank(const AlignRankParams p) {
  constexpr bool EUC = MET == MKE_METRIC_EUCLIDEAN;
  __shared__ float s_gold[MKE_BLOCK / 64][32];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int strip0 = blockIdx.x * SIMT_BM + wv * 32;
  float a[KS * 8];
  float gold[16], sqi[16], rti[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    sqi[reg] = (EUC && r < p.n1) ? p.sq1[r] : 0.f;
    rti[reg] = (CSLS && r < p.n1) ? p.csls_row[r] : 0.f;
  }
  {
    const int r = strip0 + l31;
    const bool ok = r < p.n1;
    simt_load_fragment<KS>(p.emb1 + (int64_t)(ok ? r : 0) * p.ld1, ok, half, a);
    // gold similarity of row i = column i, from the SAME fma chain as the sweep computes it (bit-identical, so the row
    // never counts itself): the strip's 32 gold columns as a B fragment, diagonal of the 32 x 32 product
    float b[KS * 8];
    simt_load_fragment<KS>(p.emb2 + (int64_t)(ok ? r : 0) * p.ld2, ok, half, b);  // n2 >= n1: the row exists
    const f32x16 d = simt_fragment_product<KS>(a, b);
    const float sqj = (EUC && ok) ? p.sq2[r] : 0.f;  // this lane's column of the product is r
    const float rsj = (CSLS && ok) ? p.csls_col[r] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = simt_row(reg, half);
      if (m == l31) s_gold[wv][m] = rescore<MET, CSLS>(d[reg], sqi[reg], sqj, rti[reg], rsj);
    }
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) gold[reg] = s_gold[wv][simt_row(reg, half)];
  }
  int cnt[16];
  int eq[TIES ? 16 : 1];
  float bestv[16];
  int bestc[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    cnt[reg] = 0;
    bestv[reg] = RankBest<EX>::kStart;
    bestc[reg] = RankBest<EX>::kStartCol;
    if (TIES) eq[reg] = 0;
  }
  const int ntiles = (p.n2 + SIMT_BN_FOR(KS) - 1) / SIMT_BN_FOR(KS);
  const int t0 = blockIdx.y * p.tiles_per_chunk;
  const int t1 = min(ntiles, t0 + p.tiles_per_chunk);
  simt_sweep<KS>(a, p.emb2, p.ld2, p.n2, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    const float sqj = (EUC && col_ok) ? p.sq2[col] : 0.f;
    const float rsj = (CSLS && col_ok) ? p.csls_col[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float s = rescore<MET, CSLS>(acc[reg], sqi[reg], sqj, rti[reg], rsj);
      cnt[reg] += (col_ok && s > gold[reg]) ? 1 : 0;
      if (TIES) eq[reg] += (col_ok && s == gold[reg]) ? 1 : 0;
      // columns ascend: the lowest column wins a tie (EX: also against the start value -inf, which a column may equal)
      if (col_ok && (s > bestv[reg] || (EX && s == bestv[reg] && col < bestc[reg]))) { bestv[reg] = s; bestc[reg] = col; }
    }
  });
  // fold the 32 lanes of each half (they hold different columns of the same 16 rows)
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int c = cnt[reg];
    int ce = TIES ? eq[reg] : 0;
    float bv = bestv[reg];
    int bc = bestc[reg];
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      c += __shfl_xor(c, off, 64);
      if (TIES) ce += __shfl_xor(ce, off, 64);
      const float ov = __shfl_xor(bv, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    const int row = simt_row(reg, half, strip0);
    if (l31 == 0 && row < p.n1 && t0 < t1) {
      atomicAdd(&p.rank[row], c);
      if (TIES) atomicAdd(&p.ties[row], ce);
      if (!RankBest<EX>::kGuard) {
        const unsigned long long key = best_key(bv, bc);
        atomicMax(&p.best[row], key);
      }
    }
    if (RankBest<EX>::kGuard && l31 == 0 && row < p.n1 && t0 < t1 && bc != RankBest<EX>::kStartCol) {  // else: all NaN in this chunk
      const unsigned long long key = best_key(bv, bc);
      atomicMax(&p.best[row], key);
    }
  }
}

// Column split and grid of either entry point's launch: enough (row block, column chunk) items to fill the chip several times
// over, a chunk at least 16 tiles.  simt_split(.., 6144, 16, cap) starts from ceil(6144 / row_blocks) <= 6144 chunks and only
// lowers that, so the cap cannot bind; 6144 is passed to say so.
static dim3 rank_grid(AlignRankParams& p, int kpad) {
  const SimtSplit sp = simt_split(p.n1, p.n2, kpad, 6144, 16, 6144);
  p.tiles_per_chunk = sp.tiles_per_chunk;
  return dim3((unsigned)((p.n1 + SIMT_BM - 1) / SIMT_BM), (unsigned)sp.chunks);
}

}  // namespace mke

extern "C" int mke_align_rank(const float* emb1, int ld1, const float* emb2, int ld2, int kpad, int64_t n1, int64_t n2,
                              int32_t* rank, int32_t* ties, uint64_t* best, void* stream) {
  using namespace mke;
  const SweepOperands o = {"", true, n1, n2, kpad, ld1, ld2, MKE_METRIC_INNER, nullptr, nullptr, nullptr, nullptr};
  int rc = check_operands(o, {OP_ROWS});
  if (rc != MKE_OK) return rc;
  if (n1 == 0) return MKE_OK;
  if (!emb1 || !emb2 || !rank || !best) { set_error("mke_align_rank: NULL pointer"); return MKE_E_NULL; }
  rc = check_operands(o, {OP_KPAD, OP_LD});
  if (rc != MKE_OK) return rc;
  if (n2 < n1) { set_error("gold column = row index needs n2 >= n1"); return MKE_E_SHAPE; }
  rc = check_operands(o, {OP_WIDTH});
  if (rc != MKE_OK) return rc;
  AlignRankParams p = {};
  p.emb1 = emb1; p.ld1 = ld1; p.emb2 = emb2; p.ld2 = ld2; p.n1 = (int)n1; p.n2 = (int)n2; p.rank = rank; p.ties = ties;
  p.best = (unsigned long long*)best;
  const dim3 grid = rank_grid(p, kpad);
  hipStream_t st = (hipStream_t)stream;
  (void)simt_for_kpad(kpad, [&](auto ks) {  // true: OP_WIDTH has passed
    constexpr int KS = decltype(ks)::value;
    if (ties) hipLaunchKernelGGL((k_align_rank<KS, MKE_METRIC_INNER, false, true, false>), grid, dim3(MKE_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((k_align_rank<KS, MKE_METRIC_INNER, false, false, false>), grid, dim3(MKE_BLOCK), 0, st, p);
  });
  return check_launch("k_align_rank");
}

extern "C" int mke_align_rank_ex(const mke_align_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_align_rank_ex: NULL args"); return MKE_E_NULL; }
  const mke_align_args& g = *args;
  const SweepOperands o = {"mke_align_rank_ex: ", true, g.n1, g.n2, g.kpad, g.ld1, g.ld2, g.metric, g.sq1, g.sq2, g.csls_row, g.csls_col};
  int rc = check_operands(o, {OP_ROWS, OP_METRIC, OP_TERMS});
  if (rc != MKE_OK) return rc;
  if (g.n1 == 0) return MKE_OK;
  if (!g.emb1 || !g.emb2 || !g.rank || !g.ties || !g.best) { set_error("mke_align_rank_ex: NULL pointer"); return MKE_E_NULL; }
  rc = check_operands(o, {OP_NORMS, OP_KPAD, OP_LD});
  if (rc != MKE_OK) return rc;
  if (g.n2 < g.n1) { set_error("mke_align_rank_ex: gold column = row index needs n2 >= n1"); return MKE_E_SHAPE; }
  rc = check_operands(o, {OP_WIDTH});
  if (rc != MKE_OK) return rc;
  AlignRankParams p = {};
  p.emb1 = g.emb1; p.ld1 = g.ld1; p.emb2 = g.emb2; p.ld2 = g.ld2; p.n1 = (int)g.n1; p.n2 = (int)g.n2;
  p.sq1 = g.sq1; p.sq2 = g.sq2; p.csls_row = g.csls_row; p.csls_col = g.csls_col;
  p.rank = g.rank; p.ties = g.ties; p.best = (unsigned long long*)g.best;
  const dim3 grid = rank_grid(p, g.kpad);
  hipStream_t st = (hipStream_t)stream;
  (void)simt_for_kpad(g.kpad, [&](auto ks) {  // true: OP_WIDTH has passed
    for_rescore(g.metric == MKE_METRIC_EUCLIDEAN, g.csls_row != nullptr, [&](auto met, auto csls) {
      hipLaunchKernelGGL((k_align_rank<decltype(ks)::value, decltype(met)::value, decltype(csls)::value, true, true>), grid,
                         dim3(MKE_BLOCK), 0, st, p);
    });
  });
  return check_launch("k_align_rank_ex");
}
