// mke_stable.hip — stable (Gale-Shapley) alignment on the device (gfx950), without the n1 x n2 matrix.
//
// What it computes = code/base/alignment.py:82-128 (`stable_alignment`) with :131-138 (`arg_sort`) and :166-219
// (`galeshapley`): the suitor-optimal stable matching between the rows of E1 (suitors) and the rows of E2 (reviewers) under
// sim(E1, E2, metric, normalize, csls_k), every suitor's list truncated to its `cut` best columns, run to its fixed point.
// The reference builds the matrix, argsorts every row and every column, and walks string-keyed dicts; a suitor proposes at
// most once per round, so only its `cut` best columns matter, and a reviewer only ever compares two values of its own
// column, so no column is sorted at all.
//
// Candidate lists (mke_stable_lists), cut <= STABLE_FAST_CUT — the k-NN refresh's form (mke_knn.hip), with the evaluator's
// metric / CSLS epilogue (rescore<MET, CSLS> of mke_rescore.h, as k_align_rank):
//   tau             per row the m-th largest re-scored similarity to a strided sample of <= 4096 columns (mke_sim_sample on
//                   b with a row stride, k_stable_rescore, mke_topk_rows), m chosen so that about 2 cut + 32 columns pass.
//                   n_b <= STABLE_LIST_CAP: no sample, tau = -inf (every column is a candidate).
//   k_stable_select the sweep of mke_simtile.h; the epilogue appends (float_key(s) << 32 | 0xFFFFFFFF - column) of every
//                   s >= tau to the row's candidate list of this column segment: a ballot per accumulator register gives
//                   each hit its slot, no atomics.  8 segments x 128 slots per row.
//   k_stable_pick   one block per row: the candidates (<= 1024 packed keys) sorted descending in LDS (sort_desc) — value
//                   descending, then column ascending, in one compare — and the first `cut` written out.  A row with
//                   fewer than `cut` candidates under a threshold, or with an overflowed segment, is flagged; the caller
//                   redoes flagged rows through the whole-row path.
// cut > STABLE_FAST_CUT, flagged rows, or a similarity matrix given by the caller — rounds of whole rows (<= 2^26 floats):
//   mke_sim_sample -> k_stable_rescore (in place; NaN becomes the negative quiet NaN, which orders below -inf in the integer
//   image) -> mke_topk_long -> k_stable_gather (packed keys of the selected columns, sort_desc, NaN dropped).
//
// Deferred acceptance (mke_stable_rounds / mke_stable_finish): one thread per suitor and round; the only atomics are the
// 64-bit max on holder[column] and the round's proposal counter.  holder only grows, so the outcome does not depend on the
// order in which proposals land: it is the unique suitor-optimal matching of the (strict, tie-broken) preferences.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_stable_select<5, inner, no CSLS>    198 VGPRs, no spill, 43,008 B of LDS per block (the sweep's tiles only), 2 waves / SIMD
//   k_stable_select<5, euclidean, CSLS>   230 VGPRs, no spill, 43,008 B of LDS per block, 2 waves / SIMD
//   k_stable_select<13 .. 20, *>          256 VGPRs + 20 .. 126 AGPRs, no spill, 33,280 .. 54,272 B of LDS, 1 wave / SIMD
//   k_stable_pick                         28 VGPRs, 8,232 B of LDS per block;  k_stable_gather  17 VGPRs, 32,768 B of LDS
//   (k_topk_partial<5, inner>, the LDS form of profiles/r07_csls.md: 220 + 32 registers and 75,776 B at k = 10, values only.)
#include "mke_rescore.h"

namespace mke {

#define STABLE_FAST_CUT 128    // cut <= this: the sweep path
#define STABLE_SEGS 8          // column segments of a row's candidate list
#define STABLE_SEG_CAP 128     // slots per segment
#define STABLE_LIST_CAP (STABLE_SEGS * STABLE_SEG_CAP)
#define STABLE_MAX_SAMPLE 4096 // columns of the threshold sample (the list mke_topk_rows holds in LDS)
#define STABLE_SORT_LDS 4096   // k_stable_gather sorts up to this many keys in LDS, more in the caller's scratch
#define STABLE_ROUND_BYTES ((int64_t)1 << 28)  // candidate slots / sample values of one round of rows

// ------------------------------------------------------------------------------------------------ candidate sweep
struct StableSelectParams {
  const float* __restrict__ a;
  int lda;
  const float* __restrict__ b;
  int ldb;
  int n_b;
  int row_lo, row_hi;
  const float* __restrict__ sq_a;
  const float* __restrict__ sq_b;
  const float* __restrict__ csls_row;
  const float* __restrict__ csls_col;
  const float* __restrict__ tau;  // [n_a], or NULL: every column is a candidate
  int n_seg, tiles_per_seg;
  unsigned long long* __restrict__ cand;  // [rows][n_seg][STABLE_SEG_CAP]
  int32_t* __restrict__ seg_count;        // [rows][n_seg]
};

// KS <= 5 (dim <= 80): two blocks per CU.  Three, as k_sim_select is held to, spill here (8 VGPRs at KS 5 without metric or
// CSLS operands): the packed 64-bit key and the epilogue's operands cost the registers the third block would need.
template <int KS, int MET, bool CSLS>
__global__ __launch_bounds__(MKE_BLOCK, KS <= 5 ? 2 : 1) void k_stable_select(const StableSelectParams p) {
  constexpr bool EUC = MET == MKE_METRIC_EUCLIDEAN;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int strip0 = p.row_lo + blockIdx.x * SIMT_BM + wv * 32;
  float a[KS * 8];
  {
    const int r = strip0 + l31;
    const bool ok = r < p.row_hi;
    simt_load_fragment<KS>(p.a + (int64_t)(ok ? r : p.row_lo) * p.lda, ok, half, a);
  }
  float tauR[16], sqi[16], rti[16];
  int cnt[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = simt_row(reg, half, strip0);
    const bool ok = r < p.row_hi;
    tauR[reg] = ok ? (p.tau ? p.tau[r] : -INFINITY) : __builtin_nanf("");  // rows past the end take nothing (v >= NaN is false)
    sqi[reg] = (EUC && ok) ? p.sq_a[r] : 0.f;
    rti[reg] = (CSLS && ok) ? p.csls_row[r] : 0.f;
    cnt[reg] = 0;
  }
  const int seg = blockIdx.y;
  const int ntiles = (p.n_b + SIMT_BN_FOR(KS) - 1) / SIMT_BN_FOR(KS);
  const int t0 = seg * p.tiles_per_seg;
  const int t1 = min(ntiles, t0 + p.tiles_per_seg);
  const unsigned lt = (1u << l31) - 1u;
  // slot of (row of accumulator register reg, position) as a 32-bit BYTE offset from p.cand: a round holds at most
  // STABLE_ROUND_BYTES of slots (the launcher bounds its rows)
  const unsigned row_stride_b = (unsigned)(p.n_seg * STABLE_SEG_CAP) * 8u;
  const unsigned base0_b = (unsigned)(((strip0 - p.row_lo + 4 * half) * p.n_seg + seg) * STABLE_SEG_CAP) * 8u;
  char* const cand_b = reinterpret_cast<char*>(p.cand);
  simt_sweep<KS>(a, p.b, p.ldb, p.n_b, t0, t1, [&](const f32x16& acc, int col, bool col_ok) {
    const float sqj = (EUC && col_ok) ? p.sq_b[col] : 0.f;
    const float rsj = (CSLS && col_ok) ? p.csls_col[col] : 0.f;
    const unsigned low = 0xFFFFFFFFu - (unsigned)col;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float v = rescore<MET, CSLS>(acc[reg], sqi[reg], sqj, rti[reg], rsj);
      const bool hit = col_ok && v >= tauR[reg];  // false for NaN and for the padding columns of the last tile
      const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
      if (m == 0) continue;  // wave-uniform
      const unsigned mh = half ? (unsigned)(m >> 32) : (unsigned)m;  // the 32 lanes of a half hold 32 columns of ONE row
      const int pos = cnt[reg] + __popc(mh & lt);
      if (hit && pos < STABLE_SEG_CAP) {
        const unsigned long long key = ((unsigned long long)float_key(v) << 32) | (unsigned long long)low;
        *reinterpret_cast<unsigned long long*>(cand_b + (base0_b + (unsigned)simt_row(reg, 0) * row_stride_b + (unsigned)pos * 8u)) = key;
      }
      cnt[reg] += __popc(mh);
    }
  });
  if (l31 == 0) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = simt_row(reg, half, strip0);
      if (r < p.row_hi) p.seg_count[(int64_t)(r - p.row_lo) * p.n_seg + seg] = cnt[reg];
    }
  }
}

__device__ __forceinline__ void write_entry(unsigned long long key, float* val, int32_t* col) {
  if (key == 0ull) { *val = -INFINITY; *col = -1; return; }  // padding (no real key is 0: float_key(s) of a non-NaN s is not)
  *val = key_float((unsigned)(key >> 32));
  *col = (int32_t)(0xFFFFFFFFu - (unsigned)key);
}

struct StablePickParams {
  const unsigned long long* __restrict__ cand;  // [rows][n_seg][STABLE_SEG_CAP]
  const int32_t* __restrict__ seg_count;        // [rows][n_seg]
  int n_seg, cut, thresholded;
  float* __restrict__ out_val;   // [rows][cut] (offset to the round's first row, as flags)
  int32_t* __restrict__ out_col;
  int32_t* __restrict__ flags;
};

__global__ __launch_bounds__(MKE_BLOCK) void k_stable_pick(const StablePickParams p) {
  __shared__ unsigned long long s_key[STABLE_LIST_CAP];
  __shared__ int s_off[STABLE_SEGS + 1];
  __shared__ int s_bad;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int tot = 0, bad = 0;
    for (int s = 0; s < p.n_seg; ++s) {
      int c = p.seg_count[row * p.n_seg + s];
      if (c > STABLE_SEG_CAP) { bad = 1; c = STABLE_SEG_CAP; }
      s_off[s] = tot;
      tot += c;
    }
    s_off[p.n_seg] = tot;
    if (p.thresholded && tot < p.cut) bad = 1;  // the estimate was too tight; without a threshold the list is just short (NaN)
    s_bad = bad;
  }
  __syncthreads();
  float* ov = p.out_val + row * p.cut;
  int32_t* oc = p.out_col + row * p.cut;
  if (s_bad) {  // block-uniform
    for (int j = tid; j < p.cut; j += MKE_BLOCK) { ov[j] = -INFINITY; oc[j] = -1; }
    if (tid == 0) p.flags[row] = 1;
    return;
  }
  const int total = s_off[p.n_seg];
  int np2 = 1;
  while (np2 < total) np2 <<= 1;
  for (int s = 0; s < p.n_seg; ++s) {
    const int n = s_off[s + 1] - s_off[s];
    const unsigned long long* src = p.cand + (row * p.n_seg + s) * (int64_t)STABLE_SEG_CAP;
    for (int i = tid; i < n; i += MKE_BLOCK) s_key[s_off[s] + i] = src[i];
  }
  for (int i = total + tid; i < np2; i += MKE_BLOCK) s_key[i] = 0ull;
  __syncthreads();
  sort_desc(s_key, np2);
  for (int j = tid; j < p.cut; j += MKE_BLOCK) write_entry(j < total ? s_key[j] : 0ull, ov + j, oc + j);
  if (tid == 0) p.flags[row] = 0;
}

// ------------------------------------------------------------------------------------------------ whole rows
struct StableRescoreParams {
  const float* __restrict__ src;  // [rows][ld_src]: dot products (or the caller's similarities)
  int64_t ld_src;
  float* __restrict__ dst;        // [rows][ld_dst]; src == dst: in place
  int64_t ld_dst;
  int m;                          // values per row
  int col_step;                   // value j belongs to column j * col_step
  int metric;                     // MKE_METRIC_*, or -1: the values are final similarities
  const float* __restrict__ sq_a;      // offset to the launch's first row, as csls_row
  const float* __restrict__ sq_b;
  const float* __restrict__ csls_row;  // NULL: no CSLS
  const float* __restrict__ csls_col;
};

__global__ __launch_bounds__(MKE_BLOCK) void k_stable_rescore(const StableRescoreParams p) {
  const int64_t row = blockIdx.x;
  const float* __restrict__ s = p.src + row * p.ld_src;
  float* __restrict__ d = p.dst + row * p.ld_dst;
  const bool euc = p.metric == MKE_METRIC_EUCLIDEAN, csls = p.csls_row != nullptr;
  const float sqi = euc ? p.sq_a[row] : 0.f;
  const float rti = csls ? p.csls_row[row] : 0.f;
  for (int j = blockIdx.y * MKE_BLOCK + threadIdx.x; j < p.m; j += gridDim.y * MKE_BLOCK) {
    const int64_t col = (int64_t)j * p.col_step;
    float v = s[j];
    if (euc && csls) v = rescore<MKE_METRIC_EUCLIDEAN, true>(v, sqi, p.sq_b[col], rti, p.csls_col[col]);
    else if (euc) v = rescore<MKE_METRIC_EUCLIDEAN, false>(v, sqi, p.sq_b[col], 0.f, 0.f);
    else if (csls) v = rescore<MKE_METRIC_INNER, true>(v, 0.f, 0.f, rti, p.csls_col[col]);
    if (v != v) v = __uint_as_float(0xFFC00000u);  // orders below -inf in float_key: selected last, dropped by the gather
    d[j] = v;
  }
}

struct StableGatherParams {
  const float* __restrict__ vals;  // [rows][ld] re-scored similarity rows
  int64_t ld;
  const int32_t* __restrict__ sel;  // [rows][cut] selected columns (mke_topk_long)
  int cut, np2;
  unsigned long long* __restrict__ sort_tmp;  // [rows][np2] when np2 > STABLE_SORT_LDS
  float* __restrict__ out_val;
  int32_t* __restrict__ out_col;
  int32_t* __restrict__ flags;
};

__global__ __launch_bounds__(MKE_BLOCK) void k_stable_gather(const StableGatherParams p) {
  __shared__ unsigned long long s_sort[STABLE_SORT_LDS];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  unsigned long long* buf = p.np2 <= STABLE_SORT_LDS ? s_sort : p.sort_tmp + row * p.np2;
  const float* __restrict__ v = p.vals + row * p.ld;
  const int32_t* __restrict__ sel = p.sel + row * p.cut;
  for (int j = tid; j < p.np2; j += MKE_BLOCK) {
    unsigned long long key = 0ull;
    if (j < p.cut) {
      const int c = sel[j];
      const float x = v[c];
      if (x == x) key = ((unsigned long long)float_key(x) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
    }
    buf[j] = key;
  }
  __syncthreads();
  sort_desc(buf, p.np2);
  for (int j = tid; j < p.cut; j += MKE_BLOCK) write_entry(buf[j], p.out_val + row * p.cut + j, p.out_col + row * p.cut + j);
  if (tid == 0) p.flags[row] = 0;
}

// ------------------------------------------------------------------------------------------------ deferred acceptance
struct StableMatchParams {
  int n_a, n_b, cut;
  const float* __restrict__ val;
  const int32_t* __restrict__ col;
  int32_t* __restrict__ ptr;
  unsigned long long* holder;
  int32_t* proposals;
  int32_t* __restrict__ match;
  int32_t* __restrict__ counts;
};

__device__ __forceinline__ bool stable_held(const StableMatchParams& p, int c, int i) {
  const unsigned long long h = __hip_atomic_load(&p.holder[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (unsigned)h == 0xFFFFFFFFu - (unsigned)i;  // a free column holds 0: its low word names no row (rows < 2^31)
}

__global__ __launch_bounds__(MKE_BLOCK) void k_stable_round(const StableMatchParams p, int64_t round) {
  if (round > 0 && p.proposals[round - 1] == 0) return;  // the fixed point was reached: nothing can change any more
  const int i = blockIdx.x * MKE_BLOCK + threadIdx.x;
  bool propose = false;
  int c = -1, pos = 0;
  if (i < p.n_a) {
    pos = p.ptr[i];
    if (pos < p.cut) {
      const int32_t* __restrict__ L = p.col + (int64_t)i * p.cut;
      c = L[pos];
      bool valid = c >= 0 && c < p.n_b;
      if (valid && round > 0) {  // it proposed at pos in an earlier round: held, or overtaken since
        if (stable_held(p, c, i)) {
          valid = false;         // nothing to do (pos stays)
        } else {
          ++pos;
          c = pos < p.cut ? L[pos] : -1;
          valid = c >= 0 && c < p.n_b;
          if (!valid) pos = p.cut;
          p.ptr[i] = pos;
        }
        propose = valid;
      } else if (valid) {
        propose = true;          // round 0: everybody proposes to the head of its list
      } else {
        p.ptr[i] = p.cut;        // an empty list
      }
    }
  }
  if (propose) {
    const unsigned long long key = ((unsigned long long)float_key(p.val[(int64_t)i * p.cut + pos]) << 32) |
                                   (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    atomicMax(&p.holder[c], key);
  }
  const uint64_t m = __builtin_amdgcn_ballot_w64(propose);
  if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(&p.proposals[round], (int)__popcll(m));
}

__global__ __launch_bounds__(MKE_BLOCK) void k_stable_finish(const StableMatchParams p) {
  __shared__ int s_m[MKE_BLOCK / 64], s_g[MKE_BLOCK / 64];
  int matched = 0, gold = 0;
  for (int i = threadIdx.x; i < p.n_a; i += MKE_BLOCK) {
    const int pos = p.ptr[i];
    int m = -1;
    if (pos < p.cut) {
      const int c = p.col[(int64_t)i * p.cut + pos];
      if (c >= 0 && c < p.n_b && stable_held(p, c, i)) m = c;
    }
    p.match[i] = m;
    matched += m >= 0 ? 1 : 0;
    gold += m == i ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    matched += __shfl_xor(matched, off, 64);
    gold += __shfl_xor(gold, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = matched; s_g[threadIdx.x >> 6] = gold; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.counts[0] = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    p.counts[1] = s_g[0] + s_g[1] + s_g[2] + s_g[3];
  }
}

struct StablePlan {
  bool whole;
  int64_t rows;        // rows per round
  int64_t samp_rows;   // rows per threshold round (sweep path)
  int64_t off_tau, off_work, off_cnt, off_sel, off_sort;
  int64_t bytes;
};

static int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

}  // namespace mke

static int stable_plan(const mke::SweepOperands& o, int cut, bool whole, bool need_kpad, mke::StablePlan* pl) {
  using namespace mke;
  pl->bytes = 0;
  pl->whole = whole || cut > STABLE_FAST_CUT;
  const int64_t n_a = o.n_a, n_b = o.n_b;
  int rc = check_operands(o, {OP_ROWS});
  if (rc == MKE_OK && need_kpad) rc = check_operands(o, {OP_KPAD});
  if (rc != MKE_OK) return rc;
  if (cut < 1 || (int64_t)cut > n_b) { set_error("%sneed 1 <= cut <= n_b (cut = %d, n_b = %lld)", o.who, cut, (long long)n_b); return MKE_E_SHAPE; }
  if (cut > (1 << 30)) { set_error("%scut above 2^30 (the sort counts with 32-bit ints)", o.who); return MKE_E_RANGE; }
  if (n_a == 0) return MKE_OK;
  if (pl->whole) {
    pl->rows = fallback_rows(n_a, n_b);
    const int64_t np2 = pow2_at_least(cut);
    pl->off_work = 0;                                              // similarity rows [rows][n_b]
    pl->off_sel = up256(pl->rows * n_b * 4);                       // selected columns [rows][cut]
    pl->off_sort = pl->off_sel + up256(pl->rows * (int64_t)cut * 4);
    pl->bytes = pl->off_sort + (np2 > STABLE_SORT_LDS ? pl->rows * np2 * 8 : 0);
    if (pl->bytes > ((int64_t)1 << 42)) { set_error("%sscratch beyond 2^42 bytes", o.who); return MKE_E_RANGE; }
    return MKE_OK;
  }
  const int64_t per_row = (int64_t)STABLE_LIST_CAP * 8;
  pl->rows = STABLE_ROUND_BYTES / per_row / SIMT_BM * SIMT_BM - SIMT_BM;  // + one strip block of slack: 32-bit byte offsets
  if (pl->rows > n_a) pl->rows = n_a;
  pl->samp_rows = STABLE_ROUND_BYTES / (STABLE_MAX_SAMPLE * 4);
  if (pl->samp_rows > n_a) pl->samp_rows = n_a;
  pl->off_tau = 0;
  pl->off_cnt = up256(n_a * 4);
  pl->off_work = pl->off_cnt + up256(pl->rows * STABLE_SEGS * 4);
  const int64_t sel_b = pl->rows * per_row, samp_b = pl->samp_rows * STABLE_MAX_SAMPLE * 4;
  pl->bytes = pl->off_work + (sel_b > samp_b ? sel_b : samp_b);
  return MKE_OK;
}

extern "C" int64_t mke_stable_lists_temp_bytes(int64_t n_a, int64_t n_b, int kpad, int cut, int whole_rows) {
  mke::StablePlan pl;
  const int rc = stable_plan({"mke_stable_lists_temp_bytes: ", false, n_a, n_b, kpad}, cut, whole_rows != 0, true, &pl);
  return rc != MKE_OK ? rc : pl.bytes;
}

extern "C" int mke_stable_lists(const mke_stable_lists_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_stable_lists: NULL args"); return MKE_E_NULL; }
  const mke_stable_lists_args& g = *args;
  const bool given = g.sim_mat != nullptr;
  const SweepOperands o = {"mke_stable_lists: ", false, g.n_a, g.n_b, g.kpad, g.lda, g.ldb, g.metric, g.sq_a, g.sq_b, g.csls_row, g.csls_col};
  StablePlan pl;
  int rc = stable_plan(o, g.cut, g.whole_rows != 0 || given, !given, &pl);
  if (rc == MKE_OK && !given) rc = check_operands(o, {OP_METRIC, OP_TERMS});
  if (rc != MKE_OK) return rc;
  if (g.sample_cols < 0) { set_error("mke_stable_lists: sample_cols < 0"); return MKE_E_SHAPE; }
  if (g.n_a == 0) return MKE_OK;
  if (!g.out_val || !g.out_col || !g.flags || !g.temp) { set_error("mke_stable_lists: NULL pointer"); return MKE_E_NULL; }
  if (given) {
    if (g.ld_sim < g.n_b) { set_error("mke_stable_lists: ld_sim below n_b"); return MKE_E_SHAPE; }
  } else {
    if (!g.a || !g.b) { set_error("mke_stable_lists: NULL pointer"); return MKE_E_NULL; }
    rc = check_operands(o, {OP_NORMS, OP_LD, OP_WIDTH});
    if (rc != MKE_OK) return rc;
  }
  if (g.temp_bytes < pl.bytes) { set_error("mke_stable_lists: temp below mke_stable_lists_temp_bytes (%lld)", (long long)pl.bytes); return MKE_E_SHAPE; }
  hipStream_t st = (hipStream_t)stream;
  char* const temp = (char*)g.temp;
  const bool euc = !given && g.metric == MKE_METRIC_EUCLIDEAN, csls = !given && g.csls_row != nullptr;

  if (pl.whole) {
    float* simrows = (float*)(temp + pl.off_work);
    int32_t* sel = (int32_t*)(temp + pl.off_sel);
    StableGatherParams gp;
    gp.vals = simrows; gp.ld = g.n_b; gp.sel = sel; gp.cut = g.cut; gp.np2 = (int)pow2_at_least(g.cut);
    gp.sort_tmp = (unsigned long long*)(temp + pl.off_sort);
    for (int64_t lo = 0; lo < g.n_a; lo += pl.rows) {
      const int64_t hi = lo + pl.rows < g.n_a ? lo + pl.rows : g.n_a;
      StableRescoreParams rp;
      rp.dst = simrows; rp.ld_dst = g.n_b; rp.m = (int)g.n_b; rp.col_step = 1; rp.sq_b = g.sq_b; rp.csls_col = g.csls_col;
      if (given) {
        rp.src = g.sim_mat + lo * g.ld_sim; rp.ld_src = g.ld_sim; rp.metric = -1;
        rp.sq_a = nullptr; rp.csls_row = nullptr; rp.sq_b = nullptr; rp.csls_col = nullptr;
      } else {
        int e = mke_sim_sample(g.a, g.lda, g.kpad, g.n_a, lo, hi, g.b, g.ldb, (int)g.n_b, simrows, stream);
        if (e) return e;
        rp.src = simrows; rp.ld_src = g.n_b; rp.metric = g.metric;
        rp.sq_a = euc ? g.sq_a + lo : nullptr; rp.csls_row = csls ? g.csls_row + lo : nullptr;
      }
      const unsigned gy = (unsigned)((g.n_b + 16 * MKE_BLOCK - 1) / (16 * MKE_BLOCK));
      hipLaunchKernelGGL(k_stable_rescore, dim3((unsigned)(hi - lo), gy < 64 ? gy : 64), dim3(MKE_BLOCK), 0, st, rp);
      int e = check_launch("k_stable_rescore");
      if (e) return e;
      e = mke_topk_long(simrows, hi - lo, g.n_b, g.n_b, g.cut, nullptr, sel, stream);
      if (e) return e;
      gp.out_val = g.out_val + lo * g.cut; gp.out_col = g.out_col + lo * g.cut; gp.flags = g.flags + lo;
      hipLaunchKernelGGL(k_stable_gather, dim3((unsigned)(hi - lo)), dim3(MKE_BLOCK), 0, st, gp);
      e = check_launch("k_stable_gather");
      if (e) return e;
    }
    return MKE_OK;
  }

  // sweep path: thresholds from a strided column sample, one sweep per round of rows, exact selection
  float* tau = (float*)(temp + pl.off_tau);
  const bool thresholded = g.sample_cols > 0 || g.n_b > STABLE_LIST_CAP;
  if (thresholded) {
    int64_t step = (g.n_b + STABLE_MAX_SAMPLE - 1) / STABLE_MAX_SAMPLE;
    if (g.sample_cols > 0 && g.n_b / g.sample_cols > step) step = g.n_b / g.sample_cols;
    const int n_samp = (int)((g.n_b + step - 1) / step);  // <= STABLE_MAX_SAMPLE; column j * step < n_b
    int64_t m = ((int64_t)n_samp * (2 * (int64_t)g.cut + 32) + g.n_b / 2) / g.n_b;
    if (m < 1) m = 1;
    if (m > n_samp) m = n_samp;
    float* samp = (float*)(temp + pl.off_work);
    for (int64_t lo = 0; lo < g.n_a; lo += pl.samp_rows) {
      const int64_t hi = lo + pl.samp_rows < g.n_a ? lo + pl.samp_rows : g.n_a;
      int e = mke_sim_sample(g.a, g.lda, g.kpad, g.n_a, lo, hi, g.b, (int)(step * g.ldb), n_samp, samp, stream);
      if (e) return e;
      StableRescoreParams rp;
      rp.src = samp; rp.ld_src = n_samp; rp.dst = samp; rp.ld_dst = n_samp; rp.m = n_samp; rp.col_step = (int)step; rp.metric = g.metric;
      rp.sq_a = euc ? g.sq_a + lo : nullptr; rp.sq_b = g.sq_b; rp.csls_row = csls ? g.csls_row + lo : nullptr; rp.csls_col = g.csls_col;
      hipLaunchKernelGGL(k_stable_rescore, dim3((unsigned)(hi - lo), 1), dim3(MKE_BLOCK), 0, st, rp);
      e = check_launch("k_stable_rescore");
      if (e) return e;
      e = mke_topk_rows(samp, nullptr, nullptr, hi - lo, 1, n_samp, (int)m, nullptr, nullptr, tau + lo, nullptr, stream);
      if (e) return e;
    }
  }
  StableSelectParams sp;
  sp.a = g.a; sp.lda = g.lda; sp.b = g.b; sp.ldb = g.ldb; sp.n_b = (int)g.n_b; sp.sq_a = g.sq_a; sp.sq_b = g.sq_b;
  sp.csls_row = g.csls_row; sp.csls_col = g.csls_col; sp.tau = thresholded ? tau : nullptr;
  const SimtSplit segs = simt_split_fixed(g.n_b, g.kpad, STABLE_SEGS);
  sp.tiles_per_seg = segs.tiles_per_chunk;
  sp.n_seg = segs.chunks;  // no empty segment
  sp.cand = (unsigned long long*)(temp + pl.off_work);
  sp.seg_count = (int32_t*)(temp + pl.off_cnt);
  StablePickParams pp;
  pp.cand = sp.cand; pp.seg_count = sp.seg_count; pp.n_seg = sp.n_seg; pp.cut = g.cut; pp.thresholded = thresholded ? 1 : 0;
  for (int64_t lo = 0; lo < g.n_a; lo += pl.rows) {
    const int64_t hi = lo + pl.rows < g.n_a ? lo + pl.rows : g.n_a;
    sp.row_lo = (int)lo; sp.row_hi = (int)hi;
    dim3 grid((unsigned)((hi - lo + SIMT_BM - 1) / SIMT_BM), (unsigned)sp.n_seg);
    simt_for_kpad(g.kpad, [&](auto ks) {
      for_rescore(euc, csls, [&](auto met, auto cs) {
        hipLaunchKernelGGL((k_stable_select<decltype(ks)::value, decltype(met)::value, decltype(cs)::value>), grid, dim3(MKE_BLOCK), 0,
                           st, sp);
      });
    });
    int e = check_launch("k_stable_select");
    if (e) return e;
    pp.out_val = g.out_val + lo * g.cut; pp.out_col = g.out_col + lo * g.cut; pp.flags = g.flags + lo;
    hipLaunchKernelGGL(k_stable_pick, dim3((unsigned)(hi - lo)), dim3(MKE_BLOCK), 0, st, pp);
    e = check_launch("k_stable_pick");
    if (e) return e;
  }
  return MKE_OK;
}

static int stable_match_params(const char* who, const mke_stable_match_args* args, bool finish, mke::StableMatchParams* p) {
  using namespace mke;
  if (!args) { set_error("%s: NULL args", who); return MKE_E_NULL; }
  const mke_stable_match_args& g = *args;
  if (g.n_a < 0 || g.n_b < 0 || g.n_a > 0x7FFFFF00LL || g.n_b > 0x7FFFFF00LL) { set_error("%s: bad n_a / n_b", who); return MKE_E_SHAPE; }
  if (g.cut < 1) { set_error("%s: cut < 1", who); return MKE_E_SHAPE; }
  if (g.n_a > 0 && (!g.val || !g.col || !g.ptr || (g.n_b > 0 && !g.holder))) { set_error("%s: NULL pointer", who); return MKE_E_NULL; }
  if (finish ? (!g.counts || (g.n_a > 0 && !g.match)) : !g.proposals) { set_error("%s: NULL pointer", who); return MKE_E_NULL; }
  p->n_a = (int)g.n_a; p->n_b = (int)g.n_b; p->cut = g.cut; p->val = g.val; p->col = g.col; p->ptr = g.ptr;
  p->holder = (unsigned long long*)g.holder; p->proposals = g.proposals; p->match = g.match; p->counts = g.counts;
  return MKE_OK;
}

extern "C" int mke_stable_rounds(const mke_stable_match_args* args, int64_t first_round, int n_rounds, void* stream) {
  using namespace mke;
  StableMatchParams p;
  const int rc = stable_match_params("mke_stable_rounds", args, false, &p);
  if (rc != MKE_OK) return rc;
  if (first_round < 0 || n_rounds < 0) { set_error("mke_stable_rounds: negative round"); return MKE_E_SHAPE; }
  if (first_round + n_rounds > args->n_proposals) { set_error("mke_stable_rounds: rounds beyond proposals[%lld]", (long long)args->n_proposals); return MKE_E_RANGE; }
  if (p.n_a == 0) return MKE_OK;
  const unsigned blocks = (unsigned)((p.n_a + MKE_BLOCK - 1) / MKE_BLOCK);
  for (int r = 0; r < n_rounds; ++r) {
    hipLaunchKernelGGL(k_stable_round, dim3(blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p, first_round + r);
    const int e = check_launch("k_stable_round");
    if (e) return e;
  }
  return MKE_OK;
}

extern "C" int mke_stable_finish(const mke_stable_match_args* args, void* stream) {
  using namespace mke;
  StableMatchParams p;
  const int rc = stable_match_params("mke_stable_finish", args, true, &p);
  if (rc != MKE_OK) return rc;
  hipLaunchKernelGGL(k_stable_finish, dim3(1), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p);
  return check_launch("k_stable_finish");
}
