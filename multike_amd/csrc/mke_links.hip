// mke_links.hip — libmultike_links.so (include/multike_links.h): the link set of self-training, edited from refresh to refresh.
// A library of its own: libmultike_hip.so, libmultike_thin.so, libmultike_keyed.so and their C-ABIs stay as they are; this file
// shares only device helpers (mke_common.h, mke_rescore.h, mke_simtile.h) with them and keeps its own error message.
//
//   k_links_scatter  inv[match[r]] = r for every row with a valid match, over an inv the call has set to -1 (the match is
//                    one-to-one: no two rows write one word).
//   k_links_edit     the row layout of mke_rows.hip: a 16-lane quarter-wavefront owns a row, lane l holds columns
//                    l, l + 16, ..., four DPP adds reduce the row.  A row that has a new pair, that is displaced or that holds
//                    nothing is decided from match / held / inv alone and reads no embedding row; only an undisplaced old link
//                    loads its two rows and forms the value the sweep compares (rescore<> of mke_rescore.h).  The seven counters:
//                    one ballot and popcount per wavefront, counter and pass of the capped grid, summed in registers, then
//                    one integer atomic per wavefront and counter.
#include <cstdarg>
#include <cstdio>

#include "../../include/multike_links.h"
#include "mke_rescore.h"

static_assert(MKE_LINKS_METRIC_INNER == MKE_METRIC_INNER && MKE_LINKS_METRIC_EUCLIDEAN == MKE_METRIC_EUCLIDEAN, "metric codes of multike_hip.h");
static_assert(MKE_LINKS_E_NULL == MKE_E_NULL && MKE_LINKS_E_SHAPE == MKE_E_SHAPE && MKE_LINKS_E_UNSUPPORTED == MKE_E_UNSUPPORTED &&
              MKE_LINKS_E_RANGE == MKE_E_RANGE, "error codes of multike_hip.h");

namespace {
thread_local char g_links_err[256] = "";
void links_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_links_err, sizeof(g_links_err), fmt, ap);
  va_end(ap);
}
}  // namespace

namespace mke {

struct LinksParams {
  const int32_t* __restrict__ held;
  const int32_t* __restrict__ match;
  int n_a, n_b;
  const float* __restrict__ a;
  const float* __restrict__ b;
  int lda, ldb;
  const float* __restrict__ sq_a;
  const float* __restrict__ sq_b;
  const float* __restrict__ term_row;
  const float* __restrict__ term_col;
  float retain;
  const float* __restrict__ new_score;
  int32_t* __restrict__ inv;
  int32_t* __restrict__ out;
  float* __restrict__ score;
  int32_t* __restrict__ counts;
};

// an entry outside [0, n_b) counts as -1
__device__ __forceinline__ int links_column(int j, int n_b) { return (unsigned)j < (unsigned)n_b ? j : -1; }

__global__ __launch_bounds__(MKE_BLOCK) void k_links_scatter(const LinksParams p) {
  const int64_t r = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (r >= p.n_a) return;
  const int j = links_column(p.match[r], p.n_b);
  if (j >= 0) p.inv[j] = (int32_t)r;
}

// Workgroups of a launch at most, 16 rows a pass each.  A wavefront keeps its seven counts in registers over its passes and adds
// them once: at most 4 * LINKS_MAX_BLOCKS adds a counter word, whatever n_a (with a workgroup per 16 rows the adds to those
// seven words, one per 4 rows, were what the launch waited for: profiles/r27_links.md)
#define LINKS_MAX_BLOCKS 512

template <int FPL, int MET, bool CSLS>
__global__ __launch_bounds__(MKE_BLOCK) void k_links_edit(const LinksParams p) {
  const int l = threadIdx.x & 15;
  int total[MKE_LINKS_COUNTS] = {0, 0, 0, 0, 0, 0, 0};  // wave-uniform
  // every lane of a workgroup makes the same number of passes: the DPP adds and the ballots below see whole wavefronts
  for (int64_t base = (int64_t)blockIdx.x * MKE_SUBS_PER_BLOCK; base < p.n_a; base += (int64_t)gridDim.x * MKE_SUBS_PER_BLOCK) {
    const int64_t i = base + (threadIdx.x >> 4);
    const bool row = i < p.n_a;
    // the 16 lanes of a row load the same two words
    const int m = row ? links_column(p.match[i], p.n_b) : -1;
    const int h = row ? links_column(p.held[i], p.n_b) : -1;
    const bool is_new = m >= 0;
    bool displaced = is_new && h >= 0 && h != m;
    bool old = false;  // an old link whose value decides
    if (!is_new && h >= 0) {
      displaced = p.inv[h] >= 0;
      old = !displaced;
    }
    // uniform over a quarter-wavefront: a DPP add below never reads a lane outside the 16 of its row
    float acc = 0.f;
    if (old) {
      float x[FPL], y[FPL];
      load_row<FPL>(p.a, i, p.lda, l, x);
      load_row<FPL>(p.b, h, p.ldb, l, y);
#pragma unroll
      for (int k = 0; k < FPL; ++k) acc = fmaf(x[k], y[k], acc);
    }
    const float dot = sub16_sum(acc);
    bool kept = false;
    float s = 0.f;
    if (old) {
      s = rescore<MET, CSLS>(dot, MET == MKE_METRIC_EUCLIDEAN ? p.sq_a[i] : 0.f, MET == MKE_METRIC_EUCLIDEAN ? p.sq_b[h] : 0.f,
                             CSLS ? p.term_row[i] : 0.f, CSLS ? p.term_col[h] : 0.f);
      kept = s >= p.retain;  // false for a NaN
    }
    const int o = is_new ? m : (kept ? h : -1);
    const bool lead = row && l == 0;
    if (lead) {
      p.out[i] = o;
      if (p.score) p.score[i] = is_new ? (p.new_score ? p.new_score[i] : 0.f) : (kept ? s : 0.f);
    }
    // one lane a row votes
    const bool flag[MKE_LINKS_COUNTS] = {o >= 0, o >= 0 && (int64_t)o == i, is_new, is_new && m == h, kept, displaced, old && !kept};
#pragma unroll
    for (int c = 0; c < MKE_LINKS_COUNTS; ++c) total[c] += __popcll(__builtin_amdgcn_ballot_w64(lead && flag[c]));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < MKE_LINKS_COUNTS; ++c)
      if (total[c]) atomicAdd(&p.counts[c], total[c]);
  }
}

}  // namespace mke

extern "C" const char* mke_links_last_error(void) { return g_links_err; }

extern "C" int mke_links_version(void) { return MKE_LINKS_VERSION; }

extern "C" int mke_links_edit(const mke_links_args* args, void* stream) {
  using namespace mke;
  if (!args) { links_error("mke_links_edit: NULL args"); return MKE_LINKS_E_NULL; }
  const mke_links_args& g = *args;
  if (g.n_a < 0 || g.n_b < 0 || g.n_a > 0x7FFFFF00LL || g.n_b > 0x7FFFFF00LL) { links_error("mke_links_edit: bad n_a / n_b"); return MKE_LINKS_E_SHAPE; }
  if (g.metric != MKE_LINKS_METRIC_INNER && g.metric != MKE_LINKS_METRIC_EUCLIDEAN) { links_error("mke_links_edit: unknown metric %d", g.metric); return MKE_LINKS_E_UNSUPPORTED; }
  if (g.retain != g.retain) { links_error("mke_links_edit: retain is NaN (-INFINITY = keep every undisplaced link)"); return MKE_LINKS_E_RANGE; }
  if ((g.csls_row == nullptr) != (g.csls_col == nullptr)) { links_error("mke_links_edit: csls_row and csls_col are both NULL or both set"); return MKE_LINKS_E_NULL; }
  if (!g.counts) { links_error("mke_links_edit: NULL pointer"); return MKE_LINKS_E_NULL; }
  hipStream_t st = (hipStream_t)stream;
  const bool empty = g.n_a == 0 || g.n_b == 0;
  if (!empty) {
    if (!g.held || !g.match || !g.a || !g.b || !g.inv || !g.out) { links_error("mke_links_edit: NULL pointer"); return MKE_LINKS_E_NULL; }
    if (g.kpad <= 0 || g.kpad % 16 != 0 || g.kpad > MKE_MAX_STRIDE) { links_error("mke_links_edit: kpad must be a multiple of 16 <= %d", MKE_MAX_STRIDE); return MKE_LINKS_E_SHAPE; }
    if (g.lda < g.kpad || g.ldb < g.kpad || g.lda % 4 != 0 || g.ldb % 4 != 0) { links_error("mke_links_edit: lda, ldb must be multiples of 4 >= kpad"); return MKE_LINKS_E_SHAPE; }
    if (!simt_kpad_ok(g.kpad)) { links_error("mke_links_edit: unsupported kpad %d", g.kpad); return MKE_LINKS_E_UNSUPPORTED; }
    if (g.metric == MKE_LINKS_METRIC_EUCLIDEAN && (!g.sq_a || !g.sq_b)) { links_error("mke_links_edit: euclidean needs sq_a and sq_b"); return MKE_LINKS_E_NULL; }
    if (g.out < g.held + g.n_a && g.held < g.out + g.n_a) { links_error("mke_links_edit: out overlaps held (the edit writes a separate array)"); return MKE_LINKS_E_UNSUPPORTED; }
  }
  hipError_t e = hipMemsetAsync(g.counts, 0, MKE_LINKS_COUNTS * sizeof(int32_t), st);
  if (e == hipSuccess && !empty) e = hipMemsetAsync(g.inv, 0xFF, (size_t)g.n_b * sizeof(int32_t), st);  // every word -1
  if (e != hipSuccess) { links_error("mke_links_edit: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  if (empty) return MKE_LINKS_OK;
  LinksParams p;
  p.held = g.held; p.match = g.match; p.n_a = (int)g.n_a; p.n_b = (int)g.n_b; p.a = g.a; p.b = g.b; p.lda = g.lda; p.ldb = g.ldb;
  p.sq_a = g.sq_a; p.sq_b = g.sq_b; p.term_row = g.csls_row; p.term_col = g.csls_col; p.retain = g.retain; p.new_score = g.new_score;
  p.inv = g.inv; p.out = g.out; p.score = g.score; p.counts = g.counts;
  hipLaunchKernelGGL(k_links_scatter, dim3((unsigned)((g.n_a + MKE_BLOCK - 1) / MKE_BLOCK)), dim3(MKE_BLOCK), 0, st, p);
  e = hipGetLastError();
  if (e != hipSuccess) { links_error("k_links_scatter: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  const int64_t blocks = (g.n_a + MKE_SUBS_PER_BLOCK - 1) / MKE_SUBS_PER_BLOCK;
  const dim3 grid((unsigned)(blocks < LINKS_MAX_BLOCKS ? blocks : LINKS_MAX_BLOCKS));
  (void)simt_for_kpad(g.kpad, [&](auto ks) {  // true: simt_kpad_ok has passed
    for_rescore(g.metric == MKE_LINKS_METRIC_EUCLIDEAN, g.csls_row != nullptr, [&](auto met, auto csls) {
      hipLaunchKernelGGL((k_links_edit<decltype(ks)::value, decltype(met)::value, decltype(csls)::value>), grid, dim3(MKE_BLOCK), 0, st, p);
    });
  });
  e = hipGetLastError();
  if (e != hipSuccess) { links_error("k_links_edit: launch failed: %s", hipGetErrorString(e)); return (int)e; }
  return MKE_LINKS_OK;
}
