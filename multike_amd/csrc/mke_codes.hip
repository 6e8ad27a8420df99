// mke_codes.hip — one code word per negative, baked when a chunk of steps is sampled (multike_hip.h, section (1c)).
//
// What the training kernel needs to know of a negative — its corrupted entity and side, whether it takes the one-gather path,
// whether its entity is referenced exactly once in its step — depends on the ids alone, and the ids of every step of a chunk
// exist before its first step runs.  Counting "exactly once" per step needs no counters: two bits per entity and step say
// "referenced" and "referenced again".
//   mark: every reference (mke_count_entity_refs' rule) sets bit 0 of its entity with a returning atomicOr; one that finds it
//         set, sets bit 1
//   bake: after all marks of the chunk, per negative: code = entity | side | fast | (bits == 01)
// A step's row of the bitmap is small (200K entities: 50 KB), so where it fits the LDS one workgroup per step does both: it
// marks into the LDS with LDS atomics, bakes out of it and writes the row out (k_code_step).  Marking in global memory costs a
// device-scope returning atomic per reference — 25 M of them per C2 epoch, 1.24 ms measured on the MI355X, more than the code
// words save — and is kept for rows that do not fit (k_code_mark, k_code_bake: one launch each per chunk, grid.y = step).
// Where the sampler itself wrote the words (its code-word form: everything but the exclusive bit), the same workgroup per step
// marks from and bakes into that one array (k_code_step_inplace).
// The row written out is read again: the update launch of a code-word step finds its rows in it (mke_update_table.bits — pair 11,
// and pair 01 where a positive names the row) instead of in touched flags that the score launch would have to store.
#include "mke_common.h"

namespace mke {

struct CodeParams {
  const int32_t* __restrict__ ph;   // epoch arrays, indexed by epoch position
  const int32_t* __restrict__ pr;
  const int32_t* __restrict__ pt;
  const int64_t* __restrict__ step_off;   // device; step c of the launch = step_off[s0 + c .. s0 + c + 1]
  int s0;
  int64_t pos0;                     // step_off[s0]: negative n of position i sits at (i - pos0) * npp + n
  const int32_t* __restrict__ nh;
  const int32_t* __restrict__ nr;
  const int32_t* __restrict__ nt;
  int npp;
  int64_t row_words;                // words of one step's bitmap row
  uint32_t* __restrict__ bits;
  int32_t* __restrict__ code;
};

__device__ __forceinline__ void code_mark(uint32_t* __restrict__ row, int e) {
  const uint32_t b = 1u << ((e & 15) * 2);
  if (atomicOr(&row[e >> 4], b) & b) atomicOr(&row[e >> 4], b << 1);
}

__global__ __launch_bounds__(MKE_BLOCK) void k_code_mark(const CodeParams p) {
  const int c = blockIdx.y;
  const int64_t lo = p.step_off[p.s0 + c], n = p.step_off[p.s0 + c + 1] - lo;
  uint32_t* __restrict__ row = p.bits + (int64_t)c * p.row_words;
  const int64_t total = n * (1 + p.npp);
  const int32_t* __restrict__ nh = p.nh + (lo - p.pos0) * p.npp;
  const int32_t* __restrict__ nt = p.nt + (lo - p.pos0) * p.npp;
  for (int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MKE_BLOCK) {
    if (i < n) {
      code_mark(row, p.ph[lo + i]);
      code_mark(row, p.pt[lo + i]);
    } else {
      const int64_t k = i - n;
      const int64_t g = lo + (int64_t)((uint64_t)k / (uint32_t)p.npp);
      const int a = nh[k], b = nt[k];
      if (a != p.ph[g]) code_mark(row, a);
      if (b != p.pt[g]) code_mark(row, b);
    }
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_code_bake(const CodeParams p) {
  const int c = blockIdx.y;
  const int64_t lo = p.step_off[p.s0 + c], n = p.step_off[p.s0 + c + 1] - lo;
  const uint32_t* __restrict__ row = p.bits + (int64_t)c * p.row_words;
  const int64_t total = n * p.npp, o = (lo - p.pos0) * p.npp;
  for (int64_t k = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; k < total; k += (int64_t)gridDim.x * MKE_BLOCK) {
    const int64_t g = lo + (int64_t)((uint64_t)k / (uint32_t)p.npp);
    const int nh = p.nh[o + k], nr = p.nr[o + k], nt = p.nt[o + k];
    const bool dh = nh != p.ph[g], dt = nt != p.pt[g];
    const int e = dh ? nh : nt;
    const uint32_t two = (row[e >> 4] >> ((e & 15) * 2)) & 3u;
    p.code[o + k] = e | (dh ? MKE_CODE_HEAD : 0) | ((nr == p.pr[g] && dh != dt) ? MKE_CODE_FAST : 0) | (two == 1u ? MKE_CODE_EXCL : 0);
  }
}

constexpr int CODE_STEP_BLOCK = 1024;
constexpr int64_t CODE_LDS_BYTES = 64 << 10;   // dynamic LDS a launch gets without asking for more: rows of up to 262,144 entities

// One workgroup per step: row zeroed, marked and read in the LDS.  Four items per thread and pass, ids loaded before the first
// mark, so that a wavefront keeps eight loads in flight (one workgroup per CU is all the occupancy there is).
__global__ __launch_bounds__(CODE_STEP_BLOCK) void k_code_step(const CodeParams p) {
  extern __shared__ uint32_t s_row[];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t lo = p.step_off[p.s0 + c];
  const int n = (int)(p.step_off[p.s0 + c + 1] - lo), npp = p.npp, n_neg = n * npp;   // the launcher checks that a step's negatives fit 31 bits
  const int64_t o = (lo - p.pos0) * npp;
  const int32_t* __restrict__ nh = p.nh + o;
  const int32_t* __restrict__ nr = p.nr + o;
  const int32_t* __restrict__ nt = p.nt + o;
  const int32_t* __restrict__ ph = p.ph + lo;
  const int32_t* __restrict__ pr = p.pr + lo;
  const int32_t* __restrict__ pt = p.pt + lo;
  for (int w = tid; w < (int)p.row_words; w += CODE_STEP_BLOCK) s_row[w] = 0u;
  __syncthreads();
  for (int i = tid; i < n; i += CODE_STEP_BLOCK) {
    code_mark(s_row, ph[i]);
    code_mark(s_row, pt[i]);
  }
  constexpr int V = 4;
  for (int k0 = tid; k0 < n_neg; k0 += V * CODE_STEP_BLOCK) {
    int a[V], b[V], ha[V], tb[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      const bool live = k < n_neg;
      const int kk = live ? k : 0, g = (int)((uint32_t)kk / (uint32_t)npp);
      a[v] = nh[kk]; b[v] = nt[kk]; ha[v] = live ? ph[g] : a[v]; tb[v] = live ? pt[g] : b[v];   // not live: nothing differs, nothing marked
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (a[v] != ha[v]) code_mark(s_row, a[v]);
      if (b[v] != tb[v]) code_mark(s_row, b[v]);
    }
  }
  __syncthreads();
  for (int k0 = tid; k0 < n_neg; k0 += V * CODE_STEP_BLOCK) {
    int a[V], r[V], b[V], ha[V], hr[V], tb[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      const int kk = k < n_neg ? k : 0, g = (int)((uint32_t)kk / (uint32_t)npp);
      a[v] = nh[kk]; r[v] = nr[kk]; b[v] = nt[kk]; ha[v] = ph[g]; hr[v] = pr[g]; tb[v] = pt[g];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      const bool dh = a[v] != ha[v], dt = b[v] != tb[v];
      const int e = dh ? a[v] : b[v];
      const uint32_t two = (s_row[e >> 4] >> ((e & 15) * 2)) & 3u;
      if (k < n_neg)
        p.code[o + k] = e | (dh ? MKE_CODE_HEAD : 0) | ((r[v] == hr[v] && dh != dt) ? MKE_CODE_FAST : 0) | (two == 1u ? MKE_CODE_EXCL : 0);
    }
  }
  uint32_t* __restrict__ row = p.bits + (int64_t)c * p.row_words;
  for (int w = tid; w < (int)p.row_words; w += CODE_STEP_BLOCK) row[w] = s_row[w];
}

// The same step from ONE stream, in place (mke_neg_codes without id arrays): p.code holds what the sampler's code-word form wrote — the word
// without MKE_CODE_EXCL — so the entity to mark and whether it is marked at all (MKE_CODE_FAST: exactly one side differs; a
// negative without it is the positive itself here and marks nothing, as in k_code_step) are in the word, and neither the three id
// arrays nor the positive's ids per negative are read.  One 4-byte stream per item lets a thread keep sixteen loads in flight:
// a C2 step (124K negatives) is 8 mark and 8 bake passes instead of 31 + 31 of four and six streams each.
constexpr int CODE_INPLACE_V = 16;
__global__ __launch_bounds__(CODE_STEP_BLOCK) void k_code_step_inplace(const CodeParams p) {
  extern __shared__ uint32_t s_row[];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t lo = p.step_off[p.s0 + c];
  const int n = (int)(p.step_off[p.s0 + c + 1] - lo), n_neg = n * p.npp;   // the launcher checks that a step's negatives fit 31 bits
  int32_t* __restrict__ code = p.code + (lo - p.pos0) * p.npp;
  const int32_t* __restrict__ ph = p.ph + lo;
  const int32_t* __restrict__ pt = p.pt + lo;
  for (int w = tid; w < (int)p.row_words; w += CODE_STEP_BLOCK) s_row[w] = 0u;
  __syncthreads();
  for (int i = tid; i < n; i += CODE_STEP_BLOCK) {
    code_mark(s_row, ph[i]);
    code_mark(s_row, pt[i]);
  }
  constexpr int V = CODE_INPLACE_V;
  constexpr int ENT = (1 << MKE_CODE_ENT_BITS) - 1;
  for (int k0 = tid; k0 < n_neg; k0 += V * CODE_STEP_BLOCK) {
    int w[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      w[v] = k < n_neg ? code[k] : 0;   // not live: no MKE_CODE_FAST, nothing marked
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (w[v] & MKE_CODE_FAST) code_mark(s_row, w[v] & ENT);
  }
  __syncthreads();
  for (int k0 = tid; k0 < n_neg; k0 += V * CODE_STEP_BLOCK) {
    int w[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      w[v] = k < n_neg ? code[k] : 0;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int k = k0 + v * CODE_STEP_BLOCK;
      const int e = w[v] & ENT;
      const uint32_t two = (s_row[e >> 4] >> ((e & 15) * 2)) & 3u;
      if (k < n_neg) code[k] = (w[v] & ~MKE_CODE_EXCL) | (two == 1u ? MKE_CODE_EXCL : 0);
    }
  }
  uint32_t* __restrict__ row = p.bits + (int64_t)c * p.row_words;
  for (int w = tid; w < (int)p.row_words; w += CODE_STEP_BLOCK) row[w] = s_row[w];
}

// true: a step's row of the bitmap fits the LDS, the bake is the one-launch form
bool neg_codes_in_lds(int64_t n_ent) { return mke_neg_code_row_words(n_ent) * (int64_t)sizeof(uint32_t) <= CODE_LDS_BYTES; }

// the chunk's rows of the bitmap and its codes: one launch (rows in the LDS), or memset, mark, bake on `st`
int launch_neg_codes(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, const int64_t* step_off_dev, int step_begin,
                     int step_end, int64_t pos_begin, int64_t pos_end, const int32_t* neg_h, const int32_t* neg_r, const int32_t* neg_t,
                     int neg_per_pos, int64_t n_ent, uint32_t* bits, int32_t* neg_code, hipStream_t st) {
  const int n_steps = step_end - step_begin;
  CodeParams p;
  p.ph = pos_h; p.pr = pos_r; p.pt = pos_t; p.step_off = step_off_dev; p.s0 = step_begin; p.pos0 = pos_begin;
  p.nh = neg_h; p.nr = neg_r; p.nt = neg_t; p.npp = neg_per_pos;
  p.row_words = mke_neg_code_row_words(n_ent); p.bits = bits; p.code = neg_code;
  if (neg_codes_in_lds(n_ent) && (pos_end - pos_begin) * (int64_t)neg_per_pos < (1ll << 31)) {
    hipLaunchKernelGGL(k_code_step, dim3(n_steps), dim3(CODE_STEP_BLOCK), (size_t)p.row_words * sizeof(uint32_t), st, p);
    return check_launch("k_code_step");
  }
  const hipError_t e = hipMemsetAsync(bits, 0, (size_t)n_steps * (size_t)p.row_words * sizeof(uint32_t), st);
  if (e != hipSuccess) { set_error("mke_neg_codes: memset: %s", hipGetErrorString(e)); return (int)e; }
  // blocks per step: enough for the chunk's largest step on average (a longer step loops), at most 256
  const int64_t per_step = (pos_end - pos_begin + n_steps - 1) / n_steps * (1 + neg_per_pos);
  int bx = (int)std::min<int64_t>((per_step + MKE_BLOCK - 1) / MKE_BLOCK, 256);
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(k_code_mark, dim3(bx, n_steps), dim3(MKE_BLOCK), 0, st, p);
  int rc = check_launch("k_code_mark");
  if (rc) return rc;
  hipLaunchKernelGGL(k_code_bake, dim3(bx, n_steps), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_code_bake");
}

// the chunk's rows of the bitmap, and MKE_CODE_EXCL into its pre-codes: one launch; only where the rows fit the LDS
int launch_neg_codes_inplace(const int32_t* pos_h, const int32_t* pos_t, const int64_t* step_off_dev, int step_begin, int step_end,
                             int64_t pos_begin, int64_t pos_end, int neg_per_pos, int64_t n_ent, uint32_t* bits, int32_t* neg_code,
                             hipStream_t st) {
  if (!neg_codes_in_lds(n_ent) || (pos_end - pos_begin) * (int64_t)neg_per_pos >= (1ll << 31)) {
    set_error("mke_neg_codes in place: a step's bitmap row must fit %lld bytes of LDS and the chunk 2^31 negatives", (long long)CODE_LDS_BYTES);
    return MKE_E_UNSUPPORTED;
  }
  CodeParams p;
  p.ph = pos_h; p.pr = nullptr; p.pt = pos_t; p.step_off = step_off_dev; p.s0 = step_begin; p.pos0 = pos_begin;
  p.nh = p.nr = p.nt = nullptr; p.npp = neg_per_pos;
  p.row_words = mke_neg_code_row_words(n_ent); p.bits = bits; p.code = neg_code;
  hipLaunchKernelGGL(k_code_step_inplace, dim3(step_end - step_begin), dim3(CODE_STEP_BLOCK), (size_t)p.row_words * sizeof(uint32_t), st, p);
  return check_launch("k_code_step_inplace");
}

}  // namespace mke

extern "C" int64_t mke_neg_code_row_words(int64_t n_ent) { return n_ent > 0 ? (n_ent + 15) / 16 : 0; }

extern "C" int mke_neg_codes(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, const int64_t* step_off, int step_begin,
                             int step_end, int64_t pos_begin, int64_t pos_end, const int32_t* neg_h, const int32_t* neg_r,
                             const int32_t* neg_t, int neg_per_pos, int64_t n_ent, uint32_t* bits, int64_t bits_words, int32_t* neg_code,
                             void* stream) {
  using namespace mke;
  if (step_begin < 0 || step_end < step_begin || pos_end < pos_begin || pos_begin < 0) { set_error("mke_neg_codes: bad step / position range"); return MKE_E_SHAPE; }
  if (step_end == step_begin || pos_end == pos_begin) return MKE_OK;
  if (neg_per_pos < 1 || neg_per_pos > 64) { set_error("mke_neg_codes: neg_per_pos must be in [1,64], got %d", neg_per_pos); return MKE_E_UNSUPPORTED; }
  if (n_ent <= 0 || n_ent > (1ll << MKE_CODE_ENT_BITS)) { set_error("mke_neg_codes: n_ent must be in [1, 2^%d]", MKE_CODE_ENT_BITS); return MKE_E_RANGE; }
  // neg_h == neg_r == neg_t == NULL: neg_code holds the sampler's own words, baked in place (section (1c))
  const bool inplace = !neg_h && !neg_r && !neg_t;
  if (!pos_h || !pos_r || !pos_t || !step_off || (!inplace && (!neg_h || !neg_r || !neg_t)) || !bits || !neg_code) { set_error("mke_neg_codes: NULL pointer"); return MKE_E_NULL; }
  if (step_end - step_begin > 65535) { set_error("mke_neg_codes: more than 65535 steps in one call"); return MKE_E_SHAPE; }
  if ((int64_t)(step_end - step_begin) * mke_neg_code_row_words(n_ent) > bits_words) {
    set_error("mke_neg_codes: %lld words of bitmap needed, %lld given", (long long)((step_end - step_begin) * mke_neg_code_row_words(n_ent)), (long long)bits_words);
    return MKE_E_SHAPE;
  }
  if (inplace)
    return launch_neg_codes_inplace(pos_h, pos_t, step_off, step_begin, step_end, pos_begin, pos_end, neg_per_pos, n_ent, bits, neg_code,
                                    (hipStream_t)stream);
  return launch_neg_codes(pos_h, pos_r, pos_t, step_off, step_begin, step_end, pos_begin, pos_end, neg_h, neg_r, neg_t, neg_per_pos, n_ent,
                          bits, neg_code, (hipStream_t)stream);
}
