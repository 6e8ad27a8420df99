// mke_oc_own.hip — owner-bucketed negative codes of the owner-computes (multi-GPU) relation-view step (gfx950).
//
// New design (the reference is single-device).  With the codes all-gathered, every rank receives all n_all * N codes of an epoch and
// walks all of them — twice in mke_oc_em_plan, once per global step in the score launch — for the 1 / G it owns (DESIGN.md 8.1:
// the largest term of the per-epoch lists; EXPERIMENTS R5.26: the score launch bound by instruction issue).  Here the HOME rank
// sorts its share by owner before it leaves:
//   * mke_oc_bucket_codes: the share's negatives as records (epoch position, n, code) in one bucket per owner, each bucket in
//     (position, n) order — a stable partition.  The order holds by construction and without atomics, as in k_em_count / k_em_fill
//     (mke_oc_em.hip records what a cursor atomic per 64 elements cost): a wavefront per contiguous range of elements counts its
//     elements per owner (a ballot per distinct owner of a round, the running counts in lanes 0 .. G - 1), one block per owner
//     turns the counts into offsets, and the same walk stores every element at its range's offset + its ballot rank.
//   * all-to-all of the buckets (the host; equal split, `cap` records per pair of ranks, the true counts travel beside them).
//   * mke_oc_owned_index: home ranks hold contiguous position ranges, so the buckets a rank receives, concatenated in source-rank
//     order, ARE its owned negatives in (position, n) order: packed, and cut per epoch position (own_off).
// The entity-major plan then enumerates the owned list instead of every code (mke_oc_em.hip, OWN), and the score launch walks
// own_off[i] .. own_off[i + 1] instead of scanning N codes per positive (mke_oc.hip, OC_OWNED).
#include "mke_common.h"

namespace mke {

#define OWN_REC 3           // ints per record: epoch position, n, code without the flag bits
#define OWN_U 4             // codes in flight per lane and round
#define OWN_SCAN_THREADS 1024

struct BucketParams {
  const int32_t* codes;     // [total]
  int64_t total;            // n_mine * N  (< 2^31)
  int N;
  int64_t pos0;
  int G;
  int64_t cap;
  int32_t* send;            // [G][cap] records
  int32_t* wave;            // [G][n_waves]: counts per (owner, wavefront range), then their exclusive prefix per owner
  int n_waves;
  int64_t per;              // elements per wavefront range (a multiple of 64)
};

// FILL = false: wave[d][w] = elements of range w owned by d.  FILL = true (after k_own_scan): element e of range w owned by d goes
// to record wave[d][w] + (elements of d before e in the range) of bucket d — when that is below cap.
template <bool FILL>
__global__ __launch_bounds__(MKE_BLOCK) void k_own_bucket(const BucketParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x) >> 6;
  if (wave >= p.n_waves) return;                               // wave-uniform
  const OcDiv dv = oc_divisor(p.G);
  const int64_t t0 = wave * p.per, t1 = t0 + p.per < p.total ? t0 + p.per : p.total;
  int run = (FILL && lane < p.G) ? p.wave[(int64_t)lane * p.n_waves + wave] : 0;   // lane d: owner d's next record / count so far
  const uint64_t below = (1ull << lane) - 1ull;
  for (int64_t t = t0 + lane; t - lane < t1; t += 64 * OWN_U) {     // wave-uniform trip count (ballots inside)
    int code[OWN_U];
#pragma unroll
    for (int u = 0; u < OWN_U; ++u) code[u] = t + 64 * u < t1 ? (p.codes[t + 64 * u] & 0x3FFFFFFF) : -1;
#pragma unroll
    for (int u = 0; u < OWN_U; ++u) {
      const int d = code[u] >= 0 ? oc_mod(dv, code[u] >> 1) : -1;
      uint64_t todo = __ballot(d >= 0);
      while (todo) {                                           // wave-uniform: one round per distinct owner present
        const int d0 = __shfl(d, __builtin_ctzll(todo), 64);
        const uint64_t m = __ballot(d == d0);
        if constexpr (FILL) {
          const int before = __shfl(run, d0, 64);
          const int64_t k = (int64_t)before + __popcll(m & below);
          if (d == d0 && k < p.cap) {
            const uint32_t e = (uint32_t)(t + 64 * u);         // < 2^31 (checked on the host)
            const uint32_t q = e / (uint32_t)p.N;
            int32_t* rec = p.send + OWN_REC * ((int64_t)d0 * p.cap + k);
            rec[0] = (int32_t)(p.pos0 + q);
            rec[1] = (int32_t)(e - q * (uint32_t)p.N);
            rec[2] = code[u];
          }
        }
        if (lane == d0) run += __popcll(m);
        todo &= ~m;
      }
    }
  }
  if (!FILL && lane < p.G) p.wave[(int64_t)lane * p.n_waves + wave] = run;
}

// one block per owner: its n_waves counts -> exclusive prefix in place, the total -> counts[owner]
__global__ __launch_bounds__(OWN_SCAN_THREADS) void k_own_scan(int32_t* __restrict__ wave, int n_waves, int32_t* __restrict__ counts) {
  __shared__ int s_w[OWN_SCAN_THREADS / 64];
  int32_t* w = wave + (int64_t)blockIdx.x * n_waves;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = (n_waves + OWN_SCAN_THREADS - 1) / OWN_SCAN_THREADS;
  const int a = tid * K < n_waves ? tid * K : n_waves, b = a + K < n_waves ? a + K : n_waves;
  int sum = 0;
  for (int i = a; i < b; ++i) sum += w[i];
  int inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(inc, off, 64);
    if (lane >= off) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  int ex = inc - sum;
  for (int k = 0; k < wv; ++k) ex += s_w[k];
  for (int i = a; i < b; ++i) {
    const int c = w[i];
    w[i] = ex;
    ex += c;
  }
  if (tid == OWN_SCAN_THREADS - 1) counts[blockIdx.x] = ex;
}

// the need flags of a position alone, where mke_oc_plan looks for them with one code per position
__global__ __launch_bounds__(MKE_BLOCK) void k_own_need(const int32_t* __restrict__ codes, int64_t n_mine, int N, int32_t* __restrict__ need) {
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= n_mine) return;
  need[i] = N ? (int32_t)((uint32_t)codes[i * N] & (MKE_OC_NEED_HR | MKE_OC_NEED_RT)) : (int32_t)MKE_OC_NEED_HR;
}

struct IndexParams {
  const int32_t* recv; const int32_t* counts; int G; int64_t cap; int64_t n_all;
  int32_t* own_rec; int32_t* own_off;
};

// record k of source s -> record (records of the sources before s) + k of the packed list
__global__ __launch_bounds__(MKE_BLOCK) void k_own_pack(const IndexParams p) {
  const int64_t x = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (x >= p.G * p.cap) return;
  const int s = (int)(x / p.cap);
  const int64_t k = x - s * p.cap;
  int64_t pre = 0, mine = 0;
  for (int g = 0; g <= s; ++g) {
    int64_t c = p.counts[g];
    c = c < 0 ? 0 : (c > p.cap ? p.cap : c);
    if (g < s) pre += c; else mine = c;
  }
  if (k >= mine) return;
  const int32_t* src = p.recv + OWN_REC * x;
  int32_t* dst = p.own_rec + OWN_REC * (pre + k);
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

// record k starts every position after record k - 1's up to its own; the end marker (k = the list's count) the positions after the
// last record's.  A run of positions without an owned negative is written by ONE thread: the sum of all runs is n_all + 1.
__global__ __launch_bounds__(MKE_BLOCK) void k_own_offsets(const IndexParams p) {
  const int64_t k = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  int64_t n_own = 0;
  for (int g = 0; g < p.G; ++g) {
    const int64_t c = p.counts[g];
    n_own += c < 0 ? 0 : (c > p.cap ? p.cap : c);
  }
  if (k > n_own) return;
  int64_t prev = k > 0 ? (int64_t)p.own_rec[OWN_REC * (k - 1)] : -1;
  int64_t cur = k < n_own ? (int64_t)p.own_rec[OWN_REC * k] : p.n_all;
  if (prev < -1) prev = -1;
  if (cur > p.n_all) cur = p.n_all;                            // (a position outside the epoch: never from mke_oc_bucket_codes)
  for (int64_t q = prev + 1; q <= cur; ++q) p.own_off[q] = (int32_t)k;
}

}  // namespace mke

extern "C" int mke_oc_bucket_codes(const int32_t* codes, int64_t n_mine, int neg_per_pos, int64_t pos0, int n_ranks, int64_t cap,
                                   int32_t* need, int32_t* send, int32_t* counts, int32_t* scratch, void* stream) {
  using namespace mke;
  if (n_mine < 0 || neg_per_pos < 0 || neg_per_pos > 64 || pos0 < 0 || cap < 0) { set_error("mke_oc_bucket_codes: bad n_mine / neg_per_pos (<= 64) / pos0 / cap"); return MKE_E_SHAPE; }
  if (n_ranks < 1 || n_ranks > MKE_OC_MAX_RANKS) { set_error("mke_oc_bucket_codes: bad n_ranks"); return MKE_E_SHAPE; }
  if (pos0 + n_mine > 0x80000000ll || n_mine * neg_per_pos >= 0x7FFFFFFFll || cap * n_ranks >= 0x7FFFFFFFll) { set_error("mke_oc_bucket_codes: positions, codes of a share and records of a rank stay below 2^31"); return MKE_E_RANGE; }
  if (!counts || !scratch || (n_mine > 0 && !need)) { set_error("mke_oc_bucket_codes: NULL output / scratch"); return MKE_E_NULL; }
  const int64_t total = n_mine * neg_per_pos;
  if (total > 0 && (!codes || (cap > 0 && !send))) { set_error("mke_oc_bucket_codes: NULL codes / send"); return MKE_E_NULL; }
  hipStream_t st = (hipStream_t)stream;
  if (n_mine > 0) {
    hipLaunchKernelGGL(k_own_need, dim3((unsigned)((n_mine + MKE_BLOCK - 1) / MKE_BLOCK)), dim3(MKE_BLOCK), 0, st, codes, n_mine, neg_per_pos, need);
    int rc = check_launch("k_own_need");
    if (rc) return rc;
  }
  if (total == 0) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_ranks * sizeof(int32_t), st);
    if (e != hipSuccess) { set_error("mke_oc_bucket_codes: %s", hipGetErrorString(e)); return (int)e; }
    return MKE_OK;
  }
  BucketParams p;
  p.codes = codes; p.total = total; p.N = neg_per_pos; p.pos0 = pos0; p.G = n_ranks; p.cap = cap; p.send = send; p.wave = scratch;
  int64_t nw = (total + 511) / 512;                            // >= 8 rounds of 64 elements per wavefront
  if (nw > MKE_OC_BUCKET_WAVES) nw = MKE_OC_BUCKET_WAVES;
  p.n_waves = (int)nw;
  p.per = ((total + nw - 1) / nw + 63) & ~63ll;
  const dim3 wgrid((unsigned)((nw * 64 + MKE_BLOCK - 1) / MKE_BLOCK));
  hipLaunchKernelGGL(k_own_bucket<false>, wgrid, dim3(MKE_BLOCK), 0, st, p);
  int rc = check_launch("k_own_bucket");
  if (rc) return rc;
  hipLaunchKernelGGL(k_own_scan, dim3((unsigned)n_ranks), dim3(OWN_SCAN_THREADS), 0, st, scratch, p.n_waves, counts);
  if ((rc = check_launch("k_own_scan"))) return rc;
  hipLaunchKernelGGL(k_own_bucket<true>, wgrid, dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_own_bucket");
}

extern "C" int mke_oc_owned_index(const int32_t* recv, const int32_t* counts, int n_ranks, int64_t cap, int64_t n_all,
                                  int32_t* own_rec, int32_t* own_off, void* stream) {
  using namespace mke;
  if (n_ranks < 1 || n_ranks > MKE_OC_MAX_RANKS || cap < 0 || n_all < 0) { set_error("mke_oc_owned_index: bad n_ranks / cap / n_all"); return MKE_E_SHAPE; }
  if (n_all >= 0x7FFFFFFFll || cap * n_ranks >= 0x7FFFFFFFll) { set_error("mke_oc_owned_index: positions and records of a rank stay below 2^31"); return MKE_E_RANGE; }
  if (!counts || !own_off || (cap > 0 && (!recv || !own_rec))) { set_error("mke_oc_owned_index: NULL pointer"); return MKE_E_NULL; }
  IndexParams p;
  p.recv = recv; p.counts = counts; p.G = n_ranks; p.cap = cap; p.n_all = n_all; p.own_rec = own_rec; p.own_off = own_off;
  hipStream_t st = (hipStream_t)stream;
  const int64_t slots = cap * n_ranks;
  if (slots > 0) {
    hipLaunchKernelGGL(k_own_pack, dim3((unsigned)((slots + MKE_BLOCK - 1) / MKE_BLOCK)), dim3(MKE_BLOCK), 0, st, p);
    int rc = check_launch("k_own_pack");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_own_offsets, dim3((unsigned)((slots + 1 + MKE_BLOCK - 1) / MKE_BLOCK)), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_own_offsets");
}
