// mke_assign.hip — optimal one-to-one alignment on the device (gfx950): Bertsekas' forward auction in Jacobi form over the
// candidate lists of mke_stable_lists, without the n1 x n2 matrix.  The reference has no counterpart (its only one-to-one
// decoder is stable_alignment); the definition is the NumPy oracle tests/assign_oracle.py, which the device equals bit for bit.
//
// A round (include/multike_hip.h, section 9f): every row that holds no column and has not settled unmatched takes, against the
// prices at the start of the round, v1 = its largest val[k] - price[col[k]] (the lowest list position among equal values) and
// v2 = the largest of the other entries and `floor`; v1 < floor settles it unmatched for good, else it bids
// (price[j] + (v1 - v2)) + eps on its best column j.  Every column that received bids goes to the highest (the lowest row among
// equal bids), its price becomes that bid, and the row it held before bids again next round.  Every step is one f32 operation
// in the order written (adds and subtractions only: nothing a fused multiply-add could contract).
//
// Grid form, two launches per round, so that no block reads a price, owner or bid word that another block writes in the same
// launch (that ordering IS the run-to-run and oracle equality, and it needs no handshake between blocks):
//   k_assign_bid     one wavefront per row.  A row with state 0 reads col / val coalesced, gathers price[col], reduces (value,
//                    position) to the best and the second best with shuffles; lane 0 sends one 64-bit atomic max of
//                    (float_key(bid) << 32 | 0xFFFFFFFF - row) to bid[j] and parks the row as state = -(j + 2) ("bid on j,
//                    not decided"), or as INT32_MIN ("settling").  Both codes live only between the two launches of a round.
//                    A new bid is at least price + eps and the price is the last winning bid, so the bids on a column strictly
//                    increase from round to round and bid[] is never cleared (the holder[] of k_stable_round).
//   k_assign_commit  one thread per row.  A parked row reads bid[j]; if the word names it, it frees the previous owner
//                    (state 0), stores owner and price, and takes state j + 1; a loser returns to state 0.  Every item has
//                    exactly one writer: a column has one winner, and a displaced row is parked nowhere (it held a column).
//                    Counters: a wavefront ballot and one atomic add per wavefront and counter.
//   Which launch reads and writes what of progress[] and of the header in temp: the bid launch READS progress[0..1] (is
//   anybody bidding, and has the tail taken over) and block 0 WRITES the header's `ran`; the commit launch READS `ran` and
//   WRITES progress.  So a launch never reads a word that the same launch writes, and a launch after the fixed point returns
//   at once, having read one or two words.
//
// Tail form (k_assign_tail, one workgroup): the number of bidding rows never grows — a winner displaces at most one row — and
// an auction ends in hundreds to thousands of rounds with a handful of bidders, where two launches a round are all launch
// latency.  Once at most tail_cap rows are bidding, the grid launches return at once and one workgroup of MKE_BLOCK threads
// runs the remaining rounds of the call: the bidding rows compacted into LDS (and kept in temp between calls), a wavefront per
// row for the bid phase, a thread per row for the commit phase, __syncthreads() between the phases, a winner's slot handed to
// the row it displaced.  The semantics are the grid form's.
//   Memory: price, owner, state and bid words that ANOTHER wavefront of the workgroup wrote in an earlier round are never read
//   by plain loads here.  The 64-bit max executes in L2, and a plain load may be served from a line that the CU's vector L1
//   fetched before the atomic — the L1 is not refreshed by what happens in L2.  So the tail reads these four arrays with
//   relaxed agent-scope atomic loads (global_load sc1: served by L2) and writes them with relaxed agent-scope atomic stores
//   (write-through vector stores), waits for its outstanding memory operations (s_waitcnt vmcnt(0)) and then passes the
//   barrier.  The lists val / col are read-only and go through plain loads; the set of bidding rows lives in LDS.  The loop is
//   bounded by the call's n_rounds and waits on nothing but its own barrier.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see profiles/r20_assign.md.
#include "mke_select.h"

#include <math.h>

namespace mke {

#define ASSIGN_TAIL_MAX 4096      // rows the tail's LDS list holds: the largest effective tail_cap
#define ASSIGN_HDR_BYTES 256      // header of temp
#define ASSIGN_SETTLING INT32_MIN // state between the launches of a round: settles unmatched at the commit
// header words (int32) at the start of temp
#define AH_RAN 0                  // the bid launch of the current round ran (written by it, read by the commit launch)
#define AH_LIST_VALID 1           // list[] holds exactly the rows with state 0 (written by the tail; cleared by a grid commit)
#define AH_LIST_N 2
#define AH_CALL_START 4           // int64 at words 4..5: progress[0] at the first launch of the current call

struct AssignParams {
  int n_a, n_b, cut;
  const float* __restrict__ val;
  const int32_t* __restrict__ col;
  float eps, floor;
  int32_t* state;
  float* price;
  int32_t* owner;
  unsigned long long* bid;
  long long* progress;
  int cap;        // effective tail_cap, 0: no tail kernel
  int32_t* hdr;   // temp
  int32_t* list;  // temp + ASSIGN_HDR_BYTES, [cap]
  int32_t* __restrict__ match;
  int32_t* __restrict__ counts;
};

template <bool TAIL>
__device__ __forceinline__ float assign_price(const AssignParams& p, int j) {
  return TAIL ? __hip_atomic_load(&p.price[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.price[j];
}

// One wavefront, one bidding row.  Returns (in every lane) the best column, or -1: the row settles unmatched; *bid_out = the bid.
template <bool TAIL>
__device__ __forceinline__ int assign_wave_bid(const AssignParams& p, int row, float* bid_out) {
  const int lane = threadIdx.x & 63;
  const float* __restrict__ V = p.val + (int64_t)row * p.cut;
  const int32_t* __restrict__ L = p.col + (int64_t)row * p.cut;
  float b = -INFINITY, s = -INFINITY;  // best and second best of this lane's entries
  int kb = INT32_MAX;                  // list position of the best
  for (int k0 = 0; k0 < p.cut; k0 += 64) {  // wave-uniform trip count
    const int k = k0 + lane;
    const int c = k < p.cut ? L[k] : 0;
    const bool bad = k < p.cut && (c < 0 || c >= p.n_b);
    const uint64_t mb = __builtin_amdgcn_ballot_w64(bad);
    const int first_bad = mb ? (int)__builtin_ctzll(mb) : 64;  // a column outside [0, n_b) ends the list
    if (k < p.cut && lane < first_bad) {
      const float v = V[k];
      if (isfinite(v)) {                                       // a value that is not finite is skipped
        const float net = __fsub_rn(v, assign_price<TAIL>(p, c));
        if (net > b) { s = b; b = net; kb = k; }               // k grows within a lane: the lowest position keeps a tie
        else s = fmaxf(s, net);
      }
    }
    if (mb) break;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(b, off, 64), os = __shfl_xor(s, off, 64);
    const int okb = __shfl_xor(kb, off, 64);
    const bool take = ob > b || (ob == b && okb < kb);
    const float loser = take ? b : ob;
    b = take ? ob : b;
    kb = take ? okb : kb;
    s = fmaxf(fmaxf(s, os), loser);
  }
  if (!(b >= p.floor)) return -1;      // v1 < floor (kb == INT32_MAX: no entry at all, b = -inf)
  const float v2 = fmaxf(s, p.floor);  // second best: another entry, or staying unmatched
  const int j = L[kb];
  *bid_out = __fadd_rn(__fadd_rn(assign_price<TAIL>(p, j), __fsub_rn(b, v2)), p.eps);
  return j;
}

__device__ __forceinline__ unsigned long long assign_key(float bid, int row) {
  return ((unsigned long long)float_key(bid) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)row);
}

// Do the grid launches of this round run?  Rows bidding now: all of them before the first round, progress[1] after it.
__device__ __forceinline__ bool assign_grid_runs(const AssignParams& p) {
  const long long bidding = p.progress[0] == 0 ? (long long)p.n_a : p.progress[1];
  return bidding > (long long)p.cap;  // cap 0: while anybody bids; else: while the tail has not taken over
}

__global__ __launch_bounds__(MKE_BLOCK) void k_assign_bid(const AssignParams p, int first_of_call) {
  const bool runs = assign_grid_runs(p);  // nobody writes progress[] in this launch
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p.hdr[AH_RAN] = runs ? 1 : 0;
    if (first_of_call) *reinterpret_cast<long long*>(p.hdr + AH_CALL_START) = p.progress[0];
  }
  if (!runs) return;
  const int64_t row = (int64_t)blockIdx.x * (MKE_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= p.n_a || p.state[row] != 0) return;  // wave-uniform
  float bid = 0.f;
  const int j = assign_wave_bid<false>(p, (int)row, &bid);
  if ((threadIdx.x & 63) == 0) {
    if (j < 0) {
      p.state[row] = ASSIGN_SETTLING;
    } else {
      atomicMax(&p.bid[j], assign_key(bid, (int)row));
      p.state[row] = -(j + 2);
    }
  }
}

__device__ __forceinline__ void assign_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__global__ __launch_bounds__(MKE_BLOCK) void k_assign_commit(const AssignParams p) {
  if (p.hdr[AH_RAN] == 0) return;  // written by the bid launch; nobody writes it here
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  const int st = i < p.n_a ? p.state[i] : 1;
  const bool settling = st == ASSIGN_SETTLING;
  const bool parked = st <= -2 && !settling;
  bool took_free = false;
  if (parked) {
    const int j = -(st + 2);
    // (j and prev are in range whenever the caller zeroed the state before the first round; the tests of range keep a
    // caller's mistake inside the buffers)
    const unsigned long long w = j < p.n_b ? p.bid[j] : 0ull;  // complete: the atomics ran in the launch before
    if ((unsigned)w == 0xFFFFFFFFu - (unsigned)i) {
      const int prev = p.owner[j];
      if (prev > 0 && prev <= p.n_a) p.state[prev - 1] = 0;  // holds a column, so it is parked nowhere: this is its only writer
      else took_free = true;
      p.owner[j] = (int)i + 1;
      p.price[j] = key_float((unsigned)(w >> 32));
      p.state[i] = j + 1;
    } else {
      p.state[i] = 0;
    }
  } else if (settling) {
    p.state[i] = -1;
  }
  const int n_bid = (int)__popcll(__builtin_amdgcn_ballot_w64(parked));
  const int n_set = (int)__popcll(__builtin_amdgcn_ballot_w64(settling));
  const int n_free = (int)__popcll(__builtin_amdgcn_ballot_w64(took_free));
  if ((threadIdx.x & 63) == 0) {
    if (n_bid) assign_add(&p.progress[2], n_bid);
    if (n_set) assign_add(&p.progress[3], n_set);
    if (n_set + n_free) assign_add(&p.progress[1], -(long long)(n_set + n_free));  // the others bid again: losers and displaced
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the only reader and writer of progress[0] in this launch
    const long long r = p.progress[0];
    if (r == 0) assign_add(&p.progress[1], (long long)p.n_a);  // zeroed by the caller: before round 0 everybody bids
    p.progress[0] = r + 1;
    p.hdr[AH_LIST_VALID] = 0;
  }
}

template <typename T>
__device__ __forceinline__ void assign_store(T* q, T v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// every memory operation of this wavefront has completed in L2, then the workgroup's barrier
__device__ __forceinline__ void assign_phase_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(MKE_BLOCK) void k_assign_tail(const AssignParams p, int n_rounds, int tail_only) {
  __shared__ int s_rows[2][ASSIGN_TAIL_MAX];
  __shared__ int s_tgt[ASSIGN_TAIL_MAX];
  __shared__ int s_n[2];
  __shared__ int s_cnt[2];  // bids, rows settled
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long r0 = p.progress[0];  // this launch writes progress[] only at its end, from thread 0
  const long long bidding = r0 == 0 ? (long long)p.n_a : p.progress[1];
  if (bidding == 0 || bidding > (long long)p.cap) return;  // done, or the grid form's turn: block-uniform
  const long long done = tail_only ? 0 : r0 - *reinterpret_cast<const long long*>(p.hdr + AH_CALL_START);
  const long long budget = (long long)n_rounds - done;     // the rounds of this call that the grid launches left
  if (budget <= 0) return;
  // ---- the bidding rows into LDS
  if (tid == 0) { s_n[0] = 0; s_cnt[0] = 0; s_cnt[1] = 0; }
  __syncthreads();
  int n;
  if (r0 == 0) {  // nothing has run: every row bids (the header is not initialised yet)
    n = p.n_a;
    for (int i = tid; i < n; i += MKE_BLOCK) s_rows[0][i] = i;
  } else if (p.hdr[AH_LIST_VALID] != 0) {
    n = p.hdr[AH_LIST_N];
    n = n < 0 ? 0 : (n > p.cap ? p.cap : n);  // never: a list is written with `bidding` rows, at most cap
    for (int i = tid; i < n; i += MKE_BLOCK) {
      const int row = p.list[i];
      s_rows[0][i] = row >= 0 && row < p.n_a ? row : 0;
    }
  } else {        // hand-over: compact the rows with state 0 (written by earlier launches: plain loads)
    for (int i = tid; i < p.n_a; i += MKE_BLOCK) {
      if (p.state[i] == 0) {
        const int pos = atomicAdd(&s_n[0], 1);
        if (pos < ASSIGN_TAIL_MAX) s_rows[0][pos] = i;
      }
    }
    __syncthreads();
    n = s_n[0] < ASSIGN_TAIL_MAX ? s_n[0] : ASSIGN_TAIL_MAX;  // = bidding <= cap <= ASSIGN_TAIL_MAX
  }
  __syncthreads();
  long long it = 0;
  int cur = 0;
  for (; it < budget && n > 0; ++it, cur ^= 1) {
    // ---- bid phase: a wavefront per row
    for (int s = wv; s < n; s += MKE_BLOCK / 64) {
      const int row = s_rows[cur][s];
      float bid = 0.f;
      const int j = assign_wave_bid<true>(p, row, &bid);
      if (lane == 0) {
        s_tgt[s] = j;
        if (j < 0) assign_store(&p.state[row], -1);
        else atomicMax(&p.bid[j], assign_key(bid, row));
      }
    }
    if (tid == 0) s_n[cur ^ 1] = 0;
    assign_phase_barrier();
    // ---- commit phase: a thread per row; the rows that bid again go to the other list
    for (int s = tid; s < n; s += MKE_BLOCK) {
      const int row = s_rows[cur][s], j = s_tgt[s];
      int again = -1;
      if (j < 0) {
        atomicAdd(&s_cnt[1], 1);
      } else {
        atomicAdd(&s_cnt[0], 1);
        const unsigned long long w = __hip_atomic_load(&p.bid[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)w == 0xFFFFFFFFu - (unsigned)row) {
          const int prev = __hip_atomic_load(&p.owner[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (prev > 0 && prev <= p.n_a) { assign_store(&p.state[prev - 1], 0); again = prev - 1; }
          assign_store(&p.owner[j], row + 1);
          assign_store(&p.price[j], key_float((unsigned)(w >> 32)));
          assign_store(&p.state[row], j + 1);
        } else {
          again = row;
        }
      }
      if (again >= 0) s_rows[cur ^ 1][atomicAdd(&s_n[cur ^ 1], 1)] = again;  // at most n of them: one per slot
    }
    assign_phase_barrier();
    n = s_n[cur ^ 1];
  }
  // ---- the list and the counters for the next launch
  for (int i = tid; i < n; i += MKE_BLOCK) p.list[i] = s_rows[cur][i];
  if (tid == 0) {
    p.hdr[AH_LIST_N] = n;
    p.hdr[AH_LIST_VALID] = 1;
    p.progress[0] = r0 + it;
    p.progress[1] = n;
    p.progress[2] += s_cnt[0];
    p.progress[3] += s_cnt[1];
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_assign_finish(const AssignParams p) {
  __shared__ int s_c[3][MKE_BLOCK / 64];
  int matched = 0, gold = 0, settled = 0;
  for (int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; i < p.n_a; i += (int64_t)gridDim.x * MKE_BLOCK) {
    const int st = p.state[i];
    const int m = st > 0 ? st - 1 : -1;
    p.match[i] = m;
    matched += m >= 0 ? 1 : 0;
    gold += m == (int)i ? 1 : 0;
    settled += st == -1 ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    matched += __shfl_xor(matched, off, 64);
    gold += __shfl_xor(gold, off, 64);
    settled += __shfl_xor(settled, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { s_c[0][threadIdx.x >> 6] = matched; s_c[1][threadIdx.x >> 6] = gold; s_c[2][threadIdx.x >> 6] = settled; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int v = s_c[threadIdx.x][0] + s_c[threadIdx.x][1] + s_c[threadIdx.x][2] + s_c[threadIdx.x][3];
    if (v) atomicAdd(&p.counts[threadIdx.x], v);
  }
}

static int assign_cap(int tail_cap) {
  const int cap = tail_cap > 0 ? tail_cap : MKE_ASSIGN_TAIL_CAP;
  return cap < ASSIGN_TAIL_MAX ? cap : ASSIGN_TAIL_MAX;
}

}  // namespace mke

extern "C" int64_t mke_assign_temp_bytes(int64_t n_a, int64_t n_b, int tail_cap) {
  using namespace mke;
  if (n_a < 0 || n_b < 0 || n_a > 0x7FFFFF00LL || n_b > 0x7FFFFF00LL) { set_error("mke_assign_temp_bytes: bad n_a / n_b"); return MKE_E_SHAPE; }
  if (tail_cap < 0) { set_error("mke_assign_temp_bytes: tail_cap < 0"); return MKE_E_SHAPE; }
  return ASSIGN_HDR_BYTES + (int64_t)assign_cap(tail_cap) * 4;
}

static int assign_params(const char* who, const mke_assign_args* args, bool finish, mke::AssignParams* p) {
  using namespace mke;
  if (!args) { set_error("%s: NULL args", who); return MKE_E_NULL; }
  const mke_assign_args& g = *args;
  if (g.n_a < 0 || g.n_b < 0 || g.n_a > 0x7FFFFF00LL || g.n_b > 0x7FFFFF00LL) { set_error("%s: bad n_a / n_b", who); return MKE_E_SHAPE; }
  if (g.cut < 1) { set_error("%s: cut < 1", who); return MKE_E_SHAPE; }
  if (finish) {
    if (!g.counts || (g.n_a > 0 && (!g.state || !g.match))) { set_error("%s: NULL pointer", who); return MKE_E_NULL; }
  } else {
    if (!isfinite(g.eps) || !isfinite(g.floor)) { set_error("%s: eps and floor must be finite", who); return MKE_E_RANGE; }
    if (g.eps < 0x1p-14f) { set_error("%s: eps below 2^-14 (price + eps could stop being a strict increase)", who); return MKE_E_RANGE; }
    if (g.tail_cap < 0) { set_error("%s: tail_cap < 0", who); return MKE_E_SHAPE; }
    if (g.flags & ~(MKE_ASSIGN_NO_TAIL | MKE_ASSIGN_TAIL_ONLY) || g.flags == (MKE_ASSIGN_NO_TAIL | MKE_ASSIGN_TAIL_ONLY)) {
      set_error("%s: unknown flags %d", who, g.flags);
      return MKE_E_UNSUPPORTED;
    }
    if (!g.progress || (g.n_a > 0 && (!g.val || !g.col || !g.state || !g.temp || (g.n_b > 0 && (!g.price || !g.owner || !g.bid))))) {
      set_error("%s: NULL pointer", who);
      return MKE_E_NULL;
    }
    const int64_t need = ASSIGN_HDR_BYTES + (int64_t)assign_cap(g.tail_cap) * 4;
    if (g.n_a > 0 && g.temp_bytes < need) { set_error("%s: temp below mke_assign_temp_bytes (%lld)", who, (long long)need); return MKE_E_SHAPE; }
  }
  p->n_a = (int)g.n_a; p->n_b = (int)g.n_b; p->cut = g.cut; p->val = g.val; p->col = g.col; p->eps = g.eps; p->floor = g.floor;
  p->state = g.state; p->price = g.price; p->owner = g.owner; p->bid = (unsigned long long*)g.bid; p->progress = (long long*)g.progress;
  p->cap = (g.flags & MKE_ASSIGN_NO_TAIL) ? 0 : assign_cap(g.tail_cap);
  p->hdr = (int32_t*)g.temp; p->list = (int32_t*)((char*)g.temp + ASSIGN_HDR_BYTES);
  p->match = g.match; p->counts = g.counts;
  return MKE_OK;
}

extern "C" int mke_assign_rounds(const mke_assign_args* args, int n_rounds, void* stream) {
  using namespace mke;
  AssignParams p;
  const int rc = assign_params("mke_assign_rounds", args, false, &p);
  if (rc != MKE_OK) return rc;
  if (n_rounds < 0) { set_error("mke_assign_rounds: n_rounds < 0"); return MKE_E_SHAPE; }
  if (p.n_a == 0 || n_rounds == 0) return MKE_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool tail_only = (args->flags & MKE_ASSIGN_TAIL_ONLY) != 0;
  if (!tail_only) {
    const unsigned bid_blocks = (unsigned)(((int64_t)p.n_a + MKE_BLOCK / 64 - 1) / (MKE_BLOCK / 64));
    const unsigned commit_blocks = (unsigned)(((int64_t)p.n_a + MKE_BLOCK - 1) / MKE_BLOCK);
    for (int r = 0; r < n_rounds; ++r) {
      hipLaunchKernelGGL(k_assign_bid, dim3(bid_blocks), dim3(MKE_BLOCK), 0, st, p, r == 0 ? 1 : 0);
      int e = check_launch("k_assign_bid");
      if (e) return e;
      hipLaunchKernelGGL(k_assign_commit, dim3(commit_blocks), dim3(MKE_BLOCK), 0, st, p);
      e = check_launch("k_assign_commit");
      if (e) return e;
    }
  }
  if (p.cap > 0) {
    hipLaunchKernelGGL(k_assign_tail, dim3(1), dim3(MKE_BLOCK), 0, st, p, n_rounds, tail_only ? 1 : 0);
    return check_launch("k_assign_tail");
  }
  return MKE_OK;
}

extern "C" int mke_assign_finish(const mke_assign_args* args, void* stream) {
  using namespace mke;
  AssignParams p;
  const int rc = assign_params("mke_assign_finish", args, true, &p);
  if (rc != MKE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(p.counts, 0, 3 * sizeof(int32_t), st) != hipSuccess) return check_launch("mke_assign_finish: memset");
  if (p.n_a == 0) return MKE_OK;
  const int64_t blocks = ((int64_t)p.n_a + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_assign_finish, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_assign_finish");
}
