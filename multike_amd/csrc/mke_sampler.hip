// mke_sampler.hip — on-device negative sampler + known-triple hash set (gfx950).
//
// Distribution = code/base/batch.py:86-116 generate_neg_triples_fast: per positive, up
// to max_try rounds; one fair coin per round chooses the corrupted side; `need` distinct candidates are
// drawn without replacement from that side's candidate list; known triples are dropped except in the
// last round; stop at neg_per_pos.  The reference draws from CPython's Mersenne Twister through
// Manager-queue worker processes; here the stream is Philox4x32-10 keyed by (seed, stream id) and
// indexed by (positive, round, slot, attempt), so any positive can be sampled by any wavefront in any
// order and the CPU oracles (oracle/sampler_oracle.py, restated in C as mko_neg_sample_at of oracle/mke_oracle.c) reproduce
// the device output bit for bit.
//
// The kernel, k_neg_sample<GS, CODES, O32> (bound by VALU issue and by the waits of the known-triple test: 32-bit integer
// multiplies are quarter rate and a Philox4x32-10 evaluation has 40 of them; profiles/r25_sampler_issue.md):
//  * group shapes: one group of GS lanes per positive, lane q of the group = slot q of the round.  GS = 16 (neg_per_pos <= 15:
//    four positives per wavefront), 32 (<= 32: two) or 64.  Everything that is per positive (round count, collected, coin,
//    candidate list) lives in the group's lanes; wave-wide primitives (__shfl, __ballot) take group-relative indices / masks;
//  * coin in the idle lane: the round's coin block (counter word 2 = 0xFFFFFFFF) is evaluated by the group's LAST lane in the same
//    Philox evaluation in which lanes < need evaluate their first draw block (word 2 = slot) — one evaluation per round instead
//    of two; needs an idle lane (neg_per_pos < GS), else the coin keeps its own evaluation;
//  * LDS table and fix-up: "is any first draw a duplicate of an earlier slot's" is answered by inserting the draws into a
//    2 GS-slot open-addressing table of the group in LDS (compare-and-swap, ~1.2 probes); the exact sequential fix-up (slot q
//    must differ from the final draws of the slots before it) runs only when the table saw an equal value (0.3 % of the groups
//    at 25 draws from 100K);
//  * wave-uniform side: a step's positives are KG 1 first, then KG 2, so all live lanes of nearly every wavefront have ONE kg
//    (one ballot).  The rounds are instantiated once per KG with the side's place in the kernel arguments a constant, so its
//    fields are scalar loads and the side costs no per-lane round trip to the kernel arguments behind the pos_kg byte.  A mixed
//    wavefront (two per step) takes the double pass: the rounds once per KG, the other KG's groups idle;
//  * O32: positives, entity list, filter and outputs are indexed with 32-bit byte offsets on scalar bases where the launcher
//    proves that they fit (sampler_o32_fits); the 64-bit form is the fallback instantiation.  The candidate table and the
//    exact probe keep 64-bit arithmetic (their sizes are not the launcher's to know / the rare branch);
//  * prefilter: almost every candidate is NOT a known triple, and the exact answer costs the 64-bit mix64 and one random 8-byte
//    read into a table that is larger than an XCD's 4 MB L2 (8 MB per KG at 460 K triples).  In front of that probe sits a Bloom
//    filter, one bit array per set: filter_mix32 of (h, r, t) — four 32-bit multiplies — picks a word and three bits of it.  A
//    clear bit among the three answers "not known" from L2; three set bits fall through to the exact probe, so the output is
//    the unfiltered kernel's bit for bit.  0.9 % of the draws fall through at the C2 shape, a lane in a third of the wavefronts
//    (profiles/r25_sampler_issue.md, section 3; C5 unmeasured).  The library owns the filters, one per (keys, capacity), and
//    mke_tripleset_build is their only writer (see the header for what keeps filter and table in step);
//  * strided grid: a wavefront samples 64 / GS positives at a time and strides by a capped grid (SAMPLE_BLOCKS_PER_CU) instead
//    of one wavefront launched per 64 / GS positives (56 iterations per wavefront at the C2 epoch launch);
//  * Lemire's rejection threshold `(0u - n) % n` is evaluated only by lanes with l < n.
//
// CODES (mke_neg_sample with neg_r == neg_t == NULL): a kept candidate is stored as ONE word, the code word of multike_hip.h (1c) without
// MKE_CODE_EXCL, at the offset its three ids would have taken — the draw, the side and "differs from the id it replaces" are
// all in registers here, and the three id arrays (two of them copies of the positive) are never written.  p.nh is that array.
#include <array>
#include <mutex>
#include <unordered_map>

#include "mke_common.h"
#include "mke_sampler_o32.h"

namespace mke {

// 8 bits per table slot = 1 bit per byte of table: capacity is in [2n, 4n) slots for n keys, three bits set per key: 1 MB per
// KG at the C2 shape (2 MB of a 4 MB L2 for both), 15 % of the bits set, 0.9 % of the candidates still probe
// (profiles/r25_sampler_issue.md, section 3).
// Capped at 2^25 bits (4 MB) per set: past C2's size the filters no longer fit the L2 anyway, and a few MB that stay in the
// Infinity Cache in front of a table of hundreds of MB (C5: 128 MB per KG; its pass rate is unmeasured) serve better than an
// L2-sized filter that lets half of the candidates through.
constexpr int FILTER_BITS_PER_SLOT_LOG2 = 3;
constexpr int FILTER_MAX_BITS_LOG2 = 25;
constexpr int FILTER_MIN_BITS_LOG2 = 10;

// Grid cap, in workgroups per CU.  Eight are resident at once (at most 64 VGPRs: eight wavefronts per SIMD); four times as
// many measured best at every neg_per_pos (24 .. 64 per CU within 2 %, 8 as slow as no cap, C2 epoch launch:
// profiles/r25_sampler_issue.md): the workgroups that wait even out what the resident ones do not finish together.
constexpr int SAMPLE_BLOCKS_PER_CU = 32;

struct SampleParams {
  const int32_t* __restrict__ ph;
  const int32_t* __restrict__ pr;
  const int32_t* __restrict__ pt;
  const uint8_t* __restrict__ pos_kg;
  int64_t n_pos, pos_offset;
  const int32_t* __restrict__ pos_index;  // nullable: epoch position of positive i (else pos_offset + i)
  int npp, max_try;
  mke_kg_side side[2];
  uint64_t unused[3];                      // keeps every field at its offset: moving them changes the scalar register allocation of all twelve kernels
  uint32_t seed_lo, seed_hi, sid;
  int32_t* __restrict__ nh;                // the code-word form (CODES) writes its one array through this pointer
  int32_t* __restrict__ nr;
  int32_t* __restrict__ nt;
  const uint32_t* __restrict__ filter[2];  // nullable, per side: the prefilter of the side's known-triple set
  int shift[2];                            // word index = filter_mix32 >> shift
};

__device__ __forceinline__ bool set_contains_hashed(const uint64_t* __restrict__ keys, uint64_t cap, uint64_t key, uint64_t hash) {
  uint64_t slot = hash & (cap - 1);
  for (;;) {
    const uint64_t k = keys[slot];
    if (k == key) return true;
    if (k == MKE_EMPTY_KEY) return false;
    slot = (slot + 1) & (cap - 1);
  }
}
__device__ __forceinline__ bool set_contains(const uint64_t* __restrict__ keys, uint64_t cap, uint64_t key) {
  return set_contains_hashed(keys, cap, key, mix64(key));
}

// word and bits of a triple in the filter: y -> word y >> shift (shift = 32 - log2(words)), bits from y's low end
__host__ __device__ __forceinline__ uint32_t filter_mix32(uint32_t h, uint32_t r, uint32_t t) {
  uint32_t x = (h * 0x9E3779B1u) ^ (t * 0x85EBCA6Bu) ^ (r * 0xC2B2AE35u);
  x ^= x >> 15;
  return x * 0x2C1B3C6Du;
}
__host__ __device__ __forceinline__ uint32_t filter_mask32(uint32_t y, int shift) {
  // three 5-bit fields below the word index (shift >= 12: the third overlaps the second by up to three bits at the 4 MB cap)
  return (1u << (y & 31u)) | (1u << ((y >> 5) & 31u)) | (1u << ((y >> (shift - 5)) & 31u));
}

// Next accepted bounded draw in [0,n) for (positive gi, round, slot): attempts are consumed in order;
// attempt a uses word (a&3) of Philox block (a>>2).  Lemire's multiply-shift with exact rejection.  The block's word is
// chosen by selects: a dynamically indexed register array costs a stack slot or LDS.
__device__ __forceinline__ uint32_t draw_next(uint32_t gi, uint32_t round, uint32_t slot, uint32_t sid, uint32_t k0, uint32_t k1,
                                              uint32_t n, uint32_t& attempt) {
  for (;;) {
    const uint32_t blk = attempt >> 2, word = attempt & 3u;
    const Philox4 ph = philox4x32_10(gi, round | (blk << 8), slot, sid, k0, k1);
    const uint32_t x = word == 0 ? ph.v[0] : (word == 1 ? ph.v[1] : (word == 2 ? ph.v[2] : ph.v[3]));
    ++attempt;
    const uint64_t m = (uint64_t)x * (uint64_t)n;
    const uint32_t l = (uint32_t)m;
    if (l < n) {
      const uint32_t thresh = (0u - n) % n;
      if (l < thresh) continue;
    }
    return (uint32_t)(m >> 32);
  }
}

// Element idx of base; O32: byte offset formed in 32 bits, so that the access takes its base from scalar registers.
template <bool O32, class T, class I>
__device__ __forceinline__ T& elem_at(T* base, I idx) {
  if constexpr (O32) return *(T*)((char*)base + (uint32_t)((uint32_t)idx * (uint32_t)sizeof(T)));
  else return base[idx];
}

// The rounds of the wavefront's groups of KG `kg` (a constant, so every field of the side is a scalar at a fixed place of the
// kernel arguments); a lane that is not `live` belongs to a group that idles.
template <int GS, bool CODES, bool O32, int kg, class I>
__device__ __forceinline__ void sample_rounds(const SampleParams& p, const bool live, const I i, const int h, const int r,
                                              const int t, const uint32_t gi, uint32_t* __restrict__ tbl, const int gl, const int gbase) {
  constexpr int TS = 2 * GS;
  const mke_kg_side& sd = p.side[kg];
  const uint32_t sid = p.sid + (uint32_t)kg;
  const uint64_t* __restrict__ keys = sd.known_keys;
  const uint32_t* __restrict__ filter = p.filter[kg];
  const int shift = p.shift[kg];
  // the side's sizes as scalars (read here, not through a per-lane choice of kernel-argument addresses)
  const uint32_t side_n = (uint32_t)__builtin_amdgcn_readfirstlane(sd.n_ent), side_k = (uint32_t)__builtin_amdgcn_readfirstlane(sd.cand_k);
  const int N = p.npp;
  const uint64_t gmask_all = GS == 64 ? ~0ull : (((1ull << (GS & 63)) - 1ull) << gbase);
  const I obase = i * (I)N;               // first output slot of the positive
  const bool merged = N < GS;             // the group's last lane is never a draw lane: it evaluates the coin block
  int collected = live ? 0 : N;
  for (int round = 0; round < p.max_try; ++round) {
    if (!__ballot(collected < N)) break;  // every positive of the wave is done
    const int need = N - collected;       // 0 for finished groups
    const bool active = gl < need;
    bool corrupt_head;
    uint32_t first_word = 0;
    if (merged) {
      const Philox4 ph = philox4x32_10(gi, (uint32_t)round, gl == GS - 1 ? 0xFFFFFFFFu : (uint32_t)gl, sid, p.seed_lo, p.seed_hi);
      first_word = ph.v[0];               // draw lanes: attempt 0 = word 0 of block 0 of (positive, round, slot)
      corrupt_head = ((uint32_t)__shfl((int)ph.v[0], gbase + GS - 1, 64) >> 31) != 0;
    } else {
      const Philox4 cph = philox4x32_10(gi, (uint32_t)round, 0xFFFFFFFFu, sid, p.seed_lo, p.seed_hi);
      corrupt_head = (cph.v[0] >> 31) != 0;
    }
    const int x = corrupt_head ? h : t;
    bool use_tbl = false;
    if (sd.cand_table != nullptr) use_tbl = sd.cand_valid == nullptr || (live && sd.cand_valid[x] != 0);
    const uint32_t n = use_tbl ? side_k : side_n;
    uint32_t attempt = 0;
    uint32_t pos = 0xFFFFFFFFu;
    if (active) {
      bool have = false;
      if (merged) {                       // draw_next's first iteration on the word already at hand
        attempt = 1;
        const uint64_t m = (uint64_t)first_word * (uint64_t)n;
        const uint32_t l = (uint32_t)m;
        have = true;
        if (l < n) have = l >= (0u - n) % n;
        pos = (uint32_t)(m >> 32);
      }
      if (!have) pos = draw_next(gi, (uint32_t)round, (uint32_t)gl, sid, p.seed_lo, p.seed_hi, n, attempt);
    }
    // duplicate detection among first draws (q runs to the largest `need` of the wave)
    int need_max = max(need, __shfl_xor(need, 32, 64));
    if (GS == 16) need_max = max(need_max, __shfl_xor(need_max, 16, 64));
    bool dup = false;
    tbl[gl] = 0xFFFFFFFFu;
    tbl[gl + GS] = 0xFFFFFFFFu;
    if (active) {
      uint32_t sl = (pos * 0x9E3779B1u) >> (32 - (GS == 16 ? 5 : GS == 32 ? 6 : 7));
      for (;;) {
        const uint32_t old = atomicCAS(&tbl[sl], 0xFFFFFFFFu, pos);
        if (old == 0xFFFFFFFFu) break;
        if (old == pos) { dup = true; break; }
        sl = (sl + 1) & (TS - 1);
      }
    }
    if (__ballot(dup)) {
      // sequential without-replacement semantics: slot q must differ from the final draws of slots < q
      for (int q = 1; q < need_max; ++q) {
        for (;;) {
          const uint32_t v = (uint32_t)__shfl((int)pos, gbase + q, 64);
          const bool hit = q < need && gl < q && pos == v;
          const uint64_t hb = __ballot(hit);
          if (!hb) break;
          if ((hb & gmask_all) && gl == q) pos = draw_next(gi, (uint32_t)round, (uint32_t)gl, sid, p.seed_lo, p.seed_hi, n, attempt);
        }
      }
    }
    int ent = 0;
    if (active) {
      if (use_tbl) ent = sd.cand_table[(int64_t)x * (int64_t)side_k + pos];
      else ent = sd.ent_list ? elem_at<O32>(sd.ent_list, pos) : sd.ent_lo + (int32_t)pos;
    }
    const int nh = corrupt_head ? ent : h;
    const int nt = corrupt_head ? t : ent;
    bool keep = active;
    if (active && round < p.max_try - 1 && keys != nullptr) {
      bool ask = true;
      if (filter != nullptr) {            // a clear bit among the key's three: certainly not known
        const uint32_t y = filter_mix32((uint32_t)nh, (uint32_t)r, (uint32_t)nt);
        const uint32_t m = filter_mask32(y, shift);
        ask = (elem_at<true>(filter, y >> shift) & m) == m;
      }
      if (ask) {
        const uint64_t key = triple_key((uint32_t)nh, (uint32_t)r, (uint32_t)nt);
        keep = !set_contains_hashed(keys, sd.known_capacity, key, mix64(key));
      }
    }
    const uint64_t mask = (__ballot(keep) & gmask_all) >> gbase;  // this group's kept slots
    if (keep) {
      const int rank = __popcll(mask & ((1ull << gl) - 1ull));
      const I o = obase + (I)(collected + rank);
      if constexpr (CODES) {
        // ent != x: (ent, r, t) or (h, r, ent), the one-gather form; ent == x: the positive itself, entity = its tail, no flags
        elem_at<O32>(p.nh, o) = ent != x ? (ent | (corrupt_head ? MKE_CODE_HEAD : 0) | MKE_CODE_FAST) : t;
      } else {
        elem_at<O32>(p.nh, o) = nh; elem_at<O32>(p.nr, o) = r; elem_at<O32>(p.nt, o) = nt;
      }
    }
    collected += __popcll(mask);
  }
}

template <int GS, bool CODES, bool O32>
__global__ __launch_bounds__(MKE_BLOCK) void k_neg_sample(const SampleParams p) {
  using I = std::conditional_t<O32, uint32_t, int64_t>;
  constexpr int PPW = 64 / GS;
  constexpr int TS = 2 * GS;
  __shared__ uint32_t s_dup[(MKE_BLOCK / GS) * TS];
  const int lane = threadIdx.x & 63;
  const int gl = lane & (GS - 1);        // slot inside the group
  const int gbase = lane & ~(GS - 1);    // first lane of the group
  uint32_t* tbl = s_dup + (threadIdx.x / GS) * TS;
  // a wavefront takes PPW positives at a time and strides by the grid, which the launcher caps (SAMPLE_BLOCKS_PER_CU): at C2 a
  // wavefront's work per PPW positives is about 3 us, and a wavefront launched for each left the SIMDs short of wavefronts
  const I n_waves = (I)gridDim.x * (I)(MKE_BLOCK / 64);
  const I wave0 = (I)blockIdx.x * (I)(MKE_BLOCK / 64) + (I)(uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // a scalar
  for (I wave = wave0; wave * (I)PPW < (I)p.n_pos; wave += n_waves) {
    const I i = wave * (I)PPW + (I)(lane / GS);
    const bool live = i < (I)p.n_pos;
    const I ii = live ? i : (I)0;
    // the positive's ids and its kg byte are requested together
    const int h = elem_at<O32>(p.ph, ii), r = elem_at<O32>(p.pr, ii), t = elem_at<O32>(p.pt, ii);
    const int kg = p.pos_kg ? (elem_at<O32>(p.pos_kg, ii) != 0) : 0;
    const uint32_t gi = p.pos_index ? (uint32_t)elem_at<O32>(p.pos_index, ii) : (uint32_t)ii + (uint32_t)p.pos_offset;
    const uint64_t lv = __ballot(live), k1 = __ballot(live && kg != 0);
    // one pass when the live lanes are of one KG; a mixed wavefront takes a pass per KG, the other KG's groups idle in it
    // (a group is one positive, and nothing a group computes depends on another group)
    if (k1 != lv || lv == 0) sample_rounds<GS, CODES, O32, 0, I>(p, live && kg == 0, i, h, r, t, gi, tbl, gl, gbase);
    if (k1 != 0) sample_rounds<GS, CODES, O32, 1, I>(p, live && kg == 1, i, h, r, t, gi, tbl, gl, gbase);
  }
}

// the bits of a stored key in the filter.  Both writers go by the fields as the key holds them (triple_key keeps 26 / 12 / 26
// bits), which is all that k_filter_from_table has
__device__ __forceinline__ void filter_set(uint32_t* __restrict__ filter, int shift, uint64_t key) {
  const TripleIds ids = triple_of_key(key);
  const uint32_t y = filter_mix32(ids.h, ids.r, ids.t);
  atomicOr(&filter[y >> shift], filter_mask32(y, shift));
}

__global__ __launch_bounds__(MKE_BLOCK) void k_tripleset_build(const int32_t* __restrict__ h, const int32_t* __restrict__ r,
                                                               const int32_t* __restrict__ t, int64_t n,
                                                               uint64_t* __restrict__ keys, uint64_t cap,
                                                               uint32_t* __restrict__ filter, int filter_shift) {
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = triple_key((uint32_t)h[i], (uint32_t)r[i], (uint32_t)t[i]);
  if (filter) filter_set(filter, filter_shift, key);
  uint64_t slot = mix64(key) & (cap - 1);
  for (;;) {
    const unsigned long long prev =
        atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)MKE_EMPTY_KEY, (unsigned long long)key);
    if (prev == MKE_EMPTY_KEY || prev == key) return;
    slot = (slot + 1) & (cap - 1);
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_tripleset_query(const int32_t* __restrict__ h, const int32_t* __restrict__ r,
                                                               const int32_t* __restrict__ t, int64_t n,
                                                               const uint64_t* __restrict__ keys, uint64_t cap,
                                                               uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = set_contains(keys, cap, triple_key((uint32_t)h[i], (uint32_t)r[i], (uint32_t)t[i])) ? 1 : 0;
}

// A new filter starts from what its table already holds (a table may have been filled before it had a filter).
__global__ __launch_bounds__(MKE_BLOCK) void k_filter_from_table(const uint64_t* __restrict__ keys, uint64_t cap,
                                                                 uint32_t* __restrict__ filter, int filter_shift) {
  const uint64_t i = (uint64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= cap) return;
  const uint64_t key = keys[i];
  if (key == MKE_EMPTY_KEY) return;
  filter_set(filter, filter_shift, key);
}

// ---------------------------------------------------------------------------------------------------------------
// The filters: device buffers owned by the library, found by the address of the table they belong to.
// ---------------------------------------------------------------------------------------------------------------
struct TripleFilter {
  uint64_t capacity;
  uint32_t* bits;
  int shift;      // 32 - log2(number of words)
};
constexpr TripleFilter NO_FILTER{0, nullptr, 0};
static std::mutex g_filter_mu;
static std::unordered_map<const void*, TripleFilter> g_filters;

static int filter_bits_log2(uint64_t capacity) {
  int lg = 0;
  while ((1ull << lg) < capacity) ++lg;
  lg += FILTER_BITS_PER_SLOT_LOG2;
  return lg < FILTER_MIN_BITS_LOG2 ? FILTER_MIN_BITS_LOG2 : (lg > FILTER_MAX_BITS_LOG2 ? FILTER_MAX_BITS_LOG2 : lg);
}

// The filter of (keys, capacity) for a launch that only reads it; NO_FILTER when the set has none (or keys is NULL).
static TripleFilter filter_lookup(const uint64_t* keys, uint64_t capacity) {
  if (!keys) return NO_FILTER;
  std::lock_guard<std::mutex> lk(g_filter_mu);
  const auto it = g_filters.find(keys);
  if (it == g_filters.end() || it->second.capacity != capacity) return NO_FILTER;
  return it->second;
}

static void filter_forget(const void* keys) {
  std::lock_guard<std::mutex> lk(g_filter_mu);
  const auto it = g_filters.find(keys);
  if (it == g_filters.end()) return;
  (void)hipFree(it->second.bits);   // waits for the device: no launch that reads the bits is still running
  g_filters.erase(it);
}

// The filter mke_tripleset_build is about to add to; created (zeroed, then filled from the table as it stands, both on
// `st`) when the table has none.  An entry of another capacity at this address belongs to a set that is gone.
static int filter_for_build(uint64_t* keys, uint64_t capacity, hipStream_t st, TripleFilter* out) {
  std::lock_guard<std::mutex> lk(g_filter_mu);
  auto it = g_filters.find(keys);
  if (it != g_filters.end() && it->second.capacity != capacity) {
    (void)hipFree(it->second.bits);
    g_filters.erase(it);
    it = g_filters.end();
  }
  if (it != g_filters.end()) { *out = it->second; return MKE_OK; }
  const int lg = filter_bits_log2(capacity);
  const size_t bytes = (size_t)1 << (lg - 3);
  // the buffer lives on the table's device, whichever device is current
  int cur = 0, dev = 0;
  hipPointerAttribute_t attr;
  if (hipGetDevice(&cur) != hipSuccess) { set_error("mke_tripleset_build: no device"); return MKE_E_NULL; }
  dev = cur;
  if (hipPointerGetAttributes(&attr, keys) == hipSuccess) dev = attr.device; else (void)hipGetLastError();
  TripleFilter f{capacity, nullptr, 32 - (lg - 5)};
  if (dev != cur) (void)hipSetDevice(dev);
  hipError_t e = hipMalloc((void**)&f.bits, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(f.bits, 0, bytes, st);
  if (dev != cur) (void)hipSetDevice(cur);
  if (e != hipSuccess) {
    if (f.bits) (void)hipFree(f.bits);
    set_error("mke_tripleset_build: filter allocation (%zu bytes): %s", bytes, hipGetErrorString(e));
    return (int)e;
  }
  const uint64_t blocks = (capacity + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_filter_from_table, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, st, keys, capacity, f.bits, f.shift);
  const int rc = check_launch("k_filter_from_table");
  if (rc) { (void)hipFree(f.bits); return rc; }
  g_filters.emplace(keys, f);
  *out = f;
  return MKE_OK;
}

int validate_side(const mke_kg_side& sd, int neg_per_pos) {
  // random.sample raises ValueError when the population is smaller than the sample (batch.py:98,101)
  if (sd.n_ent < neg_per_pos) { set_error("candidate population (%d) smaller than neg_per_pos (%d)", sd.n_ent, neg_per_pos); return MKE_E_SHAPE; }
  if (sd.cand_table && sd.cand_k < neg_per_pos) { set_error("neighbour list (%d) shorter than neg_per_pos (%d)", sd.cand_k, neg_per_pos); return MKE_E_SHAPE; }
  if (sd.known_keys && (sd.known_capacity == 0 || (sd.known_capacity & (sd.known_capacity - 1)) != 0)) { set_error("known_capacity must be a power of two"); return MKE_E_SHAPE; }
  return MKE_OK;
}

// SAMPLE_BLOCKS_PER_CU workgroups for every CU of the current device.
static int64_t resident_blocks() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 2048; }
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    cus[dev] = n;
  }
  return (int64_t)cus[dev] * SAMPLE_BLOCKS_PER_CU;
}

// k_neg_sample<GS, CODES, O32> by [GS = 16, 32, 64][CODES][O32]
using SampleKernel = void (*)(const SampleParams);
template <int GS>
constexpr std::array<std::array<SampleKernel, 2>, 2> sample_kernels_of{{{k_neg_sample<GS, false, false>, k_neg_sample<GS, false, true>},
                                                                       {k_neg_sample<GS, true, false>, k_neg_sample<GS, true, true>}}};

int launch_neg_sample(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, int64_t n_pos, int64_t pos_offset,
                      const int32_t* pos_index,
                      const uint8_t* pos_kg, const mke_kg_side* sides, int neg_per_pos, int max_try, uint32_t seed_lo,
                      uint32_t seed_hi, uint32_t stream_id, int32_t* neg_h, int32_t* neg_r, int32_t* neg_t, hipStream_t st,
                      bool codes /* neg_h takes one code word per negative, neg_r / neg_t are not used */) {
  SampleParams p = {};
  p.ph = pos_h; p.pr = pos_r; p.pt = pos_t; p.pos_kg = pos_kg; p.n_pos = n_pos; p.pos_offset = pos_offset; p.pos_index = pos_index;
  p.npp = neg_per_pos; p.max_try = max_try;
  p.side[0] = sides[0];
  p.side[1] = pos_kg ? sides[1] : sides[0];
  for (int k = 0; k < 2; ++k) {       // a set without a filter (or with one of another capacity) is probed directly
    const TripleFilter f = filter_lookup(p.side[k].known_keys, p.side[k].known_capacity);
    p.filter[k] = f.bits;
    p.shift[k] = f.shift;
  }
  p.seed_lo = seed_lo; p.seed_hi = seed_hi; p.sid = stream_id;
  p.nh = neg_h; p.nr = neg_r; p.nt = neg_t;
  // lanes per positive: 16 (four positives per wavefront), 32, 64
  const int gs = neg_per_pos <= 15 ? 16 : (neg_per_pos <= 32 ? 32 : 64);
  const int64_t pos_per_block = (MKE_BLOCK / 64) * (64 / gs);
  int64_t blocks = (n_pos + pos_per_block - 1) / pos_per_block;
  const int64_t resident = resident_blocks();
  if (blocks > resident) blocks = resident;   // the kernel strides by its grid
  const bool o32 = sampler_o32_fits(n_pos, neg_per_pos, p.side[0].n_ent, p.side[1].n_ent);
  const auto& kernels = gs == 16 ? sample_kernels_of<16> : (gs == 32 ? sample_kernels_of<32> : sample_kernels_of<64>);
  hipLaunchKernelGGL(kernels[codes][o32], dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("k_neg_sample");
}

// ---------------------------------------------------------------------------------------------------------------
// random.sample(list, batch) for every step of an epoch in one launch (code/MultiKE_model.py:358,380,402,425,446: the
// cross-KG inference and common-space loops draw `batch` distinct list positions per step, independently per step).
// out[s * batch + i] = pi_s(i), pi_s a keyed pseudo-random permutation of [0, n): a 6-round Feistel network over the
// smallest even-width power-of-two domain >= n, cycle-walked back into [0, n) (Black & Rogaway 2002).  Distinct
// inputs give distinct outputs by construction, so no dedupe pass and no n-sized shuffle per step is needed.
// Round keys: Philox4x32-10 of (step, block 0/1, 0x5A4D504C, stream_id) under (seed_lo, seed_hi).
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t feistel_round_fn(uint32_t x, uint32_t key) {
  x = x * 0x9E3779B1u + key;
  x ^= x >> 15; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(MKE_BLOCK) void k_sample_distinct(uint32_t n, int batch, int n_steps, uint32_t seed_lo, uint32_t seed_hi,
                                                               uint32_t stream_id, int half_bits, int32_t* __restrict__ out) {
  const int step = blockIdx.y;
  const Philox4 ka = philox4x32_10((uint32_t)step, 0u, 0x5A4D504Cu, stream_id, seed_lo, seed_hi);
  const Philox4 kb = philox4x32_10((uint32_t)step, 1u, 0x5A4D504Cu, stream_id, seed_lo, seed_hi);
  const uint32_t keys[6] = {ka.v[0], ka.v[1], ka.v[2], ka.v[3], kb.v[0], kb.v[1]};
  const uint32_t mask = (1u << half_bits) - 1u;
  for (int i = blockIdx.x * MKE_BLOCK + threadIdx.x; i < batch; i += gridDim.x * MKE_BLOCK) {
    uint32_t x = (uint32_t)i;
    do {
      uint32_t l = x >> half_bits, r = x & mask;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const uint32_t t = l ^ (feistel_round_fn(r, keys[k]) & mask);
        l = r;
        r = t;
      }
      x = (l << half_bits) | r;
    } while (x >= n);
    out[(int64_t)step * batch + i] = (int32_t)x;
  }
}

}  // namespace mke

static int neg_sample_checked(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, int64_t n_pos, int64_t pos_offset,
                              const int32_t* pos_index, const uint8_t* pos_kg, const mke_kg_side* sides, int neg_per_pos, int max_try,
                              uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id, int32_t* neg_h, int32_t* neg_r, int32_t* neg_t,
                              void* stream) {
  using namespace mke;
  if (n_pos < 0) { set_error("negative n_pos"); return MKE_E_SHAPE; }
  if (n_pos == 0 || neg_per_pos == 0) return MKE_OK;
  // neg_r == neg_t == NULL: the code-word form, one word per negative into neg_h (multike_hip.h, section (1c))
  const bool codes = neg_h && !neg_r && !neg_t;
  if (!pos_h || !pos_r || !pos_t || !neg_h || (!codes && (!neg_r || !neg_t)) || !sides) { set_error("mke_neg_sample: NULL pointer"); return MKE_E_NULL; }
  for (int k = 0; codes && k < (pos_kg ? 2 : 1); ++k)   // a word holds MKE_CODE_ENT_BITS of entity (ids of lists are the caller's to keep below)
    if (!sides[k].ent_list && (sides[k].ent_lo < 0 || (int64_t)sides[k].ent_lo + sides[k].n_ent > (1ll << MKE_CODE_ENT_BITS))) {
      set_error("mke_neg_sample: code words hold entity ids below 2^%d, side %d draws up to %lld", MKE_CODE_ENT_BITS, k, (long long)sides[k].ent_lo + sides[k].n_ent);
      return MKE_E_RANGE;
    }
  if (neg_per_pos < 0 || neg_per_pos > 64) { set_error("neg_per_pos must be in [0,64], got %d", neg_per_pos); return MKE_E_UNSUPPORTED; }
  if (max_try < 1 || max_try > 255) { set_error("max_try must be in [1,255]"); return MKE_E_SHAPE; }
  for (int k = 0; k < (pos_kg ? 2 : 1); ++k) {
    const int rc = validate_side(sides[k], neg_per_pos);
    if (rc) return rc;
  }
  return launch_neg_sample(pos_h, pos_r, pos_t, n_pos, pos_offset, pos_index, pos_kg, sides, neg_per_pos, max_try, seed_lo, seed_hi,
                           stream_id, neg_h, neg_r, neg_t, (hipStream_t)stream, codes);
}

extern "C" int mke_neg_sample(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, int64_t n_pos,
                              int64_t pos_offset, const uint8_t* pos_kg, const mke_kg_side* sides, int neg_per_pos,
                              int max_try, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id, int32_t* neg_h,
                              int32_t* neg_r, int32_t* neg_t, void* stream) {
  return neg_sample_checked(pos_h, pos_r, pos_t, n_pos, pos_offset, nullptr, pos_kg, sides, neg_per_pos, max_try, seed_lo, seed_hi,
                            stream_id, neg_h, neg_r, neg_t, stream);
}

extern "C" int mke_neg_sample_at(const int32_t* pos_h, const int32_t* pos_r, const int32_t* pos_t, int64_t n_pos,
                                 const int32_t* pos_index, const uint8_t* pos_kg, const mke_kg_side* sides, int neg_per_pos,
                                 int max_try, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id, int32_t* neg_h,
                                 int32_t* neg_r, int32_t* neg_t, void* stream) {
  if (n_pos > 0 && !pos_index) { mke::set_error("mke_neg_sample_at: NULL pos_index"); return MKE_E_NULL; }
  return neg_sample_checked(pos_h, pos_r, pos_t, n_pos, 0, pos_index, pos_kg, sides, neg_per_pos, max_try, seed_lo, seed_hi,
                            stream_id, neg_h, neg_r, neg_t, stream);
}

extern "C" int mke_tripleset_build(const int32_t* h, const int32_t* r, const int32_t* t, int64_t n, uint64_t* keys,
                                   uint64_t capacity, void* stream) {
  using namespace mke;
  if (n < 0) { set_error("negative n"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!h || !r || !t || !keys) { set_error("mke_tripleset_build: NULL pointer"); return MKE_E_NULL; }
  if (capacity == 0 || (capacity & (capacity - 1)) != 0 || capacity < (uint64_t)n + 1) {
    set_error("capacity must be a power of two > n");
    return MKE_E_SHAPE;
  }
  TripleFilter f;
  const int rc = filter_for_build(keys, capacity, (hipStream_t)stream, &f);
  if (rc) return rc;
  const int64_t blocks = (n + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_tripleset_build, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, h, r, t, n,
                     keys, capacity, f.bits, f.shift);
  return check_launch("k_tripleset_build");
}

extern "C" int64_t mke_tripleset_filter_bytes(const uint64_t* keys, uint64_t capacity) {
  const mke::TripleFilter f = mke::filter_lookup(keys, capacity);
  return f.bits ? (int64_t)sizeof(uint32_t) << (32 - f.shift) : 0;
}

extern "C" int mke_tripleset_forget(const uint64_t* keys) {
  if (keys) mke::filter_forget(keys);
  return MKE_OK;
}

extern "C" int mke_tripleset_query(const int32_t* h, const int32_t* r, const int32_t* t, int64_t n,
                                   const uint64_t* keys, uint64_t capacity, uint8_t* out, void* stream) {
  using namespace mke;
  if (n < 0) { set_error("negative n"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!h || !r || !t || !keys || !out) { set_error("mke_tripleset_query: NULL pointer"); return MKE_E_NULL; }
  if (capacity == 0 || (capacity & (capacity - 1)) != 0) { set_error("capacity must be a power of two"); return MKE_E_SHAPE; }
  const int64_t blocks = (n + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_tripleset_query, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, h, r, t, n,
                     keys, capacity, out);
  return check_launch("k_tripleset_query");
}

extern "C" int mke_sample_distinct(int64_t n, int batch, int n_steps, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id,
                                   int32_t* out, void* stream) {
  using namespace mke;
  if (n < 0 || batch < 0 || n_steps < 0 || n > 0x7FFFFFFFLL || (int64_t)batch > n) { set_error("mke_sample_distinct: need 0 <= batch <= n < 2^31 (n=%lld batch=%d)", (long long)n, batch); return MKE_E_SHAPE; }
  if (batch == 0 || n_steps == 0) return MKE_OK;
  if (!out) { set_error("mke_sample_distinct: NULL output"); return MKE_E_NULL; }
  if (n_steps > 65535) { set_error("mke_sample_distinct: more than 65535 steps"); return MKE_E_SHAPE; }
  int half = 1;
  while ((1ll << (2 * half)) < n) ++half;   // domain 4^half >= n, < 4n
  int bx = (batch + MKE_BLOCK - 1) / MKE_BLOCK;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(k_sample_distinct, dim3(bx, n_steps), dim3(MKE_BLOCK), 0, (hipStream_t)stream, (uint32_t)n, batch, n_steps, seed_lo,
                     seed_hi, stream_id, half, out);
  return check_launch("k_sample_distinct");
}
