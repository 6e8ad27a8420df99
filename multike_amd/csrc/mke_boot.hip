// mke_boot.hip — self-training (bootstrapping) support on gfx950: a decoder's pairs become a link table, and a link table
// becomes 'swapping' supervision triples, both in HBM.
//
//   mke_boot_partner  partner[e] = the entity e is paired with, or -1: the table is filled with -1 (one memset) and every
//                     matched row writes its two entries.  The pairing is one-to-one and the ids of a side are distinct, so no
//                     two threads write one word.
//   mke_swap_triples  the swapping of code/base/read.py:130-164 (base/kgs.py swap_relation_triples / swap_attribute_triples) as
//                     an ORDERED stream compaction: triple k emits (partner[h], p, t) when its head is linked and then, unless
//                     heads_only, (h, p, partner[t]) when its tail is; the output holds the entries in the order of that walk.
//
// The compaction in three steps, none of which moves a cursor with atomics (the order of the output, and so the bits of every
// later sampling from it, never depends on which block ran first):
//   1. k_swap_count   a wavefront owns MKE_SWAP_TILE = 64 consecutive triples, one per lane; the two predicates become two
//                     64-bit ballots and lane 0 stores popc(heads) + popc(tails), the tile's number of entries (<= 128).
//   2. hipcub::DeviceScan::ExclusiveSum over the tile counts (int64: the total may pass 2^31) -> each tile's first position.
//                     The counts carry one extra 0 at the end whose scanned value is the total: count[0] is a copy of it.
//   3. k_swap_emit    re-reads the tile, rebuilds the ballots and stores a lane's entries at
//                         tile offset + popc(heads below the lane) + popc(tails below the lane)      (head form)
//                         ... + 1 when the head form was emitted                                    (tail form)
//                     which is the walk's order inside the tile: the entries of the lanes below come first, a triple's head
//                     form precedes its tail form.  Positions >= capacity are not stored.
// The gathers partner[h], partner[t] are made twice (count and emit) instead of carrying 2 bits per triple between the
// launches: the table is the hot data of both launches and the triples stream through once each.
#include "mke_common.h"

#include <hipcub/hipcub.hpp>

namespace mke {

static_assert(MKE_SWAP_TILE == 64, "a tile is one wavefront: one triple per lane, two 64-bit ballots");
static_assert(MKE_BLOCK % MKE_SWAP_TILE == 0, "whole tiles per workgroup");

struct PartnerParams {
  const int32_t* __restrict__ match;  // [n_a]
  const int32_t* __restrict__ ids_a;  // [n_a]
  const int32_t* __restrict__ ids_b;  // [n_b]
  int32_t* partner;                   // [n_entities]
  int n_a, n_b;
  int64_t n_entities;
};

__global__ void __launch_bounds__(MKE_BLOCK) k_boot_partner(PartnerParams p) {
  for (int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; i < p.n_a; i += (int64_t)gridDim.x * MKE_BLOCK) {
    const int m = p.match[i];
    if (m < 0 || m >= p.n_b) continue;
    const int64_t a = p.ids_a[i], b = p.ids_b[m];
    if (a < 0 || a >= p.n_entities || b < 0 || b >= p.n_entities) continue;  // a pair with an id outside the table is no link
    p.partner[a] = (int32_t)b;
    p.partner[b] = (int32_t)a;
  }
}

struct SwapParams {
  const int32_t* __restrict__ h;
  const int32_t* __restrict__ p;
  const int32_t* __restrict__ t;
  int64_t n;
  const int32_t* __restrict__ partner;
  int64_t n_entities;
  const float* __restrict__ weight;
  int heads_only;
  int32_t* out_h;
  int32_t* out_p;
  int32_t* out_t;
  float* out_w;
  int64_t capacity;
  int64_t n_tiles;    // ceil(n / MKE_SWAP_TILE)
  int64_t* tile_cnt;  // [n_tiles + 1], the last one 0
  int64_t* tile_off;  // [n_tiles + 1], the last one the total
};

// the counterpart of entity e, or -1 (an id outside the table is unlinked)
__device__ __forceinline__ int linked(const SwapParams& s, int e) {
  return (e >= 0 && (int64_t)e < s.n_entities) ? s.partner[e] : -1;
}

// Triple k of the calling lane: its ids, the counterparts of its two ends (-1 = none) and the wavefront's two ballots.
struct SwapLane {
  int h, t, ph, pt;
  unsigned long long heads, tails;
};

__device__ __forceinline__ SwapLane swap_lane(const SwapParams& s, int64_t k) {
  SwapLane l;
  l.h = l.t = l.ph = l.pt = -1;
  if (k < s.n) {
    l.h = s.h[k];
    l.t = s.t[k];
    l.ph = linked(s, l.h);
    if (!s.heads_only) l.pt = linked(s, l.t);  // heads_only: the third column is a value id, never looked up
  }
  l.heads = __ballot(l.ph >= 0);  // every lane of the wavefront is here: no lane has left the kernel
  l.tails = __ballot(l.pt >= 0);
  return l;
}

__global__ void __launch_bounds__(MKE_BLOCK) k_swap_count(SwapParams s) {
  const int64_t k = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  const int64_t tile = k / MKE_SWAP_TILE;
  const SwapLane l = swap_lane(s, k);
  if ((threadIdx.x & (MKE_SWAP_TILE - 1)) == 0 && tile <= s.n_tiles)  // tile n_tiles holds no triple: the scan's extra 0
    s.tile_cnt[tile] = (int64_t)(__popcll(l.heads) + __popcll(l.tails));
}

__global__ void __launch_bounds__(MKE_BLOCK) k_swap_emit(SwapParams s) {
  const int64_t k = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  const int64_t tile = k / MKE_SWAP_TILE;
  const SwapLane l = swap_lane(s, k);
  if (k >= s.n || (l.ph < 0 && l.pt < 0)) return;
  const unsigned long long below = (1ull << (threadIdx.x & (MKE_SWAP_TILE - 1))) - 1ull;
  int64_t pos = s.tile_off[tile] + __popcll(l.heads & below) + __popcll(l.tails & below);
  const int pred = s.p[k];
  if (l.ph >= 0) {
    if (pos < s.capacity) {
      s.out_h[pos] = l.ph;
      s.out_p[pos] = pred;
      s.out_t[pos] = l.t;
      if (s.weight) s.out_w[pos] = s.weight[l.h];
    }
    ++pos;
  }
  if (l.pt >= 0 && pos < s.capacity) {
    s.out_h[pos] = l.h;
    s.out_p[pos] = pred;
    s.out_t[pos] = l.pt;
    if (s.weight) s.out_w[pos] = s.weight[l.t];
  }
}

constexpr int64_t kSwapAlign = 256;

static int64_t swap_scan_bytes(int64_t items) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, (int)items, (hipStream_t)0);
  return ((int64_t)b + kSwapAlign - 1) / kSwapAlign * kSwapAlign;
}

}  // namespace mke

extern "C" int mke_boot_partner(const int32_t* match, const int32_t* ids_a, int64_t n_a, const int32_t* ids_b, int64_t n_b,
                                int32_t* partner, int64_t n_entities, void* stream) {
  using namespace mke;
  if (n_a < 0 || n_b < 0 || n_a > 0x7FFFFF00LL || n_b > 0x7FFFFF00LL) { set_error("mke_boot_partner: bad n_a / n_b"); return MKE_E_SHAPE; }
  if (n_entities < 0 || n_entities > 0x7FFFFFFFLL) { set_error("mke_boot_partner: n_entities must be in [0, 2^31)"); return MKE_E_SHAPE; }
  const bool pairs = n_a > 0 && n_b > 0;
  if ((n_entities > 0 && !partner) || (pairs && (!match || !ids_a || !ids_b))) { set_error("mke_boot_partner: NULL pointer"); return MKE_E_NULL; }
  if (n_entities == 0) return MKE_OK;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(partner, 0xFF, (size_t)n_entities * sizeof(int32_t), st);  // every byte 0xFF: -1
  if (e != hipSuccess) { set_error("mke_boot_partner: memset: %s", hipGetErrorString(e)); return (int)e; }
  if (!pairs) return MKE_OK;
  PartnerParams p = {match, ids_a, ids_b, partner, (int)n_a, (int)n_b, n_entities};
  const int64_t blocks = (n_a + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_boot_partner, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(MKE_BLOCK), 0, st, p);
  return check_launch("mke_boot_partner: k_boot_partner");
}

extern "C" int64_t mke_swap_temp_bytes(int64_t n) {
  using namespace mke;
  if (n < 0 || n > 0x7FFFFFFFLL) { set_error("mke_swap_temp_bytes: n must be in [0, 2^31)"); return MKE_E_SHAPE; }
  const int64_t items = (n + MKE_SWAP_TILE - 1) / MKE_SWAP_TILE + 1;
  return swap_scan_bytes(items) + 2 * ((items * (int64_t)sizeof(int64_t) + kSwapAlign - 1) / kSwapAlign * kSwapAlign);
}

extern "C" int mke_swap_triples(const mke_swap_args* args, void* stream) {
  using namespace mke;
  if (!args) { set_error("mke_swap_triples: NULL args"); return MKE_E_NULL; }
  const mke_swap_args& a = *args;
  if (a.flags != 0) { set_error("mke_swap_triples: unknown flags %d", a.flags); return MKE_E_UNSUPPORTED; }
  if (a.heads_only != 0 && a.heads_only != 1) { set_error("mke_swap_triples: heads_only must be 0 or 1, got %d", a.heads_only); return MKE_E_UNSUPPORTED; }
  if (a.n < 0 || a.n > 0x7FFFFFFFLL) { set_error("mke_swap_triples: n must be in [0, 2^31)"); return MKE_E_SHAPE; }
  if (a.capacity < 0) { set_error("mke_swap_triples: capacity < 0"); return MKE_E_SHAPE; }
  if (a.n_entities < 0 || a.n_entities > 0x7FFFFFFFLL) { set_error("mke_swap_triples: n_entities must be in [0, 2^31)"); return MKE_E_SHAPE; }
  if ((a.weight == nullptr) != (a.out_w == nullptr)) { set_error("mke_swap_triples: weight and out_w are both NULL or both set"); return MKE_E_NULL; }
  if (!a.count) { set_error("mke_swap_triples: NULL pointer (count)"); return MKE_E_NULL; }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (a.n == 0) {  // nothing to walk: no launch, count[0] = 0 by a memset on the stream
    if ((e = hipMemsetAsync(a.count, 0, sizeof(int64_t), st)) != hipSuccess) { set_error("mke_swap_triples: memset: %s", hipGetErrorString(e)); return (int)e; }
    return MKE_OK;
  }
  if (!a.h || !a.p || !a.t || (a.n_entities > 0 && !a.partner) || !a.temp || (a.capacity > 0 && (!a.out_h || !a.out_p || !a.out_t))) {
    set_error("mke_swap_triples: NULL pointer");
    return MKE_E_NULL;
  }
  if (a.temp_bytes < mke_swap_temp_bytes(a.n)) { set_error("mke_swap_triples: temp_bytes %lld below mke_swap_temp_bytes", (long long)a.temp_bytes); return MKE_E_SHAPE; }
  if (((uintptr_t)a.temp & 7u) != 0) { set_error("mke_swap_triples: temp must be 8-byte aligned"); return MKE_E_SHAPE; }
  SwapParams s = {};
  s.h = a.h; s.p = a.p; s.t = a.t; s.n = a.n; s.partner = a.partner; s.n_entities = a.n_entities; s.weight = a.weight;
  s.heads_only = a.heads_only; s.out_h = a.out_h; s.out_p = a.out_p; s.out_t = a.out_t; s.out_w = a.out_w; s.capacity = a.capacity;
  s.n_tiles = (a.n + MKE_SWAP_TILE - 1) / MKE_SWAP_TILE;
  const int64_t items = s.n_tiles + 1;
  const int64_t scan_bytes = swap_scan_bytes(items);
  const int64_t list_bytes = (items * (int64_t)sizeof(int64_t) + kSwapAlign - 1) / kSwapAlign * kSwapAlign;
  char* base = (char*)a.temp;
  s.tile_cnt = (int64_t*)(base + scan_bytes);
  s.tile_off = (int64_t*)(base + scan_bytes + list_bytes);
  // the count launch covers tile n_tiles as well (its wavefront holds no triple and stores the 0)
  const unsigned count_blocks = (unsigned)((items * MKE_SWAP_TILE + MKE_BLOCK - 1) / MKE_BLOCK);
  const unsigned emit_blocks = (unsigned)((a.n + MKE_BLOCK - 1) / MKE_BLOCK);
  hipLaunchKernelGGL(k_swap_count, dim3(count_blocks), dim3(MKE_BLOCK), 0, st, s);
  int rc = check_launch("mke_swap_triples: k_swap_count");
  if (rc != MKE_OK) return rc;
  size_t tb = (size_t)scan_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(a.temp, tb, (const int64_t*)s.tile_cnt, s.tile_off, (int)items, st)) != hipSuccess) {
    set_error("mke_swap_triples: scan: %s", hipGetErrorString(e));
    return (int)e;
  }
  if ((e = hipMemcpyAsync(a.count, s.tile_off + s.n_tiles, sizeof(int64_t), hipMemcpyDeviceToDevice, st)) != hipSuccess) {
    set_error("mke_swap_triples: copy of the count: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (a.capacity == 0) return MKE_OK;  // the caller asked for the count alone
  hipLaunchKernelGGL(k_swap_emit, dim3(emit_blocks), dim3(MKE_BLOCK), 0, st, s);
  return check_launch("mke_swap_triples: k_swap_emit");
}
