/* CPU ORACLE — test infrastructure, NOT product code.
 *
 * Plain-C restatement of the MultiKE relation-view hot path, used (a) by tests/ as a fast checker at full
 * batch sizes and (b) by bench.py's `cpu_baseline` leg (kind "port", 1 thread).  Nothing under
 * multike_amd/ links or loads this.  It restates, from the reference's semantics:
 *   - code/losses.py:4-12,30-34,44-50           logistic losses over translation scores
 *   - code/base/initializers.py:26              normalise-on-read (tf.nn.l2_normalize, eps 1e-12)
 *   - code/MultiKE_model.py:15-31,122-131       per-graph AdagradOptimizer (acc0 = 0.1, no eps), dense apply
 *   - code/base/batch.py:86-116                 generate_neg_triples_fast, on the Philox stream specified in
 *                                               oracle/sampler_oracle.py (which is the pinned statement)
 * Pinning: checked against oracle/multike_oracle.py (NumPy) and through it against the golden fixtures made
 * from the reference's own losses.py / base/batch.py (tests/test_oracle_golden.py, tests/test_oracle_c.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define MKO_L2_EPS 1e-12
#define MKO_MAX_DIM 512

#define REAL float
#define SUF f32
#include "mke_oracle_impl.h"
#undef REAL
#undef SUF

#define REAL double
#define SUF f64
#include "mke_oracle_impl.h"
#undef REAL
#undef SUF

/* ---------------- Philox4x32-10 + sampler (spec: oracle/sampler_oracle.py philox_negatives) ------------- */
static inline void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static inline uint32_t draw_next(uint32_t gi, uint32_t rnd, uint32_t slot, uint32_t sid, uint32_t k0, uint32_t k1,
                                 uint32_t n, uint32_t* attempt) {
  for (;;) {
    uint32_t o[4];
    philox(gi, rnd | ((*attempt >> 2) << 8), slot, sid, k0, k1, o);
    const uint32_t x = o[*attempt & 3u];
    ++*attempt;
    const uint64_t m = (uint64_t)x * n;
    const uint32_t l = (uint32_t)m;
    if (l < n && l < (0u - n) % n) continue;
    return (uint32_t)(m >> 32);
  }
}

static inline uint64_t tkey(uint32_t h, uint32_t r, uint32_t t) { return ((uint64_t)h << 38) | ((uint64_t)t << 12) | r; }
static inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}

/* threads used by mko_neg_sample (positives are independent; the output does not depend on it).  1 unless bench.py's
 * cpu_baseline leg raises it. */
static int mko_threads = 1;
void mko_set_threads(int n) { mko_threads = n > 0 ? n : 1; }

/* known-triple set: open addressing; keys pre-filled with 0xFF by the caller */
void mko_set_insert(const int32_t* h, const int32_t* r, const int32_t* t, int64_t n, uint64_t* keys, uint64_t cap) {
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t k = tkey((uint32_t)h[i], (uint32_t)r[i], (uint32_t)t[i]);
    uint64_t s = mix64(k) & (cap - 1);
    while (keys[s] != ~0ull && keys[s] != k) s = (s + 1) & (cap - 1);
    keys[s] = k;
  }
}
static inline int set_has(const uint64_t* keys, uint64_t cap, uint64_t k) {
  uint64_t s = mix64(k) & (cap - 1);
  for (;;) {
    if (keys[s] == k) return 1;
    if (keys[s] == ~0ull) return 0;
    s = (s + 1) & (cap - 1);
  }
}

/* positive i is stream position pos_index[i] (the device's mke_neg_sample_at), or pos_offset + i when pos_index is NULL */
int mko_neg_sample_at(const int32_t* ph, const int32_t* pr, const int32_t* pt, int64_t n_pos, int64_t pos_offset,
                      const int32_t* pos_index, int want, int max_try, const int32_t* ent_list, int32_t ent_lo, int32_t n_all,
                      const int32_t* cand_table, const uint8_t* cand_valid, int32_t cand_k, const uint64_t* keys, uint64_t cap,
                      uint32_t k0, uint32_t k1, uint32_t sid, int32_t* nh, int32_t* nr, int32_t* nt) {
  if (want > 64) return -1;
#pragma omp parallel for schedule(static) num_threads(mko_threads > 0 ? mko_threads : 1)
  for (int64_t i = 0; i < n_pos; ++i) {
    uint32_t fin[64];
    const int32_t h = ph[i], r = pr[i], t = pt[i];
    const uint32_t gi = pos_index ? (uint32_t)pos_index[i] : (uint32_t)(i + pos_offset);
    int got = 0;
    for (int rnd = 0; rnd < max_try && got < want; ++rnd) {
      const int need = want - got;
      uint32_t o[4];
      philox(gi, (uint32_t)rnd, 0xFFFFFFFFu, sid, k0, k1, o);
      const int coin = (int)(o[0] >> 31);
      const int32_t x = coin ? h : t;
      const int use_tbl = cand_table && (!cand_valid || cand_valid[x]);
      const uint32_t n = use_tbl ? (uint32_t)cand_k : (uint32_t)n_all;
      for (int q = 0; q < need; ++q) {
        uint32_t attempt = 0, p;
        for (;;) {
          p = draw_next(gi, (uint32_t)rnd, (uint32_t)q, sid, k0, k1, n, &attempt);
          int clash = 0;
          for (int z = 0; z < q; ++z) clash |= fin[z] == p;
          if (!clash) break;
        }
        fin[q] = p;
      }
      for (int q = 0; q < need; ++q) {
        const int32_t e = use_tbl ? cand_table[(int64_t)x * cand_k + fin[q]] : (ent_list ? ent_list[fin[q]] : ent_lo + (int32_t)fin[q]);
        const int32_t a = coin ? e : h, b = coin ? t : e;
        if (rnd < max_try - 1 && keys && set_has(keys, cap, tkey((uint32_t)a, (uint32_t)r, (uint32_t)b))) continue;
        const int64_t w = i * want + got++;
        nh[w] = a; nr[w] = r; nt[w] = b;
      }
    }
  }
  return 0;
}

int mko_neg_sample(const int32_t* ph, const int32_t* pr, const int32_t* pt, int64_t n_pos, int64_t pos_offset, int want,
                   int max_try, const int32_t* ent_list, int32_t ent_lo, int32_t n_all, const int32_t* cand_table,
                   const uint8_t* cand_valid, int32_t cand_k, const uint64_t* keys, uint64_t cap, uint32_t k0,
                   uint32_t k1, uint32_t sid, int32_t* nh, int32_t* nr, int32_t* nt) {
  return mko_neg_sample_at(ph, pr, pt, n_pos, pos_offset, NULL, want, max_try, ent_list, ent_lo, n_all, cand_table, cand_valid,
                           cand_k, keys, cap, k0, k1, sid, nh, nr, nt);
}
