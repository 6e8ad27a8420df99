/*
 * multike_keyed.h — C-ABI of libmultike_keyed.so: matrix-free exact neighbour selection for capped tables at large k (gfx950).
 *
 * A third library beside libmultike_hip.so (include/multike_hip.h) and libmultike_thin.so (include/multike_thin.h); both stay
 * exactly as they are.  The boundary contract is theirs: extern "C", DEVICE pointers owned by the caller, the library never
 * allocates, frees or synchronises, an entry point only enqueues kernels on the given hipStream_t (void*; NULL = the legacy
 * default stream); return value 0 = ok, < 0 = bad argument (MKE_KEYED_E_*: the values of multike_hip.h's MKE_E_*), > 0 = a
 * hipError_t from the launch; mke_keyed_last_error() returns a thread-local human-readable message for the last non-zero
 * return of THIS library.
 *
 * Row e of a capped neighbour table is the m entities of e's exact top-k set with the smallest key(seed, e, neighbour)
 * (multike_thin.h).  All arithmetic of the key is on uint64 with wrap-around:
 *     mix(x):          x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31; return x
 *     key(seed, a, b) = mix(mix(seed + 0x9E3779B97F4A7C15 * (uint64(a) + 1)) ^ uint64(uint32(b)))
 * A neighbour's key does not depend on its similarity, so a sweep that knows the key drops the neighbours that cannot be among
 * the m smallest as it finds them and only COUNTS them: the k-wide list never exists.
 *
 *   mke_sim_select_keyed: the sweep.  Rows [row_lo, row_hi) of emb ([n_cols][ld] row-major, columns >= dim zero up to kpad)
 *     against all n_cols columns (= rows 0 .. n_cols-1 of emb); s = emb[i] . emb[j] is the k-ordered fma chain of mke_sim_select.
 *     tau_lo[i - row_lo] <= tau_hi[i - row_lo] are the row's thresholds, col_ids[j] the (non-negative) entity id of working row /
 *     column j; row i is keyed by col_ids[i].  The columns' tiles are split into n_seg equal segments of seg_cap slots each.
 *       sure:  s > tau_hi.            Always counted in seg_sure[i - row_lo][seg]; stored iff key(seed, col_ids[i], col_ids[j]) < key_below.
 *       band:  tau_lo < s <= tau_hi.  Always stored.
 *       everything else (NaN included) is ignored.
 *     Stored entries are (column j, s) pairs, in column order inside their segment; seg_count[i - row_lo][seg] is the number of
 *     entries that should have been stored — it may exceed seg_cap, only the first seg_cap are kept.  Slots are assigned by wave
 *     ballots: no atomic decides a position, the same arguments give the same bytes.
 *     Errors, before any launch: a bad row / column range, n_seg outside 1 .. 64, seg_cap < 1, n_seg * seg_cap > 2^20, kpad not
 *     a supported width (the widths of mke_sim_select, and 224) or > ld, ld % 4 != 0: MKE_KEYED_E_SHAPE (an unsupported
 *     multiple of 16: MKE_KEYED_E_UNSUPPORTED); row_hi == row_lo: ok, nothing launched; a NULL pointer: MKE_KEYED_E_NULL;
 *     (row_hi - row_lo + 128) * n_seg * seg_cap > 2^29 - 1 slots in one launch: MKE_KEYED_E_RANGE (split the row range).
 *
 *   mke_keyed_finish: one workgroup per row; the row's list (its segments' first min(seg_count, seg_cap) entries, segment after
 *     segment = column order) is streamed from global memory in passes, there is no list-length limit besides n_seg * seg_cap.
 *     Row r of the call is keyed by row_ids[r]; tau_hi[r] is the threshold the sweep was given.
 *       sure = sum of seg_sure[r][*];  band = the stored entries with s <= tau_hi[r];  need = k - sure.
 *       status[r], first match wins:   2  a segment overflowed (seg_count > seg_cap)
 *                                      3  need < 0          (the k-th value is above tau_hi)
 *                                      1  need > |band|     (the k-th value is at or below tau_lo)
 *                                      4  fewer than m members have key < key_below
 *                                      0  otherwise
 *       members: the stored entries with s > tau_hi, the band entries above the need-th largest band value, and that value's
 *       first ties in list order until `need` band entries are taken (the rule of mke_topk_long and mke_topk_candidates; values
 *       compare as floats, -0 == +0).
 *     On status 0, out[r][0 .. m) holds col_ids[column] of the m members with the smallest keys (equal keys: the lowest list
 *     positions), in list order.  On any other status the row of `out` is not written.
 *     Errors, before any launch: rows < 0 or > 2^31 - 1, n_seg outside 1 .. 64, seg_cap < 1, n_seg * seg_cap > 2^20, not
 *     1 <= m < k (m == k is not a case of this kernel): MKE_KEYED_E_SHAPE; rows == 0: ok, nothing launched; a NULL pointer:
 *     MKE_KEYED_E_NULL.
 */
#ifndef MULTIKE_KEYED_H
#define MULTIKE_KEYED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKE_KEYED_OK 0
#define MKE_KEYED_E_NULL (-1)
#define MKE_KEYED_E_SHAPE (-2)
#define MKE_KEYED_E_UNSUPPORTED (-3)
#define MKE_KEYED_E_RANGE (-4)
#define MKE_KEYED_MAX_SEG 64
#define MKE_KEYED_MAX_LIST (1 << 20)

typedef struct mke_keyed_candidate {
  int32_t idx;
  float sim;
} mke_keyed_candidate;

const char* mke_keyed_last_error(void);

int mke_sim_select_keyed(const float* emb, int ld, int kpad, int64_t n_cols, int64_t row_lo, int64_t row_hi, const float* tau_lo,
                         const float* tau_hi, const int32_t* col_ids, uint64_t seed, uint64_t key_below, int n_seg, int seg_cap,
                         mke_keyed_candidate* cand, int32_t* seg_count, int32_t* seg_sure, void* stream);

int mke_keyed_finish(const mke_keyed_candidate* cand, const int32_t* seg_count, const int32_t* seg_sure, int64_t rows, int n_seg,
                     int seg_cap, const float* tau_hi, const int32_t* row_ids, const int32_t* col_ids, int k, int m, uint64_t seed,
                     uint64_t key_below, int32_t* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
