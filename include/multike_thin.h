/*
 * multike_thin.h — C-ABI of libmultike_thin.so: capped neighbour tables of the truncated sampler (gfx950).
 *
 * A library of its own beside libmultike_hip.so, whose C-ABI (include/multike_hip.h, MKE_VERSION 107) it leaves exactly as
 * it is: nothing there is added, moved or renumbered.  The boundary contract is that header's: extern "C", DEVICE pointers
 * owned by the caller, the library never allocates, frees or synchronises, the entry point only enqueues kernels on the given
 * hipStream_t (void*; NULL = the legacy default stream); return value 0 = ok, < 0 = bad argument (the values of that header's
 * MKE_E_NULL = -1 and MKE_E_SHAPE = -2), > 0 = a hipError_t from the launch; mke_thin_last_error() returns a thread-local
 * human-readable message for the last non-zero return of THIS library.
 *
 * New design: the reference keeps all k = int((1 - truncated_epsilon) * |E|) neighbours of every entity
 * (code/base/batch.py:119-150), a table that grows with |E|^2; the sampler only needs a uniform draw from that set.
 *
 *   mke_idlist_thin: for each of the `rows` lists ids[r][0 .. k) (row stride ld_ids >= k) keep m of the k positions and write
 *     their entries to out[r][0 .. m) IN LIST ORDER.  All arithmetic below is on uint64 with wrap-around.
 *       mix(x):     x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31; return x
 *       key(r, p) = mix(mix(seed + 0x9E3779B97F4A7C15 * (uint64(row_ids[r]) + 1)) ^ uint64(uint32(ids[r][p])))
 *     row_ids[r] is the (non-negative) entity id that keys row r; row_ids == NULL keys row r by r itself.
 *     Position p of row r is kept iff the pair (key(r, p), p) is among the m lexicographically smallest pairs of that row:
 *     the m smallest keys, and among equal keys the lowest positions.  m == k copies the list.
 *     The key is a function of the seed and of the two ids only, so a row's kept SET does not depend on the order of its
 *     list (distinct ids), on the row's place in the call, on how the rows are split over calls, or on the device; for a
 *     fixed list every m-subset of distinct ids is as likely as any other over the seeds, i.e. each entry is kept with
 *     probability m / k.  No atomic decides an output position: the same arguments give the same bytes.
 *     Errors, before any launch: rows < 0, k < 1, m < 1, m > k, ld_ids < k: MKE_E_SHAPE; rows == 0: MKE_OK, nothing launched;
 *     ids or out NULL: MKE_E_NULL.  One workgroup per row, rows * k of any size (64-bit addressing), any number of rows.
 */
#ifndef MULTIKE_THIN_H
#define MULTIKE_THIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* mke_thin_last_error(void);

int mke_idlist_thin(const int32_t* ids /* [rows][k], row stride ld_ids */, int64_t rows, int k, int64_t ld_ids,
                    const int32_t* row_ids /* [rows]: the entity id that keys row r; NULL = r */,
                    int m, uint64_t seed, int32_t* out /* [rows][m] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
