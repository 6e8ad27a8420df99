/*
 * multike_sparse.h — C-ABI of libmultike_sparse.so: Sinkhorn re-scoring on the support of the candidate lists (gfx950).
 *
 * A fifth library beside libmultike_hip.so (include/multike_hip.h), libmultike_thin.so, libmultike_keyed.so and
 * libmultike_links.so; all four stay exactly as they are.  The boundary contract is theirs: extern "C", DEVICE pointers owned by
 * the caller, the library never allocates, frees or synchronises and keeps no state, an entry point only enqueues work on the
 * given hipStream_t (void*; NULL = the legacy default stream); return value 0 = ok, < 0 = bad argument (MKE_SPARSE_E_*: the
 * values of multike_hip.h's MKE_E_*), > 0 = a hipError_t; mke_sparse_last_error() returns a thread-local human-readable message
 * for the last non-zero return of THIS library.
 *
 * The support.  val_r / col_r [n_a][cut_r] are the row lists (mke_stable_lists(a, b): per row its best columns, padded with
 * column -1 / value -inf), val_c / row_c [n_b][cut_c] the column lists (mke_stable_lists(b, a)).  A list is read from its
 * front and ENDS at its first index outside the other side's range (-1 included), as mke_stable_rounds reads it.  The support
 * is the set of pairs (i, j) either list names; a pair both lists name is ONE entry and keeps the row list's value (the two
 * sweeps need not round alike).  A pair one list names twice keeps its first value.
 *
 *   mke_sparse_support writes
 *     count        [1]  int64   E = the number of entries (<= capacity)
 *     row_off      [n_a + 1]    int64   entries of row i: [row_off[i], row_off[i + 1]); row_off[n_a] = E
 *     ent_col, ent_val [E]      the entries in (row ascending, column ascending) order
 *     col_off      [n_b + 1]    int64   the same entries in (column ascending, row ascending) order:
 *     ent_row, ent_idx [E]      the entry's row and its index into ent_col / ent_val
 *     row_seg, col_seg [n + 1]  int32   the work items of mke_sparse_lse: a row with more than MKE_SPARSE_Q entries is cut
 *                               into ceil(len / MKE_SPARSE_SEG) segments, items [row_seg[i], row_seg[i + 1]); other rows have none
 *   Nothing past E is written in ent_*.  capacity (the entries ent_* hold) must be >= n_a * cut_r + n_b * cut_c.
 *   How: one 64-bit key (row, column, list) per list slot, hipcub radix sort with the value as payload, a flag per slot
 *   (valid and not the pair of its predecessor), an exclusive scan of the flags, an ordered compaction; the offsets are binary
 *   searches of the compacted rows; a second sort of (column, row) keys with the entry index as payload gives the column view.
 *   No atomic anywhere: the same lists give the same bytes.  The host reads nothing back: count, the offsets and the work
 *   items stay on the device and mke_sparse_lse takes them there (read `count` only to trim or to report).
 *   n_a * cut_r + n_b * cut_c above 0x7FFFFF00 (the sort counts with an int): MKE_SPARSE_E_RANGE.
 *   Errors: NULL args: E_NULL; n_a / n_b negative or above 0x7FFFFF00, cut_r / cut_c < 1: E_SHAPE; the slot count: E_RANGE;
 *   row_off, col_off, row_seg, col_seg or count NULL: E_NULL; then with slots: a NULL list, ent_* or temp: E_NULL; capacity below
 *   the slot count: E_SHAPE; temp_bytes below mke_sparse_support_temp_bytes: E_SHAPE.
 *
 *   mke_sparse_lse: one half-iteration over n lists of the support,
 *       out[i] = tau log sum_{e in [off[i], off[i + 1])} exp((val[idx ? idx[e] : e] - sub[other[e]]) / tau)
 *     rows: off = row_off, seg = row_seg, other = ent_col, idx = NULL; columns: off = col_off, seg = col_seg, other = ent_row,
 *     idx = ent_idx.  sub NULL = zeros.  A list without entries writes 0.0; one whose arguments are all -inf writes -inf.
 *     Evaluated as mke_align_lse: x = (v - sub) log2(e) / tau, a running (m, s) with sum = s 2^m and one v_exp_f32 of
 *     -|x - m| per entry, never an exp of a raw argument.  A list of at most MKE_SPARSE_Q entries belongs to a 16-lane group
 *     (lane l takes entries l, l + 16, ...; four fixed butterfly merges; out in float64 arithmetic rounded once).  A longer
 *     list: a wavefront per segment of MKE_SPARSE_SEG entries leaves one (m, s) in temp, then one thread per list merges its
 *     segments in segment order in float64.  Classification and segments depend on the offsets alone, no float atomic: the
 *     same arguments give the same bits.
 *     temp: mke_sparse_lse_temp_bytes(capacity) bytes (8 per possible segment).
 *     Errors: NULL args: E_NULL; n negative or above 0x7FFFFF00, capacity negative: E_SHAPE; tau not positive and finite:
 *     E_RANGE; n == 0: ok, nothing enqueued; off, seg, out NULL, or (capacity > 0) other, val, temp NULL: E_NULL; temp_bytes too
 *     small: E_SHAPE.
 */
#ifndef MULTIKE_SPARSE_H
#define MULTIKE_SPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKE_SPARSE_VERSION 1
#define MKE_SPARSE_OK 0
#define MKE_SPARSE_E_NULL (-1)
#define MKE_SPARSE_E_SHAPE (-2)
#define MKE_SPARSE_E_UNSUPPORTED (-3)
#define MKE_SPARSE_E_RANGE (-4)
#define MKE_SPARSE_Q 256
#define MKE_SPARSE_SEG 1024
#define MKE_SPARSE_MAX_SLOTS 0x7FFFFF00

typedef struct mke_sparse_support_args {
  const float* val_r;               /* [n_a][cut_r] */
  const int32_t* col_r;             /* [n_a][cut_r] */
  const float* val_c;               /* [n_b][cut_c] */
  const int32_t* row_c;             /* [n_b][cut_c] */
  int64_t n_a, n_b;
  int cut_r, cut_c;
  int64_t capacity;
  int64_t* row_off;                 /* [n_a + 1] */
  int32_t* row_seg;                 /* [n_a + 1] */
  int32_t* ent_col;                 /* [capacity] */
  float* ent_val;                   /* [capacity] */
  int64_t* col_off;                 /* [n_b + 1] */
  int32_t* col_seg;                 /* [n_b + 1] */
  int32_t* ent_row;                 /* [capacity] */
  int32_t* ent_idx;                 /* [capacity] */
  int64_t* count;                   /* [1] */
  void* temp;
  int64_t temp_bytes;
} mke_sparse_support_args;

typedef struct mke_sparse_lse_args {
  int64_t n;
  const int64_t* off;               /* [n + 1] */
  const int32_t* seg;               /* [n + 1] */
  const int32_t* other;             /* [E] */
  const float* val;                 /* [E] */
  const int32_t* idx;               /* [E] or NULL */
  const float* sub;                 /* [other side] or NULL = zeros */
  float tau;
  float* out;                       /* [n] */
  int64_t capacity;
  void* temp;
  int64_t temp_bytes;
} mke_sparse_lse_args;

const char* mke_sparse_last_error(void);
int mke_sparse_version(void);
int64_t mke_sparse_support_temp_bytes(int64_t n_a, int64_t n_b, int cut_r, int cut_c);
int mke_sparse_support(const mke_sparse_support_args* args, void* stream);
int64_t mke_sparse_lse_temp_bytes(int64_t capacity);
int mke_sparse_lse(const mke_sparse_lse_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
