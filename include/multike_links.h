/*
 * multike_links.h — C-ABI of libmultike_links.so: the link set of self-training, edited from refresh to refresh (gfx950).
 *
 * A fourth library beside libmultike_hip.so (include/multike_hip.h), libmultike_thin.so (include/multike_thin.h) and
 * libmultike_keyed.so (include/multike_keyed.h); all three stay exactly as they are.  The boundary contract is theirs:
 * extern "C", DEVICE pointers owned by the caller, the library never allocates, frees or synchronises, an entry point only
 * enqueues work on the given hipStream_t (void*; NULL = the legacy default stream); return value 0 = ok, < 0 = bad argument
 * (MKE_LINKS_E_*: the values of multike_hip.h's MKE_E_*), > 0 = a hipError_t from the launch; mke_links_last_error() returns a
 * thread-local human-readable message for the last non-zero return of THIS library.
 *
 * The candidates of a model are fixed: n_a rows and n_b columns.  The persistent state is `held` (int32 [n_a]): held[i] is the
 * column row i is linked to, or -1; it is one-to-one.  `match` (int32 [n_a], one-to-one) is this refresh's decode, as
 * mke_mutual_pairs, mke_stable_finish or mke_assign_finish write it.  An entry of held or match outside [0, n_b) counts as -1.
 *
 *   mke_links_edit: out[i], for every row i, first rule that applies:
 *       1  match[i] = j' >= 0:                                          out[i] = j'   (new; a new pair always wins)
 *       2  held[i] = j >= 0 and some row r has match[r] = j:            out[i] = -1   (displaced)
 *       3  held[i] = j >= 0:  s = the value of the pair (i, j) today;
 *              s >= retain:                                             out[i] = j    (kept)
 *              otherwise, a NaN s included:                             out[i] = -1   (expired)
 *       4  otherwise:                                                   out[i] = -1
 *     Rule 1 compares nothing.  For the mutual decoder that is not a choice: j' is i's best column and i is j' 's best row on
 *     the same values, so no old link at either end has a larger value.  The rule is the same for any other decoder's match.
 *     `out` is one-to-one: new pairs are among themselves, old links are, and a kept link has neither end in a new pair.
 *
 *     s is the value the decode's sweep compares (metric, then the re-scoring), from the decode's own operands a [n_a][lda],
 *     b [n_b][ldb] (rows zero in [dim, kpad)), sq_a / sq_b (euclidean: squared row norms), csls_row / csls_col (both or neither:
 *     CSLS means, or twice the Sinkhorn potentials):
 *         dot:  a 16-lane group owns the row; lane l: acc = 0, then acc = fma(a[i][l + 16 k], b[j][l + 16 k], acc) for
 *               k = 0 .. kpad / 16 - 1; then the tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), the same over p8 ..
 *               p15, and the sum of the two halves: kpad / 16 + 4 roundings on any path from a product to the sum
 *         v  =  dot (MKE_LINKS_METRIC_INNER), or 1 - sqrt(max(sq_a[i] + sq_b[j] - 2 dot, 0)) (MKE_LINKS_METRIC_EUCLIDEAN)
 *         s  =  v, or (2 v - csls_row[i]) - csls_col[j] with the terms
 *     It is the sweep's formula in another summation order, so s may differ from the decode's own value of the pair in the
 *     last bits.  Rows decided by rule 1, 2 or 4 read no embedding row.  retain = -INFINITY keeps every undisplaced link whose
 *     value is not NaN.
 *
 *     score (float32 [n_a], or NULL): s for a kept link; new_score[i] copied for a new pair (0 when new_score is NULL); 0
 *     where out[i] = -1.
 *     counts (int32 [MKE_LINKS_COUNTS], zeroed BY THE CALL):  [0] links out   [1] out[i] == i   [2] new pairs
 *         [3] new pairs with match[i] == held[i] (re-found)   [4] kept   [5] displaced, including a row whose own new pair
 *         differs from held[i]   [6] expired.   [0] = [2] + [4];  valid old links = [3] + [4] + [5] + [6].
 *     inv (int32 [n_b]) is the caller's scratch: the call sets it to -1 and scatters inv[match[r]] = r (the match is
 *     one-to-one: no conflict), then one launch edits (a grid of at most 512 workgroups, 16 rows a workgroup and pass; a
 *     wavefront adds its seven counts once, at its end).  No float atomic, no atomic decides a position (the counters are
 *     integer adds): the same arguments give the same bits.
 *     Errors, before anything is enqueued: NULL args or counts: MKE_LINKS_E_NULL; n_a / n_b negative or above 0x7FFFFF00:
 *     MKE_LINKS_E_SHAPE; an unknown metric: MKE_LINKS_E_UNSUPPORTED; a NaN retain: MKE_LINKS_E_RANGE; exactly one of csls_row /
 *     csls_col: MKE_LINKS_E_NULL.  Then n_a == 0 or n_b == 0: counts zeroed, nothing else, MKE_LINKS_OK.  Then held, match, a, b,
 *     inv or out NULL: MKE_LINKS_E_NULL; kpad not a multiple of 16 in [16, 320], lda / ldb not multiples of 4 >= kpad:
 *     MKE_LINKS_E_SHAPE; a multiple of 16 without an instantiation (the widths of mke_align_mutual): MKE_LINKS_E_UNSUPPORTED;
 *     euclidean without sq_a and sq_b: MKE_LINKS_E_NULL; out overlapping held: MKE_LINKS_E_UNSUPPORTED.
 */
#ifndef MULTIKE_LINKS_H
#define MULTIKE_LINKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKE_LINKS_VERSION 1
#define MKE_LINKS_OK 0
#define MKE_LINKS_E_NULL (-1)
#define MKE_LINKS_E_SHAPE (-2)
#define MKE_LINKS_E_UNSUPPORTED (-3)
#define MKE_LINKS_E_RANGE (-4)
#define MKE_LINKS_METRIC_INNER 0
#define MKE_LINKS_METRIC_EUCLIDEAN 1
#define MKE_LINKS_COUNTS 7

typedef struct mke_links_args {
  const int32_t* held;              /* [n_a] */
  const int32_t* match;             /* [n_a] */
  int64_t n_a, n_b;
  const float* a; int lda;          /* [n_a][lda] */
  const float* b; int ldb;          /* [n_b][ldb] */
  int kpad;
  int metric;
  const float* sq_a;                /* [n_a], euclidean only (nullable otherwise) */
  const float* sq_b;                /* [n_b], euclidean only */
  const float* csls_row;            /* [n_a] row term, or NULL: no re-scoring */
  const float* csls_col;            /* [n_b] column term, or NULL (NULL exactly when csls_row is) */
  float retain;
  const float* new_score;           /* [n_a] or NULL */
  int32_t* inv;                     /* [n_b] scratch */
  int32_t* out;                     /* [n_a] */
  float* score;                     /* [n_a] or NULL */
  int32_t* counts;                  /* [MKE_LINKS_COUNTS] */
} mke_links_args;

const char* mke_links_last_error(void);
int mke_links_version(void);
int mke_links_edit(const mke_links_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
