"""Float64 oracle of the sparse Sinkhorn re-scoring (include/multike_sparse.h).  NumPy only.

The support.  Row lists val_r / col_r [n_a, cut_r] and column lists val_c / row_c [n_b, cut_c]; a list is read from its front and
ends at its first index outside the other side's range (-1 = padding included).  The support is the set of pairs (i, j) either
list names; a pair both name is one entry with the ROW list's value; a pair one list names twice keeps its first value.
Entries in (row, column) order: row_off, ent_col, ent_val; the column view in (column, row) order: col_off, ent_row, ent_idx
(the entry's index in the row-major arrays).

The recurrence is sinkhorn_oracle.potentials' on the matrix that holds the entries' values and -inf everywhere else, with
sinkhorn_oracle.logsumexp; a row or column without entries has potential 0.0 (the dense recurrence would give -inf).

`VARIANTS` are the subtly wrong forms the tests must tell from the definition.
"""
from __future__ import annotations

import numpy as np

import sinkhorn_oracle as O

VARIANTS = ("duplicate_twice", "column_value", "padding_as_column", "stale_a", "empty_neg_inf", "drop_tail")


def case(n1, n2, d, noise, seed):
    """(e1 [n1, d], e2 [n2, d] float32 unit rows, S = their float32 product): n1 planted pairs (i, i) among n2 targets."""
    r = np.random.default_rng(seed)
    base = r.standard_normal((n2, d))
    e1 = base[:n1] + noise * r.standard_normal((n1, d))
    e1 = (e1 / np.linalg.norm(e1, axis=1, keepdims=True)).astype(np.float32)
    e2 = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)
    return e1, e2, e1 @ e2.T


def lists(S, cut):
    """(val float32 [n, cut], idx int32 [n, cut]): per row its `cut` best columns, value descending then column ascending,
    NaN never listed, short lists padded with -1 / -inf (mke_stable_lists' output)."""
    S = np.asarray(S, dtype=np.float32)
    n, m = S.shape
    val = np.full((n, cut), -np.inf, dtype=np.float32)
    idx = np.full((n, cut), -1, dtype=np.int32)
    for i in range(n):
        ok = np.nonzero(~np.isnan(S[i]))[0]
        order = ok[np.argsort(-S[i, ok], kind="stable")][:cut]
        val[i, :len(order)], idx[i, :len(order)] = S[i, order], order
    return val, idx


def named(val, idx, n_other, variant=None):
    """[(own, other, value)] of every list: up to the first index out of range."""
    out = []
    for own in range(idx.shape[0]):
        for k in range(idx.shape[1]):
            j = int(idx[own, k])
            if not 0 <= j < n_other:
                if variant == "padding_as_column" and j == -1 and n_other > 0:
                    out.append((own, n_other - 1, val[own, k]))     # -1 taken as an index: the last column
                    continue
                break
            out.append((own, j, val[own, k]))
    return out


def pairs(val_r, col_r, val_c, row_c, variant=None):
    """[(row, column, value)] in (row, column) order — with a variant, possibly a pair twice."""
    n_a, n_b = col_r.shape[0], row_c.shape[0]
    by_row = named(val_r, col_r, n_b, variant)
    by_col = [(i, j, v) for j, i, v in named(val_c, row_c, n_a, variant)]
    if variant == "duplicate_twice":
        return sorted(by_row + by_col, key=lambda t: t[:2])
    first, second = (by_col, by_row) if variant == "column_value" else (by_row, by_col)
    seen = {}
    for i, j, v in first + second:
        seen.setdefault((i, j), v)
    return [(i, j, seen[i, j]) for i, j in sorted(seen)]


def support(val_r, col_r, val_c, row_c):
    """dict of the arrays mke_sparse_support writes (count as an int)."""
    n_a, n_b = col_r.shape[0], row_c.shape[0]
    ent = pairs(val_r, col_r, val_c, row_c)
    rows = np.array([e[0] for e in ent], dtype=np.int64)
    cols = np.array([e[1] for e in ent], dtype=np.int64)
    vals = np.array([e[2] for e in ent], dtype=np.float32)
    view = np.lexsort((rows, cols)) if len(ent) else np.zeros(0, dtype=np.int64)
    return dict(count=len(ent), row_off=np.searchsorted(rows, np.arange(n_a + 1)).astype(np.int64), ent_col=cols.astype(np.int32),
                ent_val=vals, col_off=np.searchsorted(cols[view], np.arange(n_b + 1)).astype(np.int64),
                ent_row=rows[view].astype(np.int32), ent_idx=view.astype(np.int32))


def masked(n_a, n_b, rows, cols, vals):
    """The n_a x n_b float64 matrix of the entries, -inf outside the support."""
    M = np.full((n_a, n_b), -np.inf)
    M[rows, cols] = np.asarray(vals, dtype=np.float64)
    return M


def lse_masked(M, sub, tau):
    """sinkhorn_oracle.lse over a masked matrix; a row without entries gives 0.0."""
    out = np.zeros(M.shape[0])
    some = np.isfinite(M).any(axis=1) if M.shape[1] else np.zeros(M.shape[0], dtype=bool)
    if some.any():
        out[some] = O.lse(M[some], sub, tau)
    return out


def potentials(n_a, n_b, rows, cols, vals, iters, tau):
    """(a [n_a], b [n_b]) float64: sinkhorn_oracle.potentials' recurrence on the masked matrix."""
    M = masked(n_a, n_b, rows, cols, vals)
    a, b = np.zeros(n_a), np.zeros(n_b)
    for _ in range(int(iters)):
        a = lse_masked(M, b, tau)
        b = lse_masked(M.T, a, tau)
    return a, b


def lse_lists(n, own, other, vals, sub, tau, seg=None, variant=None):
    """out [n] float64 from the entry list itself (a pair may stand twice): out[i] = tau log sum over the entries owned by i of
    exp((value - sub[other]) / tau).  seg: lists longer than it are summed segment by segment and the segments merged, as the
    device does; 'drop_tail' loses the ragged last segment, 'empty_neg_inf' gives -inf to a list without entries."""
    own, other = np.asarray(own, dtype=np.int64), np.asarray(other, dtype=np.int64)
    with np.errstate(invalid="ignore"):                       # -inf - -inf of a wrong variant: a NaN, dropped below
        x = (np.asarray(vals, dtype=np.float64) - (0.0 if sub is None else np.asarray(sub, dtype=np.float64)[other])) / tau
    out = np.zeros(n)
    for i in range(n):
        xi = x[own == i]
        xi = xi[xi > -np.inf]
        if len(xi) == 0:
            out[i] = -np.inf if variant == "empty_neg_inf" or (own == i).any() else 0.0
            continue
        if seg is not None and len(xi) > seg:
            whole = len(xi) // seg * seg
            parts = [xi[s:s + seg] for s in range(0, whole if variant == "drop_tail" else len(xi), seg)]
            xi = np.array([O.logsumexp(p, 0) for p in parts])
        out[i] = tau * O.logsumexp(xi, 0)
    return out


def potentials_lists(n_a, n_b, ent, iters, tau, variant=None, seg=None):
    """(a, b) from [(row, column, value)]: the same recurrence entry by entry; 'stale_a': the column pass reads the a of the
    iteration before."""
    rows, cols, vals = (np.array([e[k] for e in ent]) for k in range(3)) if len(ent) else (np.zeros(0, dtype=np.int64),) * 3
    a, b = np.zeros(n_a), np.zeros(n_b)
    for _ in range(int(iters)):
        old = a
        a = lse_lists(n_a, rows, cols, vals, b, tau, seg, variant)
        b = lse_lists(n_b, cols, rows, vals, old if variant == "stale_a" else a, tau, seg, variant)
    return a, b


def hand_case():
    """(val_r, col_r, val_c, row_c) of a 5 x 7 instance, cut_r 3, cut_c 2: the pairs (4, 0) and (1, 1) stand in both lists with
    differing values, row 1 has a -1 with a finite value in the middle of its list (the (1, 3) behind it is not named), row 3 an
    index past the range (the (3, 0) behind it is not named), column 4 a row past the range; row 2 and column 3 are empty."""
    inf = np.inf
    val_r = np.array([[0.9, 0.4, -inf], [0.8, 0.3, 0.7], [-inf, -inf, -inf], [0.5, 0.6, 0.2], [0.65, 0.55, 0.45]], dtype=np.float32)
    col_r = np.array([[2, 5, -1], [1, -1, 3], [-1, -1, -1], [6, 7, 0], [0, 2, 6]], dtype=np.int32)
    val_c = np.array([[0.66, 0.35], [0.81, -inf], [0.9, 0.55], [-inf, -inf], [0.1, 0.2], [0.41, -inf], [0.5, 0.45]], dtype=np.float32)
    row_c = np.array([[4, 1], [1, -1], [0, 4], [-1, -1], [3, 5], [0, -1], [3, 4]], dtype=np.int32)
    return val_r, col_r, val_c, row_c
