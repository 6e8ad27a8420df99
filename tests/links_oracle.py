"""NumPy oracle of the link-set edit of self-training (mke_links_edit, include/multike_links.h).  No GPU code.

The candidates are fixed: n_a rows, n_b columns.  `held` [n_a] is the link set kept across refreshes (held[i] = the column of
row i or -1, one-to-one), `match` [n_a] this refresh's one-to-one decode; an entry outside [0, n_b) counts as -1.  S [n_a, n_b]
holds the value of every pair today, in the units the decode compares (`values`).  For every row i, the first rule that applies:

    1  match[i] = j' >= 0                                   out[i] = j'     new: a new pair always wins, nothing is compared
    2  held[i] = j >= 0 and some r has match[r] = j         out[i] = -1     displaced
    3  held[i] = j >= 0:   S[i, j] >= retain                out[i] = j      kept
                           otherwise (a NaN included)       out[i] = -1     expired
    4  otherwise                                            out[i] = -1

score[i] = S[i, j] of a kept link, new_score[i] of a new pair (0 without new_score), 0 where out[i] = -1.
counts = (links out, out[i] == i, new, new with match[i] == held[i], kept, displaced — a row whose own new pair differs from
held[i] included —, expired)."""
from __future__ import annotations

import numpy as np

INNER, EUCLIDEAN = 0, 1
COUNTS = ("links", "gold", "new", "refound", "kept", "displaced", "expired")


def clean(x, n_b):
    """int64 copy of a link vector with everything outside [0, n_b) set to -1."""
    x = np.asarray(x, dtype=np.int64)
    return np.where((x >= 0) & (x < n_b), x, -1)


def _value(dot, sq_a, sq_b, t_row, t_col, metric):
    with np.errstate(invalid="ignore"):
        v = dot
        if metric == EUCLIDEAN:
            x = sq_a + sq_b - 2.0 * dot
            v = 1.0 - np.sqrt(np.where(x > 0.0, x, 0.0))    # fmaxf(x, 0) of mke_rescore.h: 0 for a NaN x too, so v = 1 there
        elif metric != INNER:
            raise ValueError(f"metric {metric}")
        return v if t_row is None else (2.0 * v - t_row) - t_col


def _f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def values(a, b, metric=INNER, sq_a=None, sq_b=None, terms=None):
    """float64 [n_a, n_b]: the value the decode compares for every pair, from its own operands a [n_a, kpad], b [n_b, kpad]:
    dot, or 1 - sqrt(max(sq_a[i] + sq_b[j] - 2 dot, 0)); then (2 v - terms[0][i]) - terms[1][j] with re-scoring terms."""
    col = lambda x: None if x is None else _f64(x)[:, None]
    row = lambda x: None if x is None else _f64(x)[None, :]
    with np.errstate(invalid="ignore"):
        dot = _f64(a) @ _f64(b).T
    return _value(dot, col(sq_a), row(sq_b), *((col(terms[0]), row(terms[1])) if terms is not None else (None, None)), metric)


def values_held(a, b, held, metric=INNER, sq_a=None, sq_b=None, terms=None):
    """float64 [n_a]: `values` of the pairs (i, held[i]) alone, NaN where held[i] is outside [0, n_b) — for sets too large for
    the matrix."""
    h = clean(held, len(b))
    j = np.maximum(h, 0)
    at = lambda x: None if x is None else _f64(x)[j]
    with np.errstate(invalid="ignore"):
        dot = (_f64(a) * _f64(b)[j]).sum(1)
    s = _value(dot, _f64(sq_a), at(sq_b), *((_f64(terms[0]), at(terms[1])) if terms is not None else (None, None)), metric)
    return np.where(h >= 0, s, np.nan)


def edit(held, match, S, retain=-np.inf, new_score=None, n_b=None):
    """(out int32 [n_a], score float32 [n_a], counts int64 [7]) of one edit; S [n_a, n_b] as `values` gives it (any float type:
    it is compared with `retain` as it is), or with n_b given the vector of `values_held`."""
    if np.isnan(retain):
        raise ValueError("retain is NaN")
    S = np.asarray(S)
    if S.ndim == 2:
        n_a, n_b = S.shape
        value = lambda i, j: S[i, j]
    else:
        n_a = len(S)
        value = lambda i, j: S[i]
    h, m = clean(held, n_b), clean(match, n_b)
    assert len(h) == n_a and len(m) == n_a
    taken = set(m[m >= 0].tolist())                         # the columns of the new pairs
    out = np.full(n_a, -1, dtype=np.int32)
    score = np.zeros(n_a, dtype=np.float32)
    c = dict.fromkeys(COUNTS, 0)
    for i in range(n_a):
        if m[i] >= 0:
            out[i] = m[i]
            if new_score is not None:
                score[i] = new_score[i]
            c["new"] += 1
            if h[i] == m[i]:
                c["refound"] += 1
            elif h[i] >= 0:
                c["displaced"] += 1
        elif h[i] >= 0:
            s = value(i, h[i])
            if int(h[i]) in taken:
                c["displaced"] += 1
            elif s >= retain:                               # False for a NaN
                out[i] = h[i]
                score[i] = s
                c["kept"] += 1
            else:
                c["expired"] += 1
    c["links"] = int((out >= 0).sum())
    c["gold"] = int((out == np.arange(n_a)).sum())
    return out, score, np.array([c[k] for k in COUNTS], dtype=np.int64)


def one_to_one(x):
    """True when no column appears twice among the entries >= 0."""
    x = np.asarray(x)
    x = x[x >= 0]
    return len(np.unique(x)) == len(x)
