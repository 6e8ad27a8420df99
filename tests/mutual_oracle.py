"""NumPy oracle of the mutual (bidirectional) nearest-neighbour decoder (mke_align_mutual + mke_mutual_pairs).  No GPU code.

Given a score matrix S [n_a, n_b]: K = where(isnan(S), -inf, S); a row's best column is argmax(K, 1), a column's best row
argmax(K, 0) — np.argmax returns the lowest index among equal values; a row (column) whose scores are all NaN has no best,
and where the maximum is -inf the best is the lowest index that holds -inf itself, not a NaN (a NaN is never anybody's best).
match[i] = j when j is row i's best, i is column j's best and S[i, j] >= threshold."""
from __future__ import annotations

import numpy as np


def bests(S):
    """(row_col int64 [n_a], col_row int64 [n_b]): the best column of every row and the best row of every column, -1 = none."""
    S = np.asarray(S)
    n_a, n_b = S.shape
    if n_a == 0 or n_b == 0:
        return np.full(n_a, -1, dtype=np.int64), np.full(n_b, -1, dtype=np.int64)
    nan = np.isnan(S)
    K = np.where(nan, -np.inf, S)

    def best(K, nan, axis):
        # a NaN is never a best: where the maximum is -inf itself, the lowest index that really holds -inf
        idx = np.where(K.max(axis) == -np.inf, np.argmax(~nan, axis=axis), np.argmax(K, axis=axis))
        return np.where(nan.all(axis), -1, idx).astype(np.int64)

    return best(K, nan, 1), best(K, nan, 0)


def ordered32(bits):
    """The order-preserving image of float32 bit patterns (uint32): larger float <=> larger unsigned."""
    u = np.asarray(bits, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def words(S):
    """(row_best uint64 [n_a], col_best uint64 [n_b]) for a float32 S: ordered(value) << 32 | 0xFFFFFFFF - index, 0 = no best."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    row_col, col_row = bests(S)

    def pack(val, idx):
        key = (ordered32(val.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | \
            (np.uint64(0xFFFFFFFF) - np.maximum(idx, 0).astype(np.uint64))
        return np.where(idx >= 0, key, np.uint64(0))

    rv = S[np.arange(S.shape[0]), np.maximum(row_col, 0)] if S.shape[1] else np.zeros(S.shape[0], np.float32)
    cv = S[np.maximum(col_row, 0), np.arange(S.shape[1])] if S.shape[0] else np.zeros(S.shape[1], np.float32)
    return pack(np.ascontiguousarray(rv), row_col), pack(np.ascontiguousarray(cv), col_row)


def pairs(S, threshold=-np.inf):
    """(match int64 [n_a], counts (matched, match[i] == i))."""
    S = np.asarray(S)
    row_col, col_row = bests(S)
    n_a = S.shape[0]
    match = np.full(n_a, -1, dtype=np.int64)
    for i in range(n_a):
        j = row_col[i]
        if j >= 0 and col_row[j] == i and S[i, j] >= threshold:
            match[i] = j
    return match, (int((match >= 0).sum()), int((match == np.arange(n_a)).sum()))


def scores_prf(match):
    """(precision, recall, f1) in percent for gold column = row index; all 0.0 when nothing matched."""
    n = len(match)
    matched, gold = int((match >= 0).sum()), int((match == np.arange(n)).sum())
    if not matched:
        return 0.0, 0.0, 0.0
    p, r = gold / matched * 100, gold / n * 100
    return p, r, (2 * p * r / (p + r) if gold else 0.0)
