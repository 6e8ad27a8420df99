"""NumPy restatement of mke_idlist_thin, written from the text of include/multike_thin.h (not from the kernel):

    mix(x):     x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31     (uint64, wrapping)
    key(r, p) = mix(mix(seed + 0x9E3779B97F4A7C15 * (uint64(row_ids[r]) + 1)) ^ uint64(uint32(ids[r][p])))
    position p of row r is kept iff (key(r, p), p) is among the m lexicographically smallest pairs of the row;
    the kept entries are written in list order; row_ids None keys row r by r.
"""
import numpy as np

_M1, _M2, _GOLD = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)


def mix(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30); x *= _M1
        x ^= x >> np.uint64(27); x *= _M2
        x ^= x >> np.uint64(31)
    return x


def key(ids, row_ids, seed):
    """uint64 [rows, k]: the key of every position of ids int32 [rows, k]."""
    ids = np.asarray(ids, dtype=np.int32)
    rid = np.asarray(row_ids, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        row = mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + _GOLD * (rid + np.uint64(1)))
    return mix(row[:, None] ^ ids.view(np.uint32).astype(np.uint64))


def thin(ids, row_ids, m, seed):
    """int32 [rows, m]: the kept entries of every row of ids int32 [rows, k], in list order."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
    if ids.ndim == 1:
        ids = ids[None]
    rows, k = ids.shape
    assert 1 <= m <= k
    if row_ids is None:
        row_ids = np.arange(rows)
    row_ids = np.asarray(row_ids).reshape(-1)
    assert row_ids.shape[0] == rows and (row_ids >= 0).all()
    ky = key(ids, row_ids, seed)
    order = np.argsort(ky, axis=1, kind="stable")          # stable: equal keys stay in position order
    keep = np.sort(order[:, :m], axis=1)
    return np.take_along_axis(ids, keep, axis=1)
