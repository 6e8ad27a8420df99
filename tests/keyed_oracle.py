"""NumPy restatement of mke_sim_select_keyed and mke_keyed_finish, written from the text of include/multike_keyed.h (not from
the kernels), on a GIVEN float32 similarity matrix: the sweep's own arithmetic (the fma chain) is the business of the callers,
who hand in similarities that are exact.  The key is tests/thin_oracle.py's.

    sweep:   sure  s > tau_hi: counted in seg_sure, stored iff key(seed, col_ids[i], col_ids[j]) < key_below
             band  tau_lo < s <= tau_hi: stored
             stored entries in column order per segment; seg_count = how many should have been stored; the first seg_cap are kept
    finish:  status 2 overflow, 3 need < 0, 1 need > |band|, 4 fewer than m members with key < key_below, 0 else (first match);
             members = stored sure entries + the `need` largest band entries, ties at the need-th value in list order;
             out = col_ids of the m members with the smallest keys (equal keys: lowest positions), in list order
"""
import numpy as np

import thin_oracle as to


def tile_columns(kpad):
    """Columns per tile of the sweep (SIMT_BN_FOR): segments are whole tiles."""
    return 64 if kpad // 16 <= 13 else 32


def segment_of(n_cols, kpad, n_seg):
    """int [n_cols]: the segment of every column — n_seg equal parts of the tiles, the last ones possibly empty."""
    bn = tile_columns(kpad)
    ntiles = -(-n_cols // bn)
    per = -(-ntiles // n_seg)
    return (np.arange(n_cols) // bn) // per


def keys(row_id, ids, seed):
    """uint64 [len(ids)]: key(seed, row_id, ids[p])."""
    return to.key(np.asarray(ids, dtype=np.int32)[None], [int(row_id)], seed)[0]


def sweep(sim, row_lo, tau_lo, tau_hi, col_ids, seed, key_below, n_seg, seg_cap, kpad):
    """sim float32 [rows, n_cols]: the similarities of working rows row_lo .. row_lo + rows - 1 to all columns.
    -> (idx int32 [rows, n_seg, seg_cap] (-1 = unused slot), val float32 likewise, seg_count, seg_sure int32 [rows, n_seg])."""
    sim = np.asarray(sim, dtype=np.float32)
    rows, n_cols = sim.shape
    col_ids = np.asarray(col_ids, dtype=np.int32)
    seg = segment_of(n_cols, kpad, n_seg)
    idx = np.full((rows, n_seg, seg_cap), -1, dtype=np.int32)
    val = np.zeros((rows, n_seg, seg_cap), dtype=np.float32)
    cnt = np.zeros((rows, n_seg), dtype=np.int32)
    sure_n = np.zeros((rows, n_seg), dtype=np.int32)
    kb = np.uint64(key_below)
    for r in range(rows):
        s = sim[r]
        sure = s > np.float32(tau_hi[r])
        band = (s > np.float32(tau_lo[r])) & (s <= np.float32(tau_hi[r]))
        store = band | (sure & (keys(col_ids[row_lo + r], col_ids, seed) < kb))
        for g in range(n_seg):
            in_g = seg == g
            sure_n[r, g] = np.count_nonzero(sure & in_g)
            cols = np.nonzero(store & in_g)[0]                       # ascending: column order
            cnt[r, g] = len(cols)
            cols = cols[:seg_cap]
            idx[r, g, :len(cols)] = cols
            val[r, g, :len(cols)] = s[cols]
    return idx, val, cnt, sure_n


def finish(idx, val, seg_count, seg_sure, tau_hi, row_ids, col_ids, k, m, seed, key_below):
    """-> (out int32 [rows, m] (-1 where the row is not written), status int32 [rows])."""
    assert 1 <= m < k
    rows, n_seg, seg_cap = idx.shape
    col_ids = np.asarray(col_ids, dtype=np.int32)
    out = np.full((rows, m), -1, dtype=np.int32)
    status = np.zeros(rows, dtype=np.int32)
    kb = np.uint64(key_below)
    for r in range(rows):
        if (seg_count[r] > seg_cap).any():
            status[r] = 2
            continue
        need = k - int(seg_sure[r].astype(np.int64).sum())
        if need < 0:
            status[r] = 3
            continue
        li = np.concatenate([idx[r, g, :max(0, seg_count[r, g])] for g in range(n_seg)])      # the list: segment, then column
        lv = np.concatenate([val[r, g, :max(0, seg_count[r, g])] for g in range(n_seg)]).astype(np.float32)
        band = np.nonzero(lv <= np.float32(tau_hi[r]))[0]
        if need > len(band):
            status[r] = 1
            continue
        taken = band[np.argsort(-lv[band].astype(np.float64), kind="stable")[:need]]           # ties: first in list order
        member = np.sort(np.concatenate([np.nonzero(lv > np.float32(tau_hi[r]))[0], taken]))
        ky = keys(row_ids[r], col_ids[li[member]], seed)
        if np.count_nonzero(ky < kb) < m:
            status[r] = 4
            continue
        keep = np.sort(np.argsort(ky, kind="stable")[:m])                                      # equal keys: lowest positions
        out[r] = col_ids[li[member[keep]]]
    return out, status


def topk_thinned(sim_row, row_id, col_ids, k, m, seed):
    """The row both paths of neighbour_table write: the exact top k (ties at the k-th value: the first columns) in column order,
    as entity ids, thinned to m by tests/thin_oracle.py."""
    s = np.asarray(sim_row, dtype=np.float32).astype(np.float64)
    top = np.sort(np.argsort(-s, kind="stable")[:k])
    return to.thin(np.asarray(col_ids, dtype=np.int32)[top][None], [int(row_id)], m, seed)[0]
