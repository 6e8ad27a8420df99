"""The NumPy statement of what `stable_alignment` computes: the suitor-optimal stable matching of the instance in which every
suitor (row) keeps only its `cut` best reviewers (columns), by sequential deferred acceptance run to its fixed point.
Ties: among equal similarities a suitor prefers the lower column, a reviewer the lower row.  A suitor that exhausts its list
stays unmatched (-1).  Whenever the reference's galeshapley(.., cut) matches every suitor this is its result."""
import numpy as np


def lists_from_matrix(mat, cut):
    """(val float32 [n1, cut], col int32 [n1, cut]): per row the `cut` largest values with their columns, value descending then
    column ascending; NaN never enters; short lists are padded with column -1 (value -inf)."""
    mat = np.asarray(mat)
    n1 = mat.shape[0]
    val = np.full((n1, cut), -np.inf, dtype=np.float32)
    col = np.full((n1, cut), -1, dtype=np.int32)
    for i in range(n1):
        row = mat[i]
        idx = np.nonzero(~np.isnan(row))[0]
        order = idx[np.lexsort((idx, -row[idx]))][:cut]
        val[i, :len(order)] = row[order]
        col[i, :len(order)] = order
    return val, col


def deferred_acceptance(val, col, n2):
    """match int64 [n1]: sequential deferred acceptance over the lists (a column outside [0, n2) ends a list)."""
    val, col = np.asarray(val), np.asarray(col)
    n1, cut = col.shape
    ptr = np.zeros(n1, dtype=np.int64)
    holder = np.full(n2, -1, dtype=np.int64)
    hval = np.zeros(n2, dtype=np.float64)
    match = np.full(n1, -1, dtype=np.int64)
    free = list(range(n1 - 1, -1, -1))
    while free:
        i = free.pop()
        while ptr[i] < cut:
            c = int(col[i, ptr[i]])
            if c < 0 or c >= n2:
                ptr[i] = cut
                break
            v = float(val[i, ptr[i]])
            j = int(holder[c])
            if j < 0 or v > hval[c] or (v == hval[c] and i < j):
                holder[c], hval[c], match[i] = i, v, c
                if j >= 0:
                    match[j] = -1
                    ptr[j] += 1
                    free.append(j)
                break
            ptr[i] += 1
    return match


def blocking_pairs(val, col, match, n2):
    """The (suitor, column) pairs that block `match` with respect to the lists: the suitor lists the column above its own
    partner (or is unmatched) and the column prefers the suitor to its holder (or is free).  Empty for a stable matching."""
    val, col = np.asarray(val), np.asarray(col)
    n1, cut = col.shape
    holder = np.full(n2, -1, dtype=np.int64)
    hval = np.zeros(n2, dtype=np.float64)
    for i in range(n1):
        if match[i] >= 0:
            p = int(np.nonzero(col[i] == match[i])[0][0])
            holder[match[i]], hval[match[i]] = i, val[i, p]
    out = []
    for i in range(n1):
        for p in range(cut):
            c = int(col[i, p])
            if c < 0 or c >= n2 or c == match[i]:
                break
            j, v = int(holder[c]), float(val[i, p])
            if j < 0 or v > hval[c] or (v == hval[c] and i < j):
                out.append((i, c))
    return out
