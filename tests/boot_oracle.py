"""NumPy / plain-Python statements of the two definitions of the self-training kernels (include/multike_hip.h, section 9g).
Literal loops: these are the definitions, not an implementation of anything."""
import numpy as np


def partner(match, ids_a, ids_b, n_entities):
    """mke_boot_partner: all -1, then both directions of every matched row; a match outside [0, n_b) is ignored, a pair with an
    id outside [0, n_entities) is ignored as a whole."""
    out = np.full(n_entities, -1, dtype=np.int32)
    for i, j in enumerate(np.asarray(match).tolist()):
        if j < 0 or j >= len(ids_b):
            continue
        a, b = int(ids_a[i]), int(ids_b[j])
        if not (0 <= a < n_entities and 0 <= b < n_entities):
            continue
        out[a] = b
        out[b] = a
    return out


def swap(h, p, t, partner_table, heads_only=False, weight=None):
    """mke_swap_triples: walk k = 0 .. n-1; the head form if the head is linked, then (unless heads_only) the tail form if the
    tail is.  -> (int32 [m, 3], float32 [m] or None); m is the count whatever the capacity."""
    n_entities = len(partner_table)

    def linked(e):
        return int(partner_table[e]) if 0 <= e < n_entities else -1
    rows, ws = [], []
    for hk, pk, tk in zip(np.asarray(h).tolist(), np.asarray(p).tolist(), np.asarray(t).tolist()):
        if linked(hk) >= 0:
            rows.append((linked(hk), pk, tk))
            ws.append(None if weight is None else weight[hk])
        if not heads_only and linked(tk) >= 0:
            rows.append((hk, pk, linked(tk)))
            ws.append(None if weight is None else weight[tk])
    out = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    return out, (None if weight is None else np.asarray(ws, dtype=np.float32))


def swap_vector(h, p, t, partner_table, heads_only=False, weight=None):
    """The same walk in vector form (for the large cases): interleave the two forms of every triple, keep the emitted ones.
    -> (int32 [m, 3], float32 [m] or None), as `swap`."""
    h, p, t, table = (np.asarray(x, dtype=np.int64) for x in (h, p, t, partner_table))

    def linked(e):
        ok = (e >= 0) & (e < len(table))
        out = np.full(len(e), -1, dtype=np.int64)
        out[ok] = table[e[ok]]
        return out
    ph = linked(h)
    pt = np.full(len(h), -1, dtype=np.int64) if heads_only else linked(t)
    both = np.stack([np.stack([ph, p, t], axis=1), np.stack([h, p, pt], axis=1)], axis=1)          # [n, 2, 3]: head form, tail form
    keep = np.stack([ph >= 0, pt >= 0], axis=1)
    rows = both[keep].astype(np.int32).reshape(-1, 3)
    if weight is None:
        return rows, None
    weight = np.asarray(weight, dtype=np.float32)
    last = max(len(weight) - 1, 0)
    w = np.stack([weight[np.clip(h, 0, last)], weight[np.clip(t, 0, last)]], axis=1)      # clipped ids are never kept
    return rows, w[keep]
