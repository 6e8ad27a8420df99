"""The definition of the auction decoder (mke_assign_rounds / base.alignment.assignment_matching) in NumPy, its duality
certificate, and the instance recipes its tests share.  `auction` is the specification: every arithmetic step is one float32
operation in the order written, so the device must equal it bit for bit — states, prices and counters."""
import numpy as np

f32 = np.float32
SLACK = 2.0 ** -16          # what f32 rounding adds to eps per row while (largest value - floor) + eps <= 16


def auction(val, col, n2, eps, floor, max_rounds=1 << 20):
    """-> state int64 [n1] (j + 1 = holds column j, -1 = settled unmatched, 0 = still bidding: only when max_rounds ran out),
    price float32 [n2], progress [rounds run, rows still bidding, bids made, rows settled unmatched]."""
    val, col = np.asarray(val, f32), np.asarray(col)
    n1, cut = col.shape
    eps, floor = f32(eps), f32(floor)
    ok = (col >= 0) & (col < n2)
    ok &= np.logical_and.accumulate(ok, axis=1)            # a column outside [0, n2) ends the list
    ok &= np.isfinite(val)                                 # a non-finite value is skipped
    price, owner, state = np.zeros(n2, f32), np.full(n2, -1, np.int64), np.zeros(n1, np.int64)
    rounds = bids = 0
    while rounds < max_rounds:
        rows = np.nonzero(state == 0)[0]
        if rows.size == 0:
            break
        rounds += 1
        ar = np.arange(rows.size)
        c, o = col[rows], ok[rows]
        net = np.where(o, val[rows] - price[np.where(o, c, 0)], f32(-np.inf)).astype(f32)     # f32 subtraction
        k1 = np.argmax(net, axis=1)                        # the LOWEST list position among equal net values
        v1 = net[ar, k1]
        net[ar, k1] = -np.inf
        v2 = np.maximum(net.max(axis=1), floor)            # second best: another list entry, or staying unmatched
        bidding = v1 >= floor                              # v1 == floor still bids
        state[rows[~bidding]] = -1                         # for good
        r, j = rows[bidding], c[ar, k1][bidding]
        bid = ((price[j] + (v1[bidding] - v2[bidding])) + eps).astype(f32)   # three f32 operations in this order
        bids += r.size
        order = np.lexsort((r, -bid, j))                   # per column: highest bid, then lowest row
        j, r, bid = j[order], r[order], bid[order]
        first = np.r_[True, j[1:] != j[:-1]] if r.size else np.zeros(0, bool)
        for jj, rr, bb in zip(j[first], r[first], bid[first]):
            if owner[jj] >= 0:
                state[owner[jj]] = 0                       # the displaced row bids again next round
            owner[jj], price[jj], state[rr] = rr, bb, jj + 1
    return state, price, [rounds, int((state == 0).sum()), bids, int((state == -1).sum())]


def listed(val, col, n2):
    """bool [n1, cut]: the entries the auction looks at."""
    val, col = np.asarray(val, f32), np.asarray(col)
    ok = (col >= 0) & (col < n2)
    ok &= np.logical_and.accumulate(ok, axis=1)
    return ok & np.isfinite(val)


def total(val, col, n2, floor, state):
    """float64: sum of the matched values + floor * unmatched rows."""
    val, col, state = np.asarray(val, np.float64), np.asarray(col), np.asarray(state, np.int64)
    ok = listed(val, col, n2)
    s = 0.0
    for i in range(col.shape[0]):
        if state[i] > 0:
            k = np.nonzero(ok[i] & (col[i] == state[i] - 1))[0]
            assert k.size, (i, state[i])
            s += val[i, k].max()
        else:
            s += float(f32(floor))
    return s


def certificate(val, col, n2, eps, floor, state, price):
    """The duality certificate in float64 -> a list of violations (empty = the matching is within n1 * (eps + 2^-16) of the
    optimum of the truncated instance): every row within eps + 2^-16 of its best option at the final prices (eps-complementary
    slackness), nobody still bidding, every held column listed by its holder, no column held twice, no free column with a price."""
    val64, col, state = np.asarray(val, np.float64), np.asarray(col), np.asarray(state, np.int64)
    price64 = np.asarray(price, np.float64)
    n1 = col.shape[0]
    ok = listed(val, col, n2)
    slack = float(f32(eps)) + SLACK
    fl = float(f32(floor))
    bad = []
    net = np.where(ok, val64 - np.append(price64, 0.0)[np.where(ok, col, 0)], -np.inf)      # (the append: n2 = 0 has no index 0)
    best = np.maximum(net.max(axis=1, initial=-np.inf), fl) if n1 else np.zeros(0)
    for i in range(n1):
        if state[i] == 0:
            bad.append(f"row {i} is still bidding")
        elif state[i] < 0:
            if state[i] != -1:
                bad.append(f"row {i} has state {state[i]}")
            elif fl < best[i] - slack:
                bad.append(f"row {i} stays unmatched at {fl}, {best[i]} is on offer")
        else:
            k = np.nonzero(ok[i] & (col[i] == state[i] - 1))[0]
            if not k.size:
                bad.append(f"row {i} holds column {state[i] - 1}, which it does not list")
            elif net[i, k].max() < best[i] - slack:
                bad.append(f"row {i} holds column {state[i] - 1} at {net[i, k].max()}, {best[i]} is on offer")
    held = state[state > 0] - 1
    cols, cnt = np.unique(held, return_counts=True)
    bad += [f"column {c} is held {m} times" for c, m in zip(cols, cnt) if m > 1]
    free = np.ones(n2, bool)
    free[held[(held >= 0) & (held < n2)]] = False
    bad += [f"free column {j} has price {price64[j]}" for j in np.nonzero(free & (price64 != 0))[0]]
    return bad


def top_lists(sim, cut):
    """(val float32 [n1, cut], col int32 [n1, cut]) of a float32 similarity matrix: per row its `cut` best columns, value
    descending then column ascending (mke_stable_lists' order)."""
    sim = np.asarray(sim, f32)
    n1, n2 = sim.shape
    order = np.lexsort((np.broadcast_to(np.arange(n2), sim.shape), -sim), axis=1)[:, :cut]
    return np.take_along_axis(sim, order, 1), order.astype(np.int32)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def recipe_sim(kind, n1, n2, rng, dim=8):
    """The four input kinds of the adversarial recipe: 0 unit-norm Gaussians, 1 four tight clusters, 2 similarities quantised to
    quarters (exact ties in value and in bids), 3 values scaled by 6 (a wide range)."""
    if kind == 1:
        centres = _unit(rng.standard_normal((4, dim)))
        a = _unit(centres[rng.integers(0, 4, n1)] + 0.01 * rng.standard_normal((n1, dim)))
        b = _unit(centres[rng.integers(0, 4, n2)] + 0.01 * rng.standard_normal((n2, dim)))
    else:
        a, b = _unit(rng.standard_normal((n1, dim))), _unit(rng.standard_normal((n2, dim)))
    sim = (a @ b.T).astype(f32)
    if kind == 2:
        sim = (np.round(sim * 4) / 4).astype(f32)
    if kind == 3:
        sim = (sim * f32(6)).astype(f32)
    return sim


def noisy_copy(n, dim, noise, seed):
    """(e1, e2) float32 unit rows: e2 = e1 + noise, the shape of a trained alignment (gold column = row index)."""
    rng = np.random.default_rng(seed)
    e1 = _unit(rng.standard_normal((n, dim)))
    e2 = _unit(e1 + noise * rng.standard_normal((n, dim)))
    return e1.astype(f32), e2.astype(f32)
