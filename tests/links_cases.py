"""Cases of the link-set edit (mke_links_edit) that the CPU tests and the GPU tests share.  No GPU code.

structure    held / match of given sizes with every kind of row the sizes allow
exact_case   operands on which every value is exact in f32 whatever the order of the sum: dyadic entries whose products and sums
             fit 24 bits, squared distances of the held pairs that are perfect squares, dyadic re-scoring terms
unit_case    random unit rows; `retain` sits in a gap of the old links' values that is wider than `value_bound`
value_bound  how far the device's f32 value of a pair may lie from the float64 value, by counting its roundings"""
from __future__ import annotations

import numpy as np

import links_oracle as LO

KPADS = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)        # simt_for_kpad's widths
# rows: a quarter-wavefront owns a row, so a wavefront holds 4 and a workgroup 16: the edges of both, of a whole wavefront of
# workgroups' worth (64) and some hundreds; PASS_ROWS is the edge of a pass of the capped grid (LINKS_MAX_BLOCKS of mke_links.hip)
PASS_ROWS = 512 * 16
SIZES = ((1, 1), (3, 3), (4, 4), (5, 5), (63, 63), (64, 64), (65, 65), (257, 257), (40, 71), (130, 33))
U = 2.0 ** -24                                                              # unit roundoff of f32


def structure(rng, n_a, n_b):
    """(held, match) int32 [n_a], both one-to-one.  Of the held rows, in turn: re-found (match = held), a new pair of its own on
    another column, displaced through the column (a row that held nothing takes it), and three that only their value decides.
    Of the rest: a new pair on a free column, or nothing.  Then entries outside [0, n_b) in both vectors."""
    rows, cols = rng.permutation(n_a), rng.permutation(n_b)
    n_held = (2 * min(n_a, n_b) + 2) // 3
    held, match = np.full(n_a, -1, dtype=np.int64), np.full(n_a, -1, dtype=np.int64)
    held[rows[:n_held]] = cols[:n_held]
    free_rows, free_cols = list(rows[n_held:]), list(cols[n_held:])
    for p, i in enumerate(rows[:n_held]):
        kind = p % 6
        if kind == 0:
            match[i] = held[i]
        elif kind == 1 and free_cols:
            match[i] = free_cols.pop()
        elif kind == 2 and free_rows:
            match[free_rows.pop()] = held[i]
    for p, i in enumerate(list(free_rows)):
        if p % 2 == 0 and free_cols:
            match[i] = free_cols.pop()
            free_rows.remove(i)
    outside = (n_b, -7, 2 ** 31 - 1, n_b + 5, -2 ** 31)
    for p, i in enumerate(free_rows[:5]):                   # rows that hold nothing and find nothing: junk in either vector
        (held if p % 2 == 0 else match)[i] = outside[p]
    decided = [i for i in rows[:n_held] if match[i] < 0]
    if decided:
        match[decided[-1]] = n_b + 3                        # an old link beside a match that counts as -1
    assert LO.one_to_one(LO.clean(held, n_b)) and LO.one_to_one(LO.clean(match, n_b))
    return held.astype(np.int32), match.astype(np.int32)


def old_links(held, match, n_b):
    """Rows whose old link is neither replaced nor displaced: the rows rule 3 decides, and their columns."""
    h, m = LO.clean(held, n_b), LO.clean(match, n_b)
    taken = np.zeros(n_b + 1, dtype=bool)
    taken[m[m >= 0]] = True
    rows = np.nonzero((m < 0) & (h >= 0) & ~taken[np.maximum(h, 0)])[0]
    return rows, h[rows]


def _padded(x, kpad, ld):
    """[n, ld]: x, zeros up to kpad, NaN beyond (nothing may read past kpad)."""
    out = np.full((x.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :kpad] = 0.0
    out[:, :x.shape[1]] = x
    return out


DELTAS = ((), (2,), (3, 4), (1, 2, 2), (2, 3, 6))           # differences of norm 0, 2, 5, 3, 7 (halved below)


def exact_case(rng, n_a, n_b, kpad, metric, with_terms, dim=None, pad=(0, 0), poison=True, dense=True):
    """Entries are multiples of 1/2 of magnitude <= 5: a product is a multiple of 1/4 below 2^5, a sum of 320 of them below 2^14
    quarter units, so every partial sum of every order is exact in f32; so are the squared norms and sq_a + sq_b - 2 dot.  Row i
    of a held pair (i, j) is b[j] plus a difference of norm 0, 1, 5/2, 3/2 or 7/2: the squared distance is a perfect square and
    its root exact.  Terms are multiples of 1/8 in [-2, 2].  `retain` is a value that occurs, so that `>=` is not `>`.
    poison: one old link gets a NaN in its row of a, and with terms another a NaN row term.
    dense=False: case["S"] is the vector of the held pairs' values (links_oracle.values_held), not the matrix."""
    dim = kpad if dim is None else dim
    held, match = structure(rng, n_a, n_b)
    a = rng.integers(-4, 5, (n_a, dim)).astype(np.float32) * 0.5
    b = rng.integers(-4, 5, (n_b, dim)).astype(np.float32) * 0.5
    h = LO.clean(held, n_b)
    for i in np.nonzero(h >= 0)[0]:
        d = DELTAS[int(rng.integers(len(DELTAS)))]
        a[i] = b[h[i]]
        a[i, rng.choice(dim, size=len(d), replace=False)] += np.array(d, dtype=np.float32) * 0.5 * rng.choice((-1.0, 1.0), size=len(d))
    terms = None
    if with_terms:
        terms = (rng.integers(-16, 17, n_a).astype(np.float32) / 8, rng.integers(-16, 17, n_b).astype(np.float32) / 8)
    rows, cols = old_links(held, match, n_b)
    if poison and len(rows) > 2:
        a[rows[0], int(rng.integers(dim))] = np.nan
        if with_terms:
            terms[0][rows[1]] = np.nan
    sq_a, sq_b = (a * a).sum(1, dtype=np.float32), (b * b).sum(1, dtype=np.float32)
    case = dict(n_a=n_a, n_b=n_b, kpad=kpad, metric=metric, held=held, match=match, a=_padded(a, kpad, kpad + pad[0]),
                b=_padded(b, kpad, kpad + pad[1]), sq_a=sq_a if metric == LO.EUCLIDEAN else None,
                sq_b=sq_b if metric == LO.EUCLIDEAN else None, terms=terms)
    on = np.nonzero(h >= 0)[0]                             # the held pairs: no other value is ever formed
    if dense:
        S = LO.values(case["a"][:, :kpad], case["b"][:, :kpad], metric, sq_a, sq_b, terms)
        of = S[np.arange(n_a), np.maximum(h, 0)]
    else:
        S = of = LO.values_held(case["a"][:, :kpad], case["b"][:, :kpad], held, metric, sq_a, sq_b, terms)
    assert np.array_equal(of[on].astype(np.float32).astype(np.float64), of[on], equal_nan=True)       # exact in f32
    case["S"] = S.astype(np.float32)
    mine = of[rows]
    mine = mine[~np.isnan(mine)]
    case["retain"] = float(np.sort(mine)[len(mine) // 2]) if len(mine) else 0.0
    new_score = (rng.integers(-64, 65, n_a) / 32).astype(np.float32)
    if n_a > 2:                                             # copied bit for bit: a signed zero, an infinity, a NaN with a payload
        new_score[:3].view(np.uint32)[:] = (0x80000000, 0x7F800000, 0x7FC00123)
    case["new_score"] = new_score
    return case


def value_bound(a, b, kpad, metric, sq_a=None, sq_b=None, terms=None):
    """float64 [n_a, n_b]: a bound of |device value - float64 value| for finite operands, u = 2^-24.
    dot: lane l sums kpad / 16 products by fma (one rounding each), four tree adds follow: kpad / 16 + 4 roundings on the longest
    path, |error| <= gamma(kpad / 16 + 4) sum |a_k b_k|, gamma(n) = n u / (1 - n u).
    euclidean: x = sq_a + sq_b - 2 dot takes two roundings (one if contracted), |error| <= 2 e_dot + u (sq_a + sq_b) + u |x|;
    r = sqrt(x), correctly rounded: e_x / sqrt(x) + u r (the root's slope is at most 1 / sqrt(x) between x and its image, both
    positive: callers keep x away from 0); 1 - r: u |v| more.
    terms: 2 v exact; two subtractions: 2 e_v + u |2 v - t_row| + u |s|.  (1 + 2^-20) covers the products of these terms."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = kpad // 16 + 4
    e = n * U / (1.0 - n * U) * (np.abs(a64) @ np.abs(b64).T)
    v = a64 @ b64.T
    if metric == LO.EUCLIDEAN:
        ss = np.asarray(sq_a, dtype=np.float64)[:, None] + np.asarray(sq_b, dtype=np.float64)[None, :]
        x = ss - 2.0 * v
        e_x = 2.0 * e + U * ss + U * np.abs(x)
        r = np.sqrt(np.maximum(x, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(x > e_x, e_x / r + U * r + U * np.abs(1.0 - r), np.inf)       # x within its error of 0: no bound
        v = 1.0 - r
    if terms is not None:
        t = 2.0 * v - np.asarray(terms[0], dtype=np.float64)[:, None]
        e = 2.0 * e + U * np.abs(t) + U * np.abs(t - np.asarray(terms[1], dtype=np.float64)[None, :])
    return e * (1.0 + 2.0 ** -20)


def unit_case(rng, n_a, n_b, kpad, metric, with_terms, dim=None, pad=(0, 0)):
    """Random unit rows (normalised in f32), f32 squared norms, terms uniform in [0.2, 0.8).  `retain` is the middle of the gap
    of the old links' float64 values nearest their median among the gaps wider than 64 bounds; case["margin"] / case["bound"] are
    the least distance of such a value from `retain` and the largest bound among them: margin > bound, so the kept / expired
    decision of the device equals the float64 one.  (Between unit rows the squared distance is near 2, far from 0.)"""
    dim = kpad if dim is None else dim
    held, match = structure(rng, n_a, n_b)

    def unit(n):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        return (x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    a, b = unit(n_a), unit(n_b)
    sq_a, sq_b = (a * a).sum(1, dtype=np.float32), (b * b).sum(1, dtype=np.float32)
    terms = (rng.uniform(0.2, 0.8, n_a).astype(np.float32), rng.uniform(0.2, 0.8, n_b).astype(np.float32)) if with_terms else None
    case = dict(n_a=n_a, n_b=n_b, kpad=kpad, metric=metric, held=held, match=match, a=_padded(a, kpad, kpad + pad[0]),
                b=_padded(b, kpad, kpad + pad[1]), sq_a=sq_a if metric == LO.EUCLIDEAN else None,
                sq_b=sq_b if metric == LO.EUCLIDEAN else None, terms=terms)
    case["S"] = LO.values(a, b, metric, sq_a, sq_b, terms)
    case["E"] = value_bound(a, b, kpad, metric, sq_a, sq_b, terms)
    rows, cols = old_links(held, match, n_b)
    mine, bound = np.sort(case["S"][rows, cols]), float(case["E"][rows, cols].max()) if len(rows) else 0.0
    case["retain"], case["margin"], case["bound"] = 0.0, np.inf, bound
    if len(mine) == 1:
        case["retain"] = float(mine[0]) - 1.0
        case["margin"] = 1.0
    elif len(mine) > 1:
        gaps = np.diff(mine)
        wide = np.nonzero(gaps > 128 * bound)[0]
        k = wide[np.argmin(np.abs(wide - len(mine) // 2))]
        case["retain"] = float(np.float32((mine[k] + mine[k + 1]) / 2))
        case["margin"] = float(np.abs(mine - case["retain"]).min())
    case["new_score"] = rng.standard_normal(n_a).astype(np.float32)
    return case


def exact_cases(kpad, metric, with_terms):
    """The exact tier of one (width, metric, terms): every size, the larger ones with lda / ldb beyond kpad and, every other size,
    a ragged dim below kpad."""
    rng = np.random.default_rng([kpad, metric, int(with_terms), 1])
    return [exact_case(rng, n_a, n_b, kpad, metric, with_terms, dim=kpad - 3 if k % 2 else None, pad=(4, 8) if k % 3 else (0, 0))
            for k, (n_a, n_b) in enumerate(SIZES)]


def pass_edge_case(kpad, metric, with_terms):
    """One exact case of PASS_ROWS + 1 rows: its first PASS_ROWS rows are a case of their own (exactly one pass of the grid)."""
    rng = np.random.default_rng([kpad, metric, int(with_terms), 3])
    c = exact_case(rng, PASS_ROWS + 1, PASS_ROWS + 9, kpad, metric, with_terms, dense=False)
    # the one row of the second pass is to be an old link that is kept: it changes places with such a row
    rows, _ = old_links(c["held"], c["match"], c["n_b"])
    k, last = rows[c["S"][rows] >= c["retain"]][0], PASS_ROWS
    for x in (c["held"], c["match"], c["a"], c["S"], c["new_score"], c["sq_a"], None if c["terms"] is None else c["terms"][0]):
        if x is not None:
            x[[k, last]] = x[[last, k]]
    return c


def first_rows(case, n):
    """The case of the first n rows of a dense=False case (a sub-vector of a one-to-one vector is one-to-one)."""
    cut = lambda x: None if x is None else x[:n]
    out = dict(case, n_a=n, held=case["held"][:n], match=case["match"][:n], a=case["a"][:n], sq_a=cut(case["sq_a"]), S=case["S"][:n],
               new_score=case["new_score"][:n])
    if case["terms"] is not None:
        out["terms"] = (case["terms"][0][:n], case["terms"][1])
    return out


UNIT_SIZES = ((5, 5), (65, 65), (257, 257), (130, 33))


def unit_cases(kpad, metric, with_terms):
    rng = np.random.default_rng([kpad, metric, int(with_terms), 2])
    return [unit_case(rng, n_a, n_b, kpad, metric, with_terms, dim=kpad - 5 if k % 2 else None, pad=(8, 4) if k % 2 else (0, 0))
            for k, (n_a, n_b) in enumerate(UNIT_SIZES)]
