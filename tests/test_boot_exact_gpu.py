"""mke_boot_partner and mke_swap_triples on the GPU against the definitions of tests/boot_oracle.py.  Everything here is an
integer or a copied float, so every comparison is bit for bit.

Sizes: the edges of a tile (MKE_SWAP_TILE = one wavefront), of a workgroup (four tiles) and of several, 70,001, and one list
whose tile counts need more than one tile of the scan: rocPRIM scans 8-byte items in tiles of 256 threads x 8 items = 2048 by
default and no configuration of it exceeds 1024 threads x 16 items = 16384, so 2 x 16384 tiles + 77 triples span at least three."""
import numpy as np
import pytest

import boot_oracle as BO

pytestmark = pytest.mark.gpu

from multike_amd._lib import SWAP_TILE as T  # noqa: E402

SIZES = sorted({0, 1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 3 * T + 5, 255, 256, 257, 70_001})
BIG = 2 * 16384 * T + 77
PATTERNS = ("none", "every", "third", "heads", "tails", "self_loop")
SENTINEL, GUARD = -777, 96
_cache = {}


def _case(n, pattern):
    """(h, p, t, table, weight): triples over few enough entities that they repeat, ids -1 and n_entities (exactly) planted in
    both entity columns, and a table whose >= 0 entries follow the pattern (the kernel copies a table's values, it does not
    ask them to be symmetric)."""
    key = (n, pattern)
    if key not in _cache:
        rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n % 9973)
        n_ent = max(8, n // 3 + 3)
        h, t = rng.integers(0, n_ent, n), rng.integers(0, n_ent, n)
        p = rng.integers(0, 50, n)
        if n >= 8:
            spots = rng.permutation(n)[:4]
            h[spots[0]], h[spots[1]], t[spots[2]], t[spots[3]] = -1, n_ent, -1, n_ent
        values = rng.integers(0, n_ent, n_ent)
        if pattern == "none":
            on = np.zeros(n_ent, dtype=bool)
        elif pattern == "every":
            on = np.ones(n_ent, dtype=bool)
        elif pattern in ("third", "self_loop"):
            on = rng.random(n_ent) < 1 / 3
        else:
            col = h if pattern == "heads" else t
            on = np.zeros(n_ent, dtype=bool)
            on[col[(col >= 0) & (col < n_ent)]] = True
        if pattern == "self_loop" and n:
            loops = rng.permutation(n)[:max(1, n // 7)]
            h[loops] = np.clip(h[loops], 0, n_ent - 1)
            t[loops] = h[loops]
            on[h[loops[::2]]] = True                           # every other loop is linked
        table = np.where(on, values, -1).astype(np.int32)
        weight = rng.random(n_ent).astype(np.float32)
        _cache[key] = tuple(x.astype(np.int32) for x in (h, p, t)) + (table, weight)
    return _cache[key]


def _oracle(case, heads_only, weighted):
    h, p, t, table, weight = case
    fn = BO.swap if len(h) <= 4096 else BO.swap_vector
    return fn(h, p, t, table, heads_only=heads_only, weight=weight if weighted else None)


def _device(case):
    import torch
    key = ("dev", id(case))
    if key not in _cache:
        _cache[key] = (case, tuple(torch.as_tensor(x, device="cuda") for x in case))
    return _cache[key][1]


def _run(case, heads_only, weighted, capacity=None):
    """-> (rows [cap + GUARD, 3], w or None, count): outputs allocated GUARD words longer than the capacity, sentinel-filled."""
    import torch
    from multike_amd import _lib
    h, p, t, table, weight = _device(case)
    n = h.numel()
    cap = (n if heads_only else 2 * n) if capacity is None else capacity
    out = tuple(torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)) + (
        torch.full((cap + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda") if weighted else None,)
    cols, w, count = _lib.swap_triples(h, p, t, table, heads_only=heads_only, weight=weight if weighted else None, capacity=cap, out=out)
    return torch.stack(cols, dim=1).cpu().numpy(), None if w is None else w.cpu().numpy(), int(count.item())


def _assert_equal(got, want, cap):
    rows, w, count = got
    want_rows, want_w = want
    m = len(want_rows)
    assert count == m                                         # the full count whatever the capacity
    k = min(m, cap)
    assert np.array_equal(rows[:k], want_rows[:k])
    assert (rows[k:] == SENTINEL).all()                       # nothing from min(count, capacity) on, the guard words included
    if want_w is not None:
        assert np.array_equal(w[:k].view(np.int32), want_w[:k].view(np.int32)) and (w[k:] == SENTINEL).all()
    else:
        assert w is None


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_swap_equals_the_oracle(n, pattern):
    case = _case(n, pattern)
    for heads_only in (False, True):
        want = _oracle(case, heads_only, True)
        if n >= 64 and pattern not in ("none",) and not (heads_only and pattern == "tails"):
            assert 0 < len(want[0])
        if pattern == "none":
            assert len(want[0]) == 0
        if pattern == "every" and n >= 64:
            assert len(want[0]) >= (1 if heads_only else 2) * (n - 4)          # all but the planted out-of-range ids
        cap = n if heads_only else 2 * n
        _assert_equal(_run(case, heads_only, True), want, cap)
        _assert_equal(_run(case, heads_only, False), (want[0], None), cap)


def test_the_two_forms_of_the_oracle_agree_at_the_size_that_switches():
    case = _case(70_001, "self_loop")
    for heads_only in (False, True):
        a, aw = BO.swap(*case[:4], heads_only=heads_only, weight=case[4])
        b, bw = BO.swap_vector(*case[:4], heads_only=heads_only, weight=case[4])
        assert np.array_equal(a, b) and np.array_equal(aw, bw)
    h, _, t, table, _ = case
    loops = (h == t) & (h >= 0) & (table[np.clip(h, 0, len(table) - 1)] >= 0)
    assert loops.sum() > 100                                   # linked self-loops are there: two entries each, one end replaced


@pytest.mark.parametrize("n", [129, 3 * T + 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_capacity_below_the_count(n, weighted):
    case = _case(n, "every")
    want = _oracle(case, False, weighted)
    m = len(want[0])
    assert m > n
    for cap in (m, m - 1, 0):                                  # exact, one short (the last entry is not stored), count only
        _assert_equal(_run(case, False, weighted, capacity=cap), want, cap)
    want = _oracle(case, True, weighted)
    for cap in (len(want[0]), len(want[0]) - 1, 0):
        _assert_equal(_run(case, True, weighted, capacity=cap), want, cap)


def test_more_than_one_tile_of_the_scan_and_two_runs_are_the_same_bits():
    import torch
    case = _case(BIG, "third")
    want = _oracle(case, False, True)
    assert len(want[0]) > BIG // 2
    first = _run(case, False, True)
    _assert_equal(first, want, 2 * BIG)
    again = _run(case, False, True)
    assert first[2] == again[2] and np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.int32), again[1].view(np.int32))
    _assert_equal(_run(case, True, False), (_oracle(case, True, False)[0], None), BIG)
    torch.cuda.synchronize()


def test_host_surface_builds_the_list_in_hbm():
    """base.bootstrap.swap_triples: the device columns, and the host() form a reader of the list gets, are both the oracle's."""
    import torch
    from multike_amd.base.bootstrap import swap_triples
    case = _case(3 * T + 5, "third")
    h, p, t, table, weight = _device(case)
    for heads_only in (False, True):
        want, want_w = _oracle(case, heads_only, True)
        lst, n = swap_triples(np.stack(case[:3], axis=1), table, heads_only=heads_only)         # NumPy [n, 3] in
        assert n == len(lst) == len(want) and lst.dev is not None and not lst.weighted
        assert all(c.is_cuda and c.dtype == torch.int32 for c in lst.dev[0])
        assert np.array_equal(torch.stack(lst.dev[0], dim=1).cpu().numpy(), want)
        assert np.array_equal(lst.cols, want) and lst.w is None
        lst, n = swap_triples((h, p, t), table, heads_only=heads_only, weight=weight)           # device columns in
        assert lst.weighted and np.array_equal(lst.dev[1].cpu().numpy(), want_w)
        assert np.array_equal(lst.cols, want) and np.array_equal(lst.w.astype(np.float32), want_w)
    empty, n = swap_triples(np.zeros((0, 3), dtype=np.int64), table)
    assert n == 0 and len(empty) == 0 and empty.cols.shape == (0, 3)


PARTNER_CASES = {
    # name: (n_a, n_b, n_entities)
    "square": (300, 300, 700), "more_rows": (513, 200, 900), "more_columns": (90, 257, 400), "no_rows": (0, 40, 50), "no_columns": (40, 0, 50),
}


@pytest.mark.parametrize("name", sorted(PARTNER_CASES))
def test_boot_partner_equals_the_oracle(name):
    import torch
    from multike_amd import _lib
    from multike_amd.base.bootstrap import partner_table
    n_a, n_b, n_ent = PARTNER_CASES[name]
    rng = np.random.default_rng(len(name))
    ids = rng.permutation(n_ent)
    ids_a, ids_b = ids[:n_a].astype(np.int32), ids[n_a:n_a + n_b].astype(np.int32)           # distinct within and across the sides
    match = np.full(n_a, -1, dtype=np.int32)
    k = min(n_a, n_b) * 2 // 3
    rows = rng.permutation(n_a)[:k]
    match[rows] = rng.permutation(n_b)[:k]                                                     # one-to-one, a third unmatched
    if k > 8:
        free = np.setdiff1d(np.arange(n_a), rows)
        match[free[0]] = n_b                      # a match past the columns (exactly n_b, and far past): ignored
        match[free[1]] = n_b + 1000
        match[free[2]] = -5                       # below -1: ignored as -1 is
        ids_a[rows[0]], ids_a[rows[1]] = -1, n_ent            # ids outside the table, on either side: the pair leaves no trace
        ids_b[match[rows[2]]], ids_b[match[rows[3]]] = -1, n_ent
    want = BO.partner(match, ids_a, ids_b, n_ent)
    assert (want >= 0).sum() == (2 * (k - 4) if k > 8 else 0)
    stale = torch.arange(n_ent, dtype=torch.int32, device="cuda")                              # a previous table: gone after the call
    dev = lambda x: torch.as_tensor(x, device="cuda")
    got = _lib.boot_partner(dev(match), dev(ids_a), dev(ids_b), n_ent, out=stale)
    assert got is stale and np.array_equal(got.cpu().numpy(), want)
    fresh = partner_table(match, ids_a, ids_b, n_ent)                                          # NumPy in, a fresh device table out
    assert fresh.is_cuda and fresh.dtype == torch.int32 and np.array_equal(fresh.cpu().numpy(), want)
    assert np.array_equal(partner_table(dev(match).long(), dev(ids_a), ids_b, n_ent).cpu().numpy(), want)


def test_bootstrap_links_is_one_mutual_decode_and_its_table():
    """Rows with a private coordinate each: the mutual pairs are the planted permutation, whatever the threshold below 1."""
    import torch
    from multike_amd.base.bootstrap import bootstrap_links
    n1, n2, n_ent = 70, 90, 400
    rng = np.random.default_rng(5)
    col_of = rng.permutation(n2)[:n1]
    e1, e2 = np.zeros((n1, 96), dtype=np.float32), np.zeros((n2, 96), dtype=np.float32)
    e1[np.arange(n1), np.arange(n1)] = 1.0
    e2[col_of, np.arange(n1)] = 1.0
    e2[:, 95] += 0.25                                          # a direction every column shares and no row has
    ids = rng.permutation(n_ent)
    ids1, ids2 = ids[:n1], ids[n1:n1 + n2]
    partner, match, counts, score = bootstrap_links(e1, torch.as_tensor(e2, device="cuda"), ids1, ids2, n_ent, threshold=0.5, scores=True)
    assert np.array_equal(match.cpu().numpy(), col_of) and counts.cpu().tolist() == [n1, int((col_of == np.arange(n1)).sum())]
    assert np.array_equal(partner.cpu().numpy(), BO.partner(col_of, ids1, ids2, n_ent))
    assert score.shape == (n1,) and float(score.min()) > 0.9
    partner, match, counts = bootstrap_links(e1, e2, ids1, ids2, n_ent, threshold=0.99)       # 1 / sqrt(1 + 1/16) = 0.970 < 0.99
    assert (match.cpu().numpy() == -1).all() and (partner.cpu().numpy() == -1).all() and counts.cpu().tolist() == [0, 0]
