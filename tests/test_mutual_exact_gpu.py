"""mke_align_mutual + mke_mutual_pairs, bit-exact: the `rank_ex` cases of sweep_cases.py (integer operands in NaN-poisoned
buffers, guard entries behind every vector: every similarity is exact in float32) against the NumPy oracle of
mutual_oracle.py, and against the `best` words of mke_align_rank_ex on the same buffers.  Three families of the file's own:
column ties ACROSS row blocks (the table's shapes hardly have any), n_a > n_b (the table has none: its gold column needs
n_b >= n_a), and NaN / -inf through the re-scoring terms.  Assertions are equality of 64-bit words and of integers."""
import numpy as np
import pytest

import mutual_oracle as MO
import sweep_cases as sc

pytestmark = pytest.mark.gpu

ids = lambda c: c.id
FLAGS = (0, 1, 2, 3)             # the default column fold and MKE_MUTUAL_NO_LDS_FOLD / MKE_MUTUAL_FILTER: the same words


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Problem:
    """Operands of one call on the device, poisoned and guarded as sweep_cases lays them out, and the oracle's score matrix."""

    def __init__(self, c, A=None, sq_a=None, rt=None, rs=None):
        from multike_amd import _lib
        ops, bn = sc.operands(c), sc.bn_for(c.kpad)
        A = ops.A if A is None else A
        sq_a, rt, rs = (ops.sq_a if sq_a is None else sq_a), (ops.rt if rt is None else rt), (ops.rs if rs is None else rs)
        self.c, self.n_a, self.n_b = c, A.shape[0], ops.B.shape[0]
        self.a = _dev(sc.embed(A, c.kpad, sc.LD_EXTRA_A, bn))[:self.n_a]
        self.b = _dev(sc.embed(ops.B, c.kpad, sc.LD_EXTRA_B, bn))[:self.n_b]
        g = lambda v: _dev(sc.guarded(v, bn))[:v.shape[0]]
        self.code = _lib.METRIC_EUCLIDEAN if c.euclidean else _lib.METRIC_INNER
        self.sq_a, self.sq_b = (g(sq_a), g(ops.sq_b)) if c.euclidean else (None, None)
        self.rt, self.rs = (g(rt), g(rs)) if c.csls else (None, None)
        with np.errstate(invalid="ignore"):
            self.S = sc.rescore32(sc.int_dots(A, ops.B).astype(np.float32), sq_a, ops.sq_b, rt, rs, c.euclidean, c.csls)

    def mutual(self, flags=0):
        from multike_amd import _lib
        return _lib.align_mutual(self.a, self.b, self.c.kpad, self.code, self.sq_a, self.sq_b, self.rt, self.rs, flags=flags)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _index(words):
    return (np.uint64(0xFFFFFFFF) - (words & np.uint64(0xFFFFFFFF))).astype(np.int64)


def _check(p, flags=(0,)):
    """Words and pairings of a problem against the oracle; returns the oracle's (match, counts) without a threshold."""
    import torch
    from multike_amd import _lib
    want_rb, want_cb = MO.words(p.S)
    for f in flags:
        rb, cb = p.mutual(f)
        got_rb, got_cb = _u64(rb), _u64(cb)
        live_r, live_c = got_rb != 0, got_cb != 0
        assert (_index(got_rb[live_r]) < p.n_b).all() and (_index(got_cb[live_c]) < p.n_a).all(), f   # no guard row or column is named
        assert np.array_equal(got_rb, want_rb), (f, np.nonzero(got_rb != want_rb)[0][:8])
        assert np.array_equal(got_cb, want_cb), (f, np.nonzero(got_cb != want_cb)[0][:8])
    rb, cb = p.mutual(0)
    free, (matched, _) = MO.pairs(p.S)
    attained = np.sort(p.S[np.arange(p.n_a), np.maximum(free, 0)][free >= 0])
    thresholds = [-np.inf, np.inf] + ([float(attained[len(attained) // 2])] if matched else [])   # one attained value: >= is inclusive
    for thr in thresholds:
        want_match, want_counts = MO.pairs(p.S, np.float32(thr))
        match, counts = _lib.mutual_pairs(rb, cb, thr)
        assert match.dtype == torch.int32 and np.array_equal(match.cpu().numpy(), want_match), thr
        assert tuple(counts.cpu().tolist()) == want_counts, thr
        if thr == np.inf:
            assert want_counts == (0, 0)
        elif thr != -np.inf:
            assert 0 < want_counts[0] <= matched                                # the pair that attains the threshold stays
    return free, matched


@pytest.mark.parametrize("c", sc.cases_of("rank_ex"), ids=ids)
def test_align_mutual_on_the_rank_ex_cases(c):
    import torch
    from multike_amd import _lib
    p = Problem(c)
    assert np.array_equal(p.S.view(np.int32), sc.scores(c).view(np.int32))      # the table's own oracle matrix
    _, matched = _check(p)
    assert 0 < matched and (matched < c.n_a or c.n_a == 1)                      # never none, never all (but the one-row shape): the assertions bite
    rank, ties = (torch.zeros(c.n_a, dtype=torch.int32, device="cuda") for _ in range(2))
    best = torch.zeros(c.n_a, dtype=torch.int64, device="cuda")
    _lib.align_rank_ex(p.a, p.b, c.kpad, rank, ties, best, p.code, p.sq_a, p.sq_b, p.rt, p.rs)
    rb, cb = p.mutual()
    assert torch.equal(rb, best)                                                # word for word the rank kernel's `best`
    rb2, cb2 = p.mutual()
    assert torch.equal(rb, rb2) and torch.equal(cb, cb2)


def _own_case(tag, kpad, n_a, n_b, mode, ragged=True, L=3):
    return sc.Case("rank_ex", tag, kpad, kpad - 5 if ragged else kpad, n_a, n_b, mode=mode, L=L)


@pytest.mark.parametrize("mode", ["inner+csls", "euclidean"])
@pytest.mark.parametrize("kpad", [80, 320])
def test_column_ties_across_row_blocks(kpad, mode):
    """257 rows = three row blocks.  The row holding the planted maximum is copied into rows 130 and 256 (with its row term and
    squared norm): every planted column's maximum is attained in all three blocks, whose atomics arrive in any order; the
    lowest row must win.  An ordinary row is copied into another block as well."""
    c = _own_case("na257-ties", kpad, 257, 16 * sc.bn_for(kpad) + 1, mode)
    ops = sc.operands(c)
    assert ops.max_row >= 0 and ops.max_row < 128 and len(ops.dup_cols) >= 4
    A, sq_a, rt = ops.A.copy(), ops.sq_a.copy(), ops.rt.copy()
    plain = 9                                                                   # B[9] == A[9]: column 9's best row
    assert plain not in (ops.zero_row, ops.max_row)
    for src, dst in ((ops.max_row, 130), (ops.max_row, 256), (plain, 200)):
        A[dst], sq_a[dst], rt[dst] = A[src], sq_a[src], rt[src]
    p = Problem(c, A=A, sq_a=sq_a, rt=rt)
    _, col_row = MO.bests(p.S)
    dups = np.array(ops.dup_cols)
    assert (col_row[dups] == ops.max_row).all()                                 # the precondition: the ties exist, the lowest row is the oracle's
    assert (p.S[130, dups] == p.S[ops.max_row, dups]).all() and (p.S[256, dups] == p.S[ops.max_row, dups]).all()
    tied = np.nonzero((p.S[plain] == p.S.max(0)) & (col_row == plain))[0]       # ordinary columns whose maximum rows 9 and 200 share
    assert len(tied) > 0 and (p.S[200, tied] == p.S[plain, tied]).all()
    _check(p, FLAGS)
    _, cb = p.mutual()
    got = _index(_u64(cb))
    assert (got[dups] == ops.max_row).all() and (got[tied] == plain).all()


@pytest.mark.parametrize("kpad,shape,mode", [(80, "257x20", "inner"), (320, "257x20", "euclidean+csls"),
                                             (80, "129xBN+1", "euclidean"), (320, "129xBN+1", "inner+csls")])
def test_more_rows_than_columns(kpad, shape, mode):
    n_a, n_b = (257, 20) if shape == "257x20" else (129, sc.bn_for(kpad) + 1)
    p = Problem(_own_case("tall", kpad, n_a, n_b, mode, ragged=n_b == 20, L=40 if n_b == 20 else 3))
    _, matched = _check(p, FLAGS)
    assert 0 < matched <= n_b


@pytest.mark.parametrize("kpad,mode", [(80, "inner+csls"), (320, "inner+csls"), (128, "euclidean+csls")])
def test_nan_and_minus_inf_through_the_rescoring_terms(kpad, mode):
    """The operands stay exact; the terms carry the specials.  One row term NaN: that row's similarities are all NaN, its word
    stays 0 and no column names it.  One column term NaN: that column's word stays 0 and no row names it.  One column term
    +inf: that column's values are -inf (NaN in the NaN row): it publishes (-inf, row 0)."""
    bn = sc.bn_for(kpad)
    c = _own_case("specials", kpad, 129, 2 * bn + bn // 2 + 1, mode)
    ops = sc.operands(c)
    rt, rs = ops.rt.copy(), ops.rs.copy()
    nan_row, nan_col, inf_col = 40, bn + 3, 2 * bn + 1                          # the second and the third tile
    assert not {nan_col, inf_col} & set(ops.dup_cols)
    rt[nan_row], rs[nan_col], rs[inf_col] = np.nan, np.nan, np.inf
    p = Problem(c, rt=rt, rs=rs)
    assert np.isnan(p.S[nan_row]).all() and np.isnan(p.S[:, nan_col]).all()
    assert (p.S[np.arange(129) != nan_row, inf_col] == -np.inf).all()
    _check(p, FLAGS)
    rb, cb = (_u64(t) for t in p.mutual())
    assert rb[nan_row] == 0 and cb[nan_col] == 0
    assert not (_index(cb[cb != 0]) == nan_row).any() and not (_index(rb[rb != 0]) == nan_col).any()
    assert cb[inf_col] == np.uint64((0x007FFFFF << 32) | 0xFFFFFFFF)            # ordered(-inf), row 0
    # a row of -inf: its term +inf; it publishes (-inf, the lowest column that is not NaN)
    rt[nan_row] = np.inf
    p = Problem(c, rt=rt, rs=rs)
    _check(p)
    rb, _ = (_u64(t) for t in p.mutual())
    assert rb[nan_row] == np.uint64((0x007FFFFF << 32) | 0xFFFFFFFF)            # (-inf, column 0)


def test_empty_sides_and_out_words():
    import torch
    from multike_amd import _lib
    a = torch.zeros(5, 16, device="cuda")
    e = torch.zeros(0, 16, device="cuda")
    for x, y in ((a, e), (e, a), (e, e)):
        rb, cb = _lib.align_mutual(x, y, 16)
        assert rb.shape == (x.shape[0],) and cb.shape == (y.shape[0],) and not rb.any() and not cb.any()
        match, counts = _lib.mutual_pairs(rb, cb)
        assert match.tolist() == [-1] * x.shape[0] and counts.tolist() == [0, 0]
    rb, cb = _lib.align_mutual(a, a, 16)                                         # all similarities 0: everybody's best is index 0
    match, counts = _lib.mutual_pairs(rb, cb, 0.0)
    assert match.tolist() == [0, -1, -1, -1, -1] and counts.tolist() == [1, 1]
    match, counts = _lib.mutual_pairs(rb, cb, 1e-30)
    assert match.tolist() == [-1] * 5 and counts.tolist() == [0, 0]
