"""mke_links_edit (mke_links.hip, libmultike_links.so: include/multike_links.h) against tests/links_oracle.py on the cases of
tests/links_cases.py: all 13 widths x {inner, euclidean} x {no terms, terms}; rows at the edges of a quarter-wavefront's 4 rows a
wavefront and 16 a workgroup and, at the narrowest and the widest row, of a pass of the capped grid (512 workgroups: 8192 rows
and one more); n_a != n_b both ways, lda / ldb beyond kpad with NaN behind kpad, a ragged dim below kpad with its zero pad.

Exact tier: every value is exact in f32 in any order of the sum, so `out`, `counts` and the bit patterns of `score` equal the
oracle's; all four outputs are poisoned first.
Float64 tier: random unit rows.  The device's value of a pair: lane l of the row's 16 sums its kpad / 16 products by fma in
column order, then ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), the same over p8 .. p15, and the two halves — kpad / 16 + 4
roundings on any path —, then the metric and the re-scoring of mke_rescore.h; links_cases.value_bound counts these roundings and
is not fitted.  No deciding value lies within that bound of `retain` (tests/test_links_cases.py checks the cases), so `out` and
`counts` are exact there too and a kept link's score is within the bound of the float64 value."""
import numpy as np
import pytest
import torch

import links_cases as LC
import links_oracle as LO
from gpu_util import dev_f32, dev_i32

pytestmark = pytest.mark.gpu

POISON = 0x7FC00BAD                                          # a NaN as a float, a column far outside as an int


def _run(c, retain=None, score=True, new_score=True):
    from multike_amd import _lib
    a, b = dev_f32(c["a"]), dev_f32(c["b"])
    f = lambda x: None if x is None else dev_f32(x)
    poison = lambda n: torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    out = (poison(c["n_a"]), poison(c["n_a"]).view(torch.float32) if score else None, poison(c["n_b"]), poison(7))
    terms = c["terms"] or (None, None)
    o, s, counts = _lib.links_edit(dev_i32(c["held"]), dev_i32(c["match"]), a, b, c["kpad"], c["metric"], f(c["sq_a"]), f(c["sq_b"]),
                                   f(terms[0]), f(terms[1]), retain=c["retain"] if retain is None else retain,
                                   new_score=f(c["new_score"]) if new_score else None, out=out)
    assert o is out[0] and s is out[1] and counts is out[3]
    return o.cpu().numpy(), None if s is None else s.cpu().numpy(), counts.cpu().numpy(), out[2].cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("terms", [False, True])
@pytest.mark.parametrize("metric", [LO.INNER, LO.EUCLIDEAN])
@pytest.mark.parametrize("kpad", LC.KPADS)
def test_exact_tier(kpad, metric, terms):
    for c in LC.exact_cases(kpad, metric, terms):
        for retain in (c["retain"], float("-inf")):
            want = LO.edit(c["held"], c["match"], c["S"], retain, c["new_score"])
            out, score, counts, inv = _run(c, retain)
            where = (kpad, metric, terms, c["n_a"], c["n_b"], retain)
            assert np.array_equal(out, want[0]), where
            assert np.array_equal(counts, want[2]), (where, counts, want[2])
            assert np.array_equal(_bits(score), _bits(want[1])), where
            m = LO.clean(c["match"], c["n_b"])
            want_inv = np.full(c["n_b"], -1)
            want_inv[m[m >= 0]] = np.nonzero(m >= 0)[0]
            assert np.array_equal(inv, want_inv), where


@pytest.mark.parametrize("terms", [False, True])
@pytest.mark.parametrize("metric", [LO.INNER, LO.EUCLIDEAN])
@pytest.mark.parametrize("kpad", [LC.KPADS[0], LC.KPADS[-1]])
def test_exact_tier_at_the_edge_of_a_grid_pass(kpad, metric, terms):
    whole = LC.pass_edge_case(kpad, metric, terms)
    for c in (LC.first_rows(whole, LC.PASS_ROWS), whole):
        want = LO.edit(c["held"], c["match"], c["S"], c["retain"], c["new_score"], n_b=c["n_b"])
        out, score, counts, _ = _run(c)
        assert want[0][-1] >= 0 or c is not whole                              # the row of the second pass is a kept link
        assert np.array_equal(out, want[0]) and np.array_equal(counts, want[2]), (c["n_a"], counts, want[2])
        assert np.array_equal(_bits(score), _bits(want[1])), c["n_a"]


@pytest.mark.parametrize("terms", [False, True])
@pytest.mark.parametrize("metric", [LO.INNER, LO.EUCLIDEAN])
@pytest.mark.parametrize("kpad", LC.KPADS)
def test_float64_tier(kpad, metric, terms):
    for c in LC.unit_cases(kpad, metric, terms):
        assert c["margin"] > c["bound"]
        want = LO.edit(c["held"], c["match"], c["S"], c["retain"], c["new_score"])
        out, score, counts, _ = _run(c)
        where = (kpad, metric, terms, c["n_a"], c["n_b"])
        assert np.array_equal(out, want[0]) and np.array_equal(counts, want[2]), where
        rows, cols = LC.old_links(c["held"], c["match"], c["n_b"])
        kept = rows[out[rows] >= 0]
        err = np.abs(score[kept].astype(np.float64) - c["S"][kept, out[kept]])
        print(where, "kept", len(kept), "largest error / bound", float((err / c["E"][kept, out[kept]]).max()) if len(kept) else 0.0)
        assert (err <= c["E"][kept, out[kept]]).all(), where
        rest = np.ones(c["n_a"], dtype=bool)
        rest[kept] = False
        assert np.array_equal(_bits(score[rest]), _bits(want[1][rest])), where       # copied or zero: bit for bit


def test_two_runs_give_the_same_bits_and_optional_arguments():
    c = LC.unit_case(np.random.default_rng(3), 257, 257, 208, LO.EUCLIDEAN, True, dim=200, pad=(4, 4))
    first, again = _run(c), _run(c)
    assert all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y) for x, y in zip(first, again))
    out, score, counts, _ = _run(c, new_score=False)                           # no new_score: a new pair's score is 0
    assert np.array_equal(out, first[0]) and np.array_equal(counts, first[2])
    new = LO.clean(c["match"], 257) >= 0
    assert (_bits(score[new]) == 0).all() and np.array_equal(_bits(score[~new]), _bits(first[1][~new]))
    out, score, counts, _ = _run(c, score=False)                               # no score array
    assert score is None and np.array_equal(out, first[0]) and np.array_equal(counts, first[2])


def test_empty_sides_zero_the_counters_and_nothing_else():
    from multike_amd import _abi_links as al, _lib
    import ctypes as C
    counts = torch.full((7,), POISON, dtype=torch.int32, device="cuda")
    out = torch.full((5,), POISON, dtype=torch.int32, device="cuda")
    for n_a, n_b in ((0, 5), (5, 0), (0, 0)):
        counts.fill_(POISON)
        args = al.mke_links_args(held=None, match=None, n_a=n_a, n_b=n_b, a=None, lda=0, b=None, ldb=0, kpad=0, metric=0, retain=0.0,
                                 out=out.data_ptr(), counts=counts.data_ptr())
        assert _lib.links_lib().mke_links_edit(C.byref(args), _lib._stream()) == 0
        assert counts.cpu().tolist() == [0] * 7 and (out.cpu().numpy() == POISON).all()
    # the binding gives the rows of a set without columns their -1
    from multike_amd.base.bootstrap import edit_links
    a, b = torch.zeros(5, 16, device="cuda"), torch.zeros(0, 16, device="cuda")
    o, s, n = edit_links(np.arange(5), np.arange(5), (a, b, 16, 0, None, None))
    assert o.cpu().tolist() == [-1] * 5 and s.cpu().tolist() == [0.0] * 5 and n.cpu().tolist() == [0] * 7


def test_edit_links_takes_the_operands_of_the_decode():
    """base.bootstrap.edit_links on alignment._mutual_operands' tuple: one preparation for the decode and the edit, CSLS terms
    included; a kept link's score is the decode's own value of the pair up to the two summation orders."""
    from multike_amd.base import alignment, bootstrap
    rng = np.random.default_rng(8)
    n, d = 90, 40
    e1 = rng.standard_normal((n, d)).astype(np.float32)
    e2 = (e1 + 0.3 * rng.standard_normal((n, d))).astype(np.float32)[rng.permutation(n)]
    for csls_k in (0, 3):
        ops = alignment._mutual_operands(e1, e2, "inner", True, csls_k, None)
        assert len(ops) == 7 and (ops[6] is None) == (csls_k == 0)
        match, counts, row_best = alignment._mutual_decode(ops, None)
        m2, c2, rb2 = alignment._mutual(e1, e2, "inner", True, csls_k, None, None)
        assert torch.equal(match, m2) and torch.equal(counts, c2) and torch.equal(row_best, rb2)
        best = alignment._best_value(row_best)
        none = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        out, score, cnt = bootstrap.edit_links(none, match, ops, None, best)
        assert torch.equal(out, match) and cnt.cpu().tolist()[:3] == [counts[0].item(), counts[1].item(), counts[0].item()]
        on = (match >= 0).cpu().numpy()
        assert np.array_equal(_bits(score.cpu().numpy()[on]), _bits(best.cpu().numpy()[on]))
        # the same pairs as an old set with nothing new: all kept, at the sweep's value up to rounding
        out, score, cnt = bootstrap.edit_links(match, none, ops, None)
        assert torch.equal(out, match) and cnt.cpu().tolist() == [counts[0].item(), counts[1].item(), 0, 0, counts[0].item(), 0, 0]
        a, b, kpad, code, _, _, terms = ops
        E = LC.value_bound(a.cpu().numpy(), b.cpu().numpy(), kpad, code, None, None, None if terms is None else tuple(t.cpu().numpy() for t in terms))
        rows = np.nonzero(on)[0]
        # the sweep's own chain (MFMA, k-ordered) has kpad roundings: both values are within their bounds of the float64 one
        wide = E[rows, match.cpu().numpy()[rows]] * (kpad / (kpad // 16 + 4) + 1)
        assert (np.abs(score.cpu().numpy()[rows].astype(np.float64) - best.cpu().numpy()[rows]) <= wide).all()
        with pytest.raises(Exception, match="NaN"):
            bootstrap.edit_links(match, none, ops, float("nan"))
