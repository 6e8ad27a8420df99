"""The reference-alone half of the exact similarity-sweep tests (sweep_cases.py): the table covers every (client, kpad)
instantiation and the edge list, every case is exact in float32, the float32 oracle of the inner modes equals a brute-force
float64 evaluation, the planted structure is really there and the poison lies only outside the logical operand.
Runs without a GPU."""
import numpy as np
import pytest

import sweep_cases as sc

CASES = sc.ALL_CASES
ids = lambda c: c.id


def test_table_covers_every_instantiation():
    assert len({c.id for c in CASES}) == len(CASES)
    assert sc.KPADS == (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)
    for client in sc.CLIENTS:
        mine = sc.cases_of(client)
        for kpad in sc.KPADS:                                   # every width at the two shapes
            bn = sc.bn_for(kpad)
            shapes = {(c.n_a, c.n_b) for c in mine if c.kpad == kpad}
            nb2 = 2 * bn + bn // 2 + 1
            na2 = min(129, nb2) if client in ("rank", "rank_ex", "sim_select", "knn") else 129    # rows that are columns too
            assert {(33, 16 * bn + 1), (na2, nb2)} <= shapes, (client, kpad)
        assert any(c.dim < c.kpad for c in mine) and any(c.dim == c.kpad for c in mine)
        assert {c.L for c in mine} >= {3, 40}
        for kpad in sc.REGIME_KPADS:                            # the edge list for one width of each regime
            bn = sc.bn_for(kpad)
            k = [c for c in mine if c.kpad == kpad]
            assert {c.n_b for c in k} >= {20, bn - 1, bn, bn + 1, 16 * bn, 16 * bn + 1, 33 * bn + 31}, (client, kpad)
            assert {c.n_a for c in k} >= {1, 32, 33, 128, 129, 257}, (client, kpad)
            assert all(c.n_a == c.n_b for c in k if c.n_b == 20)
    assert {sc.regime(k) for k in sc.REGIME_KPADS} == {"double", "single64", "single32"} == {sc.regime(k) for k in sc.KPADS}
    for kpad in sc.REGIME_KPADS:
        of = lambda client: [c for c in sc.cases_of(client) if c.kpad == kpad]
        assert {c.variant for c in of("rank")} == {"ties", "noties"}
        assert {c.mode for c in of("rank_ex")} == set(sc.MODES)
        assert {(c.mode, c.variant) for c in of("stable")} == {(m, v) for m in sc.MODES for v in ("sweep", "sample", "whole", "simmat")}
        sweeps = [c for c in of("stable") if c.variant == "sweep"]
        assert {c.k for c in sweeps if c.n_b <= 1024} >= {1, 100, 128}
        assert any(c.k > 128 for c in of("stable")) and any(c.variant == "whole" and c.k <= 128 for c in of("stable"))
        sel = of("sim_select")
        assert {(c.row_lo, c.row_hi) for c in sel} >= {(1, 34), (100, 229)} and any(c.row_lo == 0 and c.n_a == c.n_b for c in sel)
        assert {c.n_seg for c in sel} == {1, 3, 16}
        bn = sc.bn_for(kpad)
        assert any(c.n_seg > (c.n_b + bn - 1) // bn for c in sel)                  # empty segments
        smp = of("sim_sample")
        assert {c.n_b for c in smp} >= {1, bn + 1, 8 * bn + 1} and any(c.row_lo % 32 for c in smp)
        two = [c for c in smp if c.n_b == 8 * bn + 1][0]
        assert [(b - a + bn - 1) // bn for a, b in sc.chunk_bounds(two)] == [5, 4]
        assert {(c.k, c.mode) for c in of("topk_mean")} >= {(k, m) for k in (1, 7, 32, 33, 300) for m in sc.MODES[:2]}
        assert {c.n_seg for c in of("knn")} >= {1, 2, 4}
        s1 = [c for c in of("rank") if c.n_b == 16 * bn + 1][0]
        assert [(b - a + bn - 1) // bn for a, b in sc.chunk_bounds(s1)] == [9, 8]
        s3 = [c for c in of("rank_ex") if c.n_b == 33 * bn + 31][0]
        assert [(b - a + bn - 1) // bn for a, b in sc.chunk_bounds(s3)] == [12, 12, 10]
    short = [c for c in sc.cases_of("topk_mean") if c.tag == "short-chunk"]
    assert short and all(sc.chunk_bounds(c)[-1][1] - sc.chunk_bounds(c)[-1][0] < c.k <= 32 for c in short)
    assert all(c.n_a <= 300 and (c.n_b <= 2200 or c.tag == "short-chunk") for c in CASES)
    assert sc.LD_EXTRA_A != sc.LD_EXTRA_B and {sc.LD_EXTRA_A, sc.LD_EXTRA_B} == {4, 12}


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_case_is_exact_and_planted(c):
    assert c.L * c.L * c.dim < 2 ** 24 and 4 * c.L * c.L * c.dim < 2 ** 24
    ops = sc.operands(c)
    for m in (ops.A, ops.B):
        assert m.dtype == np.float32 and np.array_equal(m, np.rint(m)) and np.abs(m).max() <= c.L
    assert np.array_equal(ops.sq_a.astype(np.float64), (ops.A.astype(np.float64) ** 2).sum(1))
    assert np.array_equal(ops.sq_b.astype(np.float64), (ops.B.astype(np.float64) ** 2).sum(1))
    for r in (ops.rt, ops.rs):
        assert np.array_equal(r * 8, np.rint(r * 8)) and np.abs(r).max() <= 2
    S = sc.scores(c)
    assert S.dtype == np.float32 and S.shape == (c.n_a, c.n_b) and not np.isnan(S).any()
    if not c.euclidean:                                          # float32, one operation at a time == float64 brute force
        assert np.array_equal(S.astype(np.float64), sc.scores64(c))
    else:                                                        # the radicand is an exact non-negative integer
        r = slice(c.row_lo, c.row_hi)
        w = ops.sq_a[r].astype(np.float64)[:, None] + ops.sq_b.astype(np.float64)[None, :] - 2.0 * sc.int_dots(ops.A[r], ops.B)
        assert w.min() >= 0 and w.max() < 2 ** 24
        if not c.csls:
            assert np.abs(S.astype(np.float64) - (1.0 - np.sqrt(w))).max() <= 2.0 ** -24 * max(1.0, np.sqrt(w.max()))
    # planted structure
    lo = c.row_lo
    z = ops.zero_row - lo
    assert 0 <= z < c.n_a and not ops.A[ops.zero_row].any()
    if c.mode == "inner":
        assert np.all(S[z] == 0)
    bounds = [b for b in sc.chunk_bounds(c) if b[0] < b[1]]
    chunk_of = lambda col: [i for i, (a, b) in enumerate(bounds) if a <= col < b][0]
    if c.n_b >= 12:
        assert ops.dup_cols and len({ops.B[d].tobytes() for d in ops.dup_cols}) == 1
        bn = sc.bn_for(c.kpad)
        assert set(ops.dup_cols) >= {x for x in (bn - 1, bn, c.n_b - 1) if x < c.n_b}
        if len(bounds) >= 2:
            assert {bounds[0][1] - 1, bounds[0][1], bounds[-1][0] - 1, bounds[-1][0]} <= set(ops.dup_cols)
        assert ops.max_cols or c.n_a == 1                       # a lone row is the zero row
    if ops.max_cols:
        m, (c1, c2) = ops.max_row - lo, ops.max_cols
        assert 0 <= m < c.n_a and m != z and c1 < c2 and S[m, c1] == S[m, c2] == S[m].max()
        assert np.argmax(S[m]) == c1 or c.client in sc.SELF_CLIENTS   # (the row itself is a column there)
        if len(bounds) >= 2:
            assert chunk_of(c1) == 0 and chunk_of(c2) == len(bounds) - 1   # the row maximum sits in two chunks
    if c.client in ("rank", "rank_ex"):
        greater, ties, best, _ = sc.rank_oracle(S)
        assert ties.min() >= 1
        if c.n_b >= 12:
            assert ties.max() > 1 and ops.tie and ties[ops.tie[0]] >= 2 and ops.tie[0] != ops.tie[1]
        if c.n_a >= 8:                                           # neither all zero nor hopeless
            assert greater.min() == 0 and greater.max() > 0 and (greater == 0).sum() < c.n_a
    if c.client == "sim_select":
        tau = sc.select_taus(c, S)
        cnt, _ = sc.select_oracle(S, tau, sc.chunk_bounds(c), c.seg_cap)
        if c.n_a >= 4:
            assert (cnt > c.seg_cap).any() and (cnt.sum(1) == 0).any()
        if c.n_a >= 8 and c.n_b >= 64:
            assert ((cnt > 0) & (cnt <= c.seg_cap)).any()
        strict = np.arange(c.n_a) % 4 == 1                       # thresholds equal to an attained value
        assert np.all((S[strict] == tau[strict, None]).any(1))


@pytest.mark.parametrize("c", [c for c in CASES if c.tag in ("s1", "s2", "modes", "samp")], ids=ids)
def test_poison_lies_outside_the_operand(c):
    ops, bn = sc.operands(c), sc.bn_for(c.kpad)
    a_buf, b_buf = sc.buffers(c)
    for buf, mat, extra in ((a_buf, ops.A, sc.LD_EXTRA_A if c.client not in sc.SELF_CLIENTS else sc.LD_EXTRA_B), (b_buf, ops.B, sc.LD_EXTRA_B)):
        n = mat.shape[0]
        assert buf.shape == (n + bn, c.kpad + extra) and buf.dtype == np.float32 and buf.flags.c_contiguous
        assert np.array_equal(buf[:n, :c.dim], mat) and not buf[:n, c.dim:c.kpad].any()
        assert np.isnan(buf[n:]).all() and np.isnan(buf[:, c.kpad:]).all()
        assert np.isnan(buf).sum() == buf.size - n * c.kpad
    g = sc.guarded(ops.sq_b, bn)
    assert g.shape == (c.n_b + bn,) and np.array_equal(g[:c.n_b], ops.sq_b) and np.all(g[c.n_b:] == sc.GUARD)
    # a guard entry read as a squared norm gives similarity 1, as a CSLS term a value above every real one
    one = sc.rescore32(np.zeros((1, 1), np.float32), ops.sq_a[:1], g[-1:], ops.rt[:1], ops.rs[:1], True, False)
    big = sc.rescore32(np.zeros((1, 1), np.float32), ops.sq_a[:1], ops.sq_b[:1], ops.rt[:1], g[-1:], False, True)
    assert one[0, 0] == 1.0 and big[0, 0] > 1e29


def test_both_outcomes_of_the_knn_chain_are_reached():
    seen = set()
    for c in sc.cases_of("knn"):
        if c.n_b > 1100:
            continue
        ops = sc.operands(c)
        S = sc.scores(c)
        samp, m = sc.knn_plan(c)
        tau = sc.kth_largest(S[:, samp], m)
        seen |= set(sc.knn_status_oracle(c, S, tau).tolist())
    assert seen == {0, 1, 2}


def test_stable_sample_cases_flag_some_rows_and_not_all():
    for c in sc.cases_of("stable"):
        if c.variant != "sample" or c.mode != "inner":
            continue
        flags = sc.stable_flags_oracle(c, sc.scores(c), sc.sample_cols_of(c))
        assert 0 < flags.sum() < c.n_a, c.id


def test_list_oracles_on_a_hand_made_row():
    S = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 0.0, np.nan]], dtype=np.float32)
    assert sc.topk_sets(S[:, :6], 2).tolist() == [[1, 2]] and sc.topk_sets(S[:, :6], 4).tolist() == [[0, 1, 2, 4]]
    assert sc.kth_largest(S[:, :6], 4).tolist() == [1.0]
    assert sc.topk_means(S[:, :6], 4).tolist() == [2.5]
    val, col = sc.stable_lists_oracle(S, 7)
    assert col.tolist() == [[1, 2, 4, 0, 5, 3, -1]] and val[0, :6].tolist() == [3, 3, 3, 1, 0, -2] and val[0, 6] == -np.inf
    cnt, st = sc.select_oracle(S[:, :6], np.array([1.0], np.float32), [(0, 4), (4, 6), (6, 6)], 1)
    assert cnt.tolist() == [[2, 1, 0]] and [x.tolist() for x in st[0]] == [[1], [4], []]
    cnt, _ = sc.select_oracle(S[:, :6], np.array([1.0], np.float32), [(0, 6)], 8, strict=False)
    assert cnt.tolist() == [[4]]
    g, t, b, v = sc.rank_oracle(np.array([[0, 0, 0], [5, 1, 5], [2, 2, 1]], dtype=np.float32))
    assert g.tolist() == [0, 2, 2] and t.tolist() == [3, 1, 1] and b.tolist() == [0, 0, 0] and v.tolist() == [0, 5, 2]
