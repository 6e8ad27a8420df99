"""The reference-alone half of the exact optimizer-kernel tests (update_cases.py): the table covers every instantiation,
chunk, row shape, listed value and grid cap of the update kernels; every exact case stays within 24 bits; the float32
arithmetic, run one rounding at a time (plain and with the two a - b c contracted), equals the float64 reference where that
is exact and stays within half the derived bound where it is not; and every mutant of the reference -- a kernel that is
subtly wrong -- breaks the comparison the device test makes, on at least one case.  Bitmap tables (BIT_CASES, BIT_LAUNCHES: the
visited set from a bitmap row and the step's positives) are held the same way, with nine mutants of their own.  Runs without a GPU."""
import numpy as np
import pytest

import rows_cases as rc
import update_cases as uc

f32, f64 = np.float32, np.float64
ROWS = uc.cases_of("rows")
SMALL = [c for c in ROWS if c.n <= 20000]


def test_table_covers_the_shapes():
    assert uc.STRIDES == tuple(16 * f for f in uc.FPLS) and len(uc.FPLS) == 13
    assert uc.N_CHUNK4 == (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257) and uc.N_LARGE == (16385, 16400, 16448, 16449)
    assert uc.chunk_of(16384) == 4 and uc.chunk_of(16385) == 16 and uc.chunk_of(16385, 64) == 64 and uc.chunk_of(16384, 64) == 4
    assert uc.chunk_of(500000) == 16 and uc.chunk_of(uc.N_BY_SIZE) == 64
    for stride in uc.STRIDES:
        dims = set(rc.table_dims(stride))
        assert dims >= {stride, stride - 1, stride - 15} and (stride != 80 or 75 in dims)
        mine = [c for c in ROWS if c.stride == stride]
        small = [c for c in mine if c.copies == 1 and not c.n_hot and not c.n_ranks and not c.special and c.n <= 257]
        assert {(c.dim, c.n) for c in small} >= {(d, n) for d in dims for n in uc.N_CHUNK4}, stride
        assert {c.pattern for c in small} == set(uc.PATTERNS), stride
        assert {c.lr for c in small} >= {1.0, 0.25} and {c.refcount for c in small} == {True, False}
        assert any(c.n == uc.N_SMALL_MAX for c in mine)
        for ch in (16, 64):                                       # both forced chunks at every row count, on this stride's row shape
            big = [c for c in mine if c.chunk == ch and c.copies == 1 and not c.tier2]
            assert {c.n for c in big} >= set(uc.N_LARGE), (stride, ch)
            assert {uc.row_shape(c.n, stride, ch) for c in big} == {"quarter" if ch == 16 else ("wave" if stride % 64 == 0 else "quarter64")}
        assert {c.copies for c in mine if c.n <= 257} >= set(uc.COPIES)
        assert {(c.chunk, c.copies) for c in mine if c.n > uc.N_SMALL_MAX} >= {(16, 2), (64, 2)}
        t2 = [c for c in mine if c.special and c.n == 17]           # tier 2 at every width and ragged dim, with the planted rows
        assert {(c.dim, c.opt, c.normalize) for c in t2} == {(d, o, n) for d in dims for o, n in (("sgd", 1), ("adagrad", 0), ("adagrad", 1))}
    assert (1, 16) in {(c.dim, c.stride) for c in ROWS if c.special}                                    # dim = 1
    assert {uc.row_shape(c.n, c.stride, c.chunk) for c in ROWS if c.copies == 8} == {"quarter", "quarter64", "wave"}
    assert {uc.row_shape(c.n, c.stride, c.chunk) for c in ROWS if c.special} == {"quarter", "wave"}
    assert {c.lr for c in ROWS if c.tier2} == set(uc.LRS)
    by_size = uc.cases_of("rows", tag="bysize")
    assert [(c.n, c.stride, c.chunk, c.pattern) for c in by_size] == [(500001, 64, 0, "sparse")]
    hub = [c for c in ROWS if c.n_hot]                              # hub rows: both HB, every copy count, all three row shapes
    assert {(c.n_hot, c.hot_copies) for c in hub} == {(h, k) for h in uc.N_HOT for k in uc.HOT_COPIES}
    for pick in (lambda c: c.stride <= 80, lambda c: c.stride > 80):
        assert {c.hot_copies for c in hub if pick(c)} == set(uc.HOT_COPIES)
    assert {uc.row_shape(c.n, c.stride, c.chunk) for c in hub} == {"quarter", "quarter64", "wave"}
    for c in hub:
        o = uc.rows_ops(c)
        rows = np.nonzero(o.hot_slot[:c.n] >= 0)[0]
        assert len(rows) == c.n_hot and (o.hot_slot[:c.n] == -1).sum() == c.n - c.n_hot
        if c.n_hot > 1 and o.touched is not None:
            assert o.visited[rows].any() and not o.visited[rows].all(), c.id
    assert {bool(uc.rows_ops(c).visited[uc.rows_ops(c).hot_slot[:c.n] >= 0].any()) for c in hub if c.n_hot == 1} == {True, False}
    shard = [c for c in ROWS if c.n_ranks]
    assert {c.n_ranks for c in shard} == set(uc.N_RANKS)
    assert {uc.row_shape(c.n, c.stride, c.chunk, shard=True) for c in shard} == {"quarter", "quarter64"}
    for c in shard:
        o = uc.rows_ops(c)
        k = (o.slot_of[:c.n] >= 0).sum(1)
        assert (k == 0).any() and (k == 1).any() and ((k > 1).any() or c.n_ranks == 1), c.id
        assert c.n_ranks <= 16 or (o.slot_of[:c.n, 16:] >= 0).any()
        assert o.grad is None and o.touched is None and np.array_equal(o.visited, k > 0)
    names = {L.name: L for L in uc.LAUNCHES}                       # launches of several tables
    assert {len(L.tables) for L in uc.LAUNCHES} >= {2, 3, 4}
    assert [t.n for t in names["chunks-4-16-4"].tables] == [20, 16400, 4]
    assert [uc.chunk_of(t.n, t.chunk) for t in names["chunks-4-16-4"].tables] == [4, 16, 4]
    assert [uc.chunk_of(t.n, t.chunk) for t in names["chunks-4-64-4-wave"].tables] == [4, 64, 4]
    assert {tuple(t.n == 0 for t in L.tables) for L in uc.LAUNCHES} >= {(True, False, False), (False, True, False), (False, False, True),
                                                                        (True, True)}
    assert any(len({t.normalize for t in L.tables}) == 2 for L in uc.LAUNCHES)
    assert any({(bool(t.n_ranks), t.copies) for t in L.tables} == {(True, 1), (False, 8)} for L in uc.LAUNCHES)
    counts = [L.count for L in uc.LAUNCHES if L.count]
    assert sorted(cc.total for cc in counts) == sorted(uc.COUNT_TOTALS) and max(cc.total for cc in counts) > 1024 * uc.BLOCK
    for cc in counts:
        o = uc.count_ops(cc)
        n_neg = cc.n_pos * cc.neg_per_pos
        g = np.arange(n_neg) // max(cc.neg_per_pos, 1)
        assert n_neg < 100 or ((o.neg_h[:n_neg] == o.pos_h[g]).any() and (o.neg_t[:n_neg] == o.pos_t[g]).any())
    # the dense rules
    for stride in uc.STRIDES:
        mine = uc.cases_of("dense_rows", stride=stride)
        assert {(c.dim, c.n) for c in mine} >= {(d, n) for d in rc.table_dims(stride) for n in uc.DENSE_ROWS_N}
        assert {(c.opt, c.hyper, c.normalize) for c in mine} == {(o, h, n) for o in ("adam", "adadelta") for h in ("half", "tf") for n in (0, 1)}
    assert uc.DENSE_ROWS_PASS == 131073 and {c.n for c in uc.cases_of("dense_rows", tag="pass")} == {131073}
    assert {c.stride for c in uc.cases_of("dense_rows", tag="pass")} == {16}
    assert uc.DENSE_OPT_N == (1, 255, 256, 257, 524288, 524289) and uc.DENSE_N == (1, 255, 256, 257, 262145)
    assert {(c.n, c.opt, c.hyper) for c in uc.cases_of("dense_opt")} == {(n, o, h) for n in uc.DENSE_OPT_N for o in ("adam", "adadelta")
                                                                          for h in ("half", "tf")}
    assert {(c.n, c.opt, c.lr) for c in uc.cases_of("dense")} == {(n, o, lr) for n in uc.DENSE_N for o in ("sgd", "adagrad") for lr in (1.0, 0.25)}


def test_a_violated_bound_fails():
    b = uc.Bound()
    b.add("fits", 2 ** 24 - 1, 1.0)
    b.check()
    b.add("one too many", 2 ** 24, 1.0)
    with pytest.raises(AssertionError, match="24 bits"):
        b.check()
    # and the exactness test of a row sum: quarters fit, a sum with a 2^-30 term next to 320 sixteenths does not
    assert uc.dyadic_sum_exact(np.array([[0.25, -0.75, 1.0], [0.0, 0.0, 0.0]])).all()
    assert not uc.dyadic_sum_exact(np.array([[20.0, 2.0 ** -30]])).any()
    assert uc.lowbit(np.array([0.75, 0.0, 3 * 2.0 ** -40]))[[0, 2]].tolist() == [0.25, 2.0 ** -40] and np.isinf(uc.lowbit(np.array([0.0])))[0]


def check_operands(c, o):
    n, d, st = c.n, c.dim, c.stride
    assert np.isnan(o.table[n]).all() and np.isnan(o.acc[n]).all() and not o.table[:n, d:].any()
    assert np.array_equal(o.acc[:n, d:], np.full((n, st - d), uc.ACC_PAD)) and (o.acc[:n, :d] > 0).all()
    normal = np.ones(n, bool)
    if c.special and n >= 3:
        normal[1] = False
        assert not o.table[0].any() and (o.table[1, :d] == f32(2.0 ** -30)).all() and (o.table[2].astype(f64) ** 2).sum() == 1.0
        assert o.visited[:3].all() or c.pattern == "none"
    assert rc.is_quarters(o.table[:n][normal])
    if o.grad is not None:
        rows = c.copies * n + c.hot_copies * c.n_hot * bool(c.n_hot)
        assert o.grad.shape == (rows + 1, st) and (o.grad[rows] == uc.SENTINEL).all()
        G = o.grad[:c.copies * n].reshape(c.copies, n, st)
        assert (G[:, ~o.visited] == uc.SENTINEL).all() and rc.is_quarters(G[:, o.visited]) and not G[:, o.visited][..., d:].any()
        if c.n_hot:
            H = o.grad[n:rows].reshape(c.hot_copies, c.n_hot, st)
            on = o.visited[np.argsort(np.where(o.hot_slot[:n] >= 0, o.hot_slot[:n], 1 << 30))[:c.n_hot]]
            assert (H[:, ~on] == uc.SENTINEL).all() and rc.is_quarters(H[:, on])
    if o.touched is not None:
        assert o.touched.shape == (n + 64,) and (o.touched[n:] == uc.TAG).all() and np.array_equal(o.touched[:n] == uc.TAG, o.visited)
    if o.slot_of is not None:
        used = np.zeros(len(o.src_rows), bool)
        for r in range(c.n_ranks):
            s = o.slot_of[:n, r]
            assert len(set(s[s >= 0])) == (s >= 0).sum() and s.max(initial=-1) < o.capacity
            used[r * o.capacity + s[s >= 0]] = True
        assert rc.is_quarters(o.src_rows[used]) and (o.src_rows[~used] == uc.SENTINEL).all() and (o.slot_of[n] == 0).all()
    if o.ref_count is not None:
        assert (o.ref_count > 0).all() and o.ref_count.shape == (n + 1,)


def exercise_rows(c, ratios):
    """Operands, Bound, the identity of the reference with itself, float32 against float64."""
    o = uc.rows_ops(c)
    o.bound.check()
    want = uc.rows_reference(c)
    if c.n > 257 and not c.tier2 and c.n not in (uc.N_SMALL_MAX, uc.N_LARGE[-1]) and c.copies == 1 and not c.n_hot and not c.n_ranks:
        return        # the plain large tables differ from their neighbours in the row count alone: Bound and reference only
    check_operands(c, o)
    problems, _ = uc.check_rows(o, uc.apply_reference(o, want), want)
    assert not problems, (c.id, problems)
    v = want["rows"]
    if c.pattern == "none":
        assert len(v) == 0
    if "grad" in want:
        assert not want["grad"][:c.copies * c.n].reshape(c.copies, c.n, c.stride)[:, v].any()        # every copy of a visited row is zero
        if c.n_hot:
            hs = o.hot_slot[v][o.hot_slot[v] >= 0]
            assert not want["grad"][c.n:-1].reshape(c.hot_copies, c.n_hot, c.stride)[:, hs].any()    # and every hub copy
    if "slot_of" in want:
        assert (want["slot_of"][v] == -1).all() and np.array_equal(want["slot_of"][c.n], o.slot_of[c.n])
    if "ref_count" in want:
        assert not want["ref_count"][v].any() and (np.delete(want["ref_count"], v) > 0).all()
    for mode in ("f32", "fma") if c.tier2 or c.n <= 257 else ("f32",):      # exact cases: contraction changes nothing
        problems, r = uc.check_rows(o, uc.apply_reference(o, uc.rows_reference(c, mode)), want)
        assert not problems, (c.id, mode, problems)
        for k, x in r.items():
            assert x <= 0.5, (c.id, mode, k, x)                   # the emulation stays within half the bound
            key = (c.opt, c.normalize, k)
            ratios[key] = max(ratios.get(key, 0.0), x)
    if c.tier2 and len(v):
        val, err = want["table"]
        assert err is not None and not err[:, c.dim:].any() and not val[:, c.dim:].any()       # pad columns: exactly zero
        assert (err[:, :c.dim] > 0).all() and np.isfinite(err).all()
        if c.opt == "adagrad":
            assert np.array_equal(want["acc"][0][:, c.dim:], o.acc[v][:, c.dim:])              # acc pad: unchanged bit for bit
            assert (want["acc"][1] is None) == (not c.normalize)


@pytest.mark.parametrize("stride", uc.STRIDES)
def test_rows_cases_are_exact_or_bounded(stride):
    ratios = {}
    for c in SMALL:
        if c.stride == stride:
            exercise_rows(c, ratios)
    assert {k[:2] for k in ratios} == {("sgd", 1), ("adagrad", 0), ("adagrad", 1)}, ratios


def test_rows_case_by_size():
    (c,) = uc.cases_of("rows", tag="bysize")
    o = uc.rows_ops(c)
    o.bound.check()
    assert 100 < o.visited.sum() <= 302 and o.visited[0] and o.visited[-1] and uc.row_shape(c.n, c.stride) == "wave"
    want = uc.rows_reference(c)
    assert want["table"][1] is None and len(want["rows"]) == o.visited.sum()


def test_launch_tables_and_the_count_rule():
    for t in uc.launch_tables():
        exercise_rows(t, {})
    for L in uc.LAUNCHES:
        refs = uc.launch_reference(L)
        assert len(refs) == len(L.tables)
        if L.name == "all-empty":
            assert sum(uc.launch_blocks(L)) == 0
    cc = uc.CountCase(85, 2)
    o = uc.count_ops(cc)
    slow = o.ref_count.copy()
    for i in range(cc.n_pos):
        slow[o.pos_h[i]] += 1
        slow[o.pos_t[i]] += 1
        for k in range(cc.neg_per_pos):
            n = i * cc.neg_per_pos + k
            slow[o.neg_h[n]] += o.neg_h[n] != o.pos_h[i]
            slow[o.neg_t[n]] += o.neg_t[n] != o.pos_t[i]
    assert np.array_equal(uc.count_reference(cc), slow) and slow[cc.n_ent] == o.ref_count[cc.n_ent]


def dense_full(c, o, step):
    return {k: np.concatenate([np.asarray(v[0], dtype=f32), getattr(o, k)[c.n:]]) for k, v in step.items()}


@pytest.mark.parametrize("kernel", ("dense_rows", "dense_opt", "dense"))
def test_dense_cases_are_exact_or_bounded(kernel):
    seen_exact, unbounded = set(), []
    for c in uc.cases_of(kernel):
        o = uc.dense_ops(c)
        o.bound.check()
        n, d = c.n, c.dim
        assert np.isnan(o.table[n]).all() and not o.table[:n, d:].any() and all((g[n] == uc.SENTINEL).all() and not g[:n, d:].any() for g in o.grads)
        assert all(rc.is_quarters(g[:n]) and (g[:n] == 0).all(1).any() == (n > 3) for g in o.grads)
        if kernel == "dense_rows":
            assert (o.s1[:n, d:] == uc.SENTINEL).all() and (o.s2[:n, d:] == uc.SENTINEL).all() and not o.s1[:n, :d].any()
        want = uc.dense_reference(c)
        assert len(want) == (1 if kernel == "dense" else uc.STEPS)
        exact = uc.dense_exact(c)
        seen_exact |= {(c.opt, name) for name in exact}
        if uc.unbounded(want) > 0:
            unbounded.append(c)
        for step in want:
            for name, (val, err) in step.items():
                assert (err is None) == (name in exact), (c.id, name)
                assert np.array_equal(bits32(val[:, d:]), bits32(getattr(o, name)[:n, d:])), (c.id, name)     # pad: 0 / SENTINEL stay
        for mode in ("f32", "fma"):
            for w, g in zip(want, uc.dense_reference(c, mode)):
                problems, r = uc.check_dense(o, dense_full(c, o, g), w, n)
                assert not problems and all(x <= 0.5 for x in r.values()), (c.id, mode, problems, r)
    if kernel == "dense_rows":      # only where the Jacobian cancels the gradient to rounding noise does Adam's quotient lose its bound
        assert seen_exact == {("adam", "s1"), ("adam", "s2"), ("adadelta", "s1")}
        assert unbounded and all(c.opt == "adam" and c.normalize for c in unbounded) and len(unbounded) <= 4
    else:
        assert not unbounded


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.int32)


def test_adagrad_pad_needs_a_positive_accumulator():
    """The sentence in section (2) of the header: 0 rsq(0) is NaN, so accumulator pad columns must be positive (0.1)."""
    ar = uc.Arith("f32")
    with np.errstate(divide="ignore", invalid="ignore"):
        w, a = uc.rule_adagrad(ar, ar.lift([0.0, 0.0]), ar.lift([0.0, 0.0]), ar.lift([0.0, uc.ACC_PAD]), 0.25)
    assert np.isnan(w[0]) and w[1] == 0 and a[1] == uc.ACC_PAD
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "multike_hip.h")) as f:
        assert "accumulator pad columns must be positive" in " ".join(f.read().split())


# ----------------------------------------------------------------------------------------------------- the mutants
def broken_by(mutant, cases):
    """The cases on which a kernel with this fault fails the comparison of the device test."""
    out = []
    for c in cases:
        o = uc.rows_ops(c)
        problems, _ = uc.check_rows(o, uc.apply_reference(o, uc.rows_reference(c, mutant=mutant)), uc.rows_reference(c))
        if problems:
            out.append((c, problems))
    return out


PICK = {
    "skip_last_copy": lambda c: c.copies > 1 and c.n <= 65,
    "copies_not_zeroed": lambda c: c.copies > 1 and c.n <= 65,
    "last_hub_twice": lambda c: c.n_hot and c.n <= 65,
    "coef_one_inv": lambda c: c.normalize and c.n == 17 and c.stride in (16, 80),
    "keep_projection": lambda c: c.normalize and c.special and c.n == 17 and c.stride in (16, 80, 320),
    "old_acc": lambda c: c.opt == "adagrad" and c.n == 17 and c.stride in (16, 80),
    "stale_tag": lambda c: c.pattern == "old" and c.n <= 257 and c.stride in (16, 80),
    "skip_fifth_bit": lambda c: c.n > 16384 and c.stride == 16 and not c.n_ranks,
    "pad_written": lambda c: c.dim < c.stride and c.n <= 17 and c.stride in (16, 80),
    "reset_below_16": lambda c: c.n_ranks and c.n <= 65,
    "refcount_all": lambda c: c.refcount and c.n <= 65 and c.stride in (16, 80),
}


@pytest.mark.parametrize("mutant", list(PICK))
def test_every_mutant_breaks_a_case(mutant):
    cases = [c for c in ROWS if PICK[mutant](c)]
    hit = broken_by(mutant, cases)
    assert hit, mutant
    if mutant in ("skip_last_copy", "copies_not_zeroed", "last_hub_twice", "stale_tag", "reset_below_16"):
        assert all("exact reference" in " ".join(p) or "differs from the reference" in " ".join(p) for _, p in hit)   # tier 1: bits
    if mutant in ("coef_one_inv", "keep_projection", "old_acc"):
        assert all(any("error / bound" in x for x in p) for _, p in hit)                                                 # tier 2: the bound
    if mutant == "skip_fifth_bit":      # chunks of 16 and of 64, quarter-waves and whole wavefronts alike; never a chunk of 4
        assert {c.chunk for c, _ in hit} == {16, 64}
        assert not broken_by(mutant, [c for c in ROWS if c.n <= 257 and c.stride == 16 and not c.n_ranks and c.copies == 1 and not c.n_hot][:40])
    if mutant == "keep_projection":
        assert any(c.dim >= 15 for c, _ in hit)         # the planted gradient of the 2^-30 row: sum g = dim
    if mutant == "reset_below_16":
        assert {c.n_ranks for c, _ in hit} == {17, 64}
    if mutant == "last_hub_twice":      # every copy count, on both sides of HB
        assert {c.hot_copies for c, _ in hit} == set(uc.HOT_COPIES)


def test_routing_and_count_mutants_break_a_launch():
    hit = []
    for L in uc.LAUNCHES:
        if sum(b > 0 for b in uc.launch_blocks(L)) < 2:
            continue
        want, bad = uc.launch_reference(L), uc.launch_reference(L, mutant="route_first_block")
        for t, w, b in zip(L.tables, want, bad):
            o = uc.rows_ops(t)
            if uc.check_rows(o, uc.apply_reference(o, b), w)[0]:
                hit.append((L.name, t.tag))
    assert ("chunks-4-16-4", "t1") in hit and ("empty-first", "t2") in hit and ("empty-middle", "t2") in hit, hit
    assert not any(tag in ("t0", "e0") for _, tag in hit if _ != "empty-first")           # the first table is never the one that loses rows
    for L in uc.LAUNCHES:
        if L.count and L.count.total > 100:
            assert not np.array_equal(uc.count_reference(L.count), uc.count_reference(L.count, "count_repeats")), L.name


# ----------------------------------------------------------------------------------------------------- bitmap tables
BITS = uc.BIT_CASES
BIT_SMALL = [c for c in BITS if c.n <= 1023]


def list_stats(c, o):
    """Per wavefront of the list segment: how many of its entries name a row with pair 01."""
    pair = uc.pairs_of(o.bits, c.n)
    ent = np.concatenate([o.pos_h[:c.n_pos], o.pos_t[:c.n_pos]])
    return [int((pair[ent[lo:lo + uc.LIST_WAVE]] == 1).sum()) for lo in range(0, 2 * c.n_pos, uc.LIST_WAVE)]


def check_bit_operands(c, o):
    n, P = c.n, c.n_pos
    words = (n + 15) // 16
    assert o.bits.dtype == np.uint32 and o.bits.shape == (words + 2,) and (o.bits[words:] == 0xFFFFFFFF).all()
    if n % 16:
        assert o.bits[words - 1] >> np.uint32(2 * (n % 16)) == (1 << (2 * (16 - n % 16))) - 1          # the junk pairs: 11
    assert o.pos_h.shape == o.pos_t.shape == (P + uc.LIST_PAD,) and o.pos_h.dtype == np.int32
    pair = uc.pairs_of(o.bits, n)
    ent = np.concatenate([o.pos_h[:P], o.pos_t[:P]])
    assert ((ent >= 0) & (ent < n)).all()
    named = np.bincount(ent, minlength=n)
    # the bake's invariant: a pair-01 row is named at most once; a row named twice or by h and t of one positive is 11 or unvisited
    assert (named[pair == 1] <= 1).all()
    assert not ((o.pos_h[:P] == o.pos_t[:P]) & (pair[o.pos_h[:P]] == 1)).any()
    assert np.array_equal(o.visited, (pair == 3) | ((pair == 1) & (named > 0)))
    for pad in (o.pos_h[P:], o.pos_t[P:]):                      # behind the lists: rows a visit would spoil
        assert ((pair[pad] == 1) & (named[pad] == 0)).all() or not ((pair == 1) & (named == 0)).any()
    # the gradient of an unvisited row is SENTINEL whatever its pair
    assert (o.grad[:n][~o.visited] == uc.SENTINEL).all() and rc.is_quarters(o.grad[:n][o.visited])
    assert o.touched is None or (o.touched == uc.TAG).all()
    return pair, named


def test_bitmap_table_covers_the_shapes():
    assert uc.N_BITS == (1, 15, 16, 17, 31, 32, 33, 255, 257) and uc.N_POS == (0, 1, 3, 4, 5, 8, 9, 15, 16, 17, 33, 300) and uc.LIST_WAVE == 8
    small = [c for c in BITS if c.n <= 257 and not c.n_hot]
    assert {c.n_pos for c in small} == set(uc.N_POS) and {c.lpat for c in small} == set(uc.LIST_PATTERNS)
    kinds = {k: 0 for k in ("01 unnamed", "00 named", "10", "10 named", "11 named twice", "h == t")}
    for stride in uc.STRIDES:
        mine = [c for c in BITS if c.stride == stride]
        assert {c.n for c in mine} >= set(uc.N_BITS) | set(uc.N_BITS_LARGE), stride
        assert {(c.n, c.chunk) for c in mine if c.n > uc.N_SMALL_MAX and not c.n_hot} == {(n, ch) for n in uc.N_BITS_LARGE for ch in (16, 64)}
        assert {uc.row_shape(c.n, stride, c.chunk) for c in mine if c.chunk == 64} == {"wave" if stride % 64 == 0 else "quarter64"}
        assert {(c.opt, c.normalize) for c in mine} >= {("sgd", 0), ("sgd", 1), ("adagrad", 0), ("adagrad", 1)}
        assert {c.lr for c in mine} == set(uc.LRS) and {c.refcount for c in mine} == {True, False} and any(c.special for c in mine)
        # every q of the list walk with k = 0 and k = 1, and every q of the chunk walk, at a ragged dim of this width
        deal = [c for c in mine if c.n == 1023 and c.n_pos == 100]
        assert {c.lpat for c in deal} == {"q0", "q1", "q2", "q3"} and {c.pattern for c in deal} == {"q0", "q1", "q2"}
        assert all(c.dim < stride for c in deal)
        for c in deal:
            q = int(c.lpat[1])
            st = list_stats(c, uc.rows_ops(c))
            assert len(st) == 25 and st == [4 * (i % 2) + 1 + q for i in range(25)], (c.id, st[:6])
        large = [c for c in mine if c.n > uc.N_SMALL_MAX and not c.n_hot]          # the chunk walk's q patterns where a chunk has 16 and 64 pairs
        assert {c.pattern for c in large} == {"q0", "q1", "q2", "q3"} and all(c.dim < stride for c in large)
    for c in BITS:
        if c.n > 1023 and c.stride not in (16, 80, 64):
            continue
        o = uc.rows_ops(c)
        pair, named = check_bit_operands(c, o)
        kinds["01 unnamed"] += int(((pair == 1) & (named == 0)).any())
        kinds["00 named"] += int(((pair == 0) & (named > 0)).any())
        kinds["10"] += int(((pair == 2) & (named == 0)).any())
        kinds["10 named"] += int(((pair == 2) & (named > 0)).any())
        kinds["11 named twice"] += int(((pair == 3) & (named > 1)).any())
        kinds["h == t"] += int((o.pos_h[:c.n_pos] == o.pos_t[:c.n_pos]).any())
        if c.lpat == "all" and c.n_pos >= 4 and c.n >= 255 and c.pattern not in ("all", "q3"):
            assert list_stats(c, o)[0] == uc.LIST_WAVE                                # all eight entries of a wavefront set
        if c.lpat == "none":
            assert not any(list_stats(c, o))
        if c.special and c.lpat != "none":
            assert o.visited[:3].all() and pair[1] == 1 and pair[0] == 3          # the 2^-30 row goes through the list
        if c.n_hot:
            hub = np.nonzero(o.hot_slot[:c.n] >= 0)[0]
            assert len(hub) == c.n_hot
            by_list, by_chunk = hub[(pair[hub] == 1) & o.visited[hub]], hub[pair[hub] == 3]
            assert (len(by_list) >= 1 and len(by_chunk) >= 1) if c.n_hot > 1 else (len(by_list) + len(by_chunk) == 1), c.id
    assert all(kinds.values()), kinds
    hub = [c for c in BITS if c.n_hot]
    assert {(c.n_hot, c.hot_copies) for c in hub if c.n == 65} == {(h, k) for h in uc.N_HOT for k in uc.HOT_COPIES}
    assert {uc.row_shape(c.n, c.stride, c.chunk) for c in hub} == {"quarter", "quarter64", "wave"}
    one = [uc.pairs_of(uc.rows_ops(c).bits, c.n)[uc.rows_ops(c).hot_slot[:c.n] >= 0][0] for c in hub if c.n_hot == 1 and c.n == 65]
    assert set(one) == {1, 3}                                   # the single hub row: through the list, and through the chunk walk
    # launches: production (flagged relation table with copies, then the bitmap table), with the rider, alone, without positives
    names = {L.name: L for L in uc.BIT_LAUNCHES}
    prod = [L for L in uc.BIT_LAUNCHES if L.name.startswith("production-s")]
    assert {(L.tables[0].copies, L.tables[0].bits, L.tables[1].bits) for L in prod} == {(2, False, True), (8, False, True)}
    assert sorted(L.count.total for L in uc.BIT_LAUNCHES if L.count)[:3] == [1, 255, 257] and sum(bool(L.count) for L in uc.BIT_LAUNCHES) == 4
    assert all(uc.list_blocks(L) > 0 and L.tables[1].bits for L in uc.BIT_LAUNCHES if L.count)
    assert len(names["bitmap-alone"].tables) == 1 and names["bitmap-no-positives"].tables[1].n_pos == 0
    assert uc.list_blocks(names["bitmap-no-positives"]) == 0 and uc.list_blocks(names["bitmap-alone"]) == 3
    assert {uc.list_blocks(uc.Launch("x", (c,))) for c in small} >= {0, 1, 2, 19}      # partial last block of 32 entries: 2 n_pos = 34, 66, 600


@pytest.mark.parametrize("stride", uc.STRIDES)
def test_bitmap_cases_are_exact_or_bounded(stride):
    ratios = {}
    for c in BITS:
        if c.stride == stride and (c.n <= 1023 or c.chunk == 64):
            o = uc.rows_ops(c)
            o.bound.check()
            want = uc.rows_reference(c)
            assert np.array_equal(want["rows"], np.nonzero(o.visited)[0]), c.id
            problems, _ = uc.check_rows(o, uc.apply_reference(o, want), want)
            assert not problems, (c.id, problems)
            assert not want["grad"][:c.n][want["rows"]].any() and (np.delete(want["grad"][:c.n], want["rows"], 0) == uc.SENTINEL).all()
            if c.n > 1023:
                continue
            for mode in ("f32", "fma"):
                problems, r = uc.check_rows(o, uc.apply_reference(o, uc.rows_reference(c, mode)), want)
                assert not problems, (c.id, mode, problems)
                for k, x in r.items():
                    assert x <= 0.5, (c.id, mode, k, x)
                    ratios[(c.opt, c.normalize, k)] = max(ratios.get((c.opt, c.normalize, k), 0.0), x)
    assert {k[:2] for k in ratios} == {("sgd", 1), ("adagrad", 0), ("adagrad", 1)}, ratios


def test_bitmap_launches():
    for L in uc.BIT_LAUNCHES:
        for t, want in zip(L.tables, uc.launch_reference(L)):
            o = uc.rows_ops(t)
            o.bound.check()
            if t.bits:
                check_bit_operands(t, o)
            assert not uc.check_rows(o, uc.apply_reference(o, want), want)[0], (L.name, t.id)


BIT_PICK = {
    "chunk_takes_01": lambda c: c.n <= 1023,
    "list_takes_11": lambda c: c.n <= 1023 and c.n_pos,
    "list_h_only": lambda c: c.n <= 1023 and c.n_pos,
    "tail_not_rebased": lambda c: c.n <= 1023 and c.n_pos,
    "skip_fifth_entry": lambda c: c.n <= 1023 and c.n_pos,
    "drop_last_wave": lambda c: c.n <= 1023 and c.n_pos,
    "pair_word_r5": lambda c: c.n <= 1023,
    "junk_pairs_honoured": lambda c: c.n <= 1023,
}


@pytest.mark.parametrize("mutant", list(BIT_PICK))
def test_every_bitmap_mutant_breaks_a_case(mutant):
    """(The unmutated reference passes the same comparison on every case: test_bitmap_cases_are_exact_or_bounded.)"""
    hit = broken_by(mutant, [c for c in BITS if BIT_PICK[mutant](c)])
    assert len(hit) >= 2, mutant
    ids = {c.id for c, _ in hit}
    if mutant == "skip_fifth_entry":        # only wavefronts with five or more set entries: k = 1 of every q, and "all"
        assert all(max(list_stats(c, uc.rows_ops(c)), default=0) >= 5 for c, _ in hit)
        assert {c.lpat for c, _ in hit} >= {"q0", "q1", "q2", "q3", "all"}
    if mutant == "drop_last_wave":
        assert all((2 * c.n_pos) % uc.LIST_WAVE for c, _ in hit) and {c.n_pos for c, _ in hit} >= {1, 3, 5, 9, 17, 33}
    if mutant == "tail_not_rebased":
        assert {c.n_pos for c, _ in hit} >= {1, 3, 4, 8, 16, 300}
    if mutant == "junk_pairs_honoured":
        assert all(c.n % 16 for c, _ in hit) and {c.n for c, _ in hit} >= {1, 15, 17, 31, 33, 255, 257}
    if mutant == "list_takes_11":
        assert any("exact reference" in " ".join(p) for _, p in hit)
    assert ids


def test_list_blocks_counted_as_update_blocks_breaks_the_first_table():
    hit = []
    for L in uc.BIT_LAUNCHES:
        if not uc.list_blocks(L):
            continue
        for t, w, b in zip(L.tables, uc.launch_reference(L), uc.launch_reference(L, mutant="list_blocks_as_update")):
            o = uc.rows_ops(t)
            if uc.check_rows(o, uc.apply_reference(o, b), w)[0]:
                hit.append((L.name, t.tag))
    assert ("production-s80-c2", "rel") in hit and ("production-count-257", "rel") in hit and ("bitmap-alone", "ent") in hit, hit
    assert set(BIT_PICK) | {"list_blocks_as_update"} == set(uc.BIT_MUTANTS) and len(uc.BIT_MUTANTS) == 9


def test_mutant_list_is_the_issues():
    assert set(PICK) | {"route_first_block", "count_repeats"} == set(uc.MUTANTS) and len(uc.MUTANTS) == 13
