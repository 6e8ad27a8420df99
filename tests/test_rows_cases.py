"""The reference-alone half of the exact row-kernel tests (rows_cases.py): the table covers every instantiation, shape and
row count of the kernels of mke_rows.hip, every exact case stays within 24 bits (so float32 arithmetic in two different
summation orders equals the float64 reference bit for bit), the poison lies only outside the logical operands, the tolerance
tier's smallest term cannot hide in its loss tolerance, and the widths no kernel exists for are refused before any launch.
Runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import rows_cases as rc
from oracle import multike_oracle as mo

CASES = rc.ALL_CASES
ids = lambda c: c.id
RT = 3e-6                          # loss tolerance of the generic logistic tier (tests/test_losses_gpu.py)


def test_table_covers_the_shapes():
    assert rc.STRIDES == (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)
    assert rc.COUNTS == (0, 1, 15, 16, 17, 255, 257)
    assert rc.PASS_LOSS == (32768, 32769, 70001) and rc.PASS_ROWS == (65536, 65537, 140001)
    assert {rc.dense_fpl(d) for d in rc.DENSE_DIMS} == set(rc.FPLS)            # every instantiation of the dense kernels
    assert set(rc.DENSE_DIMS) >= {1, 15, 16, 17, 75, 128, 129, 144, 145, 176, 177, 208, 209, 256, 257, 304, 320}
    assert {(d + 15) // 16 for d in rc.DENSE_DIMS} >= {9, 11, 14, 15, 17, 18, 19}      # widths that round up through dense_fpl
    assert rc.dense_fpl(129) == 10 and rc.dense_fpl(177) == 12 and rc.dense_fpl(209) == 16 and rc.dense_fpl(257) == 20
    # dense kernels: every dim x ld x count, both signs with and without weights, the no-gradient path
    for kernel in ("galign", "glog"):
        mine = rc.cases_of(kernel)
        for dim in rc.DENSE_DIMS:
            k = [c for c in mine if c.dim == dim]
            assert {(c.width, c.n) for c in k} >= {(dim + e, n) for e in rc.LD_EXTRA for n in rc.COUNTS}, (kernel, dim)
            assert any(c.variant.startswith("nograd") for c in k)
            if kernel == "glog":
                assert {(c.sign, c.variant) for c in k} >= {(s, v) for s in (1, -1) for v in ("w", "now")}, dim
        big = [c for c in mine if c.n > 1000]
        assert {c.n for c in big} == set(rc.PASS_LOSS) and all(c.dim <= 16 for c in big)
        assert any(c.width > c.dim for c in big) and any(c.variant.startswith("nograd") or kernel == "glog" for c in big)
    assert {c.sign for c in rc.cases_of("glog") if c.n > 1000} == {1, -1}
    # table kernels: every stride x its dims x count
    for stride in rc.STRIDES:
        dims = set(rc.table_dims(stride))
        assert dims >= {stride, stride - 1, stride - 15} and (stride != 80 or 75 in dims)
        al = rc.cases_of("align", width=stride)
        assert {(c.dim, c.n) for c in al} >= {(d, n) for d in dims for n in rc.COUNTS}
        assert {c.variant for c in al if c.n >= 15} == set(rc.ALIGN_PATTERNS), stride
        assert {c.weight for c in al} == set(rc.WEIGHTS)
        for var in ("copy", "norm"):
            g = rc.cases_of("gather", width=stride, variant=var)
            assert {(c.dim, c.n) for c in g} >= {(d, n) for d in dims for n in rc.COUNTS}
            assert {c.idx for c in g if c.n >= 15} == {"null", "rep"}
        seen = set()
        for c in rc.cases_of("gather", width=stride, variant="norm"):
            seen |= set(rc.gather_ops(c).special)
        assert seen == {"zero", "tiny", "underflow", "unit"}, stride
        pr = rc.cases_of("probe", width=stride)
        assert {(c.variant, c.n) for c in pr} >= {(v, n) for v in ("a", "ab", "abc") for n in rc.COUNTS}
    heavy = rc.cases_of("align", tag="heavy")
    assert {(c.rows, c.n) for c in heavy} >= {(7, 500), (3000, 4000)} and any(c.variant == "self" for c in heavy)
    ap = rc.cases_of("align", tag="pass")
    assert {c.n for c in ap} == set(rc.PASS_LOSS) and all(c.dim <= 16 for c in ap)
    assert {c.variant for c in ap} >= {"dup", "self", "loss_only", "same"}
    for kernel in ("gather", "probe"):
        big = [c for c in rc.cases_of(kernel) if c.n > 1000]
        assert {c.n for c in big} == set(rc.PASS_ROWS) and all(c.dim <= 16 and c.variant != "norm" for c in big)
    assert {c.idx for c in rc.cases_of("gather", tag="pass")} == {"null", "rep"}
    st = rc.cases_of("steps")                                                     # k_align_batch: every stride, ragged dims among them
    assert {c.width for c in st} == set(rc.STRIDES) and (75, 80) in {(c.dim, c.width) for c in st}
    assert {c.width - c.dim for c in st} >= {0, 1, 15} and all(rc.dense_fpl(c.dim) * 16 == c.width for c in st)
    assert all(c.n <= 257 or c.dim <= 16 or c.tag == "heavy" for c in CASES)      # large n only at narrow rows
    # the column guard of the dense loads: with ld = dim + 16 and the tail row a load without it stays inside the buffer
    for dim in rc.DENSE_DIMS:
        assert rc.dense_fpl(dim) * 16 <= 2 * (dim + 16)


def test_a_violated_bound_fails():
    b = rc.Bound()
    b.add("fits", 2 ** 24 - 1, 1.0)
    b.check()
    b.add("one too many", 2 ** 24, 1.0)
    with pytest.raises(AssertionError, match="24 bits"):
        b.check()
    b = rc.Bound()
    b.add("unit is no power of two", 1.0, 0.3)
    with pytest.raises(AssertionError):
        b.check()


def _eq(a32, b64):
    """float32 result == float64 reference, bit for bit after the conversion (and the conversion itself exact)."""
    a32 = np.asarray(a32)
    assert a32.dtype == np.float32
    return np.array_equal(a32.astype(np.float64), np.asarray(b64, dtype=np.float64))


def _loss32(x32, order):
    return rc.thread_sums32(x32, rc.LOSS_BLOCKS, order).astype(np.float64).sum()


@pytest.mark.parametrize("c", rc.cases_of("galign"), ids=ids)
def test_gathered_alignment_case_is_exact(c):
    o = rc.galign_ops(c)
    o.bound.check()
    assert rc.is_quarters(o.a) and rc.is_quarters(o.b) and o.a.shape == (c.n, c.dim)
    a, b = o.a.astype(np.float32), o.b.astype(np.float32)
    d = a - b
    for order in ("lanes", "reverse"):
        x = rc.rowsum32(d * d, order)
        assert _loss32(x, order) == o.loss
    assert _eq(d * np.float32(2.0), o.ga)
    assert o.loss == mo.alignment_loss(o.a, o.b)
    buf = rc.poisoned(a, c.width)
    assert buf.shape == (c.n + 1, c.width) and np.array_equal(buf[:c.n, :c.dim], a)
    assert np.isnan(buf).sum() == buf.size - c.n * c.dim
    if c.n > 2:
        assert not d[1].any() and np.all(np.abs(d[2]) == 2.0)


@pytest.mark.parametrize("c", rc.cases_of("glog"), ids=ids)
def test_saturated_logistic_case_is_exact(c):
    o = rc.glog_ops(c)
    o.bound.check()
    for m in (o.h, o.r, o.t):
        assert rc.is_quarters(m, o.L) and m.shape == (c.n, c.dim)
    assert o.L == 1 or c.dim < 15
    h, r, t = (m.astype(np.float32) for m in (o.h, o.r, o.t))
    e = (h + r) - t                                             # the kernel's order
    assert _eq(e, o.h + o.r - o.t)
    w = np.ones(c.n, np.float32) if o.w is None else o.w.astype(np.float32)
    assert (o.w is None) == c.variant.endswith("now")
    assert np.all(np.log2(w) == np.rint(np.log2(w)))
    thr = rc.SAT_POS if c.sign > 0 else rc.SAT_NEG
    for order in ("lanes", "reverse"):
        x = rc.rowsum32(e * e, order)
        assert _eq(x, o.x) and np.array_equal(o.x, np.rint(o.x)) and (c.n == 0 or o.x.min() >= thr)
        # softplus_f / sigmoid_f in float32, with IEEE exp / log / reciprocal in place of the device's fast ones
        z = np.float32(c.sign) * x
        with np.errstate(over="ignore"):
            one = np.float32(1.0) + np.exp(-np.abs(z))
            term = np.maximum(z, np.float32(0.0)) + np.log(one)
            sig = np.float32(1.0) / (np.float32(1.0) + np.exp(-z))
        assert np.all(one == 1.0) and np.all(sig == (1.0 if c.sign > 0 else 0.0))
        assert _loss32(w * term, order) == o.loss
        coef = np.float32(2.0) * np.float32(c.sign) * w * sig
        assert np.array_equal(e * coef[:, None], o.gh.astype(np.float32))     # == : the sign of a zero is open
    with np.errstate(over="ignore"):
        ref = mo.logistic_term_grads(o.h, o.r, o.t, float(c.sign), o.w)
    if c.sign > 0:     # float64 knows exp(-32): the saturated values are its limit, reached to well below float32 resolution
        np.testing.assert_allclose(ref[0], o.loss, rtol=1e-13, atol=0)
        np.testing.assert_allclose(ref[1], o.gh, rtol=1e-13, atol=0)
    else:
        assert abs(ref[0]) <= c.n * 1e-55 and (c.n == 0 or np.abs(ref[1]).max() < 1e-50) and o.loss == 0.0 and not o.gh.any()


@pytest.mark.parametrize("c", rc.cases_of("gather"), ids=ids)
def test_gather_case(c):
    o = rc.gather_ops(c)
    assert o.table.shape == (c.rows, c.width) and o.table.dtype == np.float32
    assert (o.idx is None) == (c.idx == "null")
    src = np.arange(c.n) if o.idx is None else o.idx
    assert len(src) == c.n and (c.n == 0 or (src.min() >= 0 and src.max() < c.rows))
    if c.idx == "rep" and c.n >= 15:
        assert len(np.unique(src)) < c.n                        # repeated ids
    if c.variant == "copy":
        assert np.isnan(o.table[:, c.dim:]).all() and rc.is_quarters(o.table[:, :c.dim])
        assert o.ref.dtype == np.float32 and np.array_equal(o.ref, o.table[src, :c.dim])
        return
    assert not o.table[:, c.dim:].any()                         # the normalised read sums the whole stride
    rows64 = o.table[src, :c.dim].astype(np.float64)
    assert np.array_equal(o.ref, mo.l2_normalize_rows(rows64))
    t64 = o.table.astype(np.float64)
    ssq32 = (o.table * o.table).sum(1)
    assert not o.table[0].any()
    assert np.all(o.table[1, :c.dim] == np.float32(2.0 ** -30)) and 0 < (t64[1] ** 2).sum() < rc.L2_EPS
    assert ssq32[2] == 0.0 and o.table[2, 0] != 0.0             # the squares underflow in float32
    assert (t64[3] ** 2).sum() == 1.0
    for name, at in o.special.items():
        got = o.ref[at]
        if name == "zero":
            assert not got.any()
        elif name == "unit":
            assert np.array_equal(got, rows64[at])
        else:
            np.testing.assert_allclose(got, rows64[at] * 1e6, rtol=1e-12)


@pytest.mark.parametrize("c", rc.cases_of("probe"), ids=ids)
def test_probe_case_is_exact(c):
    o = rc.probe_ops(c)
    o.bound.check()
    mats = [m for m in (o.a, o.b, o.c) if m is not None]
    assert len(mats) == len(c.variant) and all(rc.is_quarters(m) and m.shape == (c.rows, c.width) for m in mats)
    zero = np.zeros_like(o.a)
    b, cc = (o.b if o.b is not None else zero), (o.c if o.c is not None else zero)
    assert _eq(rc.rowsum32((o.a + b) + cc, "lanes")[o.idx], o.ref)
    assert _eq(rc.rowsum32(o.a + (b + cc), "reverse")[o.idx], o.ref)
    assert len(o.idx) == c.n and (c.n < 15 or len(np.unique(o.idx)) < c.n)


@pytest.mark.parametrize("c", rc.cases_of("align"), ids=ids)
def test_align_case_is_exact(c):
    o = rc.align_ops(c)
    o.bound.check()
    for t in (o.ta, o.tb):
        assert t.shape == (c.rows, c.width) and rc.is_quarters(t[:, :c.dim]) and not t[:, c.dim:].any()
    assert np.log2(c.weight) == np.rint(np.log2(c.weight))
    for order in ("lanes", "reverse"):
        loss, ga, gb = rc.align_f32(c, order)
        assert loss == o.loss and _eq(ga, o.ga) and _eq(gb, o.gb)
    A, B = o.ta.astype(np.float64), o.tb.astype(np.float64)
    L, ga, gb = mo.alignment_step_dense(A, B, None, None, o.ia, o.ib, 0.0, weight=c.weight, a_norm=False, b_norm=False, update=False)
    assert L == o.loss
    if c.variant == "self":
        assert o.ta is o.tb and o.ga is o.gb and np.array_equal(ga + gb, o.ga)
        assert c.n < 3 or (not np.array_equal(o.ia, o.ib) and o.ib[0] == o.ia[1] and o.ia[2] == o.ib[2])
    else:
        assert np.array_equal(ga, o.ga) and np.array_equal(gb, o.gb)
    assert not o.ga[:, c.dim:].any() and not o.gb[:, c.dim:].any()
    assert np.array_equal(np.nonzero(o.hit_a)[0], np.unique(np.concatenate([o.ia, o.ib]) if c.variant == "self" else o.ia))
    n = c.n
    if c.variant == "same":
        assert np.array_equal(o.ia, o.ib) and len(np.unique(o.ia)) == n
    elif c.variant in ("diff", "self") and n >= 2:
        assert not np.array_equal(o.ia, o.ib)
    elif c.variant == "shared" and n >= 2:
        assert o.ib[0] == o.ia[-1]
    if c.tag == "heavy":
        hits = np.bincount(o.ia, minlength=c.rows)
        assert hits.max() >= (50 if c.rows == 7 else 4)             # many atomic adds onto one row
    if c.tag != "heavy":
        assert not o.hit_a[-2:].any() and not o.hit_b[-2:].any()    # some flags must keep their old value


@pytest.mark.parametrize("c", rc.cases_of("steps"), ids=ids)
def test_steps_case_is_exact(c):
    o = rc.steps_ops(c)
    o.bound.check()
    sizes = np.diff(o.off)
    assert len(sizes) == 4 and sizes[1] == 0 and (sizes[[0, 2, 3]] > 0).all()          # three steps and an empty one between
    assert rc.STEPS_LR == 2.0 ** -3 and [(a, b) for a, b, _ in rc.STEPS_TERMS] == [(0, 1), (0, 2), (0, 3), (2, 3)]
    for t in o.tables:
        assert rc.is_quarters(t[:, :c.dim]) and not t[:, c.dim:].any()
    for s in (0, 2, 3):
        a = o.ia[o.off[s]:o.off[s + 1]]
        assert len(np.unique(a)) < len(a)                                                # duplicates in every step
    for order in ("lanes", "reverse"):
        T, losses, _ = rc.steps_replay(o.tables, o.ia, o.ib, o.off, np.float32, order)
        assert np.array_equal(losses, o.losses)
        for got, want in zip(T, o.final):
            assert _eq(got, want)
    # the float64 replay, composed from the oracle: alignment_step_dense(update=False) per term, one SGD step per table
    T = [t.astype(np.float64) for t in o.tables]
    for s in range(4):
        a, b = o.ia[o.off[s]:o.off[s + 1]], o.ib[o.off[s]:o.off[s + 1]]
        G = [np.zeros_like(t) for t in T]
        for k, (p, q, w) in enumerate(rc.STEPS_TERMS):
            L, ga, gb = mo.alignment_step_dense(T[p], T[q], None, None, a, b, rc.STEPS_LR, weight=w, a_norm=False, b_norm=False, update=False)
            assert L == o.losses[s, k]
            G[p] += ga
            G[q] += gb
        for k in range(4):
            if k != rc.STEPS_CONSTANT:
                T[k] -= rc.STEPS_LR * G[k]
    for got, want in zip(T, o.final):
        assert np.array_equal(got, want)
    assert np.array_equal(o.final[rc.STEPS_CONSTANT], o.tables[rc.STEPS_CONSTANT])
    assert not np.array_equal(o.final[0], o.tables[0]) and o.losses[1].sum() == 0.0 and (o.losses[[0, 2, 3]] > 0).all()


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("dim", rc.DENSE_DIMS)
def test_generic_tier_smallest_term_cannot_hide(dim, sign):
    """A lost row changes the loss by its term: every term is more than ten times the absolute loss tolerance."""
    g = rc.glog_generic(dim, sign)
    assert len(g.terms) <= 600 and g.w.min() >= 0.25 and g.w.max() <= 1.0
    assert g.terms.min() > 10 * RT * abs(g.loss), (g.terms.min(), RT * abs(g.loss))
    ref = mo.logistic_term_grads(g.h.astype(np.float64), g.r.astype(np.float64), g.t.astype(np.float64), float(sign), g.w.astype(np.float64))
    np.testing.assert_allclose(ref[0], g.loss, rtol=1e-12)
    np.testing.assert_allclose(ref[1], g.gh, rtol=1e-9, atol=1e-15)
    assert g.zero.sum() >= 2 and not ((g.h + g.r) - g.t)[g.zero].any()
    np.testing.assert_allclose(g.terms[g.zero], g.w[g.zero].astype(np.float64) * np.log(2.0), rtol=1e-12)


@pytest.mark.parametrize("sign", [1, -1])
def test_generic_tier_extreme_rows(sign):
    g = rc.glog_generic(75, sign, n=64, n_extreme=8)
    z = sign * g.x[g.extreme]
    assert g.extreme.sum() == 8 and np.abs(z).min() >= 79.9 and np.abs(z).max() <= 110.1
    assert np.isfinite(g.loss) and np.isfinite(g.gh).all()
    with np.errstate(over="ignore"):
        assert sign > 0 or np.isinf(np.exp(np.float32(g.x[g.extreme]))).any()       # float32 exp(+x) overflows
        assert sign < 0 or (np.exp(np.float32(-g.x[g.extreme])) < np.float32(1.2e-38)).any()   # exp(-x) goes denormal
    ok = ~g.extreme if sign < 0 else np.ones(len(g.terms), bool)     # sign -1: the extreme rows' terms are ~e^-80 by construction
    assert g.terms[ok].min() > 10 * RT * abs(g.loss)


# ----------------------------------------------------------------------------------------------------- refusals (no launch)
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def test_unsupported_widths_are_refused_before_any_launch(lib):
    from multike_amd import _lib
    p, null = C.c_void_p(16), C.c_void_p(0)
    i64, i32, f32 = C.c_int64, C.c_int, C.c_float
    bad = rc.REFUSED_STRIDE
    assert bad % 16 == 0 and bad // 16 not in rc.FPLS and bad < _lib.MAX_STRIDE and rc.REFUSED_DIM == _lib.MAX_STRIDE + 1
    rcode = lib.mke_align_fwd_bwd(p, i32(0), p, i32(0), i32(bad), i32(bad - 3), p, p, i64(5), f32(1.0), p, p, p, p, C.c_int32(1), p, null)
    assert rcode == -3 and b"unsupported stride 144" in lib.mke_last_error()
    assert lib.mke_gather_rows(p, i32(1), i32(bad), i32(bad), null, i64(5), p, null) == -3
    assert lib.mke_probe_rows(p, null, null, i32(bad), p, i64(5), p, null) == -3
    plan = _lib.AlignPlanStruct()
    off = (C.c_int64 * 2)(0, 5)
    plan.n_tables, plan.n_terms, plan.stride, plan.dim, plan.n_steps = 2, 1, bad, bad, 1
    for k in (0, 1):
        plan.tables[k].table, plan.tables[k].n_rows = 16, 8
    plan.terms[0].a, plan.terms[0].b, plan.terms[0].weight = 0, 1, 1.0
    plan.ia, plan.ib, plan.loss_partials, plan.step_off = 16, 16, 16, C.addressof(off)
    plan.optimizer, plan.lr, plan.tag_base = _lib.OPT_SGD, 0.125, 1
    assert lib.mke_align_steps(C.byref(plan), null) == -3 and b"unsupported stride 144" in lib.mke_last_error()
    d = rc.REFUSED_DIM
    assert lib.mke_gathered_alignment_fwd_bwd(p, p, i64(5), i32(d), i32(d), p, p, p, null) == -2
    assert lib.mke_gathered_logistic_fwd_bwd(p, p, p, null, i64(5), i32(d), i32(d), i32(1), p, p, p, p, null) == -2
    assert lib.mke_gathered_alignment_fwd_bwd(p, p, i64(5), i32(17), i32(16), p, p, p, null) == -2          # ld < dim
    assert lib.mke_gathered_alignment_fwd_bwd(p, p, i64(5), i32(17), i32(17), p, null, p, null) == -1        # one gradient of two
    assert lib.mke_align_fwd_bwd(p, i32(0), p, i32(0), i32(32), i32(33), p, p, i64(5), f32(1.0), p, p, p, p, C.c_int32(1), p, null) == -2
    assert lib.mke_align_fwd_bwd(p, i32(0), p, i32(0), i32(32), i32(17), p, p, i64(5), f32(1.0), p, null, p, p, C.c_int32(1), p, null) == -1
