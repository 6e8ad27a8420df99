"""oc_cases.py without a device: the case table reaches every instantiation and every item of the issue's axes, the staging holds
what it promises, the reference agrees with the dense float64 oracle the trainer tests use (and its two routings, atomics and
entity-major, with each other), the quarter inputs of the bit-for-bit parts are exact, and every mutant of the routing layer and
of the formula moves a compared value by more than 4 bounds or flips a structural output on some case of the table."""
import numpy as np
import pytest

import oc_cases as oc
from oracle import multike_oracle as mo
from rows_cases import SENTINEL, STRIDES, table_dims
from update_cases import dyadic_sum_exact

f64 = np.float64
SMALL = [c for c in oc.CASES if c.tag != "trip"]


def test_table_reaches_every_instantiation_and_axis():
    """260 instantiations of the two score kernels (kernel x 13 widths x 5 forms x divisor); every width and table dim for bases /
    apply / gv_sum / pass2 (every case runs them) and, through a long row per width case, for the combine and the partial slots;
    the group sizes, ranks, positives, options and trips."""
    seen = {oc.instantiation(r) for r in oc.RUNS}
    assert seen == oc.all_instantiations() and len(seen) == 260
    for stride in STRIDES:
        rs = [r for r in oc.RUNS if r.case.stride == stride and r.case.tag == "width"]
        # k_oc_em_combine and the partial-slot branch of k_oc_em_pass2 at this width: a long row on the rank under test, with an
        # even and an odd count of partials among the cases
        partials = set()
        for c in {r.case for r in rs}:
            L = oc.em_lists(c, oc.stage(c), c.rank)
            partials |= {p1 - p0 for _, p0, p1 in oc.em_items(L[:, 0])[1]}
        assert any(n % 2 for n in partials) and any(n % 2 == 0 for n in partials), (stride, partials)
        assert {r.case.dim for r in rs} >= set(table_dims(stride))
        for dim in table_dims(stride):
            assert {(r.case.G, r.form, r.quarter) for r in rs if r.case.dim == dim} == {(G, f, q) for G in (3, 4) for f in oc.FORMS for q in (0, 1)}
    grp = [r for r in oc.RUNS if r.case.tag == "group"]
    assert {r.case.N for r in grp if r.case.stride == 80} == set(oc.GROUPS)
    assert {r.case.stride for r in grp} == {16, 80, 320}
    rk = [r.case for r in oc.RUNS if r.case.tag == "ranks"]
    assert {(c.G, c.rank) for c in rk} == {(G, r) for G in oc.RANKS for r in {0, G // 2, G - 1}}
    assert {c.n_pos for c in rk} == set(oc.N_POS) and any(c.chunks == 2 for c in rk)
    per = lambda c: -(-c.n_pos // c.G)
    assert any(c.n_pos > 1 and per(c) * (c.G - 1) >= c.n_pos for c in rk), "an empty last home slice"
    assert any(per(c) * (c.G - 1) < c.n_pos < per(c) * c.G for c in rk), "a short last home slice"
    assert {quarter for r in oc.RUNS if r.case.tag == "rule" for quarter in [oc.quarter_of(r.case, r.quarter)]} == {True, False}
    cs = oc.CASES
    assert {c.rel_copies for c in cs} >= set(oc.REL_COPIES) and {c.hot_copies for c in cs if c.hot} == set(oc.HOT_COPIES)
    assert {c.scale for c in cs} == {1.0, 0.5} and {c.opt for c in cs} == {"adagrad", "sgd"} and {c.pos_w for c in cs} == {True, False}
    assert any(not c.refcount for c in cs) and any(c.vec == "sat" for c in cs)
    assert {c.chunks for c in cs if c.long} == {1, 2, 4}
    trips = {(c.n_pos, c.N): r for r in oc.RUNS for c in [r.case] if c.tag == "trip"}
    assert set(trips) == {(8192 + 3, 1), (32768 + 5, 15)}
    assert not oc.quarter_of(trips[(8195, 1)].case, trips[(8195, 1)].quarter) and oc.quarter_of(trips[(32773, 15)].case, trips[(32773, 15)].quarter)
    assert 32773 * (15 + 2) > 2048 * 256 and 8195 > oc.LOSS_PARTIALS * 4 and 32773 > oc.LOSS_PARTIALS * 16


@pytest.mark.parametrize("c", [c for c in SMALL if c.n_pos >= 5 and not c.long], ids=lambda c: c.id)
def test_staging_holds_the_constructed_positives(c):
    S = oc.stage(c)
    G, r, N = c.G, c.rank, c.N
    assert S.pt[4] == S.ph[4] and S.ph[3] == S.ph[0] and S.pr[4] == S.pr[2]
    assert not S.ent[:, c.dim:].any() and not S.rel[:, c.dim:].any()
    norms = np.linalg.norm(S.ent.astype(f64), axis=1)
    assert norms.min() >= 0.49 and norms.max() <= 2.01
    for k, (lo, hi) in enumerate(S.parts):                            # slots: a numbering per owner, the owned lists in slot order
        for g in range(G):
            assert (S.sh[lo + S.own_h[k][g]] == np.arange(len(S.own_h[k][g]))).all() and (S.ph[lo + S.own_h[k][g]] % G == g).all()
            assert (S.st[lo + S.own_t[k][g]] == np.arange(len(S.own_t[k][g]))).all() and (S.pt[lo + S.own_t[k][g]] % G == g).all()
        assert S.per[k] * G >= hi - lo
    # the silent mutant's premise: no negative corrupts the head of a positive whose RT does not travel, and the other way round
    if N:
        assert not (S.cside.astype(bool) & (S.st < 0)[:, None]).any() and not ((S.cside == 0) & (S.sh < 0)[:, None]).any()
        assert (S.cent[0] % G == r).all() and (G == 1 or (S.cent[1] % G != r).all())
        assert S.sh[2] >= 0 and (N < 2 or S.st[2] >= 0)
        assert S.equal[3, N - 1] and S.cent[3, N - 1] == S.pt[3] and S.cside[3, N - 1] == 0
        every = np.concatenate([S.cent.ravel(), S.ph, S.pt])
        assert (every == S.X).sum() == 1 and (every == S.Y).sum() == 2
        rc = oc.ref_counts(c, S, int(S.part_of[0]), r)
        assert rc[S.X // G] == 1
    assert (oc.Ref(c)._codes_seen() & oc.CODE_MASK == (S.cent << 1 | S.cside)).all()      # the code buffer read as the kernels read it
    if c.hot:
        assert S.hot_slot[r][S.Hb // G] >= 0 and (S.cent == S.Hb).sum() == 1 and (S.ph == S.Hb).sum() == 2


def test_long_lists_have_the_lengths_of_the_issue():
    for c in (c for c in oc.CASES if c.long):
        L = oc.em_lists(c, oc.stage(c), c.rank)
        rows, n = np.unique(L[:, 0], return_counts=True)
        assert set(n[rows < c.n_local]) >= set(oc.LONG_LISTS)
        items, longs, n_part = oc.em_items(L[:, 0])
        segs = {p1 - p0 for _, p0, p1 in longs}
        assert any(s % 2 for s in segs) and any(s % 2 == 0 for s in segs)          # an odd and an even count of partials
        assert any(row >= c.n_local for row, _, _ in longs)                        # a long relation row: the combine stores it
        coef, vall, gvs = oc.pass2_inputs(c)                                       # quarters: every list's sum is exact in any order
        assert dyadic_sum_exact(np.concatenate([v.reshape(1, -1) for v in vall + gvs], 1)).all()
        assert np.abs(coef).max() <= 1 and (np.log2(np.abs(coef)) % 1 == 0).all() and max(n) * 32 < 2 ** 24


def _neg_triples(S):
    P, N = S.cent.shape
    p = np.repeat(np.arange(P), N)
    side = S.cside.ravel().astype(bool)
    e = S.cent.ravel()
    return np.where(side, e, S.ph[p]), S.pr[p], np.where(side, S.pt[p], e)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_reference_agrees_with_the_dense_oracle(c):
    """The chained reference (values carried in float64) against relation_view_step_dense on the same global batch: the loss,
    every rank's rows and accumulators, the relation table — for both routings.  Differences are float64 rounding."""
    S = oc.stage(c)
    ent, rel, ae, ar_ = (a.astype(f64) for a in (S.ent, S.rel, S.acc_e, S.acc_r))
    ent0 = ent.copy()
    loss, ghat_e, ghat_r = mo.relation_view_step_dense(ent, rel, ae, ar_, (S.ph, S.pr, S.pt), _neg_triples(S), c.lr,
                                                       pos_w=None if S.pw is None else S.pw.astype(f64), scale=c.scale, update=c.opt == "adagrad")
    if c.opt == "sgd":
        ent -= c.lr * mo.l2_normalize_rows_backward(ent0, ghat_e)
        rel -= c.lr * mo.l2_normalize_rows_backward(S.rel.astype(f64), ghat_r)
    R = oc.Ref(c, 0, "", staged=False)
    for form in ("em",) + (("atm",) if c.chunks == 1 else ()):
        o = R.step(form)
        assert abs(o["loss"][0] - loss) <= 1e-9 * max(1.0, abs(loss)), (form, o["loss"][0], loss)
        assert np.isfinite(o["loss"][1]) and o["loss"][1] < 1e-3 * max(1.0, abs(loss))
        for g in range(c.G):
            n = len(ent[g::c.G])
            for name, want in (("ent", ent), ("acc", ae)):
                val, err = o[name][g]
                np.testing.assert_allclose(val[:n], want[g::c.G], rtol=0, atol=1e-9, err_msg=f"{form} {name} rank {g}")
                # a bound that still holds something.  A row of m references sums m terms c d of some 30 roundings each (two row sums of
                # depth FPL + 6, rsq, exp, rcp, the products); the Jacobian divides by a norm >= 0.5 (x 2) and the accumulator's 2 g dg
                # doubles it once more: 128 (m + 8) ulps of the row's largest entry (of 1 below 1) — a wrong sign of ONE term is 2 |c d|
                scale = np.maximum(1.0, np.abs(np.nan_to_num(val)).max(1))[:c.n_local]
                m = np.bincount(oc.em_lists(c, S, g)[:, 0], minlength=c.n_local + c.n_rel)[:c.n_local]
                assert np.isfinite(err).all() and (err[:c.n_local].max(1) <= 128 * (m + 8) * 2.0 ** -23 * scale).all(), (form, name, g, err.max())
        np.testing.assert_allclose(o["rel"][0][:c.n_rel], rel, rtol=0, atol=1e-9)
        np.testing.assert_allclose(o["rel_acc"][0][:c.n_rel], ar_, rtol=0, atol=1e-9)


def outputs(R: oc.Ref, run: oc.Run) -> dict:
    """Everything the device tests compare for the rank under test, by name."""
    c, S = R.c, R.S
    g = c.rank
    atm = run.form == "atm"
    out = {}
    K = len(S.parts)
    for k in range(K):
        out[f"send{k}"] = R.send(k, g)
        s = R.score(k, g, run.form if atm else "em")
        for name, v in s.items():
            if name in ("grad_entries", "in_place_rows") or (name == "coef" and atm) or (name == "mirror" and run.form not in ("mir", "mirown")):
                continue                                             # (what the device test of this form does not compare)
            out[f"score{k}.{name}"] = v
        gv = R.gv(k, g)
        out[f"gv{k}"] = gv
        if atm:
            for name, v in R.apply(k, g, *R._relay(*gv), s).items():
                if name != "row_sums":
                    out[f"apply{k}.{name}"] = v
    if not atm:
        coef, vall, gvs = oc.pass2_inputs(c)
        z = np.zeros
        p2 = R.pass2(g, (coef.astype(f64), z(coef.shape)), [(v.astype(f64), z(v.shape)) for v in vall], [(v.astype(f64), z(v.shape)) for v in gvs])
        for name in ("ent", "acc", "rel_grad", "partials"):
            out[f"pass2.{name}"] = p2[name]
    o = R.step("atm" if atm else "em")
    for name in ("ent", "acc"):
        out[f"step.{name}"] = o[name][g]
    out["step.rel"], out["step.loss"] = o["rel"], o["loss"]
    return out


POOL = [r for r in oc.RUNS if r.case.tag != "trip" and (r.case.stride in (16, 32, 80))]


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_mutant_is_caught(mutant):
    """A condition on the case table: some case moves a compared value by more than 4 bounds, or flips a structural output."""
    order = sorted(POOL, key=lambda r: (r.case.tag not in {"last_segment_dropped": ("long",), "odd_partial_dropped": ("long",),
                                                            "hub_in_place": ("opt",), "chunk_ignored": ("ranks", "long")}.get(mutant, ("ranks", "group")),))
    # a proof that means what it says: the wave kernel's last round dropped where full rounds remain, writer 0 skipped where
    # there are others, the coefficient index where coefficients are compared
    fits = {"wave_last_round": lambda r: r.case.N >= 17 and not oc.quarter_of(r.case, r.quarter), "gv_skip_writer0": lambda r: r.case.G > 1,
            "coef_no_plus1": lambda r: r.form != "atm" and r.case.N > 0, "drop_17th": lambda r: r.case.N > 17}.get(mutant, lambda r: True)
    for r in [r for r in order if fits(r)][:400]:
        a, b = outputs(oc.Ref(r.case, r.quarter), r), outputs(oc.Ref(r.case, r.quarter, mutant), r)
        hit = [k for k in a if oc.moved(a[k], b[k])]
        if hit:
            print(f"MUTANT {mutant}: {r.id}: {hit[:4]}")
            return
    pytest.fail(f"no case of the table catches {mutant}")


def test_sentinel_is_no_value_of_the_reference():
    c = [c for c in SMALL if c.tag == "width"][0]
    s = oc.Ref(c).score(0, c.rank, "atm")
    assert (s["g_all"][0] == SENTINEL).any() and (s["coef"][0] == SENTINEL).any() and (np.abs(s["g_all"][0][s["g_all"][0] != SENTINEL]) < 100).all()


def test_saturating_vectors_do_what_they_are_for():
    """The staged vectors of the "sat" case, in float32 as the kernel sees them: among the negatives the rank under test scores,
    some have exp(-y) = 0 (coefficient +-0, loss term 0: y above 88 flushes), some y in [0, 16]; one of its positives has
    1 + exp(-x) = 1 in float32 (sigmoid 1: x above 17)."""
    f32 = np.float32
    for c in (c for c in oc.CASES if c.vec == "sat"):
        R = oc.Ref(c, 0)
        R._ensure()
        ni, oi = R._scored(0, c.rank)
        y, x = R.n_y.val[ni, 0].astype(f32), R.o_x.val[oi, 0].astype(f32)
        with np.errstate(under="ignore"):
            t = np.exp(-y.astype(np.float64))
        assert (t < 2.0 ** -126).sum() >= 3 and (y <= 16).sum() >= 3, (c.id, np.sort(y))
        assert ((f32(1) + np.exp(-x.astype(np.float64)).astype(f32)) == f32(1)).any() and (x < 16).any(), (c.id, np.sort(x))
