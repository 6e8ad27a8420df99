"""score_cases.py without a device: the exactness conditions of tier 1, the float32 model inside the reference's bounds on every
run, every mutant of the model caught by a comparison of the case table, and the table reaching all 12 x 13 instantiations.
The same for the code-word forms (CW_RUNS): all 26 instantiations in every (ids, flags) combination, tier 1 exact, the model inside
the reference, seven mutants of the word routing caught; and, from the words alone, that the bitmap and the step's positives name
exactly the rows the flag form flags on the sampler's shape of a batch -- and a counterexample where they do not."""
import numpy as np
import pytest

import score_cases as sc
import update_cases as uc
from rows_cases import SAT_NEG, SAT_POS, STRIDES

f64 = np.float64
CASES = list({r.case.id: r.case for r in sc.RUNS}.values())


def test_table_reaches_every_instantiation():
    """Twelve per width: deterministic x exclusive, 32-bit offsets x lane ids, plain x exclusive, each for one and two groups per
    wavefront; and every structural item of the issue's list."""
    seen = {sc.instantiation(r.case, r.form) for r in sc.RUNS if r.case.npp}
    assert seen == sc.all_instantiations() and len(seen) == 12 * 13
    for stride in STRIDES:
        rs = [r for r in sc.RUNS if r.case.stride == stride]
        assert {r.case.dim for r in rs} >= set(sc.table_dims(stride))
        assert {r.case.npp for r in rs if r.case.tier == 1} >= set(sc.NPPS) | {0}
        assert {r.case.copies for r in rs} >= set(sc.REL_COPIES)
        assert {(r.case.n_hot, r.case.hot_copies) for r in rs if r.case.n_hot} >= {(n, k) for n in (1, 5) for k in sc.HOT_COPIES}
        sl = [(r.case.npp, sc.splits_of(r.case, r.form)) for r in rs if r.case.tag == "slices"]
        assert set(sl) >= {(10, 1), (10, 2), (10, 3), (10, 10), (10, 4), (9, 4), (5, 4)}, sl
        edge = (31, 32) if stride > 128 else (64, 65)
        assert [sc.qpg_of(r.case, r.form) for r in rs if r.case.tag == "half" and r.form.half == -1] == [2, 4]
        assert {(r.case.npp, r.form.half) for r in rs if r.case.tag == "half"} == {(n, h) for n in edge for h in (-1, 0, 64)}
        assert any(r.case.fwd_only for r in rs) and any(r.case.special for r in rs)
    assert {r.case.n_pos for r in sc.RUNS if r.case.tag == "pass"} == {8193, 16385, 32769}
    assert {r.case.rider for r in sc.RUNS if r.case.rider} == set(sc.COUNT_TOTALS)


@pytest.mark.parametrize("stride", STRIDES)
def test_tier1_is_exact(stride):
    """Bound.check(), every triple saturated, and the float64 sums representable in float32."""
    for c in (c for c in CASES if c.stride == stride and c.tier == 1):
        o = sc.ops(c)
        o.bound.check()
        E, R = o.ent.astype(f64), o.rel.astype(f64)
        xs = [((E[h] + R[r] - E[t]) ** 2).sum(1) for h, r, t in ((o.ph, o.pr, o.pt), (o.nh[:c.n_neg], o.nr[:c.n_neg], o.nt[:c.n_neg]))]
        assert min(x.min() for x in xs if len(x)) >= SAT_NEG >= SAT_POS, c.id
        assert not o.ent[:-1, c.dim:].any() and not o.rel[:-1, c.dim:].any()


@pytest.mark.parametrize("stride", STRIDES)
def test_model_within_reference(stride):
    worst = {}
    for r in (r for r in sc.RUNS if r.case.stride == stride):
        want = sc.reference(r.case, r.form)
        problems, ratios = sc.compare(sc.buffers_of(sc.reference(r.case, r.form, "f32")), want)
        for k, v in ratios.items():
            print(f"RATIO model:{k} {v:.4f} {r.id}")
            worst[k] = max(worst.get(k, 0.0), v)
        assert not problems, (r.id, problems)
        if r.case.tier == 2:                                         # a bound of inf would hold nothing
            for name in ("grad_ent", "grad_rel", "stage_rows", "ent", "acc"):
                if name in want:
                    assert np.isfinite(want[name][1]).all(), (r.id, name)
            assert np.isfinite(want["loss"][1])
            if sc.excl_of(r.case, r.form) and r.case.kinds == "unique":
                assert len(want["in_place_rows"]) == r.case.n_neg
    for k, v in worst.items():
        print(f"RATIO model:s{stride}:{k} {v:.4f}")


MUTANT_POOL = [r for r in sc.RUNS if r.case.stride in (16, 32, 80) and r.case.n_pos <= 64]


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_mutant_is_caught(mutant):
    """Each kind of subtly wrong kernel fails a comparison of the table (and the unmutated model passes it, above)."""
    hits = 0
    for r in MUTANT_POOL:
        problems, _ = sc.compare(sc.buffers_of(sc.reference(r.case, r.form, "f32", mutant)), sc.reference(r.case, r.form))
        hits += bool(problems)
        if hits >= 2:
            break
    assert hits >= 2 or (hits and mutant in ("drop_last_odd_group", "rider_scores")), mutant


@pytest.mark.parametrize("mutant", sc.SILENT_MUTANTS)
def test_silent_mutants_change_nothing(mutant):
    """Why two of the issue's mutants are not in MUTANTS: they add zeros (see score_cases.MUTANTS)."""
    for r in (r for r in sc.RUNS if r.case.stride == 80 and r.case.tag == "slices"):
        a, b = (sc.buffers_of(sc.reference(r.case, r.form, "f32", m)) for m in ("", mutant))
        assert all(np.array_equal(sc.canon(a[k]) if a[k].dtype == np.float32 else a[k], sc.canon(b[k]) if b[k].dtype == np.float32 else b[k]) for k in a)


# ----------------------------------------------------------------------------------------------------- the code-word forms
CW_CASES = list({r.case.id: r.case for r in sc.CW_RUNS}.values())


def test_cw_table_reaches_every_instantiation():
    """13 widths x two groupings = 26, each in every (ids, flags) combination; and the places of the positive drawn as its own
    negative: first and second id block, a slice that is not slice 0, the only negative of a group."""
    seen = {sc.instantiation(r.case, r.form) for r in sc.CW_RUNS}
    assert seen == sc.cw_instantiations() and len(seen) == 26
    assert not seen & sc.all_instantiations() and len(sc.forms_cw()) == 8 and len(sc.forms12()) == 12
    for stride in STRIDES:
        rs = [r for r in sc.CW_RUNS if r.case.stride == stride]
        for tier in (1, 2):
            combos = {(sc.qpg_of(r.case, r.form), r.form.ids, r.form.flags) for r in rs if r.case.tier == tier and r.case.kinds == "own"}
            assert combos == {(q, i, f) for q in (2, 4) for i in (0, 1) for f in (0, 1)}, (stride, tier)
        assert {r.case.npp for r in rs if r.case.tier == 1} == set(sc.NPPS)
        assert {(sc.qpg_of(r.case, r.form), r.form.flags) for r in rs if r.case.kinds == "mixed"} == {(q, f) for q in (2, 4) for f in (0, 1)}
        assert {r.case.dim for r in rs} >= set(sc.table_dims(stride)) and any(r.case.n_hot for r in rs)
        assert {(r.case.ent_norm, r.case.opt) for r in rs if r.case.tier == 2} >= {(1, "adagrad"), (0, "sgd"), (1, "sgd")}
        sl = [r for r in rs if r.case.tag == "slices"]
        assert sl and all(sc.splits_of(r.case, r.form) == 3 and sc.qpg_of(r.case, r.form) == 4 for r in sl)
        assert {(r.form.ids, r.form.flags) for r in sl} == {(i, f) for i in (0, 1) for f in (0, 1)}
        assert sum(r.case.tag == "free" for r in rs) == 2
    excl_slow, scattered = {}, {}
    for c in CW_CASES:
        if c.kinds != "own":
            continue
        o = sc.ops(c)
        g, n = np.arange(c.n_neg) // c.npp, np.arange(c.n_neg) % c.npp
        own = (o.nh[:c.n_neg] == o.ph[g]) & (o.nt[:c.n_neg] == o.pt[g])
        assert np.array_equal(own, sc.own_positions(c.npp, c.n_neg)), c.id          # no draw equals the id it replaces
        assert (o.nr[:c.n_neg] == o.pr[g]).all() and ((o.nh[:c.n_neg] != o.ph[g]) & (o.nt[:c.n_neg] != o.pt[g])).sum() == 0
        w, sw = sc.codes_of(c), sc.sampler_words(c)
        assert np.array_equal(sw[own], o.pt[g][own]) and ((sw[~own] & sc.CODE_FAST) != 0).all() and not (sw & sc.CODE_EXCL).any()
        assert np.array_equal(w & ~np.int32(sc.CODE_EXCL), sw)
        assert own.any() and (c.npp == 1 or (own & (n == 0)).any()) and (own & (n == c.npp - 1)).any(), c.id
        if c.npp in (100, 130):
            assert (own & (n == 70)).any()                                           # the second id block of 32 and of 64 lanes
        if c.npp == 65:
            assert (own & (n == 64)).any()
        if c.npp == 1:
            assert own[0] and not own.all()                                          # the only negative of a group
        if c.tag == "slices":
            per = -(-c.npp // 3)
            assert (own & (n // per == 2)).any()
        if c.tier == 2 and c.tag != "free":
            x = (w & sc.CODE_EXCL) != 0
            fast = (w & sc.CODE_FAST) != 0
            scattered[c.stride] = scattered.get(c.stride, 0) + int((~x & fast).sum())        # fast rows that collide: scattered
            assert c.npp == 1 or (x & fast).any(), c.id                                  # rows finished in place
            excl_slow[c.stride] = excl_slow.get(c.stride, 0) + int((x & ~fast).sum())
        if c.tag == "mask":
            assert ((w[~own] & sc.CODE_ENT_MASK) >= 65536).all() and sc.sizes(c)[0] == 70000 and c.stride == 16
    assert {c.npp for c in CW_CASES if c.kinds == "own"} >= {1, 65, 100, 130}
    assert set(scattered) == set(STRIDES) and min(scattered.values()) >= 100
    assert set(excl_slow) == set(STRIDES) and all(excl_slow.values())                # EXCL on a word without FAST, at every width


@pytest.mark.parametrize("stride", STRIDES)
def test_cw_tier1_is_exact(stride):
    for c in (c for c in CW_CASES if c.stride == stride and c.tier == 1):
        o = sc.ops(c)
        o.bound.check()
        E, R = o.ent.astype(f64), o.rel.astype(f64)
        xs = [((E[h] + R[r] - E[t]) ** 2).sum(1) for h, r, t in ((o.ph, o.pr, o.pt), (o.nh[:c.n_neg], o.nr[:c.n_neg], o.nt[:c.n_neg]))]
        assert min(x.min() for x in xs if len(x)) >= SAT_NEG >= SAT_POS, c.id
        assert not o.ent[:-1, c.dim:].any() and not o.rel[:-1, c.dim:].any()


@pytest.mark.parametrize("stride", STRIDES)
def test_cw_model_within_reference(stride):
    """The float32 model inside the reference on every code-word run; the reference is the one of the x1-o1-l1 form with the
    same routing, without ref_count and (flags = 0) without the entity flags; ids = 0 gives what ids = 1 gives."""
    for r in (r for r in sc.CW_RUNS if r.case.stride == stride):
        want = sc.reference(r.case, r.form)
        problems, ratios = sc.compare(sc.buffers_of(sc.reference(r.case, r.form, "f32")), want)
        for k, v in ratios.items():
            print(f"RATIO model:cw:{k} {v:.4f} {r.id}")
        assert not problems, (r.id, problems)
        assert "ref_count" not in want and ("touched_ent" in want) == bool(r.form.flags) and "touched_rel" in want
        base = sc.reference(r.case, r.form._replace(cw=0, ids=1, flags=1))
        assert set(base) - set(want) == {"ref_count"} | (set() if r.form.flags else {"touched_ent"})
        assert want.pop("cw") is True
        for k in want:
            a, b = want[k], base[k]
            if isinstance(a, tuple):
                assert np.array_equal(a[0], b[0], equal_nan=True) and (a[1] is None) == (b[1] is None), (r.id, k)
                assert a[1] is None or np.array_equal(a[1], b[1], equal_nan=True), (r.id, k)
            else:
                assert np.array_equal(a, b), (r.id, k)
        w = sc.codes_of(r.case)
        xf = (w & (sc.CODE_EXCL | sc.CODE_FAST)) == (sc.CODE_EXCL | sc.CODE_FAST)
        assert sorted(want["in_place_rows"]) == sorted(w[xf] & sc.CODE_ENT_MASK), r.id      # in-place rows: exactly the EXCL words (with FAST)
        if r.case.tier == 2:
            for name in ("grad_ent", "grad_rel", "ent", "acc"):
                assert np.isfinite(want[name][1][:-1]).all(), (r.id, name)
            assert np.isfinite(want["loss"][1])


CW_POOL = [r for r in sc.CW_RUNS if r.case.stride in (16, 80)]


@pytest.mark.parametrize("mutant", sc.CW_MUTANTS)
def test_cw_mutant_is_caught(mutant):
    """Each fails a comparison of the table in tier 2 on at least two runs (the unmutated model passes the same comparison), and
    the mutants of the forms without ids or flags fail on such runs."""
    hits = []
    for r in CW_POOL:
        want, model = sc.reference(r.case, r.form), sc.buffers_of(sc.reference(r.case, r.form, "f32"))
        if mutant == "cw_flags_listed":                              # the reverse direction: a reference that lists the flags
            problems, _ = sc.compare(model, sc.reference(r.case, r.form, "bound", mutant))
        else:
            problems, _ = sc.compare(sc.buffers_of(sc.reference(r.case, r.form, "f32", mutant)), want)
        if problems:
            assert not sc.compare(model, want)[0]
            hits.append(r)
    assert len(hits) >= 2, mutant
    if mutant in ("cw_slow_skipped", "cw_slow_entity_head"):
        assert all(not r.form.ids for r in hits) and {sc.qpg_of(r.case, r.form) for r in hits} == {2, 4}
    if mutant == "cw_flags_listed":
        assert all(not r.form.flags for r in hits) and len(hits) == sum(not r.form.flags for r in CW_POOL)
    if mutant == "cw_mask16":
        assert {r.case.tag for r in hits} == {"mask"} and len(hits) == 8
    if mutant in ("cw_excl_ignored", "cw_excl_without_fast", "cw_head_inverted"):
        assert {(r.form.ids, r.form.flags) for r in hits if r.case.tier == 2} == {(i, f) for i in (0, 1) for f in (0, 1)}


def visited_by_bitmap(c):
    """Pair 11, and pair 01 named by a positive: the rows the update launch of a code-word step visits."""
    o = sc.ops(c)
    n_ent, _ = sc.sizes(c)
    _, row = sc.step_codes(c)
    r = np.arange(n_ent)
    pair = (row[r >> 4] >> ((r & 15) * 2).astype(np.uint32)) & 3
    named = np.zeros(n_ent, bool)
    named[o.ph], named[o.pt] = True, True
    assert not (pair == 2).any()
    return (pair == 3) | ((pair == 1) & named), pair


@pytest.mark.parametrize("stride", STRIDES)
def test_bitmap_and_positives_are_the_flagged_rows(stride):
    """For the sampler's shape of a batch (and every batch whose words without FAST stand for their positive) bitmap + positives
    name exactly the rows the flag form flags.  For batches with two-sided or other-relation negatives they do NOT: such a
    negative's entity, referenced once and by no positive, takes an add in the scratch (the flag form flags it), has pair 01
    and is named by no list entry -- the update launch of the bitmap form never visits it.  Hence the precondition the header
    states at mke_update_table.bits."""
    cases = {c.id: c for c in [r.case for r in sc.RUNS] + CW_CASES if c.stride == stride and c.npp > 0 and not c.fwd_only and c.n_pos <= 64}
    lost_somewhere = 0
    for c in cases.values():
        o = sc.ops(c)
        n_ent, _ = sc.sizes(c)
        flagged = sc.reference(c, sc.Form(0, 1, 1, 1, 0, 1), "f32")["touched_ent"][:n_ent] == sc.TAG
        visited, pair = visited_by_bitmap(c)
        assert not (visited & ~flagged).any(), c.id                   # never a row without a gradient
        lost = np.nonzero(flagged & ~visited)[0]
        if c.kinds in ("own", "fast", "unique", "dup"):
            assert not len(lost), (c.id, lost)
            continue
        N = c.n_neg
        g = np.arange(N) // c.npp
        nh, nr, nt = o.nh[:N], o.nr[:N], o.nt[:N]
        slow = ~((nr == o.pr[g]) & ((nh != o.ph[g]) != (nt != o.pt[g])))
        foreign = set(nh[slow & (nh != o.ph[g])]) | set(nt[slow & (nt != o.pt[g])])
        assert set(lost) <= foreign and (pair[lost] == 1).all(), c.id
        lost_somewhere += bool(len(lost))
    assert lost_somewhere, "the counterexample: a once-referenced entity of a negative without FAST that is not its positive"


def test_empty_slices_are_in_the_table():
    r = [r for r in sc.RUNS if r.case.tag == "slices" and r.case.npp in (9, 5) and r.form.splits == 4][0]
    per = -(-r.case.npp // 4)
    assert sc.splits_of(r.case, r.form) == 4 and 3 * per >= r.case.npp


@pytest.mark.parametrize("rcase", sc.REDUCE_CASES, ids=lambda r: f"n{r.n_slots}-seg{r.seg}-s{r.stride}")
def test_reduce_cases_are_exact(rcase):
    rows, keys, order, ge, gr, te, tr, R, bd = sc.reduce_ops(rcase)
    bd.check()                                                       # multiples of 1/4, at most 300 of them: exact in double and float
    n = rcase.n_slots
    assert (np.diff(keys[:n]) >= 0).all() and sorted(order[:n]) == list(range(n))
    assert (keys[:n] == sc.KEY_FILL).sum() == n // 3


def test_count_cases():
    for total in sc.COUNT_TOTALS:
        cc = sc.count_case(total)
        assert not np.array_equal(uc.count_reference(cc), uc.count_reference(cc, "count_repeats")) or cc.neg_per_pos == 0
