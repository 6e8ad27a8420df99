"""score_cases.py without a device: the exactness conditions of tier 1, the float32 model inside the reference's bounds on every
run, every mutant of the model caught by a comparison of the case table, and the table reaching all 12 x 13 instantiations."""
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
