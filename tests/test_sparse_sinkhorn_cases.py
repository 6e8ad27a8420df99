"""The sparse Sinkhorn oracle (sparse_sinkhorn_oracle.py) on the CPU: its support on a hand-made instance, its recurrence against
the dense oracle at full support, its two evaluations against each other, and every subtly wrong variant told from it."""
import numpy as np
import pytest

import sinkhorn_oracle as O
import sparse_sinkhorn_oracle as SO

N1, N2, D, NOISE, TAU, ITERS, CUT = 200, 260, 24, 1.1, 0.05, 5, 8


def _triples(lists_, variant=None):
    return SO.pairs(*lists_, variant=variant)


def _arrays(ent):
    return (np.array([e[k] for e in ent]) for k in range(3))


def test_the_support_of_the_hand_case():
    s = SO.support(*SO.hand_case())
    assert s["count"] == 9
    assert s["row_off"].tolist() == [0, 2, 4, 4, 6, 9]
    assert s["ent_col"].tolist() == [2, 5, 0, 1, 4, 6, 0, 2, 6]
    assert s["ent_val"].tolist() == np.array([0.9, 0.4, 0.35, 0.8, 0.1, 0.5, 0.65, 0.55, 0.45], dtype=np.float32).tolist()
    assert s["col_off"].tolist() == [0, 2, 3, 5, 5, 6, 7, 9]
    assert s["ent_row"].tolist() == [1, 4, 1, 0, 4, 3, 0, 3, 4]
    assert s["ent_idx"].tolist() == [2, 6, 3, 0, 7, 4, 1, 5, 8]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_full_support_is_the_dense_recurrence(seed):
    _, _, S = SO.case(N1, N2, D, NOISE, seed)
    lists_ = SO.lists(S, N2) + SO.lists(S.T, N1)
    rows, cols, vals = _arrays(_triples(lists_))
    assert len(rows) == N1 * N2
    a, b = SO.potentials(N1, N2, rows, cols, vals, ITERS, TAU)
    da, db = O.potentials(S, ITERS, TAU)
    assert np.abs(a - da).max() <= 1e-12 and np.abs(b - db).max() <= 1e-12


def test_the_two_evaluations_agree():
    """The masked-matrix definition and the entry-list evaluation (whole and in segments, as the device sums a long list)."""
    for lists_, n_a, n_b in ((SO.hand_case(), 5, 7),) + tuple(
            (SO.lists(S, CUT) + SO.lists(S.T, CUT), N1, N2) for S in (SO.case(N1, N2, D, NOISE, 0)[2],)):
        ent = _triples(lists_)
        rows, cols, vals = _arrays(ent)
        a, b = SO.potentials(n_a, n_b, rows, cols, vals, ITERS, TAU)
        for seg in (None, 2, 5):
            a2, b2 = SO.potentials_lists(n_a, n_b, ent, ITERS, TAU, seg=seg)
            assert np.abs(a - a2).max() <= 1e-12 and np.abs(b - b2).max() <= 1e-12
    assert a[2] == 0.0 or n_a != 5


def test_empty_lists_have_potential_zero():
    ent = _triples(SO.hand_case())
    a, b = SO.potentials(5, 7, *_arrays(ent), ITERS, TAU)
    assert a[2] == 0.0 and b[3] == 0.0 and np.isfinite(a).all() and np.isfinite(b).all()


@pytest.mark.parametrize("variant", SO.VARIANTS)
def test_a_wrong_variant_is_told_apart(variant):
    lists_ = SO.hand_case()
    a, b = SO.potentials(5, 7, *_arrays(_triples(lists_)), ITERS, TAU)
    ent = _triples(lists_, variant if variant in ("duplicate_twice", "column_value", "padding_as_column") else None)
    wa, wb = SO.potentials_lists(5, 7, ent, ITERS, TAU, variant=variant, seg=2)
    with np.errstate(invalid="ignore"):
        err = max(np.nan_to_num(np.abs(wa - a), nan=np.inf).max(), np.nan_to_num(np.abs(wb - b), nan=np.inf).max())
    assert err > 1e-4, (variant, err)


def test_the_planted_case_leaves_no_row_out():
    """The end-to-end GPU test compares ranks on rows whose gap is at least 8 times the potentials' bound: on the oracle's own
    support that is every row of this case (seeds 0, 1, 2), and the support is a small part of the matrix."""
    for seed in (0, 1, 2):
        _, _, S = SO.case(N1, N2, D, NOISE, seed)
        s = SO.support(*(SO.lists(S, CUT) + SO.lists(S.T, CUT)))
        rows = np.repeat(np.arange(N1), np.diff(s["row_off"]))
        a, b = SO.potentials(N1, N2, rows, s["ent_col"], s["ent_val"], ITERS, TAU)
        assert s["count"] < 0.06 * N1 * N2
        M = float(np.abs(S).max() + max(np.abs(a).max(), np.abs(b).max()))
        bound = ITERS * (O.bound(TAU, int(np.diff(s["row_off"]).max()), M) + O.bound(TAU, int(np.diff(s["col_off"]).max()), M))
        gap = O.rank_oracle(2.0 * O.scores(S, a, b))[3]
        assert int((gap < 8 * bound).sum()) == 0
