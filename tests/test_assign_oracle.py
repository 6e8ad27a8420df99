"""The auction's definition (tests/assign_oracle.py) against scipy's exact assignment, without a GPU: on forty adversarial small
instances — unit-norm Gaussians, four tight clusters, similarities quantised to quarters (exact ties), values scaled by 6 — the
oracle's total is within n_a * (eps + 2^-16) of the optimum of the truncated instance, the matching is one-to-one, nobody is
still bidding and the duality certificate is empty."""
import numpy as np
import pytest

import assign_oracle as AO

scipy_optimize = pytest.importorskip("scipy.optimize")

EPS = (2.0 ** -14, 1e-3, 0.05)
UNLISTED = -1e9


def _instance(s):
    """Instance s of the recipe: n1 < 120, n2 < 140, cut 1..12; kind, eps and floor rule cycle through all 24 combinations.
    At eps = 2^-14 the sizes stay below 30: the rounds grow like (value range) / eps, and the oracle is a Python loop."""
    rng = np.random.default_rng(1000 + s)
    kind, eps, median_floor = s % 4, EPS[(s // 4) % 3], (s // 12) % 2 == 1
    top1, top2 = (30, 30) if eps < 1e-4 else (120, 140)
    n1, n2, cut = int(rng.integers(1, top1)), int(rng.integers(1, top2)), int(rng.integers(1, 13))
    val, col = AO.top_lists(AO.recipe_sim(kind, n1, n2, rng), min(cut, n2))
    floor = float(np.median(val)) if median_floor else float(val.min() - 1)
    return val, col, n2, eps, floor


def dense_optimum(val, col, n2, floor):
    """The optimum of the truncated instance by scipy: the lists as a dense float64 matrix, one private "unmatched" column of
    value floor per row, unlisted pairs hugely negative."""
    n1 = col.shape[0]
    ok = AO.listed(val, col, n2)
    m = np.full((n1, n2 + n1), UNLISTED)
    for i in range(n1):
        np.maximum.at(m[i], col[i][ok[i]], val[i][ok[i]].astype(np.float64))
    m[np.arange(n1), n2 + np.arange(n1)] = float(np.float32(floor))
    r, c = scipy_optimize.linear_sum_assignment(m, maximize=True)
    return m[r, c].sum()


@pytest.mark.parametrize("s", range(40))
def test_oracle_is_within_the_bound_of_the_optimum(s):
    val, col, n2, eps, floor = _instance(s)
    n1 = col.shape[0]
    assert (float(val.max()) - floor) + eps <= 16                       # the range the f32 bound rests on
    state, price, progress = AO.auction(val, col, n2, eps, floor)
    assert progress[1] == 0 and (state != 0).all()                      # nobody is still bidding
    held = state[state > 0] - 1
    assert np.unique(held).size == held.size                            # one-to-one
    assert progress[3] == (state == -1).sum() and held.size + progress[3] == n1
    gap = dense_optimum(val, col, n2, floor) - AO.total(val, col, n2, floor, state)
    print(f"instance {s}: n1 {n1} n2 {n2} cut {col.shape[1]} eps {eps} rounds {progress[0]} gap {gap:.3g} bound {n1 * (eps + AO.SLACK):.3g}")
    assert gap <= n1 * (eps + AO.SLACK)
    assert AO.certificate(val, col, n2, eps, floor, state, price) == []


def test_certificate_reports_what_it_must():
    val = np.array([[1.0, 0.5], [0.9, 0.2]], dtype=np.float32)
    col = np.array([[0, 1], [0, 1]], dtype=np.int32)
    state, price, _ = AO.auction(val, col, 2, 0.01, -1.0)
    assert AO.certificate(val, col, 2, 0.01, -1.0, state, price) == []
    assert any("still bidding" in m for m in AO.certificate(val, col, 2, 0.01, -1.0, [1, 0], price))
    assert any("held 2 times" in m for m in AO.certificate(val, col, 2, 0.01, -1.0, [1, 1], price))
    assert any("on offer" in m for m in AO.certificate(val, col, 2, 0.01, -1.0, state[::-1], np.zeros(2)))      # the worse pairing
    assert any("free column" in m for m in AO.certificate(val, col, 2, 0.01, -1.0, [1, -1], [0.0, 0.3]))
    assert any("does not list" in m for m in AO.certificate(val[:, :1], col[:, :1], 2, 0.01, -1.0, [1, 2], np.zeros(2)))


def test_list_rules_of_the_oracle():
    inf = np.inf
    val = np.array([[inf, 0.9, 0.8, 0.7], [0.9, 0.5, -inf, 0.1], [0.95, 0.9, 0.1, 0.0]], dtype=np.float32)
    col = np.array([[0, 1, -1, 2], [1, 0, 2, 7], [1, 5, 2, 0]], dtype=np.int32)       # -1 / 7 / 5 end a list (n2 = 3)
    state, price, progress = AO.auction(val, col, 3, 0.01, -1.0)
    # row 0 skips its +inf entry and never sees column 2; row 2 sees column 1 only; rows 0, 1, 2 all want column 1
    assert AO.listed(val, col, 3).tolist() == [[False, True, False, False], [True, True, False, False], [True, False, False, False]]
    assert state.tolist() == [-1, 1, 2] and progress[1] == 0 and progress[3] == 1
    assert AO.certificate(val, col, 3, 0.01, -1.0, state, price) == []
