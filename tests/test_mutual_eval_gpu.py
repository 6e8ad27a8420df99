"""The mutual nearest-neighbour decoder end to end on the GPU (base.alignment.mutual_alignment / mutual_pairs and the drivers'
hyper-parameter `mutual`) against the float64 oracle of mutual_oracle.py.

The data are built so that no decision is close: the test ASSERTS that, in float64, every row's and every column's best
exceeds its second best by more than 2e-5 — about four times the f32 rounding of these unit-row similarities and of their
re-scoring terms (75 x 2^-24 = 4.5e-6 each) — and then requires EQUALITY of the pairing and of precision / recall / F1, not a
tolerance."""
import contextlib
import io
import re

import numpy as np
import pytest

import mutual_oracle as MO
import sinkhorn_oracle as SO

pytestmark = pytest.mark.gpu

N1, N2, DIM = 300, 340, 75
GAP = 2e-5
CSLS_K = 10
SINKHORN = (4, 0.1)
VARIANTS = {"inner": ("inner", 0), "euclidean": ("euclidean", 0), "inner_csls": ("inner", CSLS_K), "euclidean_csls": ("euclidean", CSLS_K)}
_cache = {}


def _data():
    if "e" not in _cache:
        rng = np.random.default_rng(20261019)
        e1 = rng.standard_normal((N1, DIM))
        e2 = rng.standard_normal((N2, DIM))
        near = e1 + 0.05 * rng.standard_normal((N1, DIM))
        keep = np.arange(N1) % 3 != 2
        e2[:N1][keep] = near[keep]
        unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
        _cache["e"] = (unit(e1).astype(np.float32), unit(e2).astype(np.float32))
    return _cache["e"]


def _topk_mean(M, k):
    return -np.sort(-M, axis=1)[:, :k].mean(1)


def _matrix64(variant, swap=False):
    """The (re-scored) similarity matrix of a variant in float64, rows = the first operand."""
    key = ("M", variant, swap)
    if key not in _cache:
        e1, e2 = (x.astype(np.float64) for x in _data())
        if swap:
            e1, e2 = e2, e1
        e1, e2 = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (e1, e2))      # normalize=True
        metric, k = VARIANTS.get(variant, ("inner", 0))
        S = e1 @ e2.T
        if metric == "euclidean":
            sq1, sq2 = (e1 * e1).sum(1), (e2 * e2).sum(1)
            S = 1.0 - np.sqrt(np.maximum(sq1[:, None] + sq2[None, :] - 2.0 * S, 0.0))
        if k:
            S = (2.0 * S - _topk_mean(S, k)[:, None]) - _topk_mean(S.T, k)[None, :]
        if variant == "sinkhorn":
            a, b = SO.potentials(S, *SINKHORN)
            S = 2.0 * SO.scores(S, a, b)            # the device compares 2 (s - a - b); the doubling changes no order
        _cache[key] = S
    return _cache[key]


def _gap(S):
    """The smallest distance between a best and a second best, over all rows and all columns."""
    r = -np.sort(-S, axis=1)
    c = -np.sort(-S, axis=0)
    return min((r[:, 0] - r[:, 1]).min(), (c[0] - c[1]).min())


def _assert_decisive(S, what):
    gap = _gap(S)
    print(f"{what}: smallest best-to-second gap {gap:.3e}")
    assert gap > GAP, (what, gap)                   # the precondition of the equalities below


def _run(variant, **kw):
    from multike_amd.base.alignment import mutual_alignment
    e1, e2 = _data()
    metric, k = VARIANTS.get(variant, ("inner", 0))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = mutual_alignment(e1, e2, metric, True, k, 8, sinkhorn=SINKHORN if variant == "sinkhorn" else None, **kw)
    return res, out.getvalue()


@pytest.mark.parametrize("variant", sorted(VARIANTS) + ["sinkhorn"])
def test_mutual_alignment_equals_the_float64_oracle(variant):
    S = _matrix64(variant)
    _assert_decisive(S if variant != "sinkhorn" else S / 2.0, variant)      # Sinkhorn: the gap in similarity units, s - a - b
    want, (matched, gold) = MO.pairs(S)
    assert 200 <= matched < N1 and gold == 200                              # two of three rows have a counterpart; the rest mostly has none
    (match, precision, recall, f1), text = _run(variant)
    assert match.dtype == np.int64 and match.shape == (N1,)
    assert np.array_equal(match, want)
    assert (precision, recall, f1) == MO.scores_prf(want)
    assert precision == gold / matched * 100 and recall == gold / N1 * 100
    m = re.fullmatch(r"mutual alignment precision = (\d+\.\d{3})%, recall = (\d+\.\d{3})%, f1 = (\d+\.\d{3})%, matched = (\d+), "
                     r"time = \d+\.\d{3} s \n", text)
    assert m, text
    assert m.groups() == ("{:.3f}".format(precision), "{:.3f}".format(recall), "{:.3f}".format(f1), str(matched))


@pytest.mark.parametrize("variant", ["inner", "inner_csls"])
def test_threshold_applies_to_the_value_the_decoder_compares(variant):
    S = _matrix64(variant)
    free, _ = MO.pairs(S)
    vals = np.sort(S[np.arange(N1), np.maximum(free, 0)][free >= 0])
    lo, hi = len(vals) // 4, 3 * len(vals) // 4
    at = lo + int(np.argmax(np.diff(vals[lo:hi])))                           # the widest step of the middle half
    thr = float(0.5 * (vals[at] + vals[at + 1]))                             # between two attained values
    assert vals[at + 1] - vals[at] > GAP                                     # more than 1e-5 from both: twice their f32 rounding
    want, (matched, gold) = MO.pairs(S, thr)
    assert 0 < matched < (free >= 0).sum()
    (match, precision, recall, f1), _ = _run(variant, threshold=thr)
    assert np.array_equal(match, want) and (precision, recall, f1) == MO.scores_prf(want)
    (match, precision, recall, f1), _ = _run(variant, threshold=float("inf"))
    assert (match == -1).all() and (precision, recall, f1) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_mutual_pairs_with_the_operands_swapped_is_the_transpose(variant):
    """340 x 300: more rows than columns, no gold labels.  Every decision has a gap, so the pairing is the same set of pairs
    whichever side is the rows."""
    import torch
    from multike_amd.base.alignment import mutual_pairs
    e1, e2 = _data()
    metric, k = VARIANTS[variant]
    St = _matrix64(variant, swap=True)
    _assert_decisive(St, variant + " swapped")
    want_t, _ = MO.pairs(St)
    match_t, score_t = mutual_pairs(e2, e1, metric, True, k)
    match, score = mutual_pairs(e1, e2, metric, True, k)
    assert match_t.is_cuda and match_t.dtype == torch.int32 and score_t.dtype == torch.float32 and score_t.shape == (N2,)
    match_t, match = match_t.cpu().numpy(), match.cpu().numpy()
    assert np.array_equal(match_t, want_t)
    pairs = {(i, j) for i, j in enumerate(match.tolist()) if j >= 0}
    assert pairs == {(i, j) for j, i in enumerate(match_t.tolist()) if i >= 0} and len(pairs) >= 200
    assert np.array_equal(match, MO.pairs(_matrix64(variant))[0])
    # score = the value of the row's best column, matched or not.  Plain inner product of unit rows: 75 products folded in f32
    # (75 x 2^-24) plus the two rows' own normalisation, below 2 x 75 x 2^-24
    if variant == "inner":
        assert np.abs(score.cpu().numpy() - _matrix64(variant).max(1)).max() < 2 * 75 * 2.0 ** -24
        assert np.abs(score_t.cpu().numpy() - St.max(1)).max() < 2 * 75 * 2.0 ** -24


def _strip_times(text):
    return re.sub(r"time = \d+\.\d+ s|costs time \d+\.\d+ s", "time", text)


def test_drivers_with_mutual(monkeypatch):
    from multike_amd import MultiKE_Late as late
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.base.alignment import mutual_alignment
    from multike_amd.synthetic import SyntheticData, synthetic_args
    dim = 24
    data = SyntheticData(n_ent=1600, n_rel=20, n_attr=16, n_values=300, dim=dim, seed=13, shared_structure=0.8)
    n1 = data.kgs.entities_num // 2
    rng = np.random.default_rng(2)
    base = rng.standard_normal((n1, dim)).astype(np.float32)
    nm = np.concatenate([base, base + 0.8 * rng.standard_normal((n1, dim)).astype(np.float32)])
    data.local_name_vectors = nm / np.linalg.norm(nm, axis=1, keepdims=True)
    args = synthetic_args(dim=dim, batch_size=801, attribute_batch_size=601, entity_batch_size=499, neg_triple_num=6,
                          learning_rate=0.03, ITC_learning_rate=0.05, max_epoch=1, shared_learning_max_epoch=1, start_valid=1,
                          eval_freq=1, start_predicate_soft_alignment=2, seed=3, output="/tmp/multike_out_mutual/", csls=10,
                          mutual=1)
    model = MultiKE_CV(data, args, data.predicate_align_model)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        model.run()
    lines = out.getvalue().splitlines()
    tests = [i for i, l in enumerate(lines) if l.endswith("test results:")]
    assert len(tests) >= 1 and sum(l.startswith("mutual alignment precision = ") for l in lines) == len(tests)

    calls = []

    def spy(e1, e2, *a, **kw):
        calls.append((e1, e2, a, kw))
        return mutual_alignment(e1, e2, *a, **kw)
    monkeypatch.setattr(late, "mutual_alignment", spy)

    def capture(fn):
        with contextlib.redirect_stdout(io.StringIO()) as o:
            fn(model)
        return o.getvalue()
    for fn in (late.test, late.test_WVA):
        del calls[:]
        with_mutual = capture(fn)
        extra = [l for l in with_mutual.splitlines() if l.startswith("mutual alignment precision = ")]
        assert len(extra) == 1 and with_mutual.splitlines()[-1] == extra[0] and len(calls) == 1
        e1, e2, a, kw = calls[0]
        assert a[:3] == ('inner', True, 10) and kw["threshold"] is None and kw["sinkhorn"] is None   # re-scored as the test is
        with contextlib.redirect_stdout(io.StringIO()) as o:
            match, precision, recall, f1 = mutual_alignment(e1, e2, 'inner', True, 10, 8)
        assert _strip_times(o.getvalue().strip()) == _strip_times(extra[0].strip())                  # the same numbers
        assert (match >= 0).sum() > 0 and "matched = {},".format((match >= 0).sum()) in extra[0]
        model.args.mutual_threshold = 1e9                                                            # nothing reaches it
        assert "precision = 0.000%, recall = 0.000%, f1 = 0.000%, matched = 0," in capture(fn) and calls[-1][3]["threshold"] == 1e9
        del model.args.mutual_threshold
        del model.args.mutual                                     # the key absent: the printed output of a test is unchanged
        absent = capture(fn)
        model.args.mutual = 0
        off = capture(fn)
        model.args.mutual = 1
        assert "mutual" not in absent and _strip_times(absent) == _strip_times(off)
        kept = [l for l in _strip_times(with_mutual).splitlines() if not l.startswith("mutual alignment")]
        assert kept == _strip_times(absent).splitlines()
