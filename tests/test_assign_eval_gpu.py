"""The auction decoder end to end on the GPU (base.alignment.assignment_alignment and the drivers' hyper-parameter `assign_cut`)
on the inputs of tests/golden/stable_golden.npz: all six cases, CSLS where the case has it, plus one Sinkhorn run.

assignment_alignment must equal the NumPy definition (tests/assign_oracle.py) on the lists THE DEVICE ITSELF produced — the
lists of candidate_lists, which the stable tests pin exactly — so a last-ulp difference between the device's and float64
similarities cannot flip the comparison: it is an equality, not a tolerance."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

import assign_oracle as AO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ["inner_sq", "inner_wide", "inner_csls", "euclid", "euclid_csls", "cosine_raw"]
SINKHORN = (4, 0.1)
EPS = 1e-3
LINE = (r"optimal assignment precision = (\d+\.\d{3})%, recall = (\d+\.\d{3})%, f1 = (\d+\.\d{3})%, matched = (\d+), rounds = (\d+), "
        r"time = \d+\.\d{3} s ")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "stable_golden.npz"))


def _device_lists(e1, e2, metric, normalize, k, cut, sinkhorn=None):
    """The lists assignment_alignment takes, by the same calls."""
    from multike_amd.base import alignment as AL
    operands = AL.prepare_operands(e1, e2, metric, normalize, "cuda")
    a, b, kpad, code, sq1, sq2 = operands
    val, col, _ = AL.candidate_lists(a, b, kpad, max(1, min(cut, b.shape[0])), code, sq1, sq2, AL._rescoring_terms(operands, k, sinkhorn))
    return val.cpu().numpy(), col.cpu().numpy()


def _check(e1, e2, metric, normalize, k, cut, sinkhorn=None, **kw):
    from multike_amd.base.alignment import assignment_alignment
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        match, precision, recall, f1 = assignment_alignment(e1, e2, metric, normalize, k, 8, cut=cut, eps=EPS, sinkhorn=sinkhorn, **kw)
    n1, n2 = len(e1), len(e2)
    val, col = _device_lists(e1, e2, metric, normalize, k, cut, sinkhorn)
    ok = AO.listed(val, col, n2)
    floor = kw.get("floor")
    if floor is None:
        floor = float(val[ok].min()) - 1.0              # the default: any listed pair beats staying unmatched
    assert (float(val[ok].max()) - floor) + EPS <= 16
    state, price, progress = AO.auction(val, col, n2, EPS, floor)
    assert progress[1] == 0
    assert match.dtype == np.int64 and match.shape == (n1,)
    assert np.array_equal(match, np.where(state > 0, state - 1, -1))
    assert AO.certificate(val, col, n2, EPS, floor, np.where(match >= 0, match + 1, -1), price) == []
    matched, gold = int((match >= 0).sum()), int((match == np.arange(n1)).sum())
    assert precision == (gold / matched * 100 if matched else 0.0) and recall == (gold / n1 * 100 if matched else 0.0)
    assert f1 == (2 * precision * recall / (precision + recall) if gold else 0.0)
    lines = out.getvalue().splitlines()
    assert len(lines) == 2 and re.fullmatch(r"generating candidate lists costs time \d+\.\d{3} s ", lines[0]), lines
    m = re.fullmatch(LINE, lines[1])
    assert m, lines[1]
    assert m.groups() == ("{:.3f}".format(precision), "{:.3f}".format(recall), "{:.3f}".format(f1), str(matched), str(progress[0]))
    return match, progress


@pytest.mark.parametrize("case", CASES)
def test_golden_inputs_equal_the_oracle_on_the_device_lists(golden, case):
    n1, n2, d, k, normalize, cut = (int(x) for x in golden[case + "/meta"])
    match, progress = _check(golden[case + "/e1"], golden[case + "/e2"], str(golden[case + "/metric"]), bool(normalize), k, cut)
    print(f"{case}: n1 {n1} n2 {n2} cut {cut} csls {k} progress {progress}, differs from the stable matching in "
          f"{int((match != golden[case + '/match']).sum())} rows")
    assert (match >= 0).all() and len(set(match.tolist())) == n1            # n2 >= n1 and the default floor: everybody is matched


def test_sinkhorn_and_an_explicit_floor(golden):
    case = "inner_sq"
    n1, n2, d, k, normalize, cut = (int(x) for x in golden[case + "/meta"])
    e1, e2 = golden[case + "/e1"], golden[case + "/e2"]
    _check(e1, e2, "inner", True, 0, cut, sinkhorn=SINKHORN)
    val, _ = _device_lists(e1, e2, "inner", True, 0, cut)
    floor = float(np.median(val[:, 0]))                                     # half the rows' best pair is worth less than staying unmatched
    match, progress = _check(e1, e2, "inner", True, 0, cut, floor=floor)
    assert progress[3] > 0 and (match == -1).sum() == progress[3]


def test_round_limit_and_value_range(golden, monkeypatch):
    from multike_amd import _lib
    from multike_amd.base import alignment as AL
    case = "inner_sq"
    e1, e2 = golden[case + "/e1"], golden[case + "/e2"]
    real = AL.assignment_matching
    monkeypatch.setattr(AL, "assignment_matching", lambda *a, **kw: real(*a, max_rounds=2, **kw))
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(_lib.MultiKEHipError, match="eps = 0.001"):
        AL.assignment_alignment(e1, e2, "inner", True, 0, 8, cut=100, eps=EPS)
    monkeypatch.undo()
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(_lib.MultiKEHipError, match="exceeds 16"):
        AL.assignment_alignment(e1, e2, "inner", True, 0, 8, cut=100, eps=EPS, floor=-20.0)


def _strip_times(text):
    return re.sub(r"time = \d+\.\d+ s|costs time \d+\.\d+ s", "time", text)


def test_drivers_with_assign_cut(monkeypatch):
    from multike_amd import MultiKE_Late as late
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.base.alignment import assignment_alignment
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
                          eval_freq=1, start_predicate_soft_alignment=2, seed=3, output="/tmp/multike_out_assign/", csls=10,
                          assign_cut=20)
    model = MultiKE_CV(data, args, data.predicate_align_model)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        model.run()
    lines = out.getvalue().splitlines()
    tests = [i for i, l in enumerate(lines) if l.endswith("test results:")]
    assert len(tests) >= 1 and sum(l.startswith("optimal assignment precision = ") for l in lines) == len(tests)

    calls = []

    def spy(e1, e2, *a, **kw):
        calls.append((e1, e2, a, kw))
        return assignment_alignment(e1, e2, *a, **kw)
    monkeypatch.setattr(late, "assignment_alignment", spy)

    def capture(fn):
        with contextlib.redirect_stdout(io.StringIO()) as o:
            fn(model)
        return o.getvalue()
    for fn in (late.test, late.test_WVA):
        del calls[:]
        with_assign = capture(fn)
        got = with_assign.splitlines()
        extra = [l for l in got if l.startswith("optimal assignment precision = ")]
        assert len(extra) == 1 and got[-1] == extra[0] and got[-2].startswith("generating candidate lists costs time") and len(calls) == 1
        e1, e2, a, kw = calls[0]
        assert a[:3] == ('inner', True, 10) and kw["cut"] == 20 and kw["eps"] == 1e-3 and kw["floor"] is None and kw["sinkhorn"] is None
        with contextlib.redirect_stdout(io.StringIO()) as o:
            match, precision, recall, f1 = assignment_alignment(e1, e2, 'inner', True, 10, 8, cut=20)
        assert _strip_times(o.getvalue().splitlines()[-1].strip()) == _strip_times(extra[0].strip())      # the same numbers
        assert (match >= 0).sum() > 0 and "matched = {},".format((match >= 0).sum()) in extra[0]
        model.args.assign_floor = 1e3                                 # nothing is worth that much: everybody stays unmatched
        model.args.assign_eps = 0.5
        assert "precision = 0.000%, recall = 0.000%, f1 = 0.000%, matched = 0, rounds = 1," in capture(fn)
        assert calls[-1][3]["floor"] == 1e3 and calls[-1][3]["eps"] == 0.5
        del model.args.assign_floor, model.args.assign_eps
        del model.args.assign_cut                                     # the key absent: the printed output of a test is unchanged
        absent = capture(fn)
        model.args.assign_cut = 0
        off = capture(fn)
        model.args.assign_cut = 20
        assert "optimal assignment" not in absent and _strip_times(absent) == _strip_times(off)
        kept = _strip_times(with_assign).splitlines()[:-2]
        assert kept == _strip_times(absent).splitlines()
