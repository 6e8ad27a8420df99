"""Stable (Gale-Shapley) alignment on the GPU (mke_stable_lists + mke_stable_rounds + mke_stable_finish): the matching kernels
alone on hand-made lists against the NumPy oracle (tests/stable_oracle.py), the candidate lists of both kernel paths against
`similarity.sim` on the same device tensors, the whole pipeline (oracle on the device's own lists, no blocking pair, run-to-run
identical), the reference's own matching (tests/golden/stable_golden.npz), and the drivers with the hyper-parameter
`stable_cut`."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import stable_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the matching kernels alone
def _device_match(val, col, n2, batch=32):
    from multike_amd.base.alignment import stable_matching
    v = torch.as_tensor(np.ascontiguousarray(val, dtype=np.float32)).cuda()
    c = torch.as_tensor(np.ascontiguousarray(col, dtype=np.int32)).cuda()
    match, matched, gold, rounds = stable_matching(v, c, n2, batch=batch)
    match = match.cpu().numpy().astype(np.int64)
    assert matched == int((match >= 0).sum()) and gold == int((match == np.arange(len(match))).sum())
    return match, rounds


def _hand_made(name):
    rng = np.random.default_rng(7)
    if name == "chain70":            # one shared order: a single suitor settles per round, 70 rounds over three batches of 32
        col = np.tile(np.arange(70, dtype=np.int32), (70, 1))
        val = np.tile(np.linspace(1.0, 0.0, 70, dtype=np.float32), (70, 1)) + np.arange(70, dtype=np.float32)[:, None]
        return val, col, 70
    if name == "all_equal":          # only the tie rules decide: lower column for a suitor, lower row for a reviewer
        col = np.tile(np.arange(40, dtype=np.int32), (33, 1))
        return np.full((33, 40), 0.5, dtype=np.float32), col, 40
    if name == "small_ints":         # many ties
        mat = rng.integers(0, 4, size=(90, 110)).astype(np.float32)
        val, col = O.lists_from_matrix(mat, 25)
        return val, col, 110
    if name == "too_short":          # 40 suitors compete for 5 columns with lists of 3: 35 stay unmatched
        col = np.stack([rng.permutation(5)[:3] for _ in range(40)]).astype(np.int32)
        return -np.sort(-rng.standard_normal((40, 3)).astype(np.float32), axis=1), col, 5
    if name == "more_suitors":       # n_a > n_b with full lists
        mat = rng.standard_normal((300, 64)).astype(np.float32)
        val, col = O.lists_from_matrix(mat, 64)
        return val, col, 64
    if name == "one":
        return np.array([[0.3, 0.1]], dtype=np.float32), np.array([[4, 2]], dtype=np.int32), 6
    if name == "none":
        return np.zeros((0, 5), dtype=np.float32), np.zeros((0, 5), dtype=np.int32), 9
    if name == "padded":             # lists padded with -1, one of them empty, NaN rows of a matrix
        mat = rng.standard_normal((50, 30)).astype(np.float32)
        mat[rng.random((50, 30)) < 0.85] = np.nan
        mat[3] = np.nan
        val, col = O.lists_from_matrix(mat, 12)
        assert (col == -1).any() and (col[3] == -1).all()
        return val, col, 30
    raise KeyError(name)


@pytest.mark.parametrize("name", ["chain70", "all_equal", "small_ints", "too_short", "more_suitors", "one", "none", "padded"])
def test_matching_kernels_equal_the_oracle_on_hand_made_lists(name):
    val, col, n2 = _hand_made(name)
    want = O.deferred_acceptance(val, col, n2)
    got, rounds = _device_match(val, col, n2)
    assert np.array_equal(got, want), name
    got1, rounds1 = _device_match(val, col, n2, batch=1)          # the batch size changes nothing
    assert np.array_equal(got1, want) and rounds1 == rounds, name
    if name == "chain70":
        assert rounds == 70 and got.tolist() == list(range(69, -1, -1))   # the reviewers prefer the higher rows' values
    if name == "all_equal":
        assert got.tolist() == list(range(33))
    if name == "too_short":
        assert int((got < 0).sum()) == 35
    if name == "more_suitors":
        assert int((got >= 0).sum()) == 64 and len(set(got[got >= 0].tolist())) == 64
    if name == "none":
        assert rounds == 0 and got.size == 0
    assert O.blocking_pairs(val, col, got, n2) == [], name


# ------------------------------------------------------------------------------------------------ 2. the candidate lists
N1, N2 = 300, 333                    # three row blocks, several column chunks, a ragged last tile
CUTS = (1, 32, 100, 128, 129, 333)   # both sides of the 128 threshold between the sweep path and the whole-row path
MODES = {"inner": ("inner", True, 0), "euclid": ("euclidean", False, 0), "inner_csls": ("inner", True, 10),
         "euclid_csls": ("euclidean", True, 10)}
_cache = {}


def _inputs(d):
    if ("in", d) not in _cache:
        rng = np.random.default_rng(100 + d)
        base = rng.standard_normal((N2, d)).astype(np.float32)
        e2 = base + 0.15 * rng.standard_normal((N2, d)).astype(np.float32)
        e1 = (base[:N1] + 0.9 * rng.standard_normal((N1, d))).astype(np.float32)
        for j in range(7, N2, 7):    # every 7th target row repeats its predecessor: exact ties in every row
            e2[j] = e2[j - 1]
        _cache["in", d] = (torch.as_tensor(e1).cuda(), torch.as_tensor(e2).cuda())
    return _cache["in", d]


def _matrix(d, mode):
    """The reference of a case, computed once: similarity.sim on the same device tensors."""
    if ("M", d, mode) not in _cache:
        from multike_amd.base import similarity as S
        metric, normalize, k = MODES[mode]
        e1, e2 = _inputs(d)
        _cache["M", d, mode] = S.sim(e1, e2, metric, normalize, k).cpu().numpy()
    return _cache["M", d, mode]


def _lists(d, mode, cut, sample_cols=0):
    key = ("L", d, mode, cut, sample_cols)
    if key not in _cache:
        from multike_amd.base.alignment import candidate_lists, csls_means, prepare_operands
        metric, normalize, k = MODES[mode]
        e1, e2 = _inputs(d)
        a, b, kpad, code, sq1, sq2 = prepare_operands(e1, e2, metric, normalize, "cuda")
        assert kpad == {12: 16, 75: 80, 200: 208}[d]
        csls = csls_means(a, b, kpad, code, sq1, sq2, k) if k else None
        val, col, redone = candidate_lists(a, b, kpad, cut, code, sq1, sq2, csls, sample_cols=sample_cols)
        _cache[key] = (val.cpu().numpy(), col.cpu().numpy(), redone)
    return _cache[key]


def _band(mode):
    return (1e-5, 1e-5) if "csls" in mode else (1e-5, 2e-6)       # (rtol, atol): the bands of tests/test_csls_abi.py


def _check_lists(M, val, col, cut, mode, what):
    rtol, atol = _band(mode)
    rows = np.arange(M.shape[0])[:, None]
    assert val.shape == col.shape == (M.shape[0], cut), what
    assert (col >= 0).all() and (col < M.shape[1]).all(), what    # no NaN here: full lists, no padding column of the last tile
    s = np.sort(col, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), what                    # unique
    ref = M[rows, col]
    np.testing.assert_allclose(val, ref, rtol=rtol, atol=atol, err_msg=str(what))
    assert (val[:, 1:] <= val[:, :-1]).all(), what                # non-increasing
    eq = val[:, 1:] == val[:, :-1]
    assert (col[:, 1:][eq] > col[:, :-1][eq]).all(), what         # equal values: ascending columns
    rest = M.copy()
    rest[rows, col] = -np.inf
    top = rest.max(axis=1)                                        # the best unlisted column
    last = val[:, -1]
    assert (top <= last + atol + rtol * np.abs(last)).all(), what
    if mode == "inner":                                           # the sweep's products are bit-identical wherever they are computed
        wv, wc = O.lists_from_matrix(M, cut)
        assert np.array_equal(col, wc) and np.array_equal(val, wv), what


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("d", [12, 75, 200])
def test_lists_against_sim_on_the_same_tensors(d, mode):
    M = _matrix(d, mode)
    for cut in CUTS:
        val, col, redone = _lists(d, mode, cut)
        assert redone == 0                                        # 333 columns: every column is a candidate, nothing to redo
        _check_lists(M, val, col, cut, mode, (d, mode, cut))
    dup = np.arange(7, N2, 7)
    val, col, _ = _lists(d, mode, N2)
    pos = np.argsort(col, axis=1)                                 # position of every column in the full list
    assert (val[np.arange(N1)[:, None], pos[:, dup]] == val[np.arange(N1)[:, None], pos[:, dup - 1]]).all()
    assert (pos[:, dup] == pos[:, dup - 1] + 1).all()             # a duplicated row sits right behind its lower-numbered twin


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("d,sample_cols,cut", [(12, 64, 32), (75, 64, 100), (75, 8, 100), (200, 16, 128), (12, 333, 1)])
def test_thresholded_sweep_and_redone_rows_give_the_same_lists(d, mode, sample_cols, cut):
    """A forced column sample puts these small shapes through what large inputs take: a per-row threshold, and rows whose
    estimate came out too tight redone as whole rows.  The lists are the unthresholded ones, bit for bit with the inner
    product; with a metric / CSLS the redone rows go through another kernel's epilogue, so the values agree to the band."""
    val0, col0, _ = _lists(d, mode, cut)
    val, col, redone = _lists(d, mode, cut, sample_cols)
    print(f"d={d} {mode} cut={cut} sample_cols={sample_cols}: {redone} rows redone")
    _check_lists(_matrix(d, mode), val, col, cut, mode, (d, mode, cut, sample_cols))
    if mode == "inner":
        assert np.array_equal(col, col0) and np.array_equal(val, val0)
    if sample_cols == 8:
        assert redone > 0                                         # 6 of 9 sampled values: the estimate must miss for some of 300 rows


@pytest.mark.parametrize("mode", ["inner", "euclid_csls"])
def test_automatic_threshold_past_the_candidate_capacity(mode):
    """1500 x 5000, above the 1024 columns a row's candidate segments hold: the threshold comes from the automatic sample
    (every second column), 79 column tiles split into 8 segments, flagged rows (if any) are redone.  Reference: a stable
    descending sort of sim(...) on the device (equal values keep their column order)."""
    from multike_amd.base import similarity as S
    from multike_amd.base.alignment import candidate_lists, csls_means, prepare_operands
    metric, normalize, k = MODES[mode]
    g = torch.Generator(device="cuda").manual_seed(11)
    e2 = torch.randn(5000, 32, device="cuda", generator=g)
    e2[7::7] = e2[6:-1:7]
    e1 = e2[:1500] + 1.5 * torch.randn(1500, 32, device="cuda", generator=g)
    a, b, kpad, code, sq1, sq2 = prepare_operands(e1, e2, metric, normalize, "cuda")
    csls = csls_means(a, b, kpad, code, sq1, sq2, k) if k else None
    M = S.sim(e1, e2, metric, normalize, k)
    wv, wc = torch.sort(M, dim=1, descending=True, stable=True)
    for cut in (100, 128):
        val, col, redone = candidate_lists(a, b, kpad, cut, code, sq1, sq2, csls)
        print(f"1500 x 5000 {mode} cut={cut}: {redone} rows redone")
        assert redone < 150                                       # the estimate aims at 2 cut + 32 candidates: misses are rare
        if mode == "inner":
            assert torch.equal(col.long(), wc[:, :cut]) and torch.equal(val, wv[:, :cut])
        _check_lists(M.cpu().numpy(), val.cpu().numpy(), col.cpu().numpy(), cut, "inner_csls" if k else mode, (mode, cut))
    whole = candidate_lists(a, b, kpad, 129, code, sq1, sq2, csls)    # the same rows through the whole-row path
    assert torch.equal(whole[1][:, :128], col) or mode != "inner"


@pytest.mark.parametrize("mode", ["inner", "euclid_csls"])
def test_sim_mat_given_by_the_caller(mode):
    from multike_amd.base.alignment import candidate_lists
    M = _matrix(75, mode)
    wide = torch.full((N1, N2 + 3), float("nan"), device="cuda")  # a row stride above n2
    wide[:, :N2] = torch.as_tensor(M).cuda()
    for cut in (100, 129):
        for mat in (torch.as_tensor(M).cuda(), wide[:, :N2]):
            val, col, _ = candidate_lists(None, None, 0, cut, sim_mat=mat)
            wv, wc = O.lists_from_matrix(M, cut)                  # the caller's values are used as they are: exact
            assert np.array_equal(col.cpu().numpy(), wc) and np.array_equal(val.cpu().numpy(), wv), (mode, cut)
        if mode == "inner":                                       # and the operands give the same lists
            val, col, _ = _lists(75, mode, cut)
            assert np.array_equal(col, wc) and np.array_equal(val, wv)


def test_nan_never_enters_a_list_and_short_lists_are_padded():
    from multike_amd.base.alignment import candidate_lists
    rng = np.random.default_rng(5)
    M = rng.standard_normal((40, 50)).astype(np.float32)
    M[rng.random(M.shape) < 0.7] = np.nan
    M[7] = np.nan
    val, col, _ = candidate_lists(None, None, 0, 30, sim_mat=torch.as_tensor(M).cuda())
    wv, wc = O.lists_from_matrix(M, 30)
    assert (wc == -1).any() and np.array_equal(col.cpu().numpy(), wc) and np.array_equal(val.cpu().numpy(), wv)
    # through the operands: a NaN row of E2 is a NaN column of every list, in both paths
    e1, e2 = (t.clone() for t in _inputs(12))
    e2[5] = float("nan")
    e2[300:] = float("nan")
    from multike_amd.base.alignment import prepare_operands
    a, b, kpad, code, _, _ = prepare_operands(e1, e2, "inner", False, "cuda")
    for cut in (128, 333):
        val, col, _ = candidate_lists(a, b, kpad, cut, code)
        col = col.cpu().numpy()
        assert not np.isin(col, [5] + list(range(300, 333))).any()
        assert ((col >= 0).sum(1) == min(cut, 299)).all() and (np.diff((col < 0).astype(int), axis=1) >= 0).all()


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("d", [12, 75, 200])
def test_match_is_the_oracle_on_the_device_lists_and_has_no_blocking_pair(d, mode):
    for cut in CUTS:
        val, col, _ = _lists(d, mode, cut)
        got, _ = _device_match(val, col, N2)
        assert np.array_equal(got, O.deferred_acceptance(val, col, N2)), (d, mode, cut)
        assert O.blocking_pairs(val, col, got, N2) == [], (d, mode, cut)
        held = got[got >= 0]
        assert len(set(held.tolist())) == len(held)               # one-to-one
        if cut == N2:
            assert (got >= 0).all()                               # full lists, n2 >= n1: everybody is matched


@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_runs_are_bit_identical(mode):
    from multike_amd.base.alignment import stable_alignment
    metric, normalize, k = MODES[mode]
    e1, e2 = _inputs(75)
    runs = []
    for _ in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            runs.append(stable_alignment(e1, e2, metric, normalize, k, 4, cut=100))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert runs[0][0].dtype == np.int64 and runs[0][0].shape == (N1,)
    val, col, _ = _lists(75, mode, 100)
    assert np.array_equal(runs[0][0], O.deferred_acceptance(val, col, N2))


# ------------------------------------------------------------------------------------------------ 4. the reference's matching
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "stable_golden.npz"))


@pytest.mark.parametrize("case", ["inner_sq", "inner_wide", "inner_csls", "euclid", "euclid_csls", "cosine_raw"])
def test_reference_parity(golden, case):
    from multike_amd.base.alignment import stable_alignment
    n1, n2, d, k, normalize, cut = (int(x) for x in golden[case + "/meta"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        match, precision = stable_alignment(golden[case + "/e1"], golden[case + "/e2"], str(golden[case + "/metric"]),
                                            bool(normalize), k, 8, cut=cut)
    assert np.array_equal(match, golden[case + "/match"]), case
    lines = out.getvalue().splitlines()
    assert len(lines) == 2 and re.fullmatch(r"generating candidate lists costs time \d+\.\d{3} s ", lines[0]), lines
    m = re.fullmatch(r"stable alignment precision = (\d+\.\d{3})%, time = \d+\.\d{3} s ", lines[1])
    assert m and m.group(1) == "{:.3f}".format(float(golden[case + "/precision"])), lines
    assert abs(precision - float(golden[case + "/precision"])) < 1e-3


# ------------------------------------------------------------------------------------------------ 5. the drivers
def _strip_times(text):
    return re.sub(r"time = \d+\.\d+ s|costs time \d+\.\d+ s", "time", text)


def test_drivers_with_stable_cut():
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.MultiKE_Late import test as late_test, test_WVA
    from multike_amd.synthetic import SyntheticData, synthetic_args
    dim = 24
    data = SyntheticData(n_ent=1600, n_rel=20, n_attr=16, n_values=300, dim=dim, seed=13, shared_structure=0.8)
    n1 = data.kgs.entities_num // 2
    rng = np.random.default_rng(2)
    base = rng.standard_normal((n1, dim)).astype(np.float32)
    nm = np.concatenate([base, base + 0.8 * rng.standard_normal((n1, dim)).astype(np.float32)])
    data.local_name_vectors = nm / np.linalg.norm(nm, axis=1, keepdims=True)
    args = synthetic_args(dim=dim, batch_size=801, attribute_batch_size=601, entity_batch_size=499, neg_triple_num=6,
                          learning_rate=0.03, ITC_learning_rate=0.05, max_epoch=2, shared_learning_max_epoch=1, start_valid=1,
                          eval_freq=1, start_predicate_soft_alignment=2, seed=3, output="/tmp/multike_out_stable/", csls=10,
                          stable_cut=100)
    model = MultiKE_CV(data, args, data.predicate_align_model)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        model.run()
    lines = out.getvalue().splitlines()
    labels = [i for i, l in enumerate(lines) if l.endswith("results:")]
    tests = [i for i in labels if "test results:" in lines[i]]
    assert len(tests) >= 4 and len(tests) < len(labels)
    for i in labels:                                              # after each test block, and only there
        nxt = min([j for j in labels if j > i] + [len(lines)])
        block = [l for l in lines[i + 1:nxt] if "results" in l or "candidate lists" in l or "stable alignment" in l]
        if i in tests:
            assert len(block) >= 3 and block[0].startswith("quick results with csls: csls=10"), block
            assert block[1].startswith("generating candidate lists costs time ") and \
                block[2].startswith("stable alignment precision = "), block
        else:
            assert not any("stable alignment" in l or "candidate lists" in l for l in block), block
    assert sum("stable alignment precision" in l for l in lines) == len(tests)

    def capture(fn):
        with contextlib.redirect_stdout(io.StringIO()) as o:
            fn(model)
        return _strip_times(o.getvalue())
    for fn in (late_test, test_WVA):
        with_stable = capture(fn)
        assert with_stable.count("stable alignment precision = ") == 1
        del model.args.stable_cut                                 # the key absent: the printed output of a test is unchanged
        absent = capture(fn)
        model.args.stable_cut = 0
        off = capture(fn)
        model.args.stable_cut = 100
        assert "stable" not in absent and absent == off
        kept = [l for l in with_stable.splitlines() if "stable alignment" not in l and "candidate lists" not in l]
        assert kept == absent.splitlines()
