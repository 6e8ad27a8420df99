"""The sparse Sinkhorn re-scoring end to end through the public functions of multike_amd.base.alignment: the potentials on the
support the device built against the float64 oracle (sparse_sinkhorn_oracle.py) within the counted bound, ranks and ties on every
row that wins or loses by a margin, full support against the dense golden cases, and every decoder taking
sinkhorn=(iters, tau, cut).

The case is the planted one of the oracle module: n1 200, n2 260, d 24, noise 1.1, seed 0, normalised, cut 8, 5 iterations,
tau 0.05.  Bound of the potentials: iters * (bound(tau, longest row, M) + bound(tau, longest column, M)), M = the largest
|value| + the largest |potential| (sinkhorn_oracle.bound is the counted bound of one log-sum-exp call, and log-sum-exp is
1-Lipschitz in the potentials it subtracts).  Ranks are compared where the gap of 2 (s - a - b) to the nearest other column is
at least 8 times that bound: twice the error of a and of b, the rounding of the device's own s against the oracle's, and the
kernel's 2 s - 2 a - 2 b in f32."""
import contextlib
import io
import os

import numpy as np
import pytest

import sinkhorn_oracle as O
import sparse_sinkhorn_oracle as SO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N1, N2, D, NOISE, SEED, CUT, ITERS, TAU = 200, 260, 24, 1.1, 0, 8, 5, 0.05
OPTION = (ITERS, TAU, CUT)


def _similarity(e1, e2, metric):
    a, b = e1.astype(np.float64), e2.astype(np.float64)
    if metric == "inner":
        return a @ b.T
    d2 = (a * a).sum(1)[:, None] - 2.0 * (a @ b.T) + (b * b).sum(1)[None, :]
    return 1.0 - np.sqrt(np.maximum(d2, 0.0))


def _checked(metric):
    """Everything the tests of one metric share, computed once: the operands, the device's support and potentials, the oracle's
    potentials on that support, the bound."""
    from multike_amd.base import alignment as al
    e1, e2, _ = SO.case(N1, N2, D, NOISE, SEED)
    ops = al.prepare_operands(e1, e2, metric, True, "cuda")
    s = al.sparse_support(ops, CUT)
    E = s.entries()
    row_off, col_off = s.row_off.cpu().numpy(), s.col_off.cpu().numpy()
    rows = np.repeat(np.arange(N1), np.diff(row_off))
    cols, vals = s.ent_col.cpu().numpy()[:E], s.ent_val.cpu().numpy()[:E]
    a, b = SO.potentials(N1, N2, rows, cols, vals, ITERS, TAU)
    M = float(np.abs(vals).max() + max(np.abs(a).max(), np.abs(b).max()))
    bound = ITERS * (O.bound(TAU, int(np.diff(row_off).max()), M) + O.bound(TAU, int(np.diff(col_off).max()), M))
    pa, pb = al.sparse_sinkhorn_potentials(s, ITERS, TAU)
    return dict(e1=e1, e2=e2, ops=ops, support=s, E=E, rows=rows, cols=cols, vals=vals, a=a, b=b, bound=bound, pa=pa, pb=pb,
                S=_similarity(e1, e2, metric), row_off=row_off, col_off=col_off)


@pytest.fixture(scope="module")
def checked():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = _checked(metric)
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", ["inner", "euclidean"])
def test_potentials_and_ranks_against_the_oracle(checked, metric):
    from multike_amd.base.alignment import alignment_counts
    c = checked(metric)
    # the support is what the lists of the float64 similarity name, wherever no two candidates are closer than f32 can tell
    lens_r, lens_c = np.diff(c["row_off"]), np.diff(c["col_off"])
    assert lens_r.min() >= CUT and lens_c.min() >= CUT and c["E"] < 0.06 * N1 * N2
    assert np.abs(c["vals"] - c["S"][c["rows"], c["cols"]]).max() <= 1e-5
    ea = float(np.abs(c["pa"].cpu().numpy().astype(np.float64) - c["a"]).max())
    eb = float(np.abs(c["pb"].cpu().numpy().astype(np.float64) - c["b"]).max())
    print(f"{metric}: {c['E']} of {N1 * N2} pairs, longest row {lens_r.max()}, longest column {lens_c.max()}; potential errors "
          f"{ea:.3e} (rows) {eb:.3e} (columns), bound {c['bound']:.3e}, ratio {max(ea, eb) / c['bound']:.3f}")
    assert ea <= c["bound"] and eb <= c["bound"]
    greater, ties, best = alignment_counts(c["e1"], c["e2"], True, metric=metric, sinkhorn=OPTION)
    want_g, want_t, want_best, gap = O.rank_oracle(2.0 * O.scores(c["S"], c["a"], c["b"]))
    sure = gap >= 8 * c["bound"]
    print(f"{metric}: {int((~sure).sum())} of {N1} rows left out; oracle Hits@1 {np.mean(want_g == 0) * 100:.1f}")
    assert (~sure).sum() <= 0.05 * N1
    g, t = greater.cpu().numpy(), ties.cpu().numpy()
    assert np.array_equal(g[sure], want_g[sure]) and np.array_equal(t[sure], want_t[sure])
    top = want_g == 0
    assert np.array_equal(best.cpu().numpy()[sure & top], want_best[sure & top])


def test_same_bits_twice(checked):
    import torch
    from multike_amd.base import alignment as al
    c = checked("inner")
    s, again = c["support"], al.sparse_support(c["ops"], CUT)
    for name in ("row_off", "col_off", "row_seg", "col_seg", "count"):
        assert torch.equal(getattr(s, name), getattr(again, name)), name
    for name in ("ent_col", "ent_val", "ent_row", "ent_idx"):
        assert torch.equal(getattr(s, name)[:c["E"]].view(torch.int32), getattr(again, name)[:c["E"]].view(torch.int32)), name
    pa, pb = al.sparse_sinkhorn_potentials(again, ITERS, TAU)
    assert torch.equal(pa.view(torch.int32), c["pa"].view(torch.int32)) and torch.equal(pb.view(torch.int32), c["pb"].view(torch.int32))
    r_t, r_s = al.sparse_sinkhorn_terms(c["ops"], *OPTION)
    assert torch.equal(r_t, 2.0 * c["pa"]) and torch.equal(r_s, 2.0 * c["pb"])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sinkhorn_golden.npz"))


@pytest.mark.parametrize("name", ["inner_100", "inner_sq", "inner_wide", "euclid"])
def test_full_support_is_the_dense_rescoring(golden, name):
    import torch
    from multike_amd.base import alignment as al
    n1, n2, d, normalize, iters = (int(x) for x in golden[name + "/meta"])
    tau, M, metric = float(golden[name + "/tau"]), float(golden[name + "/M"]), str(golden[name + "/metric"])
    bound = iters * (O.bound(tau, n2, M) + O.bound(tau, n1, M))                 # the dense test's own _pot_bound
    ops = al.prepare_operands(golden[name + "/e1"], golden[name + "/e2"], metric, bool(normalize), "cuda")
    _, option = al._check_rescoring(0, (iters, tau, n2))
    assert option == (iters, tau, n2)
    s = al.sparse_support(ops, n2)                                              # cut clamped to n1 on the columns' side
    assert s.entries() == n1 * n2
    r_t, r_s = al._rescoring_terms(ops, 0, option)
    ea = float(np.abs(0.5 * r_t.cpu().numpy().astype(np.float64) - golden[name + "/a"]).max())
    eb = float(np.abs(0.5 * r_s.cpu().numpy().astype(np.float64) - golden[name + "/b"]).max())
    print(f"{name}: full support, potential errors {ea:.3e} (rows) {eb:.3e} (columns), 2L-bound {bound:.3e}")
    assert ea <= bound and eb <= bound
    over = al._rescoring_terms(ops, 0, (iters, tau, 10 ** 6))                   # any larger cut is the same support
    assert torch.equal(over[0], r_t) and torch.equal(over[1], r_s)
    # the 2-tuple is the dense function, bit for bit
    assert al._check_rescoring(0, (iters, tau)) == (0, (iters, tau))
    dense = al.sinkhorn_terms(*ops, iters, tau)
    routed = al._rescoring_terms(ops, 0, (iters, tau))
    assert torch.equal(routed[0], dense[0]) and torch.equal(routed[1], dense[1])


def test_every_decoder_takes_the_option(checked):
    import torch
    from multike_amd import _lib
    from multike_amd.base import alignment as al
    from multike_amd.base.bootstrap import bootstrap_links
    c = checked("inner")
    e1, e2, ops = c["e1"], c["e2"], c["ops"]
    a, b, kpad, code, sq1, sq2 = ops
    terms = (2.0 * c["pa"], 2.0 * c["pb"])                                      # held against the oracle above
    with contextlib.redirect_stdout(io.StringIO()):
        # the rank kernel has a hand-over of the terms
        got = al.alignment_counts(e1, e2, True, metric="inner", sinkhorn=OPTION)
        want = al.alignment_counts(e1, e2, True, metric="inner", csls=terms)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        # stable matching and the auction: the same lists and rounds from the terms
        val, col, _ = al.candidate_lists(a, b, kpad, 20, code, sq1, sq2, terms)
        match, matched, gold, _ = al.stable_matching(val, col, N2)
        got_match, precision = al.stable_alignment(e1, e2, "inner", True, 0, 1, cut=20, sinkhorn=OPTION)
        assert np.array_equal(got_match, match.cpu().numpy().astype(np.int64)) and precision == gold / matched * 100
        listed = (col >= 0) & torch.isfinite(val)
        floor = float(torch.where(listed, val, torch.full_like(val, float("inf"))).min()) - 1.0
        want_assign, _, _ = al.assignment_matching(val, col, N2, 1e-3, floor)
        got_assign = al.assignment_alignment(e1, e2, "inner", True, 0, 1, cut=20, sinkhorn=OPTION)[0]
        assert np.array_equal(got_assign, want_assign.cpu().numpy().astype(np.int64))
        # the mutual decoder and self-training's decode
        want_match, _, row_best = al._mutual_decode(ops + (terms,), None)
        got_match, score = al.mutual_pairs(e1, e2, "inner", True, sinkhorn=OPTION)
        assert torch.equal(got_match, want_match) and torch.equal(score.view(torch.int32), al._best_value(row_best).view(torch.int32))
        assert int((want_match >= 0).sum()) > N1 // 2
        mm = al.mutual_alignment(e1, e2, "inner", True, 0, 1, sinkhorn=OPTION)[0]
        assert np.array_equal(mm, want_match.cpu().numpy().astype(np.int64))
        ids1, ids2 = np.arange(N1, dtype=np.int32), np.arange(N1, N1 + N2, dtype=np.int32)
        partner, boot_match, counts = bootstrap_links(e1, e2, ids1, ids2, N1 + N2, sinkhorn=OPTION)
        assert torch.equal(boot_match, want_match)
        assert torch.equal(partner, _lib.boot_partner(want_match, torch.as_tensor(ids1).cuda(), torch.as_tensor(ids2).cuda(), N1 + N2))
        assert int(counts[0]) == int((want_match >= 0).sum())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        _, hits1, _, _ = al.greedy_alignment(e1, e2, [1, 5], 1, "inner", True, 0, True, sinkhorn=OPTION)
    assert buf.getvalue().startswith(f"accurate results with sinkhorn: iters={ITERS}, tau={TAU}, cut={CUT}, hits@[1, 5] = ")
    want_g = O.rank_oracle(2.0 * O.scores(c["S"], c["a"], c["b"]))[0]
    assert abs(hits1 - np.mean(want_g == 0) * 100) <= 100.0 * 0.05             # the rows the margin leaves out, at most


def test_options_and_refusals():
    from multike_amd import _lib
    from multike_amd.base import alignment as al
    from multike_amd.base.similarity import sim
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args, sinkhorn_option
    assert default_args().sinkhorn_cut == 0
    assert sinkhorn_option(default_args(sinkhorn_iters=10)) == (10, 0.05)
    assert sinkhorn_option(default_args(sinkhorn_iters=10, sinkhorn_cut=0)) == (10, 0.05)
    assert sinkhorn_option(default_args(sinkhorn_iters=10, sinkhorn_cut=100)) == (10, 0.05, 100)
    assert sinkhorn_option(default_args(sinkhorn_cut=100)) is None                 # no iterations: off
    with pytest.raises(_lib.MultiKEHipError, match="csls and sinkhorn_iters are both set"):
        sinkhorn_option(default_args(sinkhorn_iters=10, sinkhorn_cut=100, csls=10))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k are both set: choose one re-scoring"):
        al._check_rescoring(10, OPTION)
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k are both set: choose one re-scoring"):
        al._check_rescoring(0, OPTION, csls=(None, None))
    for bad in ((5, 0.05, 0), (5, 0.05, -1), (5, 0.05, 2.5)):
        with pytest.raises(_lib.MultiKEHipError, match="cut >= 1"):
            al._check_rescoring(0, bad)
    with pytest.raises(_lib.MultiKEHipError, match="finite tau > 0"):
        al._check_rescoring(0, (5, 0.0, 8))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn_iters"):
        _ShardedMixin()._init_sharded(None, default_args(sinkhorn_iters=10, sinkhorn_cut=100), None, 0, 2)
    e = np.eye(4, dtype=np.float32)
    with pytest.raises(_lib.MultiKEHipError, match="matrix-free"):
        sim(e, e, sinkhorn=OPTION)
    assert al._check_rescoring(0, (5, 0.05, 8.0)) == (0, (5, 0.05, 8))
