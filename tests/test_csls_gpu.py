"""CSLS re-scoring and the euclidean metric of the alignment evaluator on the GPU (mke_align_topk_mean + mke_align_rank_ex):
against the reference's own evaluator (tests/golden/csls_golden.npz), against the float64 oracle (tests/csls_oracle.py),
exact top-k means on tied / zero / duplicated rows (both kernel paths), determinism, memory at 60K x 60K, the plain path
unchanged, errors, and the drivers (single-GPU and sharded) with the hyper-parameter `csls`."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import csls_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOP_K = [1, 5, 10, 50]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "csls_golden.npz"))


def _means(e1, e2, k, metric="inner", normalize=True):
    from multike_amd.base.alignment import csls_means, prepare_operands
    a, b, kpad, code, sq1, sq2 = prepare_operands(e1, e2, metric, normalize, "cuda")
    r_t, r_s = csls_means(a, b, kpad, code, sq1, sq2, k)
    return r_t.cpu().numpy(), r_s.cpu().numpy()


def test_against_the_reference_fixture(golden):
    from multike_amd.base.alignment import greedy_alignment
    for c in golden["cases"]:
        n1, n2, d, k, normalize, dup = (int(x) for x in golden[c + "/meta"])
        metric = str(golden[c + "/metric"])
        e1, e2 = golden[c + "/e1"], golden[c + "/e2"]
        r_t, r_s = _means(e1, e2, k, metric, bool(normalize))
        np.testing.assert_allclose(r_t, golden[c + "/r_t"], rtol=1e-6, atol=1e-6, err_msg=c)
        np.testing.assert_allclose(r_s, golden[c + "/r_s"], rtol=1e-6, atol=1e-6, err_msg=c)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            pairs, hits1, mr, mrr = greedy_alignment(e1, e2, TOP_K, 8, metric, bool(normalize), k, True)
        assert f"accurate results with csls: csls={k}, hits@{TOP_K}" in out.getvalue()
        if not dup:       # every gap >= 1e-4 (generator): the ranks are the reference's exactly
            assert hits1 == float(golden[c + "/hits"][0]), c
            np.testing.assert_allclose(mr, float(golden[c + "/mr"]), rtol=1e-9)
            np.testing.assert_allclose(mrr, float(golden[c + "/mrr"]), rtol=1e-9)
            assert sorted(pairs) == [tuple(p) for p in golden[c + "/pairs"].tolist()], c
        else:             # duplicated columns: the decided rows agree, the tied ones score their expectation
            from multike_amd.base.alignment import alignment_counts
            g, t, _ = alignment_counts(e1, e2, bool(normalize), metric=metric, csls_k=k)
            g, t = g.cpu().numpy(), t.cpu().numpy()
            sure = golden[c + "/gap"] >= 1e-4
            assert np.array_equal(g[sure], golden[c + "/rank"][sure]) and np.array_equal(t[sure], np.ones(sure.sum()))
            assert np.array_equal(g[~sure], golden[c + "/rank"][~sure]) and np.array_equal(t[~sure], golden[c + "/ties"][~sure])


@pytest.mark.parametrize("n1,n2,d,metric,normalize", [
    (1000, 1777, 75, "inner", True), (33, 33, 4, "inner", True), (4097, 6000, 256, "inner", True),
    (500, 501, 100, "euclidean", False), (700, 900, 300, "cosine", False), (640, 700, 320, "euclidean", True)])
def test_ranks_vs_float64_oracle(n1, n2, d, metric, normalize):
    from multike_amd.base.alignment import alignment_counts
    rng = np.random.default_rng(n1 + d)
    base = rng.standard_normal((n2, d)).astype(np.float32)
    e2 = base + 0.3 * rng.standard_normal((n2, d)).astype(np.float32)
    e1 = (base[:n1] + 1.0 * rng.standard_normal((n1, d))).astype(np.float32)
    k = min(10, n1 - 2)
    g, t, _ = alignment_counts(e1, e2, normalize, metric=metric, csls_k=k)
    cs, r_t, r_s = O.csls64(e1, e2, metric, normalize, k)
    ge, _ = O.counts(cs)
    err = np.abs(g.cpu().numpy() - ge)
    assert np.mean(err == 0) > 0.995 and err.max() <= 2, (np.mean(err == 0), err.max())
    mt, ms = _means(e1, e2, k, metric, normalize)
    np.testing.assert_allclose(mt, r_t, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ms, r_s, rtol=2e-5, atol=2e-5)


def _integer_rows(rng, n, d, lo=-2, hi=3):
    """Small integers: every dot product is exact in f32 (on any path), so the top-k multiset is known exactly."""
    return rng.integers(lo, hi, size=(n, d)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 7, 10, 32, 33, 64, 300, 5000])
def test_topk_means_exact_on_ties_zero_and_duplicated_rows(k):
    from multike_amd import _lib
    from multike_amd.base.alignment import csls_means, prepare_operands
    rng = np.random.default_rng(k)
    n1, n2, d = 5200, 6100, 16
    e1 = _integer_rows(rng, n1, d)
    e2 = _integer_rows(rng, n2, d, -1, 2)            # heavy ties: few distinct dot products
    e1[5] = 0.0                                       # zero rows (every similarity 0)
    e2[17] = 0.0
    e1[100:140] = e1[99]                              # duplicated rows
    e2[200:260] = e2[3]
    a, b, kpad, code, _, _ = prepare_operands(e1, e2, "inner", False, "cuda")
    r_t, r_s = csls_means(a, b, kpad, code, None, None, k)
    s = e1.astype(np.float64) @ e2.astype(np.float64).T
    exp_t = (O.topk_mean(s, k)).astype(np.float32)
    exp_s = (O.topk_mean(s.T, k)).astype(np.float32)
    assert np.array_equal(r_t.cpu().numpy(), exp_t)
    assert np.array_equal(r_s.cpu().numpy(), exp_s)
    if k == 10:      # the euclidean path over the same integer rows: squared distances exact, the device sqrt within 1 ulp
        a, b, kpad, code, sq1, sq2 = prepare_operands(e1, e2, "euclidean", False, "cuda")
        m = _lib.align_topk_mean(a, b, kpad, k, code, sq1, sq2).cpu().numpy()
        d2 = (e1.astype(np.float64) ** 2).sum(1)[:, None] + (e2.astype(np.float64) ** 2).sum(1)[None, :] - 2 * s
        se = (1.0 - np.sqrt(np.maximum(d2, 0))).astype(np.float32).astype(np.float64)
        np.testing.assert_allclose(m, O.topk_mean(se, k).astype(np.float32), rtol=3e-7, atol=0)


def test_mid_rank_ties_and_perfect_alignment():
    from multike_amd.base.alignment import alignment_counts, greedy_alignment
    rng = np.random.default_rng(4)
    e = rng.standard_normal((300, 32)).astype(np.float32)
    g, t, best = alignment_counts(e, e.copy(), True, csls_k=10)
    assert int(g.max()) == 0 and int(t.max()) == 1 and np.array_equal(best.cpu().numpy(), np.arange(300))
    # duplicated rows on both sides: every gold ties with its duplicate under CSLS too (same similarities, same r_T / r_S)
    e2 = e.copy()
    e2[1::2] = e2[0::2]
    g, t, best = alignment_counts(e2, e2.copy(), True, csls_k=10)
    assert int(g.max()) == 0 and np.all(t.cpu().numpy() == 2)
    assert np.array_equal(best.cpu().numpy(), np.repeat(np.arange(0, 300, 2), 2))     # the lowest column wins the tie
    with contextlib.redirect_stdout(io.StringIO()):
        _, hits1, mr, mrr = greedy_alignment(e2, e2.copy(), TOP_K, 1, "inner", True, 10, True)
    assert abs(hits1 - 50.0) < 1e-9 and abs(mr - 1.5) < 1e-9 and abs(mrr - 0.75) < 1e-12


def test_two_runs_bit_identical():
    from multike_amd.base.alignment import alignment_counts, csls_means, prepare_operands
    rng = np.random.default_rng(9)
    e1 = rng.standard_normal((3000, 75)).astype(np.float32)
    e2 = rng.standard_normal((3500, 75)).astype(np.float32)
    outs = []
    for _ in range(2):
        a, b, kpad, code, sq1, sq2 = prepare_operands(e1, e2, "euclidean", True, "cuda")
        r = csls_means(a, b, kpad, code, sq1, sq2, 10)
        outs.append([x.cpu().numpy() for x in r] + [x.cpu().numpy() for x in alignment_counts(e1, e2, True, metric="euclidean", csls_k=10)])
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_plain_path_unchanged_and_errors():
    from multike_amd import _lib
    from multike_amd.base.alignment import alignment_counts, greedy_alignment
    rng = np.random.default_rng(5)
    e1 = rng.standard_normal((900, 75)).astype(np.float32)
    e2 = rng.standard_normal((1000, 75)).astype(np.float32)
    new = alignment_counts(e1, e2, True, metric="inner", csls_k=0)
    old = alignment_counts(e1, e2, True)
    for x, y in zip(new, old):
        assert torch.equal(x, y)
    # the inner fold of mke_align_rank_ex (no CSLS) agrees with mke_align_rank on the same operands
    from multike_amd.base.alignment import prepare_operands
    a, b, kpad, code, _, _ = prepare_operands(e1, e2, "inner", True, "cuda")
    rk, ti, be = (torch.zeros(900, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64))
    _lib.align_rank_ex(a, b, kpad, rk, ti, be)
    assert torch.equal(rk.long(), old[0]) and torch.equal(ti.long().clamp_min(1), old[1])
    assert torch.equal(0xFFFFFFFF - (be & 0xFFFFFFFF), old[2])
    with contextlib.redirect_stdout(io.StringIO()) as out:
        greedy_alignment(e1, e2, TOP_K, 1, "inner", True, 0, True)
    assert "csls" not in out.getvalue()
    with pytest.raises(_lib.MultiKEHipError):
        alignment_counts(e1[:20], e2[:20], True, csls_k=19)                  # k > n - 2
    with pytest.raises(_lib.MultiKEHipError):
        greedy_alignment(e1, e2, TOP_K, 1, "manhattan", False, 10, True)


def test_60k_csls_stays_far_below_the_matrix():
    from multike_amd.base.alignment import alignment_counts
    n, d = 60000, 75
    g = torch.Generator(device="cuda").manual_seed(0)
    e2 = torch.randn(n, d, device="cuda", generator=g)
    e1 = e2 + 0.5 * torch.randn(n, d, device="cuda", generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    greater, ties, best = alignment_counts(e1, e2, True, csls_k=10)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < (1 << 30), peak
    hits1 = float((greater == 0).double().mean())
    assert 0.5 < hits1 <= 1.0


def test_device_similarity_surface():
    from multike_amd.base import similarity as S
    rng = np.random.default_rng(2)
    e1 = rng.standard_normal((200, 20)).astype(np.float32)
    e2 = rng.standard_normal((260, 20)).astype(np.float32)
    for metric, normalize in (("inner", True), ("euclidean", False), ("cosine", False)):
        host = S.sim(e1, e2, metric, normalize, 10)
        dev = S.sim(torch.as_tensor(e1, device="cuda"), torch.as_tensor(e2, device="cuda"), metric, normalize, 10)
        np.testing.assert_allclose(dev.cpu().numpy(), host, rtol=1e-4, atol=2e-5)
    m = torch.as_tensor(S.sim(e1, e2, "inner", True), device="cuda")
    np.testing.assert_allclose(S.calculate_nearest_k(m, 7).cpu().numpy(), S.calculate_nearest_k(m.cpu().numpy(), 7), rtol=2e-6)


def _driver_setup():
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
                          eval_freq=1, start_predicate_soft_alignment=2, seed=3, output="/tmp/multike_out_csls/", csls=10)
    return data, args


def test_single_gpu_driver_with_csls():
    from multike_amd.MultiKE_Late import _eval_pair, _view_embeddings
    from multike_amd.MultiKE_CSL import MultiKE_CV
    data, args = _driver_setup()
    model = MultiKE_CV(data, args, data.predicate_align_model)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = model.run()
    log = out.getvalue()
    assert log.count("quick results with csls: csls=10") >= 4, log[-3000:]
    valid_lines = [l for l in log.splitlines() if "results" in l]
    k = model.kgs

    def rows(m):
        e = _view_embeddings(m, "final", (1, 1, 1))
        return e[k.test_entities1, ], e[k.test_entities2, ]
    e1, e2 = rows(model)
    from multike_amd.base.alignment import greedy_alignment
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, _, mrr = greedy_alignment(e1, e2, TOP_K, 1, "inner", True, 10, False)
    assert abs(res["final"] - mrr) < 1e-9, (res["final"], mrr)
    assert any("quick results: hits@" in l for l in valid_lines)             # validation stays plain


def test_sharded_driver_equals_single_gpu_csls():
    from multike_amd.base.alignment import alignment_counts, tie_aware_metrics
    from multike_amd.distributed_run import ShardedMultiKE_CV
    data, args = _driver_setup()
    model = ShardedMultiKE_CV(data, args, data.predicate_align_model, 0, 1)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = model.run()
    log = out.getvalue()
    assert log.count("accurate results with csls: csls=10") >= 4, log[-3000:]
    k = model.kgs
    e1 = model.rows("final", k.test_entities1)
    e2 = model.rows("final", k.test_entities2)
    g, t, _ = alignment_counts(e1, e2, True, csls_k=10)
    _, _, mrr = tie_aware_metrics(g, t, TOP_K)
    assert abs(res["final"] - mrr) < 1e-12
    # two ranks on this one GPU, one after the other: the driver's own _rank_block with its collectives replaced by a recorded
    # exchange — pass 1 records each rank's share of the r_T / r_S vector, pass 2 hands every rank the sum (the all-gather)
    # and records its Hits / MR / MRR partial sums
    store = {}

    class _Exchange:
        def __init__(self, rank, replay):
            self.rank, self.replay, self.i = rank, replay, 0

        def all_reduce(self, t):
            if self.replay and self.i == 0:
                t.copy_(sum(store[(r, 0)] for r in (0, 1)))
            else:
                store[(self.rank, self.i + 2 * self.replay)] = t.clone()
            self.i += 1

    comm = model._vc
    try:
        model.world = 2
        for replay in (False, True):
            for r in (0, 1):
                model.rank, model._vc = r, _Exchange(r, replay)
                model._rank_block(e1, e2, TOP_K, 10)
    finally:
        model._vc, model.rank, model.world = comm, 0, 1
    acc = (store[(0, 3)] + store[(1, 3)]).cpu().numpy() / e1.shape[0]
    assert abs(float(acc[-1]) - mrr) < 1e-12 and abs(float(acc[-2]) - mr_of(g, t)) < 1e-9


def mr_of(g, t):
    from multike_amd.base.alignment import tie_aware_metrics
    return tie_aware_metrics(g, t, TOP_K)[1]
