"""The multi-GPU drivers (multike_amd/distributed_run.py: `python -m multike_amd.run --gpus N`): the single-GPU schedule code
(MultiKE_CV.run / MultiKE_Late.run, pinned to the reference's loops by tests/test_schedule_golden.py) on row-sharded tables,
with rank-sharded validation / test, the rank-sharded k-NN refresh of truncated sampling and the soft-alignment list refresh.
One rank in-process, and two ranks SHARING the test box's GPU (collectives staged through gloo) against it."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import ranks

pytestmark = pytest.mark.gpu

DIM = 24


def _setup(itc_lr=0.05):
    from multike_amd.synthetic import SyntheticData, synthetic_args
    data = SyntheticData(n_ent=1600, n_rel=20, n_attr=16, n_values=300, dim=DIM, seed=13, shared_structure=0.8)
    n1 = data.kgs.entities_num // 2
    rng = np.random.default_rng(2)
    base = rng.standard_normal((n1, DIM)).astype(np.float32)
    nm = np.concatenate([base, base + 0.8 * rng.standard_normal((n1, DIM)).astype(np.float32)])
    data.local_name_vectors = nm / np.linalg.norm(nm, axis=1, keepdims=True)
    args = synthetic_args(dim=DIM, batch_size=801, attribute_batch_size=601, entity_batch_size=499, neg_triple_num=6,
                          learning_rate=0.03, ITC_learning_rate=itc_lr, max_epoch=6, shared_learning_max_epoch=3, start_valid=2,
                          eval_freq=2, start_predicate_soft_alignment=2, truncated_freq=2, truncated_epsilon=0.9,
                          neg_sampling="truncated", seed=3, output="/tmp/multike_out_sharded/")
    return data, args


def _run(method, rank, world, comm_oc=None, comm_v=None, itc_lr=0.05):
    from multike_amd.distributed_run import ShardedMultiKE_CV, ShardedMultiKE_Late
    data, args = _setup(itc_lr)
    cls = ShardedMultiKE_CV if method == "ITC" else ShardedMultiKE_Late
    model = cls(data, args, data.predicate_align_model, rank, world, comm_oc, comm_v)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = model.run()
    torch.cuda.synchronize()
    return model, res, out.getvalue()


@pytest.mark.parametrize("method", ["ITC", "SSL"])
def test_one_rank_runs_the_whole_schedule(method):
    model, res, log = _run(method, 0, 1)
    assert all(np.isfinite(v) for v in res.values()) and set(res) >= {"nv", "rv", "av", "final"}
    assert res["nv"] > 0.5 and res["final"] > 0.05            # MRR: the name view aligns; the learned shared space well above chance
    # the schedule's between-epoch work happened on the sharded state
    assert model._neighbors[0] is not None and model.m.relation.bat.side1.cand_table is not None      # truncated sampling active
    assert "generating neighbors" in log and "rv valid results:" in log and "final test results:" in log
    assert log.count("cross-kg relation inference in rel. view") == 4                                   # epochs 3..6: i > 2
    assert os.path.exists(os.path.join(model.out_folder, "ent_embeds.npy"))
    # relation-view loss went down
    rel = [float(l.split("avg. loss: ")[1].split(",")[0]) for l in log.splitlines() if " of rel. view" in l]
    assert len(rel) == 6 and rel[-1] < rel[0]
    # sharded evaluation == the single-GPU evaluator on the gathered tables
    from multike_amd.base.alignment import greedy_alignment
    full = model.rv_ent_embeds.eval()
    k = model.kgs
    with contextlib.redirect_stdout(io.StringIO()):
        _, h1, mr, mrr = greedy_alignment(full[k.test_entities1], full[k.test_entities2], model.args.top_k, 1, "inner", True, 0, True)
    np.testing.assert_allclose(res["rv"], mrr, rtol=1e-6)


def _worker(rank, world, method, itc_lr):
    from multike_amd.distributed_oc import OcHostStagedComm
    from multike_amd.distributed_views import HostStagedViewComm
    torch.cuda.set_device(0)
    model, res, log = _run(method, rank, world, OcHostStagedComm(), HostStagedViewComm(), itc_lr)
    tables = model.m.gather()
    if rank == 0:
        return res, {k: np.asarray(tables[k]) for k in ("ent", "rv", "av", "rel", "attr")}, log


@pytest.mark.timeout(900)
@pytest.mark.parametrize("method,itc_lr,elementwise", [("SSL", 0.05, True), ("ITC", 0.004, True), ("ITC", 0.05, False)])
def test_two_ranks_equal_one_rank(method, itc_lr, elementwise):
    """Sharding changes nothing but the order of fp32 sums: same batches (every draw is a function of (seed, epoch)), same
    candidate tables from the sharded k-NN refresh, same metrics from the sharded evaluator.

    Elementwise (tighter than rounds 2-3: max 2e-3 against 2e-2, mean 5e-5 against 2e-4) wherever the schedule does not itself amplify rounding noise:
    the SSL schedule, and the ITC schedule at the reference's own ITC_learning_rate (code/args.json: 0.004).  At this file's
    aggressive 0.05 the early common-space Adagrad steps expand a perturbation by up to x1000 per phase on a handful of
    (row, element) pairs (tests/test_schedule_trace_gpu.py has the derivation and the float64 finite-difference evidence is in
    profiles/r04_parity_noise.log) — two fp32 runs that differ in summation order then differ there by construction, so that
    variant asserts the statistics (mean error, metrics), not a maximum."""
    m1, r1, _ = _run(method, 0, 1, itc_lr=itc_lr)
    ref = m1.m.gather()
    r2, got, log = ranks.run_ranks(2, _worker, (method, itc_lr), limit=800)[0]
    for k in r1:
        assert abs(r2[k] - r1[k]) <= (2e-3 if elementwise else 1e-2), (k, r2[k], r1[k])   # MRR over ~500 test pairs
    for k in ("ent", "rv", "av", "rel", "attr"):
        err = np.abs(got[k] - np.asarray(ref[k]))
        if elementwise:
            # measured (profiles/r04_pytest_gpu.log run): rel (20 hub rows, thousands of fp32 terms each per step) mean 2.7e-5 / max
            # 5.3e-4; the entity tables a decade below
            assert float(np.mean(err)) < 5e-5 and float(err.max()) < 2e-3, (k, float(np.mean(err)), float(err.max()))
        else:
            assert float(np.mean(err)) < 2e-4 and float(np.quantile(err, 0.999)) < 2e-3, (k, float(np.mean(err)), float(err.max()))
    assert "generating neighbors" in log


@pytest.mark.timeout(600)
def test_command_line_launches_itself_with_gpus_2():
    """`python -m multike_amd.run --gpus 2 ...` started plainly launches torch.distributed.run itself, one process per rank
    (here: both on the test box's one GPU, collectives staged through gloo) and rank 0 prints the closing results."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, MKE_BENCH_COMM="staged", PYTHONPATH=ROOT)
    sets = ["max_epoch=2", "shared_learning_max_epoch=1", "start_valid=1", "eval_freq=1", "batch_size=700", "attribute_batch_size=500",
            "entity_batch_size=400", "neg_triple_num=4", "dim=16", "truncated_freq=1", "truncated_epsilon=0.9",
            "start_predicate_soft_alignment=0", "output=\"/tmp/multike_out_cli/\""]
    cmd = [sys.executable, "-m", "multike_amd.run", "--method", "SSL", "--gpus", "2", "--synthetic",
           json.dumps({"n_ent": 1000, "n_rel": 12, "n_attr": 10, "n_values": 200})]
    for s_ in sets:
        cmd += ["--set", s_]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("results:")]
    assert len(line) == 1, out.stdout[-2000:]
    res = json.loads(line[0][len("results:"):])
    assert set(res) == {"nv", "rv", "av", "avg", "wva", "final"} and all(np.isfinite(v) for v in res.values())
    assert out.stdout.count("wvag test results:") == 1           # printed by rank 0 only


@pytest.mark.timeout(900)
def test_sharded_driver_from_a_dataset_folder_learns_like_the_single_gpu_driver(tmp_path):
    """Dataset folder -> DataModel -> the REAL PredicateAlignModel (its `update_predicate_alignment` rebuilds the two predicate
    lists after epoch 10: `set_lists` on the sharded trainers) -> `ShardedMultiKE_CV.run()` on two KGs that share 80 % of their
    structure: the relation and attribute views learn the held-out links, to the level the single-GPU driver reaches from the
    same initial state (different batch draws: statistically, not bit for bit)."""
    from multike_amd.data_model import DataModel
    from multike_amd.distributed_run import ShardedMultiKE_CV
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.predicate_alignment import PredicateAlignModel
    from multike_amd.synthetic import synthetic_args, write_dataset_folder
    folder = str(tmp_path) + "/"
    wf = write_dataset_folder(folder, n_pairs=1500, n_extra=150, n_rel=40, n_attr=30, triples_per_entity=5.0, shared_structure=0.8)
    args = synthetic_args(training_data=folder, output=folder + "out/", word2vec_path=wf, dataset_division="631/", encoder_epoch=5,
                          encoder_active="tanh", encoder_normalize=True, retrain_literal_embeds=False, literal_normalize=True, dim=64,
                          batch_size=2000, attribute_batch_size=2000, entity_batch_size=2000, neg_triple_num=10, learning_rate=0.01,
                          ITC_learning_rate=0.01, max_epoch=24, start_valid=12, eval_freq=12, start_predicate_soft_alignment=10,
                          truncated_freq=10, truncated_epsilon=0.98, is_save=True, seed=1)
    res = {}
    for name, make in (("sharded", lambda d, p: ShardedMultiKE_CV(d, args, p, 0, 1)), ("single", lambda d, p: MultiKE_CV(d, args, p))):
        with contextlib.redirect_stdout(io.StringIO()) as out:
            data = DataModel(args)
            pam = PredicateAlignModel(data.kgs, args)
            model = make(data, pam)
            res[name] = model.run()
        log = out.getvalue()
        assert "generating neighbors" in log and log.count("valid results:") >= 6, name        # k-NN refresh, two validation rounds
        if name == "sharded":
            assert model.m._list_gen["ckgp_rel"] >= 2            # the relation-alignment list was rebuilt after epoch 10 and re-installed
    for name in res:
        assert res[name]["rv"] > 0.75 and res[name]["av"] > 0.4 and res[name]["final"] > 0.6, (name, res[name])
    for k in ("nv", "rv", "av", "final"):
        assert abs(res["sharded"][k] - res["single"][k]) < (1e-6 if k == "nv" else 0.12), (k, res)
