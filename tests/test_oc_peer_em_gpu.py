"""Peer-direct transport of the ENTITY-MAJOR sharded relation step (`OwnerComputesTrainer(peer_direct=True, entity_major=True)`):
the score launch reads the travelling vectors from the owners' send blocks, mirrors them into a local buffer and writes its
partial gradient vectors into the owners' inboxes; k_oc_gv_sum adds an inbox's writer slices in rank order; the second pass
is the collective form's, on the two local buffers.  Ranks are processes SHARING the one GPU (the blocks are mapped over
IPC exactly as between GPUs), gloo with a file rendezvous, collectives and barriers through `OcHostStagedComm` — as the
two-rank tests of tests/test_distributed_oc_gpu.py, whose helpers and shapes these tests use.

Checked: the float64 dense oracle (the tolerances of the existing two-rank test of the same computation), BIT equality
with the collective entity-major form at two ranks (the forms differ only in where the vectors and gradient vectors travel,
and a + b is one float whatever the order), an epoch boundary with the peer blocks mapped again, and three ranks (the
division form of the owner arithmetic, three writers per inbox: the rank order of the sum is what makes two runs agree)."""
import functools

import numpy as np
import pytest

import ranks
from test_distributed_oc_gpu import B, DIM, N_ENT, N_REL, NEG, SEED, _make, _reference

pytestmark = pytest.mark.gpu

PEER, COLL = "peer_direct_em", "collective_em"


def _trainer(rank, world, comm, form, cfg):
    """`_make` of the existing tests; with a per-trainer tuning (which `_make` does not pass on) the same construction in line."""
    peer = form == PEER
    kw = dict(n_ent=cfg.get("n_ent", N_ENT), dim=cfg.get("dim", DIM), neg=cfg.get("neg", NEG), b=cfg.get("b", B), zipf=cfg.get("zipf", 0.0))
    if not cfg.get("tuning"):
        return _make(rank, world, comm=comm, peer=peer, em=True, **kw)
    from multike_amd.distributed_oc import OwnerComputesTrainer
    from multike_amd.synthetic import SyntheticKGs
    from oracle import multike_oracle as mo
    kgs = SyntheticKGs(n_ent=kw["n_ent"], n_rel=N_REL, seed=SEED, zipf=kw["zipf"])
    rng = np.random.default_rng(SEED)
    ent0 = mo.xavier_truncated_normal((kw["n_ent"], kw["dim"]), rng)
    rel0 = mo.xavier_truncated_normal((N_REL, kw["dim"]), rng)
    return OwnerComputesTrainer(kgs, ent0, rel0, kw["b"], kw["neg"], rank, world, seed=SEED, lr=0.02, comm=comm, peer_direct=peer,
                                entity_major=True, tuning=cfg["tuning"])


def _worker(rank, world, forms, cfg):
    """One rank: every form of `forms` in turn on the same inputs (one process group); rank 0 reports."""
    import torch
    from multike_amd.distributed_oc import OcHostStagedComm
    torch.cuda.set_device(0)
    out = {}
    for form in forms:
        tr = _trainer(rank, world, OcHostStagedComm(), form, cfg)
        chk = tr.check()
        assert tr.em and chk["entity_major"]
        assert bool(tr.peer_direct) == (form == PEER) == chk["peer_direct"]
        assert not chk["native_step_loop"] or form == COLL
        steps = cfg["steps"] if cfg["steps"] > 0 else tr.steps - cfg["steps"]      # -k: an epoch and k steps
        if cfg.get("max_epoch"):
            assert tr.steps <= cfg["max_epoch"], tr.steps
        remapped = False
        ring = []
        for i in range(steps):
            if form == PEER and cfg.get("remap") and i == tr.steps:
                # the capacity "grows" at the boundary: every exchange buffer is allocated and the peers' blocks mapped again
                old, tr.C = tr._inbox, 0
            tr.step(i)
            if form == PEER and cfg.get("remap") and i == tr.steps:
                remapped = tr._inbox is not old and tr.C > 0
            ring.append(tr.loss_ring[(i % tr.steps) * tr.chunks].cpu().numpy().copy())     # this rank's partials of the step, raw
        torch.cuda.synchronize()
        kernel_q = bool(cfg.get("tuning", {}).get("oc_score_quarter", 0))
        res = dict(full=tr.gather_entity_table().cpu().numpy(), rel=tr.rel[:, :tr.dim].cpu().numpy().copy(), ring=np.stack(ring),
                   clean=tr.scratch_clean(), check=tr.check(), spe=tr.steps, steps=steps, remapped=remapped, quarter=kernel_q)
        res["loss"] = tr.epoch_loss()
        res["long_rows"] = tr.comm.all_gather_object(res["check"]["long_rows_per_global_step"])     # every rank's
        out[form] = res
        del tr
    if rank == 0:
        return out


RUN = dict(limit=240, group_timeout=120)     # collectives limited to 120 s: a rank that dies must not leave its peers in one for long


@functools.lru_cache(maxsize=None)
def _oracle(world, steps, neg):
    return _reference(world, steps, neg=neg)


def _assert_oracle(res, world, neg):
    e, r, losses, spe = _oracle(world, res["steps"], neg)
    assert res["steps"] <= spe and res["clean"]
    np.testing.assert_allclose(res["loss"], sum(losses), rtol=2e-6)
    np.testing.assert_allclose(res["full"], e, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(res["rel"], r, rtol=2e-4, atol=2e-6)


def _assert_same_bits(a, b):
    assert a["full"].dtype == b["full"].dtype == np.float32 and a["rel"].dtype == np.float32
    assert np.array_equal(a["full"], b["full"])
    assert np.array_equal(a["rel"], b["rel"])
    assert a["ring"].shape == b["ring"].shape and np.array_equal(a["ring"], b["ring"])     # every step's loss partials
    assert a["loss"] == b["loss"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("neg", [8, 0, 25])   # 0: positives only (every positive needs HR)
def test_two_ranks_equal_dense_oracle(neg):
    """World 2, 7 steps: owner = id & 1 (the shift / mask instantiation), each rank's score launch mirrors all 600 positives'
    vectors and sums two writer slices per owned slot."""
    res = ranks.run_ranks(2, _worker, ((PEER,), dict(steps=7, neg=neg)), **RUN)[0][PEER]
    _assert_oracle(res, 2, neg)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,cfg", [
    ("wave", dict(steps=7)),                                               # default tuning at 2 ranks: k_oc_score
    ("quarter", dict(steps=7, tuning={"oc_score_quarter": 1})),            # k_oc_score_q
    ("wide", dict(steps=3, dim=256, neg=64, b=100)),                       # FPL 16, U = 1, four code chunks per quarter
    # long rows: 32-reference segments + k_oc_em_combine.  At 3,000 entities the hubs of both KGs (~55 references per global step
    # each; the next ones stay near 32) all have odd ids — rank 0 would own no long row; at 2,600 each rank owns one of the two
    ("zipf", dict(steps=7, zipf=1.0, n_ent=2600)),
])
def test_two_ranks_equal_collective_form_bit_for_bit(name, cfg):
    """The same inputs through the peer-direct and the collective (host-staged all-gather / reduce-scatter) entity-major forms:
    the mirror holds what the all-gather would have delivered, the summed block what the reduce-scatter would have (two writers:
    a + b either way), the second pass is the same launch — tables and every step's loss partials equal as raw floats."""
    out = ranks.run_ranks(2, _worker, ((PEER, COLL), cfg), **RUN)[0]
    _assert_same_bits(out[PEER], out[COLL])
    assert out[PEER]["clean"] and out[COLL]["clean"]
    if name == "zipf":
        assert out[COLL]["check"]["long_rows_per_global_step"] > 0 and out[PEER]["check"]["long_rows_per_global_step"] > 0
        assert min(out[COLL]["long_rows"]) > 0 and out[PEER]["long_rows"] == out[COLL]["long_rows"]     # on both ranks


@pytest.mark.timeout(300)
def test_two_ranks_across_an_epoch_boundary_equal_collective_form():
    """An epoch of at most 4 global steps, then two more: the shuffle, the prefetched plan and — forced here by dropping the
    capacity at the boundary — new exchange buffers with the peers' blocks mapped a second time (`_map_peers`)."""
    out = ranks.run_ranks(2, _worker, ((PEER, COLL), dict(steps=-2, n_ent=500, max_epoch=4, remap=True)), **RUN)[0]
    assert out[PEER]["remapped"] and out[PEER]["steps"] == out[PEER]["spe"] + 2 == out[COLL]["steps"]
    _assert_same_bits(out[PEER], out[COLL])


@pytest.mark.timeout(600)
def test_three_ranks_equal_dense_oracle_and_repeat_bit_for_bit():
    """World 3: owner = id % 3 by division, three writer slices per inbox summed as (s0 + s1) + s2 on every run — two runs in
    fresh process groups agree to the bit (with the collective form gloo's own summation order decides, so that form is not the
    yardstick here); the float64 oracle is."""
    runs = [ranks.run_ranks(3, _worker, ((PEER,), dict(steps=5)), **RUN)[0][PEER] for _ in range(2)]
    _assert_oracle(runs[0], 3, NEG)
    _assert_same_bits(runs[0], runs[1])
