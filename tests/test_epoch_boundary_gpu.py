"""The epoch boundary of the relation loop: (1) the sampler's known-triple prefilter changes nothing in its output (against
the unfiltered path, which tests/test_sampler_gpu.py pins to the Python specification) and can never hide a known key;
(2) mke_epoch_positives equals the torch chain it replaced; (3) drawing the permutations one epoch ahead leaves every epoch
what it was."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Unfiltered:
    """A copy of a KnownTripleSet's table that the library never built: no prefilter, the sampler probes it directly."""

    def __init__(self, ks):
        from multike_amd import _lib
        self.keys = ks.keys.clone()
        _lib.tripleset_forget(self.keys)        # whatever an earlier table at this address left
        assert _lib.tripleset_filter_bytes(self.keys) == 0


def _known(triples):
    from multike_amd.sampling import KnownTripleSet
    t = torch.as_tensor(np.ascontiguousarray(triples, dtype=np.int32), device="cuda")
    return KnownTripleSet(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous())


def _sides(kgs, known, unfiltered):
    from multike_amd.sampling import KGSide
    return [KGSide(kgs.entities(k), _Unfiltered(known[k]) if unfiltered else known[k]) for k in (0, 1)]


def _assert_same_negatives(a, b, what):
    for x, y, name in zip(a, b, "hrt"):
        assert torch.equal(x, y), f"{what}: neg_{name} differs at {int((x != y).sum())} of {x.numel()} places"


@pytest.fixture(scope="module")
def c2():
    """The C2 epoch of bench.py: 919,908 positives of both KGs in step order, the KGs' known-triple sets."""
    from multike_amd import _lib
    from multike_amd.sampling import RelationBatcher
    from multike_amd.synthetic import SyntheticKGs
    kgs = SyntheticKGs(n_ent=200_000, n_rel=550, seed=1234)
    known = [_known(kgs.triples[k]) for k in (0, 1)]
    for ks in known:
        assert _lib.tripleset_filter_bytes(ks.keys) == ks.keys.numel()      # 8 bits per slot: 1 MB per KG here
    filt, plain = _sides(kgs, known, False), _sides(kgs, known, True)
    bat = RelationBatcher(kgs.triples[0], kgs.triples[1], filt[0], filt[1], 5000, 25, seed=1234)
    bat.shuffle()
    assert bat.pos_h.numel() == 919_908
    return kgs, known, filt, plain, bat


@pytest.mark.parametrize("N", [1, 10, 15, 25, 32, 64])
def test_filtered_sampler_equals_unfiltered_on_the_c2_epoch(c2, N):
    from multike_amd.sampling import sample_negatives
    kgs, known, filt, plain, bat = c2
    pos = (bat.pos_h, bat.pos_r, bat.pos_t)
    a = sample_negatives(pos, filt[0], N, seed=(1234, 0), stream_id=2, side1=filt[1], pos_kg=bat.pos_kg)
    b = sample_negatives(pos, plain[0], N, seed=(1234, 0), stream_id=2, side1=plain[1], pos_kg=bat.pos_kg)
    _assert_same_negatives(a, b, f"N={N}")
    # and the membership test did its work: with max_try = 10 a known triple would have to be drawn ten rounds in a row
    got = known[0].contains(a[0], a[1], a[2]) | known[1].contains(a[0], a[1], a[2])
    assert int(got.sum()) == 0


@pytest.mark.parametrize("max_try", [1, 2])
def test_filtered_sampler_equals_unfiltered_with_few_rounds(c2, max_try):
    from multike_amd.sampling import sample_negatives
    kgs, known, filt, plain, bat = c2
    pos = (bat.pos_h, bat.pos_r, bat.pos_t)
    a = sample_negatives(pos, filt[0], 25, seed=(7, 1), stream_id=4, max_try=max_try, side1=filt[1], pos_kg=bat.pos_kg)
    b = sample_negatives(pos, plain[0], 25, seed=(7, 1), stream_id=4, max_try=max_try, side1=plain[1], pos_kg=bat.pos_kg)
    _assert_same_negatives(a, b, f"max_try={max_try}")


def test_filtered_sampler_at_equals_unfiltered(c2):
    """mke_neg_sample_at (a rank's share of an epoch: explicit epoch positions) goes through the same launch."""
    from multike_amd import _lib
    from multike_amd.sampling import side_array
    kgs, known, filt, plain, bat = c2
    idx = torch.arange(3, bat.pos_h.numel(), 4, dtype=torch.int32, device="cuda")
    pos = tuple(x[idx.long()].contiguous() for x in (bat.pos_h, bat.pos_r, bat.pos_t))
    kg = bat.pos_kg[idx.long()].contiguous()
    outs = []
    for sides in (filt, plain):
        out = tuple(torch.empty(idx.numel() * 25, dtype=torch.int32, device="cuda") for _ in range(3))
        _lib.neg_sample_at(pos, idx, kg, side_array(sides[0], sides[1]), 25, 10, (1234, 0), 6, out)
        outs.append(out)
    _assert_same_negatives(outs[0], outs[1], "neg_sample_at")
    whole = tuple(torch.empty(bat.pos_h.numel() * 25, dtype=torch.int32, device="cuda") for _ in range(3))
    _lib.neg_sample((bat.pos_h, bat.pos_r, bat.pos_t), 0, bat.pos_kg, side_array(plain[0], plain[1]), 25, 10, (1234, 0), 6, whole)
    for x, w in zip(outs[0], whole):
        assert torch.equal(x, w.view(-1, 25)[idx.long()].reshape(-1))


def _dense_kg(n_ent=48, n_rel=3, share=0.8, seed=5):
    """Most (h, r, t) over a small entity range ARE triples: the filter answers "maybe" nearly always, the table says "known"
    for most candidates, and the later rounds do the work."""
    rng = np.random.default_rng(seed)
    h, r, t = np.meshgrid(np.arange(n_ent), np.arange(n_rel), np.arange(n_ent), indexing="ij")
    allt = np.stack([h.ravel(), r.ravel(), t.ravel()], 1).astype(np.int32)
    return allt[rng.random(len(allt)) < share]


@pytest.mark.parametrize("N,max_try,near", [(10, 10, False), (25, 10, True), (40, 3, False), (15, 2, True), (1, 10, False)])
def test_filtered_sampler_equals_unfiltered_on_a_dense_kg(N, max_try, near):
    from multike_amd import _lib
    from multike_amd.sampling import KGSide, sample_negatives
    tr = _dense_kg()
    ks = _known(tr)
    assert _lib.tripleset_filter_bytes(ks.keys) > 0
    sides = [KGSide(np.arange(48), ks), KGSide(np.arange(48), _Unfiltered(ks))]
    if near:                                  # truncated sampling: a neighbour list for two entities in three
        rng = np.random.default_rng(9)
        tbl = torch.as_tensor(np.stack([rng.choice(48, 44, replace=False) for _ in range(48)]).astype(np.int32), device="cuda")
        valid = torch.as_tensor((np.arange(48) % 3 != 0).astype(np.uint8), device="cuda")
        for s in sides:
            s.set_neighbours(tbl, valid)
    pos = tuple(torch.as_tensor(np.ascontiguousarray(tr[:, k]), device="cuda") for k in range(3))
    a = sample_negatives(pos, sides[0], N, seed=(3, 4), stream_id=1, max_try=max_try)
    b = sample_negatives(pos, sides[1], N, seed=(3, 4), stream_id=1, max_try=max_try)
    _assert_same_negatives(a, b, f"dense N={N} max_try={max_try} near={near}")
    if max_try == 10 and not near:            # the setting is what it claims: many first-round candidates were known
        one = sample_negatives(pos, sides[1], N, seed=(3, 4), stream_id=1, max_try=1)
        assert float(ks.contains(*one).float().mean()) > 0.5


def test_filtered_sampler_equals_unfiltered_with_a_candidate_table_at_scale():
    """A 20K-entity KG with neighbour lists (the truncated sampler's shape): cand_table rows for most entities."""
    from multike_amd.sampling import KGSide, sample_negatives
    from multike_amd.synthetic import SyntheticKGs
    kgs = SyntheticKGs(n_ent=20_000, n_rel=40, seed=3)
    known = [_known(kgs.triples[k]) for k in (0, 1)]
    filt, plain = _sides(kgs, known, False), _sides(kgs, known, True)
    rng = np.random.default_rng(2)
    lo, hi = kgs.ent_range[0]
    tbl = torch.as_tensor(rng.integers(lo, hi, (kgs.entities_num, 70)).astype(np.int32), device="cuda")
    valid = torch.as_tensor((rng.random(kgs.entities_num) < 0.8).astype(np.uint8), device="cuda")
    filt[0].set_neighbours(tbl, valid)
    plain[0].set_neighbours(tbl, valid)
    t = kgs.triples[0]
    pos = tuple(torch.as_tensor(np.ascontiguousarray(t[:, k], dtype=np.int32), device="cuda") for k in range(3))
    for N in (25, 64):
        a = sample_negatives(pos, filt[0], N, seed=(11, 0), stream_id=0)
        b = sample_negatives(pos, plain[0], N, seed=(11, 0), stream_id=0)
        _assert_same_negatives(a, b, f"cand_table N={N}")


# ---------------------------------------------------------------------------------------------------------------------
# a stale filter can never say "not known" for a key of the set
# ---------------------------------------------------------------------------------------------------------------------
def _assert_filter_hides_nothing(ks_like, truth_triples, pos, n_ent, N=25):
    """Two rounds over a dense KG: whatever round one keeps has passed the membership test.  The set under test (with whatever
    filter the library holds for it) must give what an unfiltered table of the keys it is supposed to hold gives; a filter
    that lacked one of them would let a known triple through in round one."""
    from multike_amd.sampling import KGSide, sample_negatives
    a = sample_negatives(pos, KGSide(np.arange(n_ent), ks_like), N, seed=(5, 5), stream_id=3, max_try=2)
    b = sample_negatives(pos, KGSide(np.arange(n_ent), _Unfiltered(_known(truth_triples))), N, seed=(5, 5), stream_id=3, max_try=2)
    _assert_same_negatives(a, b, "stale filter")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")


class _Table:
    """A raw key table of a given capacity, filled through the C entry points only (what a C caller holds)."""

    def __init__(self, capacity):
        self.keys = torch.full((capacity,), -1, dtype=torch.int64, device="cuda")

    def build(self, tr):
        from multike_amd import _lib
        _lib.tripleset_build(_dev(tr[:, 0]), _dev(tr[:, 1]), _dev(tr[:, 2]), self.keys)


def test_keys_added_after_sampling_started_are_in_the_filter():
    from multike_amd import _lib
    tr = _dense_kg(share=0.6, seed=1)
    half = len(tr) // 2
    pos = tuple(_dev(tr[:, k]) for k in range(3))
    tb = _Table(16384)
    _lib.tripleset_forget(tb.keys)
    tb.build(tr[:half])
    assert _lib.tripleset_filter_bytes(tb.keys) > 0
    _assert_filter_hides_nothing(tb, tr[:half], pos, 48)      # sampling has started
    tb.build(tr[half:])                                       # the second mke_tripleset_build call
    _assert_filter_hides_nothing(tb, tr, pos, 48)


def test_a_set_that_never_had_a_filter_and_gets_one_late():
    from multike_amd import _lib
    tr = _dense_kg(share=0.6, seed=2)
    half = len(tr) // 2
    pos = tuple(_dev(tr[:, k]) for k in range(3))
    tb = _Table(16384)
    _lib.tripleset_forget(tb.keys)
    tb.build(tr[:half])
    copy = _Unfiltered(tb)                                    # a table the library never built: probed directly
    _assert_filter_hides_nothing(copy, tr[:half], pos, 48)
    assert _lib.tripleset_filter_bytes(copy.keys) == 0
    _lib.tripleset_build(_dev(tr[half:, 0]), _dev(tr[half:, 1]), _dev(tr[half:, 2]), copy.keys)
    assert _lib.tripleset_filter_bytes(copy.keys) > 0         # created now, from the first half already there + the second
    _assert_filter_hides_nothing(copy, tr, pos, 48)


def test_a_new_set_at_the_address_of_a_freed_one():
    from multike_amd import _lib
    a_tr, b_tr = _dense_kg(share=0.5, seed=3), _dense_kg(share=0.5, seed=4)
    pos_a, pos_b = (tuple(_dev(t[:, k]) for k in range(3)) for t in (a_tr, b_tr))
    tb = _Table(16384)
    _lib.tripleset_forget(tb.keys)
    tb.build(a_tr)
    _assert_filter_hides_nothing(tb, a_tr, pos_a, 48)
    # freed with mke_tripleset_forget (what KnownTripleSet does), a new table at the same address
    _lib.tripleset_forget(tb.keys)
    tb.keys.fill_(-1)
    assert _lib.tripleset_filter_bytes(tb.keys) == 0
    tb.build(b_tr)
    _assert_filter_hides_nothing(tb, b_tr, pos_b, 48)
    # freed WITHOUT it (a C caller that forgot), same capacity: the old filter's bits stay, the new keys are added
    tb.keys.fill_(-1)
    tb.build(a_tr)
    _assert_filter_hides_nothing(tb, a_tr, pos_a, 48)
    # ... and with another capacity at the same address: the old filter is dropped, not reused
    tb.keys.fill_(-1)
    small = _Table.__new__(_Table)
    small.keys = tb.keys[:8192]
    small.build(b_tr)
    assert _lib.tripleset_filter_bytes(small.keys) > 0 and _lib.tripleset_filter_bytes(tb.keys) == 0
    _assert_filter_hides_nothing(small, b_tr, pos_b, 48)
    _lib.tripleset_forget(tb.keys)


def test_known_triple_set_objects_release_their_filter():
    """The Python owner: a KnownTripleSet's filter goes when the object goes, so the allocator may hand its block to anything."""
    from multike_amd import _lib
    ks = _known(_dense_kg(seed=6))
    assert _lib.tripleset_filter_bytes(ks.keys) > 0
    keys = ks.keys                                            # keeps the block (and so the address) out of the allocator
    del ks
    gc.collect()
    assert _lib.tripleset_filter_bytes(keys) == 0


# ---------------------------------------------------------------------------------------------------------------------
# mke_epoch_positives == the torch chain it replaced
# ---------------------------------------------------------------------------------------------------------------------
def _random_triples(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 20, (n, 3)).astype(np.int32)


RAGGED = [(1000, 777, 100),      # n1 + n2 not a multiple of the batch
          (1000, 50, 100),       # KG 2 used up one step before the end, KG 1 short in the last
          (300, 900, 64),
          (500, 0, 64),          # an empty KG 2
          (3, 1000, 50),         # KG 1's share of a step rounds to zero: never batched
          (5000, 4900, 5000)]    # one full step and a short one


@pytest.mark.parametrize("n1,n2,B", RAGGED)
def test_epoch_positives_equals_the_torch_chain(n1, n2, B):
    from multike_amd import _lib
    from multike_amd.sampling import KGSide, RelationBatcher
    tr1, tr2 = _random_triples(n1, 1), _random_triples(n2, 2)
    side = KGSide(np.arange(8), None, device="cpu")
    layout = RelationBatcher(tr1, tr2, side, side, B, 1, device="cpu")      # the torch chain's own gather map
    src = layout._src.cuda()
    t1, t2 = torch.as_tensor(tr1, device="cuda"), torch.as_tensor(tr2, device="cuda")
    n_pos = int(layout.off[-1])
    pos = tuple(torch.full((n_pos,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    _lib.epoch_positives(t1, t2, None, None, layout.b1, layout.b2, layout.steps, None, None, pos)      # first epoch: identity
    allt = torch.cat([t1, t2], 0)[src]
    for k in range(3):
        assert torch.equal(pos[k], allt[:, k])
    g = torch.Generator(device="cuda")
    g.manual_seed(n1 + n2)
    for epoch in range(3):                                                  # three shuffles in a row: permutations compose
        p1, p2 = torch.randperm(n1, generator=g, device="cuda"), torch.randperm(n2, generator=g, device="cuda")
        o1, o2 = torch.full_like(t1, -9), torch.full_like(t2, -9)
        _lib.epoch_positives(t1, t2, p1, p2, layout.b1, layout.b2, layout.steps, o1, o2, pos)
        e1, e2 = t1[p1], t2[p2]
        allt = torch.cat([e1, e2], 0)[src]
        assert torch.equal(o1, e1) and torch.equal(o2, e2), epoch
        for k in range(3):
            assert torch.equal(pos[k], allt[:, k]), (epoch, k)
        t1, t2 = o1, o2


class _ChainBatcher:
    """RelationBatcher's epoch boundary as it was before mke_epoch_positives: randperm (KG 1, then KG 2), gather, cat, gather."""

    def __init__(self, tr1, tr2, src, seed):
        self.t1, self.t2, self.src = torch.as_tensor(tr1, device="cuda"), torch.as_tensor(tr2, device="cuda"), src
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(seed)

    def shuffle(self):
        p1 = torch.randperm(self.t1.shape[0], generator=self.gen, device="cuda")
        p2 = torch.randperm(self.t2.shape[0], generator=self.gen, device="cuda")
        self.t1, self.t2 = self.t1[p1], self.t2[p2]

    def positives(self):
        allt = torch.cat([self.t1, self.t2], 0)[self.src]
        return tuple(allt[:, k].contiguous() for k in range(3))


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("n1,n2,B", [(1000, 777, 100), (1000, 50, 100), (500, 0, 64), (40_000, 39_000, 5000)])
def test_batcher_epochs_equal_the_torch_chain(n1, n2, B, prefetch):
    """shuffle(), and stage_next_epoch() + commit_staged(), over five epochs: the same permutations in the same order from the
    batcher's generator, with the pair drawn in line or one epoch ahead on the side stream."""
    from multike_amd.sampling import KGSide, RelationBatcher
    tr1, tr2 = _random_triples(n1, 3), _random_triples(n2, 4)
    side = KGSide(np.arange(8), None, device="cpu")
    src = RelationBatcher(tr1, tr2, side, side, B, 1, device="cpu")._src.cuda()
    spec = _ChainBatcher(tr1, tr2, src, seed=77)
    bat = RelationBatcher(tr1, tr2, side, side, B, 1, seed=77, prefetch_perms=prefetch)
    addr = [x.data_ptr() for x in (bat.pos_h, bat.pos_r, bat.pos_t)]
    for epoch in range(5):
        if epoch in (1, 2, 4):
            bat.shuffle()
            spec.shuffle()
        elif epoch == 3:
            staged = bat.stage_next_epoch()
            before = spec.positives()
            for a, b in zip((bat.pos_h, bat.pos_r, bat.pos_t), before):
                assert torch.equal(a, b)                                    # staging leaves the current epoch alone
            spec.shuffle()
            for a, b in zip(staged, spec.positives()):
                assert torch.equal(a, b)
            bat.commit_staged()
        assert bat.epoch == epoch
        for a, b in zip((bat.pos_h, bat.pos_r, bat.pos_t), spec.positives()):
            assert torch.equal(a, b), epoch
        assert torch.equal(bat.t1, spec.t1) and torch.equal(bat.t2, spec.t2)
        if epoch < 3:
            assert [x.data_ptr() for x in (bat.pos_h, bat.pos_r, bat.pos_t)] == addr     # persistent epoch buffers


def test_run_epochs_equals_shuffle_and_run_with_the_permutations_drawn_ahead():
    """Four epochs through run_epochs(4) on a batcher that draws its permutations one epoch ahead, and through four
    shuffle() + run() rounds on one that draws them in line: positives and negatives exactly, losses and tables within the
    band of test_run_epochs_prefetch_equals_plain_epochs (the step's floating-point atomics)."""
    from test_runner_gpu import _setup
    from multike_amd.runner import RelationViewRunner
    from multike_amd.sampling import RelationBatcher
    kgs, ent, rel, fresh = _setup(seed=8)
    E1, R1, b1 = fresh()
    E2, R2, b2 = fresh()
    bat1 = RelationBatcher(kgs.triples[0], kgs.triples[1], b1.side1, b1.side2, b1.batch_size, b1.neg_per_pos, seed=42, prefetch_perms=True)
    bat2 = RelationBatcher(kgs.triples[0], kgs.triples[1], b2.side1, b2.side2, b2.batch_size, b2.neg_per_pos, seed=42, prefetch_perms=False)
    r1 = RelationViewRunner(E1, R1, bat1, lr=0.01)
    r2 = RelationViewRunner(E2, R2, bat2, lr=0.01)
    seen = []

    def keep(e, r):
        seen.append((r.step_losses().cpu().numpy().copy(), [x.clone() for x in (r.bat.pos_h, r.bat.pos_r, r.bat.pos_t)],
                     [x.clone() for x in r.neg]))
    r1.run_epochs(4, on_epoch_end=keep)
    assert len(seen) == 4
    for e in range(4):
        if e > 0:
            bat2.shuffle()
        r2.run()
        loss, pos, neg = seen[e]
        for a, b in zip(pos, (bat2.pos_h, bat2.pos_r, bat2.pos_t)):
            assert torch.equal(a, b), e
        for a, b in zip(neg, r2.neg):
            assert torch.equal(a, b), e
        np.testing.assert_allclose(loss, r2.step_losses().cpu().numpy(), rtol=2e-6)
    assert bat1.epoch == bat2.epoch == 3
    np.testing.assert_allclose(E1.raw().cpu().numpy(), E2.raw().cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(R1.raw().cpu().numpy(), R2.raw().cpu().numpy(), rtol=1e-4, atol=1e-6)
