"""The relation loop sampled straight into code words (`sampler_codes`): the sampler's code-word form (mke_neg_sample /
mke_neg_sample_at without neg_r / neg_t), the in-place bake (mke_neg_codes without id arrays), the ids rebuilt from the words
(sampling.ids_from_codes), the training kernel without id arrays, and the runner that strings them together.

Every comparison of ids, code words and bitmap rows is exact: the new forms are other routes to values the existing
ones define (mke_neg_sample's ids, mke_neg_codes' words and rows).  The score step without id arrays and the runner with the
knob on are held against the same step / run with the id arrays in the bands of test_runner_codes_gpu.py (losses rtol 2e-6;
tables, accumulators and gradients rtol 1e-4 / atol 1e-6): the two differ in the order of their atomic adds and in nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_neg_codes_gpu import addr, define, dev, sync
from test_runner_gpu import _setup

pytestmark = pytest.mark.gpu
OLD_TAG, TAG = 5, 9


def words_of(pos, neg, npp, pos_begin=0):
    """Section (1c)'s word of each negative without MKE_CODE_EXCL, from its three ids (numpy, int32)."""
    from multike_amd import _lib
    ph, pr, pt = pos
    nh, nr, nt = neg
    g = pos_begin + np.arange(len(nh)) // npp
    dh, dt = nh != ph[g], nt != pt[g]
    e = np.where(dh, nh, nt).astype(np.int64)
    w = e | np.where(dh, _lib.CODE_HEAD, 0) | np.where((nr == pr[g]) & (dh != dt), _lib.CODE_FAST, 0)
    return w.astype(np.int32)


class World:
    """Two KGs of n entities each ([0, n) and [n, 2n)), positives of both in one array with pos_kg, optionally a known set per KG
    (the positives are among the known triples) and a candidate table over part of the entities."""

    def __init__(self, n, npp, known, near, P=150, seed=0):
        from multike_amd.sampling import KGSide, KnownTripleSet
        rng = np.random.default_rng([n, npp, int(known), int(near), seed])
        self.n, self.npp, self.n_ent = n, npp, 2 * n
        kg = rng.integers(0, 2, P).astype(np.uint8)
        tri = np.stack([rng.integers(0, n, 4 * P), rng.integers(0, 4, 4 * P), rng.integers(0, n, 4 * P)], 1)
        self.sides = []
        for k in (0, 1):
            ks = None
            if known:
                t = (tri + np.array([k * n, 0, k * n])).astype(np.int32)
                ks = KnownTripleSet(dev(t[:, 0].copy()), dev(t[:, 1].copy()), dev(t[:, 2].copy()))
            side = KGSide(np.arange(k * n, (k + 1) * n), ks)
            if near:
                K = min(n, npp + 5)
                tab = np.zeros((2 * n, K), dtype=np.int32)
                tab[k * n:(k + 1) * n] = np.stack([k * n + rng.choice(n, K, replace=False) for _ in range(n)])
                side.set_neighbours(dev(tab), dev((np.arange(2 * n) % 3 != 0).astype(np.uint8)))
            self.sides.append(side)
        shift = kg.astype(np.int64) * n
        p = tri[:P] + np.stack([shift, np.zeros(P, np.int64), shift], 1)
        self.pos = [np.ascontiguousarray(p[:, c], dtype=np.int32) for c in range(3)]
        self.kg = kg
        self.d_pos, self.d_kg = tuple(dev(x) for x in self.pos), dev(kg)

    def ids(self, seed=(5, 6), stream_id=3, pos_offset=17, max_try=4):
        from multike_amd.sampling import sample_negatives
        out = sample_negatives(self.d_pos, self.sides[0], self.npp, seed=seed, stream_id=stream_id, pos_offset=pos_offset, max_try=max_try,
                               side1=self.sides[1], pos_kg=self.d_kg)
        sync()
        return [x.cpu().numpy() for x in out]

    def codes(self, seed=(5, 6), stream_id=3, pos_offset=17, max_try=4, pos_index=None):
        from multike_amd import _lib
        from multike_amd.sampling import side_array
        n = len(self.pos[0]) * self.npp
        buf = dev(np.full(n + 32, -77, dtype=np.int32))
        _lib.neg_sample_codes(self.d_pos, pos_offset, pos_index, self.d_kg, side_array(*self.sides), self.npp, max_try, seed, stream_id,
                              buf[16:16 + n])
        sync()
        out = buf.cpu().numpy()
        assert (out[:16] == -77).all() and (out[16 + n:] == -77).all(), "words outside the output range"
        return out[16:16 + n]


@pytest.mark.parametrize("n", (40, 300))
@pytest.mark.parametrize("npp", (1, 3, 15, 16, 25, 33, 64))
def test_sampler_words_are_the_definition_of_its_ids(n, npp):
    """Every group shape of the kernel (16 / 32 / 64 lanes per positive), both KGs in one launch, with and without the known set
    and the candidate table: the words are (1c)'s of mke_neg_sample's ids for the same seed and offsets.  A side smaller than
    neg_per_pos is refused like mke_neg_sample refuses it."""
    from multike_amd import _lib
    if n < npp:
        w = World(n, npp, False, False)
        with pytest.raises(_lib.MultiKEHipError, match="smaller than neg_per_pos"):
            w.ids()
        with pytest.raises(_lib.MultiKEHipError, match="smaller than neg_per_pos"):
            w.codes()
        return
    for known in (False, True):
        for near in (False, True):
            w = World(n, npp, known, near)
            want = words_of(w.pos, w.ids(), npp)
            got = w.codes()
            assert np.array_equal(got, want), (known, near, np.argwhere(got != want)[:5].tolist())
            assert (want & _lib.CODE_HEAD).any() and not (want & _lib.CODE_EXCL).any()
    # the explicit-position form: mke_neg_sample_at's stream
    idx = np.random.default_rng(npp).permutation(5000)[:len(w.pos[0])].astype(np.int32)
    out = tuple(torch.empty(len(idx) * npp, dtype=torch.int32, device="cuda") for _ in range(3))
    from multike_amd.sampling import side_array
    _lib.neg_sample_at(w.d_pos, dev(idx), w.d_kg, side_array(*w.sides), npp, 4, (5, 6), 3, out)
    sync()
    assert np.array_equal(w.codes(pos_index=dev(idx)), words_of(w.pos, [x.cpu().numpy() for x in out], npp))


def degenerate_world():
    """A side of exactly neg_per_pos = 3 entities, max_try = 2, every positive a known triple: each group draws all three entities
    in round 0, where the positive's own id makes a known triple and is rejected; the last round keeps whatever it draws."""
    from multike_amd.sampling import KGSide, KnownTripleSet
    rng = np.random.default_rng(3)
    all36 = np.array([(h, r, t) for h in range(3) for r in range(4) for t in range(3)], dtype=np.int32)
    tri = all36[rng.permutation(36)[:20]]
    w = World.__new__(World)
    w.n, w.npp, w.n_ent = 3, 3, 3
    ks = KnownTripleSet(dev(tri[:, 0].copy()), dev(tri[:, 1].copy()), dev(tri[:, 2].copy()))
    w.sides = [KGSide(np.arange(3), ks)] * 2
    p = tri[rng.integers(0, 20, 200)]
    w.pos = [np.ascontiguousarray(p[:, c]) for c in range(3)]
    w.kg = np.zeros(200, np.uint8)
    w.d_pos, w.d_kg = tuple(dev(x) for x in w.pos), None
    return w


def test_the_positive_itself_is_a_word_without_flags():
    from multike_amd import _lib
    w = degenerate_world()
    ids = w.ids(max_try=2)
    got, want = w.codes(max_try=2), words_of(w.pos, ids, 3)
    assert np.array_equal(got, want)
    g = np.arange(600) // 3
    same = (ids[0] == w.pos[0][g]) & (ids[2] == w.pos[2][g])
    assert same.any() and not same.all()
    assert np.array_equal(got[same], w.pos[2][g][same])            # entity = the positive's tail, no HEAD, no FAST
    assert ((got[~same] & _lib.CODE_FAST) != 0).all()


# ------------------------------------------------------------------------------------------------------------ bake, decode
def _bake_both(w, ids, pre, off):
    """(codes, bitmap rows) of mke_neg_codes on the ids and of its in-place form on the pre-codes, steps `off` of w's positives."""
    from multike_amd import _lib
    n_steps, words = len(off) - 1, _lib.neg_code_row_words(w.n_ent)
    d_off = dev(np.asarray(off, dtype=np.int64))
    n = int(off[-1]) * w.npp
    outs = []
    for inplace in (False, True):
        bits = dev(np.full((n_steps + 1) * words, -1, dtype=np.int32))
        bits[n_steps * words:] = 0
        buf = dev(np.full(n + 32, -77, dtype=np.int32))
        if inplace:
            buf[16:16 + n] = dev(pre[:n])
            _lib.neg_codes_inplace(w.d_pos, d_off, 0, n_steps, 0, int(off[-1]), w.npp, w.n_ent, bits, buf[16:16 + n])
        else:
            _lib.neg_codes(w.d_pos, d_off, 0, n_steps, 0, int(off[-1]), [dev(x[:n]) for x in ids], w.npp, w.n_ent, bits, buf[16:16 + n])
        sync()
        out, rows = buf.cpu().numpy(), bits.cpu().numpy().view(np.uint32).reshape(n_steps + 1, words)
        assert (out[:16] == -77).all() and (out[16 + n:] == -77).all() and not rows[n_steps].any()
        outs.append((out[16:16 + n], rows[:n_steps]))
    return outs


@pytest.mark.parametrize("npp,P,off", [(25, 1037, (0, 700, 700, 1030, 1037)), (3, 150, (0, 61, 61, 140, 150)), (64, 300, (0, 257, 300))])
def test_inplace_bake_equals_the_bake_from_ids(npp, P, off):
    """Steps of unequal length, an empty one, a short last one.  A pass of the in-place form takes 16 x 1024 negatives: the first
    case has a step of 17,500 (two passes, the second partial) and steps far below one pass, the last one of 16,448 (64 past it)."""
    from multike_amd import _lib
    w = World(300, npp, True, False, P=P)
    ids, pre = w.ids(), w.codes()
    (c_ids, b_ids), (c_in, b_in) = _bake_both(w, ids, pre, off)
    assert np.array_equal(c_in, c_ids), np.argwhere(c_in != c_ids)[:5].tolist()
    assert np.array_equal(b_in, b_ids)
    n = off[-1] * npp
    want_c, want_b = define(w.pos, [x[:n] for x in ids], np.asarray(off), 0, len(off) - 1, npp, w.n_ent)
    assert np.array_equal(c_in, want_c) and np.array_equal(b_in, want_b)
    assert (c_in & _lib.CODE_EXCL).any() and not (c_in & _lib.CODE_EXCL).all()
    # a second bake of baked words changes nothing (MKE_CODE_EXCL is cleared before it is set)
    (_, _), (c_again, b_again) = _bake_both(w, ids, c_in, off)
    assert np.array_equal(c_again, c_in) and np.array_equal(b_again, b_in)


def test_inplace_bake_and_decode_of_the_degenerate_batch():
    from multike_amd.sampling import ids_from_codes
    w = degenerate_world()
    ids, pre = w.ids(max_try=2), w.codes(max_try=2)
    (c_ids, b_ids), (c_in, b_in) = _bake_both(w, ids, pre, (0, 90, 200))
    assert np.array_equal(c_in, c_ids) and np.array_equal(b_in, b_ids)
    out = tuple(torch.full((600,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    ids_from_codes(w.d_pos, 0, dev(c_in), 600, 3, out)
    sync()
    for got, want in zip(out, ids):
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("npp", (1, 25, 64))
def test_decode_gives_the_samplers_ids(npp):
    """From the pre-codes and from a later chunk of the same epoch (pos_begin > 0), with poison around the outputs."""
    from multike_amd.sampling import ids_from_codes
    w = World(300, npp, True, True)
    ids, pre = w.ids(), w.codes()
    for pos_begin in (0, 37):
        n = (len(w.pos[0]) - pos_begin) * npp
        out = tuple(torch.full((n + 32,), -77, dtype=torch.int32, device="cuda") for _ in range(3))
        ids_from_codes(w.d_pos, pos_begin, dev(pre[pos_begin * npp:]), n, npp, tuple(x[16:16 + n] for x in out))
        sync()
        for got, want in zip(out, ids):
            got = got.cpu().numpy()
            assert np.array_equal(got[16:16 + n], want[pos_begin * npp:])
            assert (got[:16] == -77).all() and (got[16 + n:] == -77).all()


# ------------------------------------------------------------------------------------------------------------ score step
def _score_batch(stride):
    """One step whose negatives include the positive itself: one round only (max_try = 1 keeps every draw), 25 draws from 1000
    entities per positive, so about one positive in 40 draws its own id."""
    from multike_amd import _lib
    from multike_amd.sampling import KGSide, side_array
    rng = np.random.default_rng(stride)
    n_ent, n_rel, P, npp, dim = 1000, 40, 400, 25, stride - 5
    pos = [rng.integers(0, n_ent, P).astype(np.int32), rng.integers(0, n_rel, P).astype(np.int32), rng.integers(0, n_ent, P).astype(np.int32)]
    d_pos = tuple(dev(x) for x in pos)
    side = KGSide(np.arange(n_ent), None)
    ids = tuple(torch.empty(P * npp, dtype=torch.int32, device="cuda") for _ in range(3))
    code = torch.empty(P * npp, dtype=torch.int32, device="cuda")
    sides = side_array(side)
    _lib.neg_sample(d_pos, 0, None, sides, npp, 1, (1, 2), 0, ids)
    _lib.neg_sample_codes(d_pos, 0, None, None, sides, npp, 1, (1, 2), 0, code)
    bits = torch.zeros(_lib.neg_code_row_words(n_ent), dtype=torch.int32, device="cuda")
    _lib.neg_codes_inplace(d_pos, dev(np.array([0, P], dtype=np.int64)), 0, 1, 0, P, npp, n_ent, bits, code)
    sync()
    c = code.cpu().numpy()
    assert ((c & _lib.CODE_FAST) == 0).sum() >= 2, "the batch must hold degenerate negatives"
    ent = np.zeros((n_ent, stride), dtype=np.float32)
    rel = np.zeros((n_rel, stride), dtype=np.float32)
    ent[:, :dim], rel[:, :dim] = rng.normal(0, 0.3, (n_ent, dim)), rng.normal(0, 0.3, (n_rel, dim))
    return dict(n_ent=n_ent, n_rel=n_rel, P=P, npp=npp, dim=dim, stride=stride, pos=d_pos, ids=ids, code=code, ent=ent, rel=rel)


def _score(b, with_ids, tune_kw=None):
    """One training step on fresh operands -> (return code, the buffers the step may write)."""
    from multike_amd import _lib
    st = b["stride"]
    d = dict(ent=dev(b["ent"]), rel=dev(b["rel"]), acc=dev(np.full_like(b["ent"], 0.1)),
             grad_ent=dev(np.zeros_like(b["ent"])), grad_rel=dev(np.zeros((2,) + b["rel"].shape, dtype=np.float32)),
             touched_ent=dev(np.full(b["n_ent"], OLD_TAG, np.int32)), touched_rel=dev(np.full(b["n_rel"], OLD_TAG, np.int32)),
             partials=dev(np.full(_lib.LOSS_PARTIALS, np.nan)))
    nh, nr, nt = (addr(x) for x in b["ids"]) if with_ids else (None, None, None)
    a = _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=b["n_ent"], ent_normalize=1, rel_table=addr(d["rel"]), n_rel=b["n_rel"],
                       rel_normalize=1, stride=st, dim=b["dim"], pos_h=addr(b["pos"][0]), pos_r=addr(b["pos"][1]), pos_t=addr(b["pos"][2]),
                       n_pos=b["P"], neg_h=nh, neg_r=nr, neg_t=nt, n_neg=b["P"] * b["npp"], neg_per_pos=b["npp"], scale=1.0,
                       grad_ent=addr(d["grad_ent"]), grad_rel=addr(d["grad_rel"]), grad_rel_copies=2, touched_ent=addr(d["touched_ent"]),
                       touched_rel=addr(d["touched_rel"]), tag=TAG, ent_acc=addr(d["acc"]), optimizer=_lib.OPT_ADAGRAD, lr=0.01,
                       loss_partials=addr(d["partials"]), neg_code=addr(b["code"]))
    tune = _lib.tuning(**(tune_kw or {}))
    a.tuning = C.addressof(tune)
    rc = _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream())
    sync()
    return rc, {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("stride", (16, 80))
def test_score_step_without_id_arrays(stride):
    b = _score_batch(stride)
    rc_ids, with_ids = _score(b, True)
    rc_no, no_ids = _score(b, False)
    assert rc_ids == 0 and rc_no == 0
    la, lb = with_ids["partials"].sum(), no_ids["partials"].sum()
    print(f"loss with ids {la!r} without {lb!r}")
    np.testing.assert_allclose(lb, la, rtol=2e-6)
    for k in ("ent", "acc", "grad_ent", "grad_rel", "rel"):
        np.testing.assert_allclose(no_ids[k], with_ids[k], rtol=1e-4, atol=1e-6, err_msg=k)
    for k in ("touched_ent", "touched_rel"):
        assert np.array_equal(no_ids[k], with_ids[k]), k
    assert (with_ids["ent"] != b["ent"]).any() and (with_ids["touched_ent"] == TAG).any()
    # where the code-word form is not legal (64-bit offsets asked for) the step without ids is refused and nothing is launched
    rc, out = _score(b, False, dict(score_offsets32=0))
    assert rc == -3, rc
    assert np.array_equal(out["ent"], b["ent"]) and np.array_equal(out["rel"], b["rel"]) and (out["acc"] == np.float32(0.1)).all()
    assert not out["grad_ent"].any() and not out["grad_rel"].any() and np.isnan(out["partials"]).all()
    assert (out["touched_ent"] == OLD_TAG).all() and (out["touched_rel"] == OLD_TAG).all()


# ------------------------------------------------------------------------------------------------------------ runner
def _tables(E, R):
    return E.raw().cpu().numpy(), R.raw().cpu().numpy()


def _agree(a, b):
    np.testing.assert_allclose(a[0], b[0], rtol=2e-6)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-6)


@pytest.fixture(scope="module")
def fresh():
    return _setup(seed=11)[3]


def _runner(fresh, knob, **kw):
    from multike_amd.runner import RelationViewRunner
    E, R, bat = fresh()
    return RelationViewRunner(E, R, bat, lr=0.01, tuning={"sampler_codes": knob}, **kw), E, R, bat


def test_two_epochs_with_the_knob_on_and_off(fresh):
    runs = [_runner(fresh, knob) for knob in (1, 0)]
    losses = [[], []]
    for ep in range(2):
        snaps = []
        for k, (r, E, R, bat) in enumerate(runs):
            if ep:
                bat.shuffle()
            r.run()
            assert r.ids_stale == (k == 0)
            losses[k].append(r.step_losses().cpu().numpy())
            snaps.append(([x.cpu().numpy() for x in r.neg], r.neg_code.cpu().numpy()))
            assert not r.ids_stale
        for a, b in zip(snaps[0][0], snaps[1][0]):
            assert np.array_equal(a, b), f"ids after epoch {ep}"
        assert np.array_equal(snaps[0][1], snaps[1][1]), f"code words after epoch {ep}"
    outs = [(np.concatenate(losses[k]),) + _tables(runs[k][1], runs[k][2]) for k in (0, 1)]
    _agree(outs[0], outs[1])
    assert all(int(r.refcount.abs().sum()) == 0 for r, _, _, _ in runs)


@pytest.mark.parametrize("k", (1, 5))
def test_split_run_equals_one_run(fresh, k):
    outs = []
    for split in (False, True):
        r, E, R, bat = _runner(fresh, 1)
        if split:
            r.run(0, k); r.run(k, None)
        else:
            r.run()
        outs.append((r.step_losses().cpu().numpy(),) + _tables(E, R))
    _agree(outs[1], outs[0])


def test_stale_flag_chunks_and_the_shuffle(fresh):
    """sample_chunk = 4: the buffers describe the LAST chunk of the run; reading `neg` decodes it once; after a shuffle the
    positives it would be decoded from are gone."""
    from multike_amd import _lib
    on, off = _runner(fresh, 1, sample_chunk=4), _runner(fresh, 0, sample_chunk=4)
    for r, _, _, _ in (on, off):
        r.run()
    r, _, _, bat = on
    assert r.ids_stale and r.plan.ids_stale and not off[0].ids_stale
    s0 = (bat.steps - 1) // 4 * 4
    n = int(bat.off[bat.steps] - bat.off[s0]) * bat.neg_per_pos
    for a, b in zip(r.neg, off[0].neg):
        assert torch.equal(a[:n], b[:n])
    assert not r.ids_stale
    assert torch.equal(r.neg_code[:n], off[0].neg_code[:n])
    _agree((r.step_losses().cpu().numpy(),) + _tables(on[1], on[2]), (off[0].step_losses().cpu().numpy(),) + _tables(off[1], off[2]))
    r.run(0, 3)                                   # one short chunk
    assert r.ids_stale
    bat.shuffle()
    with pytest.raises(_lib.MultiKEHipError, match="code words only"):
        r.neg
    r.run()                                       # the new epoch's own chunk can be read again
    assert r.neg[0].numel() > 0 and not r.ids_stale
