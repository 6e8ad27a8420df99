"""mke_relation_steps with code words (`neg_codes`, the default) against the same runner with reference counts per step:
two epochs with the knob on and off, a split run, the fallback when the bitmap's budget is zero.  Tolerances are those of
test_runner_gpu.py for native against per-step (losses rtol 2e-6, tables rtol 1e-4 / atol 1e-6)."""
import numpy as np
import pytest
import torch

from test_runner_gpu import _setup

pytestmark = pytest.mark.gpu


def _tables(E, R):
    return E.raw().cpu().numpy(), R.raw().cpu().numpy()


def _agree(a, b):
    np.testing.assert_allclose(a[0], b[0], rtol=2e-6)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-6)


def _two_epochs(fresh, knob, **kw):
    """(losses of both epochs, entity table, relation table, the runner) after two epochs with `neg_codes` = knob."""
    from multike_amd.runner import RelationViewRunner
    E, R, bat = fresh()
    r = RelationViewRunner(E, R, bat, lr=0.01, tuning={"neg_codes": knob}, **kw)
    losses = []
    for ep in range(2):
        if ep:
            bat.shuffle()
        r.run()
        losses.append(r.step_losses().cpu().numpy())
    return (np.concatenate(losses),) + _tables(E, R), r, bat


@pytest.fixture(scope="module")
def world():
    kgs, ent, rel, fresh = _setup(seed=11)
    off_out, r_off, _ = _two_epochs(fresh, 0)
    return fresh, off_out, r_off


def test_codes_on_equals_codes_off_over_two_epochs(world):
    from multike_amd import _lib
    fresh, off_out, r_off = world
    on_out, r_on, bat = _two_epochs(fresh, 1)
    assert r_on.neg_code is not None and r_on.plan.code_bits_words == r_on.steps * _lib.neg_code_row_words(r_on.ent.n_rows)
    _agree(on_out, off_out)
    assert int(r_on.refcount.abs().sum()) == 0 and int(r_off.refcount.abs().sum()) == 0
    # the negatives the loop left are the per-step sampler's, bit for bit, and the codes are the definition's of them
    N = bat.neg_per_pos
    for s in (0, bat.steps // 2, bat.steps - 1):
        lo, hi = int(bat.off[s]), int(bat.off[s + 1])
        _, neg = bat.batch(s)
        for got, want in zip(r_on.neg, neg):
            assert torch.equal(got[lo * N:hi * N], want), f"negatives of step {s}"
    ph, pt, pr = bat.pos_h.cpu().numpy(), bat.pos_t.cpu().numpy(), bat.pos_r.cpu().numpy()
    nh, nr, nt = (x.cpu().numpy() for x in r_on.neg)
    code = r_on.neg_code.cpu().numpy()
    s = bat.steps - 1                                   # the short last step
    lo, hi = int(bat.off[s]), int(bat.off[s + 1])
    g = lo + np.arange((hi - lo) * N) // N
    a, b = nh[lo * N:hi * N], nt[lo * N:hi * N]
    cnt = np.zeros(r_on.ent.n_rows, dtype=np.int64)
    for ids in (ph[lo:hi], pt[lo:hi], a[a != ph[g]], b[b != pt[g]]):
        np.add.at(cnt, ids, 1)
    dh, dt = a != ph[g], b != pt[g]
    e = np.where(dh, a, b)
    want = e | np.where(dh, _lib.CODE_HEAD, 0) | np.where((nr[lo * N:hi * N] == pr[g]) & (dh != dt), _lib.CODE_FAST, 0) | \
        np.where(cnt[e] == 1, _lib.CODE_EXCL, 0)
    assert np.array_equal(code[lo * N:hi * N], want)
    assert (want & _lib.CODE_EXCL).any() and not (want & _lib.CODE_EXCL).all()


@pytest.mark.parametrize("k", (1, 5))
def test_split_run_equals_one_run(world, k):
    from multike_amd.runner import RelationViewRunner
    fresh = world[0]
    outs = []
    for split in (False, True):
        E, R, bat = fresh()
        r = RelationViewRunner(E, R, bat, lr=0.01)
        if split:
            r.run(0, k); r.run(k, None)
        else:
            r.run()
        outs.append((r.step_losses().cpu().numpy(),) + _tables(E, R))
        assert int(r.refcount.abs().sum()) == 0
    _agree(outs[1], outs[0])


def test_chunks_that_do_not_fit_keep_the_reference_counts(world):
    """Budget zero: no scratch, every chunk runs the reference-count form; a bitmap of one chunk of 4 steps: code words with
    sample_chunk = 4.  Both agree with the knob-off run."""
    from multike_amd import _lib
    fresh, off_out, _ = world
    zero_out, r0, _ = _two_epochs(fresh, 1, code_bits_budget=0)
    assert r0.neg_code is None and r0.plan.code_bits_words == 0 and not r0.plan.code_bits
    _agree(zero_out, off_out)
    assert int(r0.refcount.abs().sum()) == 0
    words = _lib.neg_code_row_words(r0.ent.n_rows)
    small_out, r4, _ = _two_epochs(fresh, 1, sample_chunk=4, code_bits_budget=4 * 4 * words)
    assert r4.plan.code_bits_words == 4 * words
    _agree(small_out, off_out)
    assert int(r4.refcount.abs().sum()) == 0
