"""mke_sim_select_keyed and mke_keyed_finish (include/multike_keyed.h) alone, bit for bit against tests/keyed_oracle.py.

The operands make every similarity exact (entries are small integers times 2^-3: any order of the sums gives the same float), so
the oracle's similarity matrix is the sweep's and thresholds can sit exactly on occurring values.  Widths: both launch-bound
classes of the sweep (kpad <= 80 and above) and both tile widths (64 columns up to kpad 208, 32 from 224).  Every case has a row
range that starts past 0 and is no multiple of 128, column counts that are no multiple of 64, ids up to 2^31 - 1, a seed >= 2^63,
duplicated rows (exact ties at the k-th value), and rows whose thresholds are planted to reach every status."""
import numpy as np
import pytest
import torch

import keyed_oracle as ko

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 123_456_789
MAXKEY = 2 ** 64 - 1

#        kpad n_cols n_seg seg_cap, do some rows overflow     (16 segments of 257 columns leave 11 (64-column tiles) or 7 (32-column
#        tiles) empty)
CASES = [(16, 257, 1, 257, False), (16, 1000, 16, 20, True), (80, 257, 3, 128, False), (80, 1000, 1, 1000, False),
         (96, 257, 16, 64, False), (96, 1000, 3, 90, True), (208, 257, 3, 44, True), (208, 1000, 16, 64, False),
         (224, 257, 16, 32, False), (224, 1000, 3, 352, False), (320, 257, 1, 100, True), (320, 1000, 16, 512, False)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _operands(kpad, n_cols, seed):
    """emb float32 [n_cols, kpad] (the last 3 columns zero: dim < kpad), ids, and the exact similarity matrix."""
    rng = np.random.default_rng(seed)
    emb = np.zeros((n_cols, kpad), dtype=np.float32)
    emb[:, :kpad - 3] = rng.integers(-3, 4, size=(n_cols, kpad - 3)).astype(np.float32) / 8.0
    dup = rng.choice(n_cols, size=n_cols // 10, replace=False)          # duplicated rows: columns with equal similarity to every row
    emb[dup] = emb[rng.choice(n_cols, size=len(dup))]
    ids = rng.choice(2 ** 31 - 1, size=n_cols, replace=False).astype(np.int32)
    ids[100 if n_cols < 400 else 400] = 2 ** 31 - 1                      # the largest id: a column of every row and a row of every range
    sim = (emb.astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32)      # |sum| < 2^24 * 2^-6: exact
    return emb, ids, sim


def _thresholds(sim, r_hi, r_lo):
    """per row the r_hi-th and r_lo-th largest values: thresholds that sit on occurring values; rows 0 .. 2 are planted"""
    srt = -np.sort(-sim, axis=1)
    tau_hi, tau_lo = srt[:, r_hi - 1].copy(), srt[:, r_lo - 1].copy()
    tau_hi[0] = tau_lo[0] = srt[0, -1]                                   # everything but the minimum is sure: the k-th is above tau_hi
    tau_lo[1] = tau_hi[1] = srt[1, 3]                                    # an empty band under three sure hits: the k-th is below tau_lo
    tau_lo[2] = -np.inf                                                  # no lower threshold: every column is stored or counted
    return tau_lo.astype(np.float32), tau_hi.astype(np.float32)


def _same_lists(cand, cnt, sure, want):
    idx, val, w_cnt, w_sure = want
    assert np.array_equal(cnt, w_cnt) and np.array_equal(sure, w_sure)
    used = np.arange(idx.shape[2])[None, None, :] < np.minimum(w_cnt, idx.shape[2])[:, :, None]
    assert np.array_equal(cand[..., 0][used], idx[used])
    assert np.array_equal(cand[..., 1][used], val.view(np.int32)[used])  # similarity BITS


def _gpu_finish(cand, cnt, sure, tau_hi, row_ids, ids, k, m, key_below):
    from multike_amd import _lib
    out = torch.full((cand.shape[0], m), -7, dtype=torch.int32, device="cuda")
    out, status = _lib.keyed_finish(cand, cnt, sure, _dev(tau_hi), _dev(row_ids), _dev(ids), k, m, SEED, key_below, out=out)
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("kpad,n_cols,n_seg,seg_cap,some_overflow", CASES)
def test_sweep_and_finish(kpad, n_cols, n_seg, seg_cap, some_overflow):
    from multike_amd import _lib
    from multike_amd.base.batch import keyed_key_below
    emb, ids, sim = _operands(kpad, n_cols, kpad * 7 + n_cols)
    row_lo, row_hi = (37, 187) if n_cols == 257 else (301, 560)         # 150 rows in 2 blocks, 259 rows in 3
    k, m, r_hi, r_lo = (60, 12, 40, 90) if n_cols == 257 else (200, 32, 150, 280)
    tau_lo, tau_hi = _thresholds(sim[row_lo:row_hi], r_hi, r_lo)
    key_below = keyed_key_below(m, k)
    want = ko.sweep(sim[row_lo:row_hi], row_lo, tau_lo, tau_hi, ids, SEED, key_below, n_seg, seg_cap, kpad)
    cand, cnt, sure = _lib.sim_select_keyed(_dev(emb), kpad, row_lo, row_hi, _dev(tau_lo), _dev(tau_hi), _dev(ids), SEED, key_below,
                                            n_seg, seg_cap)
    _same_lists(cand.cpu().numpy(), cnt.cpu().numpy(), sure.cpu().numpy(), want)
    if n_seg == 16 and n_cols == 257:
        assert not want[2][:, 9:].any() and want[2][:, :5].any()        # segments left empty
    w_out, w_status = ko.finish(*want, tau_hi, ids[row_lo:row_hi], ids, k, m, SEED, key_below)
    out, status = _gpu_finish(cand, cnt, sure, tau_hi, ids[row_lo:row_hi], ids, k, m, key_below)
    assert np.array_equal(status, w_status)
    assert np.array_equal(out[status == 0], w_out[status == 0]) and (out[status != 0] == -7).all()      # other rows are not written
    # what the case is there for: the planted rows, an overflow where seg_cap is small, and rows that went through
    overflow = (want[2] > seg_cap).any(1)
    assert status[0] == (2 if overflow[0] else 3) and status[1] == (2 if overflow[1] else 1) and np.array_equal(status == 2, overflow)
    assert overflow.any() == some_overflow and (status == 0).sum() >= len(status) // 2
    r = int(np.nonzero(status == 0)[0][-1])
    assert np.array_equal(out[r], ko.topk_thinned(sim[row_lo + r], ids[row_lo + r], ids, k, m, SEED))


def test_sweep_key_boundary_and_whole_range():
    """key_below exactly ON the key of a sure hit (not stored) and one above it (stored); rows [0, n) in one launch; the largest
    threshold 2^64 - 1 stores every sure hit."""
    from multike_amd import _lib
    kpad, n = 80, 257
    emb, ids, sim = _operands(kpad, n, 5)
    tau_lo, tau_hi = _thresholds(sim, 40, 90)
    tau_lo[:3], tau_hi[:3] = tau_lo[3], tau_hi[3]
    sure_cols = np.nonzero(sim[10] > tau_hi[10])[0]
    key = int(ko.keys(ids[10], ids[sure_cols[:1]], SEED)[0])
    for key_below in (key, key + 1, MAXKEY, 0):
        want = ko.sweep(sim, 0, tau_lo, tau_hi, ids, SEED, key_below, 3, 128, kpad)
        got = _lib.sim_select_keyed(_dev(emb), kpad, 0, n, _dev(tau_lo), _dev(tau_hi), _dev(ids), SEED, key_below, 3, 128)
        _same_lists(*(x.cpu().numpy() for x in got), want)
        stored = want[0][10][want[0][10] >= 0]
        assert (sure_cols[0] in stored) == (key_below > key)


def _hand_lists(rng, rows, n_seg, seg_cap, n_ids, fill):
    """lists of `fill(r, g)` entries per segment: columns ascending, values on a grid of 1/4 in [0, 8) (many ties)"""
    idx = np.zeros((rows, n_seg, seg_cap), dtype=np.int32)
    val = np.zeros((rows, n_seg, seg_cap), dtype=np.float32)
    cnt = np.zeros((rows, n_seg), dtype=np.int32)
    for r in range(rows):
        cols = np.sort(rng.choice(n_ids, size=sum(fill(r, g) for g in range(n_seg)), replace=False))
        at = 0
        for g in range(n_seg):
            c = fill(r, g)
            cnt[r, g] = c
            idx[r, g, :c] = cols[at:at + c]
            val[r, g, :c] = rng.integers(0, 32, size=c) / 4.0
            at += c
    return idx, val, cnt


def _check_finish(idx, val, cnt, sure, tau_hi, row_ids, ids, k, m, key_below):
    cand = np.stack([idx, val.view(np.int32)], axis=-1)
    w_out, w_status = ko.finish(idx, val, cnt, sure, tau_hi, row_ids, ids, k, m, SEED, key_below)
    out, status = _gpu_finish(_dev(cand), _dev(cnt), _dev(sure), tau_hi, row_ids, ids, k, m, key_below)
    assert np.array_equal(status, w_status), (status, w_status)
    assert np.array_equal(out[status == 0], w_out[status == 0]) and (out[status != 0] == -7).all()
    return status


def test_finish_on_hand_made_lists():
    """The finish kernel without the sweep: need == 0, need == |band|, need one beyond the band, a sure count that the stored
    entries do not show (the sweep drops most sure hits), an empty list, an empty segment, +0 / -0."""
    rng = np.random.default_rng(11)
    rows, n_seg, seg_cap, n_ids, k, m = 8, 3, 100, 5000, 150, 20
    ids = rng.choice(2 ** 31 - 1, size=n_ids, replace=False).astype(np.int32)
    row_ids = np.array([2 ** 31 - 1, 0, 5, 77, 1000, 31, 32, 33], dtype=np.int32)
    idx, val, cnt = _hand_lists(rng, rows, n_seg, seg_cap, n_ids, lambda r, g: 0 if (r == 6 or (r == 5 and g == 1)) else 60 + 13 * g)
    tau_hi = np.full(rows, 5.0, dtype=np.float32)
    lv = [np.concatenate([val[r, g, :cnt[r, g]] for g in range(n_seg)]) for r in range(rows)]
    band = np.array([np.count_nonzero(v <= 5.0) for v in lv])
    stored_sure = np.array([np.count_nonzero(v > 5.0) for v in lv])
    sure = np.zeros((rows, n_seg), dtype=np.int32)
    sure[0, 0] = k                                  # need == 0: the members are the stored sure entries alone
    sure[1, 1] = k - band[1]                        # need == |band|: the whole band
    sure[2, 2] = k - band[2] - 1                    # one more than the band holds: status 1
    sure[3] = (k - 40) // 3 + 1, (k - 40) // 3, (k - 40) // 3 - 1     # 40 of the band, the count spread over the segments
    sure[4, 0] = k + 1                              # status 3
    sure[5, 0] = k - 7                              # a list with an empty segment
    sure[6, 0] = k                                  # an empty list with need == 0: no member, status 4
    sure[7, 0] = stored_sure[7]                     # every sure entry stored
    assert (stored_sure[[0, 1, 3, 5, 7]] >= m).all() and k - stored_sure[7] <= band[7] and band[3] >= 40
    val[7, 0, :4] = (0.0, -0.0, 0.0, -0.0)          # one value: ties are taken in list order whatever the sign of the zero
    status = _check_finish(idx, val, cnt, sure, tau_hi, row_ids, ids, k, m, MAXKEY)
    assert status.tolist() == [0, 0, 1, 0, 3, 0, 4, 0]
    # a key threshold that cuts: about 30 % of the members qualify; and one that nothing passes
    _check_finish(idx, val, cnt, sure, tau_hi, row_ids, ids, k, m, int(0.3 * 2 ** 64))
    assert _check_finish(idx, val, cnt, sure, tau_hi, row_ids, ids, k, m, 0).tolist() == [4, 4, 1, 4, 3, 4, 4, 4]
    # overflow comes first
    cnt2 = cnt.copy()
    cnt2[4, 2] = seg_cap + 1
    cnt2[0, 0] = seg_cap + 50
    assert _check_finish(idx, val, cnt2, sure, tau_hi, row_ids, ids, k, m, MAXKEY).tolist() == [2, 0, 1, 0, 2, 0, 4, 0]


def test_finish_streams_lists_of_8192_slots():
    """n_seg * seg_cap = 8192, full: 32 chunks a pass, far past what a list kernel holds in LDS (4096)."""
    rng = np.random.default_rng(12)
    rows, n_seg, seg_cap, n_ids, k, m = 3, 8, 1024, 20_000, 9000, 700
    ids = rng.choice(2 ** 31 - 1, size=n_ids, replace=False).astype(np.int32)
    idx, val, cnt = _hand_lists(rng, rows, n_seg, seg_cap, n_ids, lambda r, g: seg_cap if r < 2 else 1000 - g)
    sure = np.full((rows, n_seg), 500, dtype=np.int32)                     # need = 5000 of a band of ~5,600
    tau_hi = np.full(rows, 5.5, dtype=np.float32)
    status = _check_finish(idx, val, cnt, sure, tau_hi, np.array([9, 8, 7], dtype=np.int32), ids, k, m, int(0.2 * 2 ** 64))
    assert status.tolist() == [0, 0, 0]
