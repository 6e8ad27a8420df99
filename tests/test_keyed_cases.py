"""The definition of mke_sim_select_keyed / mke_keyed_finish (include/multike_keyed.h) as tests/keyed_oracle.py restates it: that
its status-0 rows ARE the thinned exact top-k lists, its statuses and their precedence, its boundaries, the host helpers of
`neighbour_table(keyed=)`, and what needs no device of the library: its generated module, its symbols, its refusals."""
from fractions import Fraction

import numpy as np
import pytest

import keyed_oracle as ko

SEED = 2 ** 63 + 977
MAXKEY = 2 ** 64 - 1


def _ids(rng, n, hi=2 ** 31 - 1):
    ids = rng.choice(hi, size=n, replace=False).astype(np.int32)
    ids[0] = 2 ** 31 - 1
    return ids


def _kth(row, r):
    """the r-th largest value of a row (r from 1)"""
    return np.sort(row)[::-1][r - 1]


def _run(sim, tau_lo, tau_hi, ids, k, m, key_below, n_seg=3, seg_cap=4096, kpad=16, row_lo=0, seed=SEED):
    lists = ko.sweep(sim, row_lo, tau_lo, tau_hi, ids, seed, key_below, n_seg, seg_cap, kpad)
    rows = sim.shape[0]
    return lists, ko.finish(*lists, tau_hi, ids[row_lo:row_lo + rows], ids, k, m, seed, key_below)


@pytest.mark.parametrize("n_seg,grid", [(1, 0), (3, 64), (16, 8)])
def test_status_0_rows_are_the_thinned_exact_topk(n_seg, grid):
    """Random rows (grid > 0: values on a grid of 1/grid, so that the k-th value is tied in most rows), thresholds on occurring
    values around the k-th: every row that ends with status 0 is thin_oracle.thin of the exact top-k list in column order."""
    from multike_amd.base.batch import keyed_key_below
    rng = np.random.default_rng(n_seg)
    n, rows, k, m, row_lo = 700, 40, 150, 24, 5
    sim = rng.standard_normal((rows, n)).astype(np.float32)
    if grid:
        sim = (np.round(sim * grid) / grid).astype(np.float32)
    ids = _ids(rng, n)
    tau_hi = np.array([_kth(r, 120) for r in sim], dtype=np.float32)
    tau_lo = np.array([_kth(r, 190) for r in sim], dtype=np.float32)
    (idx, val, cnt, sure), (out, status) = _run(sim, tau_lo, tau_hi, ids, k, m, keyed_key_below(m, k), n_seg=n_seg, row_lo=row_lo)
    assert (status == 0).sum() >= rows * 3 // 4, status
    for r in np.nonzero(status == 0)[0]:
        assert np.array_equal(out[r], ko.topk_thinned(sim[r], ids[row_lo + r], ids, k, m, SEED)), r
    assert (out[status != 0] == -1).all()
    # the sure hits are all counted and only a share of them is stored
    kept = ((idx >= 0) & (val > tau_hi[:, None, None])).sum((1, 2))
    assert (sure.sum(1) >= 60).all() and (kept < sure.sum(1)).all() and (kept > 0).all()


def _planted():
    """Five rows over 300 columns with k = 100, m = 10: the thresholds decide the status."""
    rng = np.random.default_rng(7)
    n, k, m = 300, 100, 10
    sim = rng.permutation(n).astype(np.float32)[None].repeat(5, 0)          # distinct values 0 .. 299; top 100: >= 200
    for r in range(5):
        sim[r] = rng.permutation(sim[r])
    ids = _ids(rng, n)
    #                 ok      overflow  k-th above tau_hi  k-th at or below tau_lo  overflow AND above
    tau_hi = np.array([220.0, 220.0,    170.0,             260.0,                   170.0], dtype=np.float32)
    tau_lo = np.array([180.0, 20.0,     150.0,             200.0,                   0.0], dtype=np.float32)
    return sim, tau_lo, tau_hi, ids, k, m


def test_planted_rows_reach_every_status_with_the_precedence():
    sim, tau_lo, tau_hi, ids, k, m = _planted()
    # 3 segments of 128, 128 and 44 columns.  seg_cap 80: rows 1 and 4 store ~280 and 300 entries, the others 149 at most
    _, (out, status) = _run(sim, tau_lo, tau_hi, ids, k, m, MAXKEY, seg_cap=80)
    assert status.tolist() == [0, 2, 3, 1, 2]
    assert np.array_equal(out[0], ko.topk_thinned(sim[0], ids[0], ids, k, m, SEED)) and (out[1:] == -1).all()
    # row 3: s == tau_lo (the k-th value itself, 200) is out, so 99 of the 100 are found: need 61 > band 60
    # key_below 0: nothing has a key below it and no sure hit is stored — 4 for the row that was fine, and only for it
    _, (out, status) = _run(sim, tau_lo, tau_hi, ids, k, m, 0, seg_cap=60)
    assert status.tolist() == [4, 2, 3, 1, 2] and (out == -1).all()
    # status 4 at the margin: exactly m - 1, then exactly m members below key_below
    ky = np.sort(ko.keys(ids[0], ids[np.argsort(-sim[0], kind="stable")[:k]], SEED))
    _, (_, status) = _run(sim[:1], tau_lo[:1], tau_hi[:1], ids, k, m, int(ky[m - 1]))
    assert status.tolist() == [4]
    _, (out, status) = _run(sim[:1], tau_lo[:1], tau_hi[:1], ids, k, m, int(ky[m - 1]) + 1)
    assert status.tolist() == [0] and np.array_equal(out[0], ko.topk_thinned(sim[0], ids[0], ids, k, m, SEED))


def test_ties_at_the_kth_value_take_the_first_columns():
    rng = np.random.default_rng(3)
    n, k = 120, 15
    sim = np.zeros((1, n), dtype=np.float32)
    high = rng.choice(n, size=10, replace=False)
    sim[0, high] = 5.0
    tied = np.setdiff1d(rng.choice(n, size=40, replace=False), high)
    sim[0, tied] = 1.0
    ids = _ids(rng, n)
    members = np.sort(np.concatenate([high, np.sort(tied)[:5]]))              # the 5.0s and the first five 1.0s by column
    ky = ko.keys(ids[0], ids[members], SEED)
    for tau_lo, tau_hi in ((0.5, 1.0), (0.0, 5.0), (0.5, 3.0)):              # the tie in the band; everything in the band; 5.0s sure
        _, (out, status) = _run(sim, [tau_lo], [tau_hi], ids, k, k - 1, MAXKEY, n_seg=3)
        assert status.tolist() == [0]
        assert np.array_equal(out[0], ids[np.delete(members, np.argmax(ky))])


def test_boundaries_of_the_thresholds_and_of_the_key():
    rng = np.random.default_rng(4)
    n = 64
    sim = rng.permutation(n).astype(np.float32)[None]                         # values 0 .. 63
    ids = _ids(rng, n)
    col = lambda v: int(np.nonzero(sim[0] == v)[0][0])
    idx, val, cnt, sure = ko.sweep(sim, 0, [40.0], [50.0], ids, SEED, MAXKEY, 1, 64, 16)
    stored = idx[0, 0, :cnt[0, 0]].tolist()
    assert col(40.0) not in stored and col(41.0) in stored                    # s == tau_lo is out
    assert col(50.0) in stored and sure[0, 0] == 13                           # s == tau_hi is band: 51 .. 63 are sure
    assert cnt[0, 0] == 23
    key51 = int(ko.keys(ids[0], ids[[col(51.0)]], SEED)[0])
    idx, _, cnt, sure = ko.sweep(sim, 0, [40.0], [50.0], ids, SEED, key51, 1, 64, 16)
    assert col(51.0) not in idx[0, 0, :cnt[0, 0]].tolist() and sure[0, 0] == 13     # key == key_below is not stored, still counted
    idx, _, cnt, _ = ko.sweep(sim, 0, [40.0], [50.0], ids, SEED, key51 + 1, 1, 64, 16)
    assert col(51.0) in idx[0, 0, :cnt[0, 0]].tolist()
    assert col(50.0) in idx[0, 0, :cnt[0, 0]].tolist()                        # the band does not look at the key


def test_segments_are_whole_tiles_and_may_be_empty():
    assert ko.tile_columns(208) == 64 and ko.tile_columns(224) == 32
    seg = ko.segment_of(257, 16, 3)                                           # 5 tiles of 64: 2 + 2 + 1
    assert np.bincount(seg, minlength=3).tolist() == [128, 128, 1]
    seg = ko.segment_of(257, 16, 16)                                          # one tile a segment: 11 segments stay empty
    assert np.bincount(seg, minlength=16).tolist() == [64] * 4 + [1] + [0] * 11
    assert np.bincount(ko.segment_of(1000, 224, 3), minlength=3).tolist() == [352, 352, 296]


def test_key_below():
    from multike_amd.base.batch import keyed_key_below
    assert keyed_key_below(1, 100) == (13 << 64) // 100                       # 1 + 4 + 8
    assert keyed_key_below(16, 100) == (40 << 64) // 100
    assert keyed_key_below(2048, 20_000) == int(Fraction(2048 + 4.0 * 2048 ** 0.5 + 8.0) * 2 ** 64 // 20_000)
    assert abs(keyed_key_below(2048, 20_000) / 2 ** 64 - 0.11185) < 1e-5
    # where the margin reaches k every key is wanted: the largest threshold, not 2^64
    assert keyed_key_below(99, 100) == MAXKEY and keyed_key_below(61, 100) == MAXKEY and keyed_key_below(60, 100) < MAXKEY
    assert keyed_key_below(1, 13) == MAXKEY and keyed_key_below(1, 14) == (13 << 64) // 14
    assert keyed_key_below(1, 2) == MAXKEY


def test_sample_ranks():
    from multike_amd.base.batch import keyed_sample_ranks
    assert keyed_sample_ranks(1500, 6000, 2048, 3) == (444, 581)              # s = 512
    assert keyed_sample_ranks(20_000, 1_000_000, 65_536, 3) == (1202, 1421)   # s = 1310.72
    assert keyed_sample_ranks(1500, 6000, 2048, 0.25) == (506, 519)
    # tiny s: the upper rank is at least the 1st, the lower one may lie beyond the sample
    assert keyed_sample_ranks(2, 1000, 10, 3) == (1, 2)
    assert keyed_sample_ranks(4, 8, 1, 3) == (1, 4)
    assert keyed_sample_ranks(100, 100, 16, 3) == (4, 29)


def test_keyed_abi_module_is_what_the_generator_writes_and_the_library_exports(tmp_path):
    import os
    import subprocess
    import sys
    import abi_header as ah
    from multike_amd import _abi, _abi_keyed, _abi_thin, _lib
    header = os.path.join(os.path.dirname(ah.HEADER), "multike_keyed.h")
    out = tmp_path / "_abi_keyed.py"
    subprocess.check_call([sys.executable, ah.GENERATOR, header, str(out)])
    assert out.read_bytes() == open(os.path.join(os.path.dirname(ah.GENERATED), "_abi_keyed.py"), "rb").read()
    assert list(_abi_keyed.FUNCTIONS) == ["mke_keyed_last_error", "mke_sim_select_keyed", "mke_keyed_finish"]
    assert not set(_abi_keyed.FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi_thin.FUNCTIONS))
    assert "#include" not in open(header).read().replace("#include <stdint.h>", "")          # the header stands alone
    assert (_abi_keyed.KEYED_E_NULL, _abi_keyed.KEYED_E_SHAPE, _abi_keyed.KEYED_E_UNSUPPORTED, _abi_keyed.KEYED_E_RANGE) == \
        (_abi.E_NULL, _abi.E_SHAPE, _abi.E_UNSUPPORTED, _abi.E_RANGE)
    if not os.path.exists(_lib.KEYED_SO_PATH):
        import __graft_entry__ as g
        g.build()
    assert ah.exported_symbols(_lib.KEYED_SO_PATH) == set(_abi_keyed.FUNCTIONS)
    L = _lib.keyed_lib()
    for name, (restype, argtypes) in _abi_keyed.FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def test_argument_errors_come_before_any_launch():
    """No device is needed: every refusal is made before a kernel is enqueued (the pointers below are never read)."""
    import ctypes as C
    from multike_amd import _abi_keyed as ak, _lib
    L = _lib.keyed_lib()
    P = 0x1000                                                                # a non-NULL address nobody dereferences
    cand = C.cast(P, C.POINTER(ak.mke_keyed_candidate))

    def select(emb=P, ld=16, kpad=16, n_cols=1000, lo=10, hi=300, tl=P, th=P, ids=P, n_seg=3, cap=100, c=cand, cnt=P, sure=P):
        return L.mke_sim_select_keyed(emb, ld, kpad, n_cols, lo, hi, tl, th, ids, SEED, 5, n_seg, cap, c, cnt, sure, None)

    def finish(c=cand, cnt=P, sure=P, rows=5, n_seg=3, cap=100, th=P, rid=P, ids=P, k=10, m=4, out=P, st=P):
        return L.mke_keyed_finish(c, cnt, sure, rows, n_seg, cap, th, rid, ids, k, m, SEED, 5, out, st, None)

    assert select(lo=7, hi=7) == 0 and finish(rows=0) == 0                    # nothing to do: nothing launched
    for kw in (dict(lo=-1), dict(lo=5, hi=4), dict(hi=1001), dict(n_cols=-1), dict(kpad=0), dict(kpad=24), dict(kpad=336),
               dict(kpad=32), dict(ld=18, kpad=16), dict(n_seg=0), dict(n_seg=65), dict(cap=0), dict(n_seg=64, cap=2 ** 14 + 1)):
        assert select(**kw) == ak.KEYED_E_SHAPE, kw
        assert b"mke_sim_select_keyed" in L.mke_keyed_last_error()
    assert select(kpad=144, ld=144) == ak.KEYED_E_UNSUPPORTED                 # a multiple of 16 with no instantiation
    for name in ("emb", "tl", "th", "ids", "cnt", "sure"):
        assert select(**{name: None}) == ak.KEYED_E_NULL and b"NULL" in L.mke_keyed_last_error(), name
    assert select(c=C.POINTER(ak.mke_keyed_candidate)()) == ak.KEYED_E_NULL
    # n_seg * seg_cap = 8192 is allowed; 2^29 slots a launch are not
    assert select(n_cols=10 ** 6, lo=0, hi=2 ** 16, n_seg=8, cap=1024) == ak.KEYED_E_RANGE and b"2^29" in L.mke_keyed_last_error()
    for kw in (dict(rows=-1), dict(rows=2 ** 31), dict(n_seg=0), dict(n_seg=65), dict(cap=0), dict(m=0), dict(m=10), dict(m=11), dict(k=1, m=1)):
        assert finish(**kw) == ak.KEYED_E_SHAPE, kw
        assert b"mke_keyed_finish" in L.mke_keyed_last_error()
    for name in ("cnt", "sure", "th", "rid", "ids", "out", "st"):
        assert finish(**{name: None}) == ak.KEYED_E_NULL and b"NULL" in L.mke_keyed_last_error(), name
    assert finish(c=C.POINTER(ak.mke_keyed_candidate)()) == ak.KEYED_E_NULL


def test_rows_per_launch_is_the_most_the_library_takes():
    """Whole launches at C5 scale sit exactly on the limit: one row more is the range error, the helper's count is inside the
    documented bound (row range + 128, times the slots, at most 2^29 - 1)."""
    import ctypes as C
    from multike_amd import _abi_keyed as ak, _lib
    from multike_amd.base.batch import keyed_rows_per_launch
    L = _lib.keyed_lib()
    P = 0x1000                                                                # never read: the refusal comes first
    cand = C.cast(P, C.POINTER(ak.mke_keyed_candidate))
    for slots, n_seg in ((512, 1), (8192, 8), (16384, 8), (2 ** 20, 64)):
        rows = keyed_rows_per_launch(slots)
        assert rows >= 1 and (rows + 128) * slots <= 2 ** 29 - 1 < (rows + 129) * slots
        rc = L.mke_sim_select_keyed(P, 16, 16, 2 ** 21, 0, rows + 1, P, P, P, 1, 1, n_seg, slots // n_seg, cand, P, P, None)
        assert rc == ak.KEYED_E_RANGE, (slots, rc)
    assert keyed_rows_per_launch(8192) == 65_407 and keyed_rows_per_launch(2 ** 30) == 1


def test_plan_of_the_automatic_rule_never_raises_and_never_leaves_the_library():
    """`keyed_plan`: n, k, cap -> path, sample and list.  The classes: the measured ones; large k / n, where the default sample's
    lower rank lies beyond what mke_topk_rows ranks (the automatic rule shrinks the sample, keyed=True says so); lists too wide
    to pay (the automatic rule keeps the whole-row path) or beyond the library (keyed=True says so)."""
    from multike_amd import _abi_keyed as ak
    from multike_amd._lib import MultiKEHipError
    from multike_amd.base.batch import (KEYED_AUTO_MAX_SLOTS, KEYED_TOP_MAX, keyed_key_below, keyed_plan, keyed_rows_per_launch,
                                        keyed_sample_ranks)
    c5 = keyed_plan(1_000_000, 20_000, 2048, False)
    assert c5 == dict(n_samp=65_536, z=3.0, r_hi=1202, r_lo=1421, top=1421, key_below=keyed_key_below(2048, 20_000), slots=8192,
                      rows=16_384)                                           # 1 GiB of candidates a launch
    assert keyed_plan(1_000_000, 20_000, 2048, False, round_floats=2 ** 32)["rows"] == keyed_rows_per_launch(8192) == 65_407
    assert keyed_plan(1_000_000, 20_000, 2048, False, round_floats=1)["rows"] == 128
    p = keyed_plan(300_000, 6_000, 2048, False)
    assert (p["n_samp"], p["r_hi"], p["r_lo"], p["slots"], p["rows"]) == (37_500, 667, 834, 8192, 16_384)
    # every call of before keeps its path
    assert keyed_plan(262_143, 6_000, 2048, False) is None and keyed_plan(262_144, 6_000, 2048, False) is not None
    assert keyed_plan(1_000_000, 2_000, 256, True) is None                   # the thresholded sweep applies
    assert keyed_plan(1_000_000, 20_000, None, False) is None and keyed_plan(1_000_000, 20_000, 20_000, False) is None
    assert keyed_plan(1_000_000, 20_000, 2048, False, keyed=False) is None
    assert keyed_plan(6000, 1500, 64, False) is None and keyed_plan(6000, 1500, 64, False, True)["n_samp"] == 750
    for cap in (None, 1500, 0):
        with pytest.raises(MultiKEHipError, match="keyed"):
            keyed_plan(6000, 1500, cap, False, True)
    # large k / n: truncated_epsilon = 0.9 at n = 1,000,000 is k = 100,000, s = 6,553 with the default sample, r_lo = 6,798
    assert keyed_sample_ranks(100_000, 1_000_000, 65_536, 3) == (6310, 6798)
    with pytest.raises(MultiKEHipError, match="n_samp"):
        keyed_plan(1_000_000, 100_000, 2048, False, True)
    p = keyed_plan(1_000_000, 100_000, 2048, False)
    assert (p["n_samp"], p["r_lo"], p["top"], p["slots"], p["rows"]) == (39_074, 4096, 4096, 16_384, 8192)
    assert keyed_sample_ranks(100_000, 1_000_000, 39_075, 3)[1] > KEYED_TOP_MAX          # the largest sample that fits
    assert keyed_plan(1_000_000, 100_000, 2048, False, None, dict(n_samp=60_000)) == p      # a given sample is shrunk as well
    for n, k in ((262_144, 250_000), (524_288, 40_000), (2_000_000, 150_000), (10 ** 7, 10 ** 6), (2 ** 31 - 256, 2 ** 30)):
        p = keyed_plan(n, k, 2048, False)                                    # never an error, never beyond the library
        assert p is None or (p["top"] <= KEYED_TOP_MAX and p["slots"] <= KEYED_AUTO_MAX_SLOTS <= ak.KEYED_MAX_LIST
                             and 128 <= p["rows"] <= keyed_rows_per_launch(p["slots"]) and 1 <= p["r_hi"] <= p["top"])
    # a band too wide to pay: half of 4,000,000 entities, 262,144 slots a row
    assert keyed_plan(4_000_000, 2_000_000, 2048, False) is None
    p = keyed_plan(4_000_000, 2_000_000, 2048, False, True, dict(n_samp=7000))
    assert (p["slots"], p["rows"]) == (262_144, 512)
    with pytest.raises(MultiKEHipError, match="slots"):                      # 2^21 slots: beyond MKE_KEYED_MAX_LIST
        keyed_plan(30_000_000, 15_000_000, 2048, False, True, dict(n_samp=7000))
    assert keyed_plan(30_000_000, 15_000_000, 2048, False) is None
    with pytest.raises(MultiKEHipError, match="keyed_params"):
        keyed_plan(1_000_000, 20_000, 2048, False, None, dict(nsamp=5))


def test_neighbour_table_refuses_keyed_without_a_cap_below_k():
    from multike_amd._lib import MultiKEHipError
    from multike_amd.base.batch import neighbour_table
    e = np.eye(8, dtype=np.float32)
    for kw in (dict(), dict(cap=4), dict(cap=5), dict(cap=None)):
        with pytest.raises(MultiKEHipError, match="keyed"):
            neighbour_table(e, list(range(8)), 4, 8, device="cuda", keyed=True, **kw)
    with pytest.raises(TypeError):                                            # keyword only
        neighbour_table(e, list(range(8)), 4, 8, "cuda", 4096, None, None, True)


def test_truncated_keyed_is_a_setting_and_unset_by_default():
    from multike_amd.utils import default_args
    assert default_args().truncated_keyed is None
    assert default_args(truncated_keyed=0).truncated_keyed == 0 and default_args(truncated_keyed=1).truncated_keyed == 1
