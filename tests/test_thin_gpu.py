"""mke_idlist_thin (mke_thin.hip, libmultike_thin.so: include/multike_thin.h) against tests/thin_oracle.py, bit for bit, through the C entry point itself: the output
sits inside a poisoned buffer whose guard entries before and after it must come back unchanged."""
import numpy as np
import pytest
import torch

import thin_oracle as to

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, -0x5A5A5A5B
KS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 5003)
ROW_IDS = np.array([2 ** 31 - 1, 0, 7, 2 ** 30 + 3, 123_456_789, 5, 2 ** 31 - 2, 99, 1_000_003, 17], dtype=np.int64)
SEEDS = (12345, 2 ** 63 + 0x1234567)


def _ms(k):
    return sorted({m for m in (1, 2, 63, 64, 65, k - 1, k) if 1 <= m <= k})


def _ids(rng, rows, k):
    ids = rng.integers(0, 2 ** 31, size=(rows, k), dtype=np.int64).astype(np.int32)
    ids[0, 0] = 0
    ids[-1, -1] = 2 ** 31 - 1
    ids[rows // 2, k // 2] = 2 ** 31 - 1 if k > 2 else ids[rows // 2, k // 2]
    if k > 3:
        ids[0, 3] = 0                                   # a repeated id: two equal keys in one row
    if rows >= 3:
        ids[1, :] = 424_242                             # all keys equal: the lowest m positions win
    return ids


def _row_ids(rows):
    return (ROW_IDS[np.arange(rows) % len(ROW_IDS)] - (np.arange(rows) // len(ROW_IDS)) * 1000).clip(0).astype(np.int32)


def _call(ids_dev, rows, k, ld, row_ids_dev, m, seed, buf):
    from multike_amd import _lib
    return _lib.thin_lib().mke_idlist_thin(ids_dev.data_ptr(), rows, k, ld, None if row_ids_dev is None else row_ids_dev.data_ptr(),
                                      m, seed, buf.data_ptr() + 4 * GUARD, torch.cuda.current_stream().cuda_stream)


def _run(ids, row_ids, m, seed, pad=0):
    """-> out int32 [rows, m] (host); asserts the guards."""
    rows, k = ids.shape
    wide = np.full((rows, k + pad), 77, dtype=np.int32)
    wide[:, :k] = ids
    d_ids = torch.as_tensor(wide, device="cuda")
    d_rid = None if row_ids is None else torch.as_tensor(np.asarray(row_ids, dtype=np.int32), device="cuda")
    buf = torch.full((GUARD + rows * m + GUARD,), POISON, dtype=torch.int32, device="cuda")
    rc = _call(d_ids, rows, k, k + pad, d_rid, m, seed, buf)
    assert rc == 0
    h = buf.cpu().numpy()
    assert (h[:GUARD] == POISON).all() and (h[GUARD + rows * m:] == POISON).all(), "wrote outside out[rows][m]"
    return h[GUARD:GUARD + rows * m].reshape(rows, m)


@pytest.mark.parametrize("k", KS)
def test_equals_the_oracle_bit_for_bit(k):
    rng = np.random.default_rng(k)
    for rows in (1, 3, 130):
        ids = _ids(rng, rows, k)
        for m in _ms(k):
            for given in (True, False):
                rid = _row_ids(rows) if given else None
                seed = SEEDS[(m + rows + given) % 2]
                got = _run(ids, rid, m, seed, pad=0 if (m + given) % 2 else 5)
                exp = to.thin(ids, rid, m, seed)
                assert np.array_equal(got, exp), (rows, k, m, given, seed)
                if rows >= 3 and m < k:
                    assert (got[1] == 424_242).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_both_seeds_and_a_wide_row_stride(seed):
    rng = np.random.default_rng(5)
    ids = _ids(rng, 7, 300)
    for rid in (_row_ids(7), None):
        assert np.array_equal(_run(ids, rid, 40, seed, pad=212), to.thin(ids, rid, 40, seed))
    a, b = _run(ids, None, 40, SEEDS[0]), _run(ids, None, 40, SEEDS[1])
    assert not np.array_equal(a, b)


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 50, size=(130, 1000)).astype(np.int32)      # many equal keys: ties in every row
    a = _run(ids, _row_ids(130), 65, SEEDS[1])
    b = _run(ids, _row_ids(130), 65, SEEDS[1])
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, to.thin(ids, _row_ids(130), 65, SEEDS[1]))


def test_binding_returns_the_rows_and_accepts_a_strided_view():
    from multike_amd import _lib
    rng = np.random.default_rng(3)
    ids = _ids(rng, 9, 257)
    wide = torch.as_tensor(np.concatenate([ids, ids[:, :7]], axis=1), device="cuda")
    rid = torch.as_tensor(_row_ids(9), device="cuda")
    out = _lib.idlist_thin(wide[:, :257], 64, SEEDS[1], row_ids=rid)
    assert out.dtype == torch.int32 and tuple(out.shape) == (9, 64)
    assert np.array_equal(out.cpu().numpy(), to.thin(ids, _row_ids(9), 64, SEEDS[1]))
    assert np.array_equal(_lib.idlist_thin(wide[:, :257].contiguous(), 257, 1).cpu().numpy(), ids)
    with pytest.raises(_lib.MultiKEHipError, match="mke_idlist_thin"):
        _lib.idlist_thin(wide[:, :257], 258, 1)


def test_refusals_return_their_code_and_leave_out_untouched():
    from multike_amd import _lib
    L = _lib.thin_lib()
    rows, k, m = 3, 10, 4
    d_ids = torch.zeros(rows, k, dtype=torch.int32, device="cuda")
    buf = torch.full((GUARD + rows * k + GUARD,), POISON, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    out = buf.data_ptr() + 4 * GUARD
    cases = [
        ("NULL ids", (None, rows, k, k, None, m, 1, out, st), _lib.E_NULL),
        ("NULL out", (d_ids.data_ptr(), rows, k, k, None, m, 1, None, st), _lib.E_NULL),
        ("k < 1", (d_ids.data_ptr(), rows, 0, k, None, m, 1, out, st), _lib.E_SHAPE),
        ("m < 1", (d_ids.data_ptr(), rows, k, k, None, 0, 1, out, st), _lib.E_SHAPE),
        ("m > k", (d_ids.data_ptr(), rows, k, k, None, k + 1, 1, out, st), _lib.E_SHAPE),
        ("ld_ids < k", (d_ids.data_ptr(), rows, k, k - 1, None, m, 1, out, st), _lib.E_SHAPE),
        ("rows < 0", (d_ids.data_ptr(), -1, k, k, None, m, 1, out, st), _lib.E_SHAPE),
    ]
    for what, args, code in cases:
        assert L.mke_idlist_thin(*args) == code, what
        assert b"mke_idlist_thin" in L.mke_thin_last_error(), what
    assert L.mke_idlist_thin(d_ids.data_ptr(), 0, k, k, None, m, 1, out, st) == 0          # rows == 0: ok, nothing launched
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == POISON).all()
