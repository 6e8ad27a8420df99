"""Mutual nearest-neighbour alignment without a GPU: the two symbols are exported and bound (version unchanged), the ctypes
structure matches the header, every argument error returns its code and its message before any launch, the hyper-parameters
and the host surface refuse what they must, and the NumPy oracle (tests/mutual_oracle.py) on a hand-written matrix."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mutual_oracle as MO
import abi_header as ah
from conftest import ROOT

NEW = ("mke_align_mutual", "mke_mutual_pairs")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def test_new_symbols_exported_and_listed(lib):
    from multike_amd import _lib
    raw = C.CDLL(_lib.SO_PATH)
    h = open(os.path.join(ROOT, "include", "multike_hip.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS
        getattr(raw, s)
        assert re.search(r"^int\s+" + s + r"\s*\(", h, flags=re.M), s
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()   # additions only
    assert callable(_lib.align_mutual) and callable(_lib.mutual_pairs)
    for name in ("MKE_MUTUAL_NO_LDS_FOLD", "MKE_MUTUAL_FILTER"):
        assert int(re.search(r"#define %s (\d+)" % name, h).group(1)) == getattr(_lib, name[4:])


def test_struct_fields_match_header():
    from multike_amd import _lib
    assert ah.members("mke_mutual_args") == [f for f, _ in _lib.MutualArgs._fields_]


def _args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(a=fake, lda=80, b=fake, ldb=80, kpad=80, n_a=100, n_b=60, metric=0, sq_a=None, sq_b=None, csls_row=None,
                csls_col=None, row_best=fake, col_best=fake, flags=0)
    base.update(over)
    return _lib.MutualArgs(**base)


def test_align_mutual_argument_errors(lib):
    fake = C.c_void_p(0x1000)

    def call(want, text, **over):
        assert lib.mke_align_mutual(C.byref(_args(**over)), None) == want, over
        msg = lib.mke_last_error().decode()
        assert msg.startswith("mke_align_mutual: ") and text in msg, (over, msg)

    assert lib.mke_align_mutual(None, None) == -1 and "mke_align_mutual: NULL args" in lib.mke_last_error().decode()
    for name in ("a", "b", "row_best", "col_best"):
        call(-1, "NULL pointer", **{name: None})
    call(-3, "unknown metric 5", metric=5)
    call(-2, "kpad must be a multiple of 16", kpad=24)
    call(-2, "kpad must be a multiple of 16", kpad=0)
    call(-2, "lda, ldb must be multiples of 4 >= kpad", lda=64)
    call(-2, "lda, ldb must be multiples of 4 >= kpad", ldb=82)
    call(-3, "unsupported kpad 224", kpad=224, lda=224, ldb=224)
    call(-1, "euclidean needs sq_a and sq_b", metric=1)
    call(-1, "euclidean needs sq_a and sq_b", metric=1, sq_a=fake)
    call(-1, "csls_row and csls_col are both NULL or both set", csls_row=fake)
    call(-1, "csls_row and csls_col are both NULL or both set", csls_col=fake)
    call(-2, "bad n_a / n_b", n_a=-1)
    call(-2, "bad n_a / n_b", n_b=1 << 31)
    call(-3, "unknown flags", flags=4)
    # no pair: success without a launch, whatever the pointers (n_a > n_b is no error: there is no gold column)
    assert lib.mke_align_mutual(C.byref(_args(n_a=0, a=None, row_best=None)), None) == 0
    assert lib.mke_align_mutual(C.byref(_args(n_b=0, b=None, col_best=None)), None) == 0


def test_mutual_pairs_argument_errors(lib):
    fake = C.c_void_p(0x1000)
    call = lambda n_a, n_b, thr, rb=fake, cb=fake, m=fake, c=fake: lib.mke_mutual_pairs(
        rb, cb, C.c_int64(n_a), C.c_int64(n_b), C.c_float(thr), m, c, None)
    assert call(10, 10, float("nan")) == -4
    assert "threshold is NaN" in lib.mke_last_error().decode()
    assert call(-1, 10, 0.0) == -2 and "mke_mutual_pairs: bad n_a / n_b" in lib.mke_last_error().decode()
    for kw in (dict(rb=None), dict(cb=None), dict(m=None), dict(c=None)):
        assert call(10, 10, 0.0, **kw) == -1, kw
        assert "mke_mutual_pairs: NULL pointer" in lib.mke_last_error().decode()


def test_hyper_parameters_and_the_sharded_driver():
    from multike_amd import _lib
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args
    assert default_args().mutual == 0 and default_args().mutual_threshold is None
    with pytest.raises(_lib.MultiKEHipError, match="mutual"):
        _ShardedMixin()._init_sharded(None, default_args(mutual=1), None, 0, 2)     # refused before any data is touched


def test_host_surface_refuses_before_the_device():
    from multike_amd import _lib
    from multike_amd.base.alignment import mutual_alignment, mutual_pairs
    e1, e2 = np.ones((5, 8), dtype=np.float32), np.ones((4, 8), dtype=np.float32)
    with pytest.raises(_lib.MultiKEHipError, match="len\\(embed2\\) >= len\\(embed1\\)"):
        mutual_alignment(e1, e2, "inner", True, 0, 4)
    with pytest.raises(_lib.MultiKEHipError, match="choose one re-scoring"):
        mutual_alignment(e2, e1, "inner", True, 10, 4, sinkhorn=(4, 0.1))
    with pytest.raises(_lib.MultiKEHipError, match="choose one re-scoring"):
        mutual_pairs(e1, e2, csls_k=10, sinkhorn=(4, 0.1))
    with pytest.raises(_lib.MultiKEHipError, match="manhattan"):
        mutual_alignment(e2, e1, "manhattan", True, 0, 4)
    with pytest.raises(_lib.MultiKEHipError, match="threshold is NaN"):
        mutual_alignment(e2, e1, "inner", True, 0, 4, threshold=float("nan"))
    with pytest.raises(_lib.MultiKEHipError, match="threshold is NaN"):
        mutual_pairs(e1, e2, threshold=float("nan"))


def test_oracle_on_a_hand_written_matrix():
    nan = np.nan
    S = np.array([[5.0, 5.0, 1.0, nan],      # row tie: columns 0 and 1, the lower wins
                  [5.0, 2.0, 7.0, nan],      # column 0 ties between rows 0 and 1, the lower row wins
                  [1.0, 6.0, 7.0, nan]],     # column 2 ties between rows 1 and 2; column 3 is all NaN
                 dtype=np.float32)
    row_col, col_row = MO.bests(S)
    assert row_col.tolist() == [0, 2, 2] and col_row.tolist() == [0, 2, 1, -1]
    match, counts = MO.pairs(S)
    assert match.tolist() == [0, 2, -1] and counts == (2, 1)           # row 2's best column prefers row 1
    assert MO.pairs(S, 5.0)[0].tolist() == [0, 2, -1]                   # >= is inclusive
    assert MO.pairs(S, np.float32(5.5))[0].tolist() == [-1, 2, -1]
    none, counts = MO.pairs(S, np.inf)
    assert none.tolist() == [-1, -1, -1] and counts == (0, 0)
    rb, cb = MO.words(S)
    assert cb[3] == 0 and rb.dtype == np.uint64
    assert int(rb[0]) == (0xC0A00000 << 32) | 0xFFFFFFFF               # ordered(5.0f = 0x40A00000), column 0
    assert int(cb[2]) == (0xC0E00000 << 32) | (0xFFFFFFFF - 1)         # 7.0f, row 1
    neg = np.array([[-1.0, -np.inf], [nan, -np.inf]], dtype=np.float32)
    rb, cb = MO.words(neg)
    assert int(rb[0]) == (0x407FFFFF << 32) | 0xFFFFFFFF               # ordered(-1.0f = 0xBF800000) = ~bits
    assert int(rb[1]) == (0x007FFFFF << 32) | (0xFFFFFFFF - 1)         # a row of NaN and -inf: (-inf, the lowest column holding it)
    assert int(cb[1]) == (0x007FFFFF << 32) | 0xFFFFFFFF               # a column of -inf: (-inf, row 0)
    assert MO.pairs(neg)[0].tolist() == [0, -1]                        # row 1's best column 1 prefers row 0
    assert MO.scores_prf(np.array([0, -1, 1, 3])) == (pytest.approx(200 / 3), 50.0, pytest.approx(2 * (200 / 3) * 50 / (200 / 3 + 50)))
    assert MO.scores_prf(np.array([-1, -1])) == (0.0, 0.0, 0.0)
