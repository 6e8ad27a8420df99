"""CSLS / metric evaluator C-ABI (version 106) without a GPU: the new symbols are exported, the ctypes structures match the
header's layout (offsets measured by the C compiler), every argument error returns its code before any launch, and
multike_amd.base.similarity on host arrays reproduces the reference's sim / csls_sim / calculate_nearest_k (fixture)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as ah
from conftest import GOLDEN, ROOT

NEW = ("mke_align_topk_mean_temp_bytes", "mke_align_topk_mean", "mke_align_rank_ex")


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
    for s in NEW:
        assert s in _lib.SYMBOLS
        getattr(raw, s)
    h = open(os.path.join(ROOT, "include", "multike_hip.h")).read()
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()


@pytest.mark.parametrize("name", ["AlignArgs", "TopkMeanArgs"])
def test_struct_layout_matches_header(name, tmp_path):
    from multike_amd import _lib
    S = getattr(_lib, name)
    struct = {"AlignArgs": "mke_align_args", "TopkMeanArgs": "mke_topk_mean_args"}[name]
    fields = [f for f, _ in S._fields_]
    assert ah.members(struct) == fields
    got = ah.offsets_and_size(tmp_path, struct, fields)
    assert got == [getattr(S, f).offset for f in fields] + [C.sizeof(S)]


def _align_args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(emb1=fake, ld1=80, emb2=fake, ld2=80, kpad=80, n1=100, n2=120, metric=0, sq1=None, sq2=None, csls_row=None,
                csls_col=None, rank=fake, ties=fake, best=fake)
    base.update(over)
    return _lib.AlignArgs(**base)


def _mean_args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(a=fake, lda=80, b=fake, ldb=80, kpad=80, n_a=100, n_b=120, metric=0, sq_a=None, sq_b=None, k=10, out=fake,
                temp=fake, temp_bytes=1 << 40)
    base.update(over)
    return _lib.TopkMeanArgs(**base)


def test_align_rank_ex_argument_errors(lib):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    call = lambda a: lib.mke_align_rank_ex(C.byref(a), None)
    assert lib.mke_align_rank_ex(None, None) == -1
    assert call(_align_args(emb1=None)) == -1
    assert call(_align_args(ties=None)) == -1
    assert call(_align_args(best=None)) == -1
    assert call(_align_args(csls_row=fake)) == -1                 # only one CSLS vector
    assert call(_align_args(csls_col=fake)) == -1
    assert call(_align_args(metric=1)) == -1                      # euclidean without the squared norms
    assert call(_align_args(metric=7)) == -3                      # unknown metric
    assert call(_align_args(kpad=24)) == -2
    assert call(_align_args(ld1=64)) == -2
    assert call(_align_args(ld2=82)) == -2
    assert call(_align_args(n1=130)) == -2                        # n2 < n1
    assert call(_align_args(n1=-1)) == -2
    assert call(_align_args(kpad=224, ld1=224, ld2=224)) == -3    # no instantiation
    assert call(_align_args(n1=0)) == 0
    assert _lib.lib().mke_last_error()


def test_topk_mean_argument_errors(lib):
    from multike_amd import _lib
    call = lambda a: lib.mke_align_topk_mean(C.byref(a), None)
    tb = lambda *a: lib.mke_align_topk_mean_temp_bytes(*[C.c_int64(a[0]), C.c_int64(a[1]), C.c_int(a[2]), C.c_int(a[3])])
    assert lib.mke_align_topk_mean(None, None) == -1
    assert call(_mean_args(k=0)) == -2
    assert call(_mean_args(k=119)) == -2                          # k <= n_b - 2
    assert call(_mean_args(k=118, n_b=120, temp_bytes=0)) == -2   # temp below the query
    assert call(_mean_args(a=None)) == -1
    assert call(_mean_args(out=None)) == -1
    assert call(_mean_args(metric=1)) == -1
    assert call(_mean_args(metric=3)) == -3
    assert call(_mean_args(kpad=40)) == -2
    assert call(_mean_args(lda=64)) == -2
    assert call(_mean_args(n_a=0)) == 0
    assert tb(100, 120, 80, 0) == -2 and tb(100, 120, 80, 119) == -2 and tb(100, 120, 33, 5) == -2 and tb(-1, 5, 80, 1) == -2
    assert tb(0, 120, 80, 10) == 0
    assert tb(100, 120, 80, 10) == 100 * 10 * 4                   # one column chunk of 2 tiles: k floats per row
    assert tb(100, 120, 80, 100) == 100 * 120 * 4                 # large k: whole similarity rows of one round
    big = tb(60000, 60000, 80, 10)
    assert 0 < big < 60000 * 64 * 10 * 4 + 1                      # bounded by 64 chunks, far from the n1 x n2 matrix
    # the scratch of the large-k path stays bounded by its row rounds (2^26 floats) plus the sort buffer
    assert tb(60000, 60000, 80, 5000) <= (1 << 26) * 4 + 1024 * 8192 * 4
    # scratch offsets are 64-bit; the large-k sort counts with 32-bit ints, so k past 2^30 is refused instead of wrapping
    assert tb(0x7FFFFF00, 0x7FFFFF00, 80, (1 << 30) + 1) == -4
    assert tb(0x7FFFFF00, 0x7FFFFF00, 80, 1 << 30) > 0
    with pytest.raises(_lib.MultiKEHipError):
        _lib.align_topk_mean_temp_bytes(10, 10, 16, 9)


UNSUPPORTED_KPADS = (144, 176, 224, 240, 272, 288, 304)  # the multiples of 16 up to MKE_MAX_STRIDE without an instantiation


def test_sweep_entry_points_refuse_a_width_without_instantiation(lib):
    """Every sweep launcher whose "no instantiation" path had no test (mke_align_rank, mke_sim_select, mke_sim_sample,
    mke_align_topk_mean on both of its paths) returns MKE_E_UNSUPPORTED with its own message once every other argument has
    passed its checks; none returns 0 without having launched.  Codes and texts as recorded from the build before the
    launch ladders became one width dispatcher (mke_align_rank's message carries no prefix)."""
    from multike_amd import _abi
    fake = C.c_void_p(0x1000)
    err = lambda: lib.mke_last_error().decode()
    for kpad in UNSUPPORTED_KPADS:
        ld = C.c_int(kpad)
        rc = lib.mke_align_rank(fake, ld, fake, ld, C.c_int(kpad), C.c_int64(100), C.c_int64(120), fake, fake, fake, None)
        assert (rc, err()) == (-3, f"unsupported kpad {kpad}")
        rc = lib.mke_sim_select(fake, ld, C.c_int(kpad), C.c_int64(120), C.c_int64(0), C.c_int64(100), fake, C.c_int(4),
                                C.c_int(64), C.cast(fake, C.POINTER(_abi.mke_candidate)), fake, None)
        assert (rc, err()) == (-3, f"mke_sim_select: unsupported kpad {kpad}")
        rc = lib.mke_sim_sample(fake, ld, C.c_int(kpad), C.c_int64(120), C.c_int64(0), C.c_int64(100), fake, ld, C.c_int(50),
                                fake, None)
        assert (rc, err()) == (-3, f"mke_sim_sample: unsupported kpad {kpad}")
        for k in (10, 100):                                       # the partial sweep, and whole rows through mke_sim_sample
            rc = lib.mke_align_topk_mean(C.byref(_mean_args(kpad=kpad, lda=kpad, ldb=kpad, k=k)), None)
            assert (rc, err()) == (-3, f"mke_align_topk_mean: unsupported kpad {kpad}")


def test_greedy_alignment_rejects_other_metrics():
    from multike_amd import _lib
    from multike_amd.base.alignment import greedy_alignment
    e = np.ones((4, 3), np.float32)
    with pytest.raises(_lib.MultiKEHipError, match="supported: 'inner', 'cosine', 'euclidean'"):
        greedy_alignment(e, e, [1], 1, "manhattan", False, 10, True)
    with pytest.raises(_lib.MultiKEHipError, match="supported"):
        greedy_alignment(e, e, [1], 1, "chebyshev", True, 0, True)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "csls_golden.npz"))


def test_similarity_on_host_arrays_matches_the_reference(golden):
    from multike_amd.base import similarity as S
    for c in golden["cases"]:
        n1, n2, d, k, normalize, dup = (int(x) for x in golden[c + "/meta"])
        metric = str(golden[c + "/metric"])
        e1, e2 = golden[c + "/e1"], golden[c + "/e2"]
        plain = S.sim(e1, e2, metric, bool(normalize))
        assert plain.dtype == np.float32 and plain.shape == (n1, n2)
        np.testing.assert_allclose(plain[:16, :24], golden[c + "/sim"], rtol=1e-5, atol=2e-6, err_msg=c)
        np.testing.assert_allclose(S.calculate_nearest_k(plain, k), golden[c + "/r_t"], rtol=1e-5, atol=2e-6, err_msg=c)
        np.testing.assert_allclose(S.calculate_nearest_k(plain.T, k), golden[c + "/r_s"], rtol=1e-5, atol=2e-6, err_msg=c)
        cs = S.sim(e1, e2, metric, bool(normalize), k)
        np.testing.assert_allclose(cs[:16, :24], golden[c + "/csls"], rtol=1e-5, atol=1e-5, err_msg=c)
        np.testing.assert_allclose(S.csls_sim(plain, k)[:16, :24], golden[c + "/csls"], rtol=1e-5, atol=1e-5, err_msg=c)
        # the gold's rank under the host CSLS matrix, on rows the fixture decides by more than rounding
        gold = cs[np.arange(n1), np.arange(n1)]
        rank = (cs > gold[:, None]).sum(1)
        sure = golden[c + "/gap"] >= 1e-4
        assert np.array_equal(rank[sure], golden[c + "/rank"][sure]), c
    with pytest.raises(Exception):
        S.calculate_nearest_k(np.zeros((3, 5), np.float32), 4)
