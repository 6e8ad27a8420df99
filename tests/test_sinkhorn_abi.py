"""Sinkhorn re-scoring C-ABI ((9d) of include/multike_hip.h) without a GPU: the new symbols are exported, listed and declared,
the ctypes structure matches the header's layout (offsets measured by the C compiler), every argument error returns its code
before any launch (invalid-argument paths only, fake pointers), the scratch query follows simt_split, and the host side
(similarity.sinkhorn_sim, the refusals, the hyper-parameters) agrees with the float64 oracle of tests/sinkhorn_oracle.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sinkhorn_oracle as O
import abi_header as ah
from conftest import GOLDEN, ROOT

NEW = ("mke_align_lse_temp_bytes", "mke_align_lse")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "multike_hip.h")).read()


def test_new_symbols_exported_listed_and_declared(lib):
    from multike_amd import _lib
    raw = C.CDLL(_lib.SO_PATH)
    h = _header()
    for s in NEW:
        assert s in _lib.SYMBOLS
        getattr(raw, s)
        assert re.search(r"\b" + s + r"\(", h), s
    assert "(9d)" in h
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()     # additions only


def test_struct_layout_matches_header(tmp_path):
    from multike_amd import _lib
    S, struct = _lib.LseArgs, "mke_lse_args"
    fields = [f for f, _ in S._fields_]
    assert fields == ["a", "lda", "b", "ldb", "kpad", "n_a", "n_b", "metric", "sq_a", "sq_b", "sub_b", "tau", "out", "temp", "temp_bytes"]
    assert ah.members(struct) == fields
    got = ah.offsets_and_size(tmp_path, struct, fields)
    assert got == [getattr(S, f).offset for f in fields] + [C.sizeof(S)]


def _args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(a=fake, lda=80, b=fake, ldb=80, kpad=80, n_a=100, n_b=120, metric=0, sq_a=None, sq_b=None, sub_b=None, tau=0.05,
                out=fake, temp=fake, temp_bytes=1 << 40)
    base.update(over)
    return _lib.LseArgs(**base)


def test_argument_errors(lib):
    fake = C.c_void_p(0x1000)
    call = lambda a: lib.mke_align_lse(C.byref(a), None)
    err = lambda: lib.mke_last_error().decode()
    assert lib.mke_align_lse(None, None) == -1 and "NULL args" in err()
    assert call(_args(n_a=-1)) == -2
    assert call(_args(n_b=-1)) == -2
    assert call(_args(n_a=0x7FFFFF01)) == -2
    assert call(_args(n_b=0)) == -2 and "n_b >= 1" in err()
    assert call(_args(n_b=0, n_a=0)) == -2
    assert call(_args(kpad=40)) == -2
    assert call(_args(kpad=0)) == -2
    assert call(_args(kpad=336, lda=336, ldb=336)) == -2
    assert call(_args(lda=64)) == -2
    assert call(_args(ldb=82)) == -2
    assert call(_args(metric=3)) == -3 and "unknown metric 3" in err()
    assert call(_args(metric=1)) == -1 and "euclidean needs" in err()
    assert call(_args(metric=1, sq_a=fake)) == -1
    assert call(_args(a=None)) == -1
    assert call(_args(b=None)) == -1
    assert call(_args(out=None)) == -1
    assert call(_args(temp=None)) == -1
    for tau in (0.0, -0.05, float("inf"), float("nan")):
        assert call(_args(tau=tau)) == -4 and "tau" in err(), tau
    assert call(_args(temp_bytes=100 * 8 - 1)) == -2 and "temp below" in err()
    for kpad in (144, 176, 224, 240, 272, 288, 304):                 # multiples of 16 without an instantiation
        assert (call(_args(kpad=kpad, lda=kpad, ldb=kpad)), err()) == (-3, f"mke_align_lse: unsupported kpad {kpad}")
    assert call(_args(n_a=0)) == 0
    assert call(_args(n_a=0, a=None, out=None, temp=None, temp_bytes=0)) == 0


def _split_chunks(rows, n_cols, kpad, target=6144, min_tiles=16, cap=64):
    """simt_split of mke_simtile.h followed by simt_split_fixed: the number of non-empty column chunks."""
    bn = 64 if kpad // 16 <= 13 else 32
    ntiles = (n_cols + bn - 1) // bn
    row_blocks = (rows + 127) // 128
    chunks = max(1, min((target + row_blocks - 1) // row_blocks, (ntiles + min_tiles - 1) // min_tiles, cap))
    per = (ntiles + chunks - 1) // chunks
    return (ntiles + per - 1) // per


def test_temp_bytes_follow_the_column_split(lib):
    from multike_amd import _lib
    tb = lambda n_a, n_b, kpad: lib.mke_align_lse_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(kpad))
    assert tb(100, 120, 80) == 100 * 8                              # one chunk: one (m, s) pair per row
    assert tb(130, 2113, 80) == 130 * 3 * 8                         # 34 tiles in three chunks of 12, 12, 10
    assert tb(0, 120, 80) == 0
    for n_a, n_b, kpad in ((1, 1, 16), (70, 90, 208), (129, 1025, 128), (129, 1025, 320), (300, 70000, 80), (60000, 60000, 80),
                           (60000, 60000, 256), (5, 10 ** 6, 320), (0x7FFFFF00, 0x7FFFFF00, 80)):
        assert tb(n_a, n_b, kpad) == n_a * _split_chunks(n_a, n_b, kpad) * 8, (n_a, n_b, kpad)
    assert tb(60000, 60000, 80) == 60000 * 14 * 8                   # 6.7 MB beside a 13.4 GiB matrix
    assert tb(-1, 5, 80) == -2 and tb(5, 0, 80) == -2 and tb(5, 5, 33) == -2 and tb(5, 5, 336) == -2
    with pytest.raises(_lib.MultiKEHipError):
        _lib.align_lse_temp_bytes(10, 0, 16)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sinkhorn_golden.npz"))


def test_fixture_cases_and_the_cap_on_rows_left_out(golden):
    assert list(golden["cases"]) == ["inner_100", "inner_sq", "inner_wide", "euclid"]
    shapes = {"inner_100": (100, 130, 16, 0.05, 10), "inner_sq": (120, 120, 20, 0.05, 10), "inner_wide": (200, 333, 75, 0.05, 10),
              "euclid": (96, 140, 12, 0.1, 30)}
    none_out = 0
    for c in golden["cases"]:
        n1, n2, d, normalize, iters = (int(x) for x in golden[c + "/meta"])
        tau = float(golden[c + "/tau"])
        assert (n1, n2, d, tau, iters) == shapes[c]
        M = float(golden[c + "/M"])
        pot_bound = iters * (O.bound(tau, n2, M) + O.bound(tau, n1, M))
        assert pot_bound == float(golden[c + "/pot_bound"]) <= 2 * iters * O.bound(tau, max(n1, n2), M)
        out = int((golden[c + "/gap"] < 4 * pot_bound).sum())
        assert out == int(golden[c + "/left_out"]) <= 0.05 * n1, c
        none_out += out == 0
    assert none_out >= 2


def test_sinkhorn_sim_on_host_arrays_matches_the_oracle(golden):
    from multike_amd.base import similarity as S
    for c in golden["cases"]:
        n1, n2, d, normalize, iters = (int(x) for x in golden[c + "/meta"])
        tau, metric = float(golden[c + "/tau"]), str(golden[c + "/metric"])
        e1, e2 = golden[c + "/e1"], golden[c + "/e2"]
        plain = S.sim(e1, e2, metric, bool(normalize))
        np.testing.assert_allclose(plain[:16, :24], golden[c + "/sim"], rtol=1e-5, atol=2e-6, err_msg=c)
        a, b = O.potentials(plain, iters, tau)
        want = O.scores(plain, a, b)
        got = S.sinkhorn_sim(plain, iters, tau)
        assert got.dtype == np.float32 and got.shape == (n1, n2)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=c)
        np.testing.assert_allclose(S.sim(e1, e2, metric, bool(normalize), sinkhorn=(iters, tau)), want, rtol=0, atol=1e-6, err_msg=c)
        # the fixture's potentials come from the reference's own similarity matrix: the same up to its float32 rounding
        np.testing.assert_allclose(a, golden[c + "/a"], rtol=0, atol=1e-4, err_msg=c)
        np.testing.assert_allclose(got[:16, :24], golden[c + "/score"], rtol=0, atol=2e-4, err_msg=c)
        # after the last column pass the columns of exp(scores / tau) sum to 1 (float64)
        pa, pb = S.sinkhorn_potentials(plain, iters, tau)
        cols = np.exp(((plain.astype(np.float64) - pa[:, None]) - pb[None, :]) / tau).sum(0)
        np.testing.assert_allclose(cols, 1.0, rtol=0, atol=1e-9, err_msg=c)
        # the gold's rank under the host matrix, on rows the fixture decides by more than rounding
        gold = got[np.arange(n1), np.arange(n1)]
        sure = golden[c + "/gap"] >= 1e-4
        assert np.array_equal((got > gold[:, None]).sum(1)[sure], golden[c + "/rank"][sure]), c


def test_sinkhorn_sim_survives_large_arguments():
    """Arguments of +-4000 / tau: the maximum is taken out of every sum."""
    from multike_amd.base import similarity as S
    mat = np.array([[200.0, -200.0, 0.0], [-200.0, 200.0, 1.0]], dtype=np.float32)
    got = S.sinkhorn_sim(mat, 5, 0.05)
    assert np.isfinite(got).all()
    a, b = O.potentials(mat, 5, 0.05)
    np.testing.assert_allclose(got, O.scores(mat, a, b), rtol=0, atol=1e-4)


def test_sinkhorn_and_csls_together_are_refused():
    from multike_amd import _lib
    from multike_amd.base import similarity as S
    from multike_amd.base.alignment import alignment_counts, alignment_ranks, greedy_alignment, stable_alignment
    e = np.eye(6, 4, dtype=np.float32) + 1.0
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k"):
        alignment_counts(e, e, csls_k=2, sinkhorn=(3, 0.05))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k"):
        alignment_ranks(e, e, csls_k=2, sinkhorn=(3, 0.05))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k"):
        greedy_alignment(e, e, [1], 1, "inner", True, 2, True, sinkhorn=(3, 0.05))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k"):
        stable_alignment(e, e, "inner", True, 2, 1, sinkhorn=(3, 0.05))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k"):
        S.sim(e, e, "inner", True, 2, sinkhorn=(3, 0.05))
    for bad in ((0, 0.05), (3, 0.0), (3, -1.0), (3, float("nan")), (2.5, 0.05)):
        with pytest.raises(_lib.MultiKEHipError, match="iters >= 1"):
            alignment_counts(e, e, sinkhorn=bad)
        with pytest.raises(_lib.MultiKEHipError, match="iters >= 1"):
            S.sinkhorn_sim(e @ e.T, *bad)


def test_hyper_parameters_and_driver_refusals():
    from multike_amd import _lib
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args, sinkhorn_option
    d = default_args()
    assert d.sinkhorn_iters == 0 and d.sinkhorn_tau == 0.05
    assert sinkhorn_option(d) is None
    assert sinkhorn_option(default_args(sinkhorn_iters=10)) == (10, 0.05)
    assert sinkhorn_option(default_args(sinkhorn_iters=4, sinkhorn_tau=0.1)) == (4, 0.1)
    with pytest.raises(_lib.MultiKEHipError, match="csls and sinkhorn_iters"):
        sinkhorn_option(default_args(sinkhorn_iters=10, csls=10))
    with pytest.raises(_lib.MultiKEHipError, match="sinkhorn_iters"):
        _ShardedMixin()._init_sharded(None, default_args(sinkhorn_iters=10), None, 0, 2)     # refused before any data is touched


def test_model_construction_refuses_csls_with_sinkhorn():
    """`csls` together with `sinkhorn_iters` raises when the model is constructed, before anything touches the device."""
    from multike_amd import _lib
    from multike_amd.MultiKE_model import MultiKE
    from multike_amd.utils import default_args
    with pytest.raises(_lib.MultiKEHipError, match="csls and sinkhorn_iters"):
        MultiKE(None, default_args(sinkhorn_iters=10, csls=5), None)
