"""Stable-alignment C-ABI without a GPU: the new symbols are exported and listed (version unchanged), the ctypes structures match
the header's layout (offsets measured by the C compiler), every argument error returns its code before any launch, the scratch
query is bounded independently of n_a * n_b, and the NumPy oracle (tests/stable_oracle.py) on this package's host similarity
reproduces the reference's matching of every fixture case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stable_oracle as O
import abi_header as ah
from conftest import GOLDEN, ROOT

NEW = ("mke_stable_lists_temp_bytes", "mke_stable_lists", "mke_stable_rounds", "mke_stable_finish")
STRUCTS = {"StableListsArgs": "mke_stable_lists_args", "StableMatchArgs": "mke_stable_match_args"}


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
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()   # additions only
    for s in NEW:
        assert re.search(r"^(?:int|int64_t)\s+" + s + r"\s*\(", h, flags=re.M), s
    assert "code/base/alignment.py:82-128" in h and ":166-219" in h and ":131-138" in h          # what each replaces


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_matches_header(name, tmp_path):
    from multike_amd import _lib
    S = getattr(_lib, name)
    struct = STRUCTS[name]
    fields = [f for f, _ in S._fields_]
    assert ah.members(struct) == fields
    got = ah.offsets_and_size(tmp_path, struct, fields)
    assert got == [getattr(S, f).offset for f in fields] + [C.sizeof(S)]


def _lists_args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(a=fake, lda=80, b=fake, ldb=80, kpad=80, n_a=100, n_b=120, metric=0, sq_a=None, sq_b=None, csls_row=None,
                csls_col=None, sim_mat=None, ld_sim=0, cut=10, whole_rows=0, sample_cols=0, out_val=fake, out_col=fake,
                flags=fake, temp=fake, temp_bytes=1 << 40)
    base.update(over)
    return _lib.StableListsArgs(**base)


def _match_args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(n_a=100, n_b=120, cut=10, val=fake, col=fake, ptr=fake, holder=fake, proposals=fake, n_proposals=64, match=fake,
                counts=fake)
    base.update(over)
    return _lib.StableMatchArgs(**base)


def test_stable_lists_argument_errors(lib):
    fake = C.c_void_p(0x1000)
    call = lambda a: lib.mke_stable_lists(C.byref(a), None)
    assert lib.mke_stable_lists(None, None) == -1
    for name in ("a", "b", "out_val", "out_col", "flags", "temp"):
        assert call(_lists_args(**{name: None})) == -1, name
    assert call(_lists_args(cut=0)) == -2
    assert call(_lists_args(cut=121)) == -2                       # cut <= n_b
    assert call(_lists_args(cut=121, whole_rows=1)) == -2
    assert call(_lists_args(n_a=-1)) == -2
    assert call(_lists_args(kpad=24)) == -2                       # not a multiple of 16
    assert call(_lists_args(kpad=224, lda=224, ldb=224)) == -3    # no instantiation
    assert call(_lists_args(lda=64)) == -2                        # below kpad
    assert call(_lists_args(ldb=82)) == -2                        # not a multiple of 4
    assert call(_lists_args(metric=1)) == -1                      # euclidean without the squared norms
    assert call(_lists_args(metric=1, sq_a=fake)) == -1
    assert call(_lists_args(metric=5)) == -3
    assert call(_lists_args(csls_row=fake)) == -1                 # one CSLS vector without the other
    assert call(_lists_args(csls_col=fake)) == -1
    assert call(_lists_args(sample_cols=-1)) == -2
    assert call(_lists_args(temp_bytes=0)) == -2                  # temp below the query
    assert call(_lists_args(cut=129, temp_bytes=100 * 120 * 4 - 1)) == -2
    assert call(_lists_args(sim_mat=fake, ld_sim=119)) == -2      # a caller's matrix narrower than n_b
    assert call(_lists_args(n_a=0)) == 0
    assert lib.mke_last_error()


def test_stable_rounds_and_finish_argument_errors(lib):
    rounds = lambda a, first=0, n=4: lib.mke_stable_rounds(C.byref(a), C.c_int64(first), C.c_int(n), None)
    finish = lambda a: lib.mke_stable_finish(C.byref(a), None)
    assert lib.mke_stable_rounds(None, C.c_int64(0), C.c_int(1), None) == -1
    assert lib.mke_stable_finish(None, None) == -1
    for name in ("val", "col", "ptr", "holder", "proposals"):
        assert rounds(_match_args(**{name: None})) == -1, name
    for name in ("val", "col", "ptr", "holder", "match", "counts"):
        assert finish(_match_args(**{name: None})) == -1, name
    assert rounds(_match_args(cut=0)) == -2 and finish(_match_args(cut=0)) == -2
    assert rounds(_match_args(n_a=-1)) == -2
    assert rounds(_match_args(), first=-1) == -2
    assert rounds(_match_args(), n=-1) == -2
    assert rounds(_match_args(), first=61, n=4) == -4             # rounds beyond the counter array
    assert rounds(_match_args(n_a=0)) == 0                        # nothing to launch
    assert rounds(_match_args(), n=0) == 0


def test_temp_bytes_is_bounded_independently_of_the_matrix(lib):
    from multike_amd import _lib
    tb = lambda n_a, n_b, kpad, cut, whole=0: lib.mke_stable_lists_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(kpad),
                                                                               C.c_int(cut), C.c_int(whole))
    assert tb(100, 120, 80, 0) == -2 and tb(100, 120, 80, 121) == -2 and tb(100, 120, 33, 5) == -2 and tb(-1, 5, 80, 1) == -2
    assert tb(0, 120, 80, 10) == 0
    matrix = 60000 * 60000 * 4
    # whole rows (cut > 128): rounds of at most 2^26 floats, plus the selected columns and the sort buffer of one round
    rows = (1 << 26) // 60000 // 128 * 128
    big = tb(60000, 60000, 80, 500)
    assert 0 < big <= (1 << 26) * 4 + rows * 500 * 4 + rows * 512 * 8 + 1024
    huge = tb(60000, 60000, 80, 5000)                             # 8192 keys per row: sorted in the scratch
    assert 0 < huge <= (1 << 26) * 4 + rows * 5000 * 4 + rows * 8192 * 8 + 1024
    # the sweep path (cut <= 128): one round of candidate slots (2^28 bytes) + a threshold and eight counters per row
    fast = tb(60000, 60000, 80, 100)
    assert 0 < fast <= (1 << 28) + 60000 * 4 + 32768 * 8 * 4 + 1024
    assert fast * 50 < matrix                                     # far below the reference's 14 GB
    assert tb(600000, 600000, 80, 100) <= (1 << 28) + 600000 * 4 + 32768 * 8 * 4 + 1024   # 100x the matrix, same rounds
    assert 0 < tb(60000, 60000, 80, 100, 1) <= (1 << 26) * 4 + rows * 100 * 4 + 1024      # flagged rows redone as whole rows
    assert tb(0x7FFFFF00, 0x7FFFFF00, 80, (1 << 30) + 1) == -4
    with pytest.raises(_lib.MultiKEHipError):
        _lib.stable_lists_temp_bytes(10, 10, 16, 11)


def test_stable_alignment_rejects_other_metrics():
    from multike_amd import _lib
    from multike_amd.base.alignment import stable_alignment
    e = np.ones((4, 3), np.float32)
    with pytest.raises(_lib.MultiKEHipError, match="supported: 'inner', 'cosine', 'euclidean'"):
        stable_alignment(e, e, "manhattan", False, 0, 1)


def test_distributed_driver_refuses_stable_cut():
    from multike_amd import _lib
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args
    assert default_args().stable_cut == 0
    args = default_args(stable_cut=100)
    with pytest.raises(_lib.MultiKEHipError, match="stable_cut"):
        _ShardedMixin()._init_sharded(None, args, None, 0, 2)     # refused before any data is touched


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "stable_golden.npz"))


def test_oracle_reproduces_the_reference_on_every_fixture_case(golden):
    from multike_amd.base import similarity as S
    assert list(golden["cases"]) == ["inner_sq", "inner_wide", "inner_csls", "euclid", "euclid_csls", "cosine_raw"]
    for c in golden["cases"]:
        n1, n2, d, k, normalize, cut = (int(x) for x in golden[c + "/meta"])
        mat = S.sim(golden[c + "/e1"], golden[c + "/e2"], str(golden[c + "/metric"]), bool(normalize), k)
        val, col = O.lists_from_matrix(mat, min(cut, n2))
        match = O.deferred_acceptance(val, col, n2)
        assert np.array_equal(match, golden[c + "/match"]), c     # the generator kept only matchings stable under +-1e-5
        assert (match >= 0).all() and len(set(match.tolist())) == n1, c
        assert O.blocking_pairs(val, col, match, n2) == [], c
        assert abs(round(float(np.mean(match == np.arange(n1))) * 100, 3) - float(golden[c + "/precision"])) < 2e-3, c
        assert int(golden[c + "/greedy_differs"]) >= 13, c        # the one-to-one constraint binds in every case


def test_oracle_on_hand_made_lists():
    # three suitors share one order; the lower row wins the tie and the others walk down their lists
    col = np.array([[0, 1, 2]] * 3, dtype=np.int32)
    val = np.ones((3, 3), dtype=np.float32)
    assert O.deferred_acceptance(val, col, 3).tolist() == [0, 1, 2]
    # lists too short: 4 suitors, 2 columns
    col = np.array([[0, 1]] * 4, dtype=np.int32)
    val = np.array([[1, 1], [2, 2], [3, 3], [4, 4]], dtype=np.float32)
    assert O.deferred_acceptance(val, col, 2).tolist() == [-1, -1, 1, 0]
    assert O.blocking_pairs(val, col, np.array([-1, -1, 1, 0]), 2) == []
    assert O.blocking_pairs(val, col, np.array([0, -1, 1, -1]), 2) != []
    v, c = O.lists_from_matrix(np.array([[1.0, np.nan, 1.0, 2.0]]), 4)
    assert c.tolist() == [[3, 0, 2, -1]] and v[0, :3].tolist() == [2.0, 1.0, 1.0]
