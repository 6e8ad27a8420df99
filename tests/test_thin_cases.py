"""The definition of mke_idlist_thin (include/multike_thin.h) as tests/thin_oracle.py restates it: its own
properties, the marginal-uniformity condition the capped neighbour tables rest on, and the refusals of
`neighbour_table(cap=, round_floats=)` that need no device."""
import numpy as np
import pytest

import thin_oracle as to


def _distinct(rng, rows, k, hi=2 ** 31 - 1):
    return np.stack([rng.choice(hi, size=k, replace=False) for _ in range(rows)]).astype(np.int32)


def test_mix_is_the_splitmix64_finaliser():
    # splitmix64's published first outputs from state 0: mix(1 * golden), mix(2 * golden)
    g = 0x9E3779B97F4A7C15
    assert [int(x) for x in to.mix(np.array([g, (2 * g) & (2 ** 64 - 1)], dtype=np.uint64))] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


@pytest.mark.parametrize("k,m", [(1, 1), (2, 1), (64, 16), (257, 64), (1000, 999)])
def test_output_is_a_subsequence_of_length_m(k, m):
    rng = np.random.default_rng(k * 1000 + m)
    ids = rng.integers(0, 50, size=(5, k)).astype(np.int32)          # repeated ids: equal keys inside a row
    out = to.thin(ids, [3, 9, 2 ** 31 - 1, 0, 77], m, seed=11)
    assert out.shape == (5, m) and out.dtype == np.int32
    for r in range(5):
        j = 0
        for x in ids[r]:                                             # greedy subsequence match
            if j < m and x == out[r, j]:
                j += 1
        assert j == m


def test_m_equal_k_is_the_identity():
    rng = np.random.default_rng(0)
    ids = rng.integers(0, 2 ** 31 - 1, size=(4, 37)).astype(np.int32)
    assert np.array_equal(to.thin(ids, None, 37, seed=5), ids)


def test_equal_keys_keep_the_lowest_positions():
    ids = np.full((1, 40), 123, dtype=np.int32)
    ids[0, 7] = 5                                                     # one other id, so that positions can be told apart
    out = to.thin(ids, [4], 10, seed=2 ** 63 + 9)
    ky = to.key(ids, [4], 2 ** 63 + 9)[0]
    exp = ids[0, :10] if ky[7] < ky[0] else np.delete(ids[0], 7)[:10]
    assert np.array_equal(out[0], exp)


def test_kept_set_is_invariant_under_a_permutation_of_the_list():
    rng = np.random.default_rng(1)
    ids = _distinct(rng, 6, 300)
    rid = [0, 1, 5, 1000, 2 ** 20, 2 ** 31 - 1]
    a = to.thin(ids, rid, 40, seed=77)
    perm = np.stack([rng.permutation(300) for _ in range(6)])
    b = to.thin(np.take_along_axis(ids, perm, axis=1), rid, 40, seed=77)
    assert np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1))
    assert not np.array_equal(a, b)                                  # the order follows the list


def test_kept_set_differs_between_rows_and_between_seeds():
    ids = np.tile(np.arange(1000, 1256, dtype=np.int32), (3, 1))      # one list under three row ids
    a = to.thin(ids, [10, 11, 12], 32, seed=1)
    assert len({tuple(r) for r in a}) == 3
    b = to.thin(ids, [10, 11, 12], 32, seed=2)
    assert all(not np.array_equal(a[r], b[r]) for r in range(3))
    # row_ids None keys row r by r
    assert np.array_equal(to.thin(ids, None, 32, seed=1), to.thin(ids, [0, 1, 2], 32, seed=1))


def test_marginal_uniformity_condition():
    """k = 64, m = 16, row id 7, ids 100..163, seeds 0..4095: every element's inclusion count lies in [885, 1163], i.e.
    1024 +- 5 standard deviations of Binomial(4096, 1/4) (sd = 27.7).  The definition measures 955..1081."""
    ids = np.arange(100, 164, dtype=np.int32)[None]
    count = np.zeros(64, dtype=np.int64)
    for seed in range(4096):
        kept = to.thin(ids, [7], 16, seed)[0]
        count[kept - 100] += 1
    print("inclusion counts: min", count.min(), "max", count.max())
    assert count.sum() == 4096 * 16
    assert count.min() >= 885 and count.max() <= 1163, (count.min(), count.max())


def test_neighbour_table_refuses_bad_cap_before_touching_a_device():
    from multike_amd._lib import MultiKEHipError
    from multike_amd.base.batch import neighbour_table
    e = np.eye(8, dtype=np.float32)
    for bad in (0, -1, -2048):
        with pytest.raises(MultiKEHipError, match="cap"):
            neighbour_table(e, list(range(8)), 4, 8, device="cuda", cap=bad)
    for bad in (0, -5):
        with pytest.raises(MultiKEHipError, match="round_floats"):
            neighbour_table(e, list(range(8)), 4, 8, device="cuda", round_floats=bad)
    with pytest.raises(TypeError):                                    # keyword only: the positional signature is unchanged
        neighbour_table(e, list(range(8)), 4, 8, "cuda", 4096, None, None, 2)


def test_refresh_seed_is_a_pure_function_of_seed_epoch_and_kg():
    from multike_amd.base.batch import refresh_seed
    seen = {refresh_seed(s, ep, kg) for s in (0, 1, 2 ** 31) for ep in (0, 20, 40, 10 ** 6) for kg in (0, 1)}
    assert len(seen) == 3 * 4 * 2 and all(0 <= x < 2 ** 64 for x in seen)
    assert refresh_seed(5, 20, 1) == refresh_seed(5, 20, 1)


def test_truncated_cap_is_a_hyper_parameter_and_off_by_default():
    from multike_amd.utils import default_args
    assert default_args().truncated_cap == 0 and default_args(truncated_cap=2048).truncated_cap == 2048


def test_thin_abi_module_is_what_the_generator_writes_and_the_library_exports(tmp_path):
    """libmultike_thin.so has a header and a generated module of its own: include/multike_hip.h, multike_amd/_abi.py and the
    symbols of libmultike_hip.so are those of before it (tests/test_abi_generated.py pins them)."""
    import os
    import subprocess
    import sys
    import abi_header as ah
    from multike_amd import _abi, _abi_thin, _lib
    header = os.path.join(os.path.dirname(ah.HEADER), "multike_thin.h")
    out = tmp_path / "_abi_thin.py"
    subprocess.check_call([sys.executable, ah.GENERATOR, header, str(out)])
    assert out.read_bytes() == open(os.path.join(os.path.dirname(ah.GENERATED), "_abi_thin.py"), "rb").read()
    assert list(_abi_thin.FUNCTIONS) == ["mke_thin_last_error", "mke_idlist_thin"] and not set(_abi_thin.FUNCTIONS) & set(_abi.FUNCTIONS)
    if not os.path.exists(_lib.THIN_SO_PATH):
        import __graft_entry__ as g
        g.build()
    assert ah.exported_symbols(_lib.THIN_SO_PATH) == set(_abi_thin.FUNCTIONS)
    L = _lib.thin_lib()
    for name, (restype, argtypes) in _abi_thin.FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    # refusals need no device: they come before any launch
    assert L.mke_idlist_thin(None, 3, 10, 10, None, 4, 1, None, None) == _abi.E_NULL and b"NULL" in L.mke_thin_last_error()
    assert L.mke_idlist_thin(None, 3, 10, 10, None, 11, 1, None, None) == _abi.E_SHAPE and b"mke_idlist_thin" in L.mke_thin_last_error()
    assert L.mke_idlist_thin(None, 0, 10, 10, None, 4, 1, None, None) == 0
