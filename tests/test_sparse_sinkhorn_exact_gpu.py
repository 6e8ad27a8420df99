"""libmultike_sparse.so on the device through its C-ABI wrappers (multike_amd._lib.sparse_support / sparse_lse) against
tests/sparse_sinkhorn_oracle.py: the support bit for bit on hand-made lists in poisoned outputs, one log-sum-exp call at every
list length at which the kernels change path, and the same bits from a second run.

The bound of one mke_sparse_lse call is sinkhorn_oracle.bound(tau, longest list, M), the counted bound of one mke_align_lse
call over as many terms: a lane's running sum holds at most len / 16 (or SEG / 64) terms and the butterflies add 4 (or 6)
merges, each one rounding of the sum and one exp ulp — fewer roundings than the sequential sum of n terms the bound counts
(n 2^-24, doubled); the segment merge and the final m + log2 s are float64, rounded to f32 once (inside the 6 * 2^-24 M term).
No further term is needed."""
import numpy as np
import pytest

import sinkhorn_oracle as O
import sparse_sinkhorn_oracle as SO

pytestmark = pytest.mark.gpu

POISON_I32 = 0x5A5A5A5A
POISON_I64 = 0x5A5A5A5A5A5A5A5A


def _consts():
    from multike_amd import _abi_sparse as ab
    return ab.SPARSE_Q, ab.SPARSE_SEG


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _poisoned(n_a, n_b, capacity):
    """A SparseSupport whose every output word is a sentinel (values: a NaN with a payload)."""
    import torch
    from multike_amd import _lib
    s = _lib.SparseSupport()
    s.n_a, s.n_b, s.capacity = n_a, n_b, capacity
    full = lambda n, dt, v: torch.full((n,), v, dtype=dt, device="cuda")
    s.row_off, s.col_off = full(n_a + 1, torch.int64, POISON_I64), full(n_b + 1, torch.int64, POISON_I64)
    s.row_seg, s.col_seg = full(n_a + 1, torch.int32, POISON_I32), full(n_b + 1, torch.int32, POISON_I32)
    s.ent_col, s.ent_row, s.ent_idx = (full(capacity, torch.int32, POISON_I32) for _ in range(3))
    s.ent_val = full(capacity, torch.int32, 0x7FC5A5A5).view(torch.float32)
    s.count = full(1, torch.int64, POISON_I64)
    s.lse_temp = torch.zeros(max(int(_lib.sparse_lib().mke_sparse_lse_temp_bytes(capacity)), 8) // 4, dtype=torch.int32, device="cuda")
    return s


def _segments(off):
    Q, SEG = _consts()
    n = np.diff(off)
    return np.concatenate([[0], np.cumsum(np.where(n > Q, (n + SEG - 1) // SEG, 0))]).astype(np.int32)


def _build(lists_, slack=5):
    from multike_amd import _lib
    val_r, col_r, val_c, row_c = lists_
    capacity = col_r.size + row_c.size + slack
    s = _poisoned(col_r.shape[0], row_c.shape[0], capacity)
    return _lib.sparse_support(_dev(val_r), _dev(col_r), _dev(val_c), _dev(row_c), out=s)


def _hold_support(s, want):
    """Every output of mke_sparse_support against the NumPy enumeration, bits of the values included; past the count untouched."""
    E = want["count"]
    assert s.entries() == E
    assert np.array_equal(s.row_off.cpu().numpy(), want["row_off"]) and np.array_equal(s.col_off.cpu().numpy(), want["col_off"])
    assert np.array_equal(s.row_seg.cpu().numpy(), _segments(want["row_off"]))
    assert np.array_equal(s.col_seg.cpu().numpy(), _segments(want["col_off"]))
    for name in ("ent_col", "ent_row", "ent_idx"):
        got = getattr(s, name).cpu().numpy()
        assert np.array_equal(got[:E], want[name]), name
        assert (got[E:] == POISON_I32).all(), name
    bits = s.ent_val.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits[:E], want["ent_val"].view(np.uint32)) and (bits[E:] == 0x7FC5A5A5).all()


def _padding(n, cut):
    return np.full((n, cut), -np.inf, dtype=np.float32), np.full((n, cut), -1, dtype=np.int32)


def _support_cases():
    r = np.random.default_rng(3)
    S = r.standard_normal((6, 9)).astype(np.float32)
    v4, i4 = SO.lists(r.standard_normal((4, 3)).astype(np.float32), 2)
    wide = SO.lists(r.standard_normal((70, 300)).astype(np.float32), 19) + SO.lists(r.standard_normal((300, 70)).astype(np.float32), 33)
    return {"hand": SO.hand_case(),
            "cut_1": SO.lists(S, 1) + SO.lists(S.T, 1),
            "n_a_0": _padding(0, 3) + (v4, i4),                  # the columns' lists name rows that do not exist
            "n_b_0": (v4, i4) + _padding(0, 2),
            "both_0": _padding(0, 1) + _padding(0, 1),
            "ragged": wide}                                        # cuts that are no multiple of 16, several workgroups


@pytest.mark.parametrize("name", ["hand", "cut_1", "n_a_0", "n_b_0", "both_0", "ragged"])
def test_support_bit_for_bit_in_poisoned_outputs(name):
    lists_ = _support_cases()[name]
    want = SO.support(*lists_)
    if name == "hand":
        assert want["count"] == 9 and 0 in np.diff(want["row_off"]) and 0 in np.diff(want["col_off"])
    if name in ("n_a_0", "n_b_0", "both_0"):
        assert want["count"] == 0
    _hold_support(_build(lists_), want)


def _lengths():
    Q, SEG = _consts()
    return [0, 1, 15, 16, 17, Q - 1, Q, Q + 1, SEG - 1, SEG, SEG + 1, 2 * SEG + 37]


def _hub_lists(seed, mirror):
    """Lists planted without a sweep: list k of the long side has lengths[k] entries, because that many lists of the other side
    (cut 1) name it; the last has 2 SEG + 37.  mirror = False: the rows are long; True: the columns are."""
    lengths = _lengths()
    r = np.random.default_rng(seed)
    owner = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    owner = np.concatenate([owner, [-1, -1, -1]]).astype(np.int32)             # three lists of the short side name nothing
    val = np.where(owner >= 0, r.uniform(-1, 1, len(owner)), -np.inf).astype(np.float32)
    named = (val[:, None], owner[:, None])
    nothing = _padding(len(lengths), 1)
    return (named + nothing) if mirror else (nothing + named)


@pytest.fixture(scope="module")
def hubs():
    """{mirror: (lists, support on the device, oracle support)}, built once and left unchanged."""
    out = {}
    for mirror in (False, True):
        lists_ = _hub_lists(11 + mirror, mirror)
        s = _build(lists_)
        want = SO.support(*lists_)
        _hold_support(s, want)
        out[mirror] = (lists_, s, want)
    return out


def _reference(want, columns, sub, tau):
    n_a, n_b = len(want["row_off"]) - 1, len(want["col_off"]) - 1
    rows = np.repeat(np.arange(n_a), np.diff(want["row_off"]))
    cols, vals = want["ent_col"], want["ent_val"]
    if columns:
        return SO.lse_lists(n_b, cols, rows, vals, sub, tau)
    return SO.lse_lists(n_a, rows, cols, vals, sub, tau)


RATIOS = {}


@pytest.mark.parametrize("tau", [0.05, 0.02])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
def test_every_list_length_within_the_bound(hubs, mirror, with_sub, tau):
    from multike_amd import _lib
    lists_, s, want = hubs[mirror]
    lengths = np.diff(want["col_off"] if mirror else want["row_off"])
    assert lengths.tolist() == _lengths()
    r = np.random.default_rng(5)
    worst = 0.0
    for columns in (False, True):
        n_other = s.n_a if columns else s.n_b
        sub = r.uniform(-0.5, 0.5, n_other).astype(np.float32) if with_sub else None
        got = _lib.sparse_lse(s, columns, tau, None if sub is None else _dev(sub)).cpu().numpy().astype(np.float64)
        ref = _reference(want, columns, sub, tau)
        n = np.diff(want["col_off"] if columns else want["row_off"])
        assert (got[n == 0] == 0.0).all() and (ref[n == 0] == 0.0).all() and (n == 0).any()
        bound = O.bound(tau, int(n.max()), 1.0 + (0.5 if with_sub else 0.0))
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / bound)
        print(f"mirror={mirror} columns={columns} sub={with_sub} tau={tau}: longest {int(n.max())}, error {err:.3e}, bound {bound:.3e}, "
              f"ratio {err / bound:.3f}")
        assert err <= bound
    RATIOS[mirror, with_sub, tau] = worst
    print(f"largest error / bound ratio so far: {max(RATIOS.values()):.3f}")


def test_same_bits_twice(hubs):
    import torch
    from multike_amd import _lib
    for mirror, (lists_, s, want) in hubs.items():
        again = _build(lists_)
        for name in ("row_off", "col_off", "row_seg", "col_seg", "ent_col", "ent_val", "ent_row", "ent_idx", "count"):
            assert torch.equal(getattr(s, name).view(torch.int32), getattr(again, name).view(torch.int32)), name
        sub_r, sub_c = (_dev(np.random.default_rng(9).uniform(-0.5, 0.5, n).astype(np.float32)) for n in (s.n_b, s.n_a))
        for tau in (0.05, 0.02):
            for columns, sub in ((False, None), (True, None), (False, sub_r), (True, sub_c)):
                first = _lib.sparse_lse(s, columns, tau, sub)
                second = _lib.sparse_lse(again, columns, tau, sub, out=torch.full_like(first, float("nan")))
                assert torch.equal(first.view(torch.int32), second.view(torch.int32))
