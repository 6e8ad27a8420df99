"""The rank kernel where its two entry points differ on purpose: rows whose similarities are all NaN or all -inf, NaN in
one column chunk only, NaN at the gold column.  Nothing else in the suite reaches these rows.

The rules (gold column = row index, s = the row's similarities as the kernel's epilogue sees them):
  rank = #{non-NaN s > gold}; ties = #{s == gold}, 0 for a NaN gold.
  mke_align_rank    best: if any similarity exceeds -3.0e38f, (max, lowest column attaining it); else best_key(-3.0e38f, 0).
  mke_align_rank_ex best: if any similarity is not NaN, (max, lowest column attaining it), -inf included; else the word stays 0.
Expected values come from a NumPy oracle over the similarity matrix, never from the device.  Operands hold small integers, as
in sweep_cases.py, so every finite dot product is exact in any summation order; assertions are equality of integers and of
bit patterns, and two runs must agree bit for bit.

Shapes: n1 = 40; n2 = 150 (one column chunk, ragged last tile) and 1100 (two chunks at kpad 16, three at kpad 256: the row's
`best` is merged by atomicMax across chunks); kpad 16 (64-column tiles) and 256 (32-column tiles).
Scenarios: "rows": one row all NaN, one row all -inf, the others ordinary — for the plain entry point through the embeddings
(a NaN row of emb1; a row (+inf, 0, ...) of emb1 against emb2[:, 0] = -1), for _ex through csls_row = NaN / +inf; "chunk": NaN
in the columns of the first chunk only (of the first tile where the sweep is one chunk) — NaN rows of emb2, or csls_col = NaN;
"gold": NaN at three gold columns only."""
import functools

import numpy as np
import pytest

import sweep_cases as sc

pytestmark = pytest.mark.gpu

N1 = 40
NAN_ROW, INF_ROW = 5, 9
GOLD_NAN = (3, 17, 39)
L = 3
FLOOR = np.float32(-3.0e38)          # where the plain entry point's running best starts


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _operands(kpad, n2):
    """Integer operands [n, kpad] (zero beyond dim = kpad - 3), squared norms, CSLS terms (multiples of 1/8).  B[:, 0] = -1: the
    plain entry point's -inf row needs it.  One +-L vector sits in row 1 of A and at columns 1 and n2 - 2 of B: that row's
    maximum lies in the first and in the last chunk, the lowest column must win.  Column n2 - 1 copies gold column 2."""
    rng = np.random.default_rng([kpad, n2, 18])
    dim = kpad - 3
    A = np.zeros((N1, kpad), np.float32)
    B = np.zeros((n2, kpad), np.float32)
    A[:, :dim] = rng.integers(-L, L + 1, (N1, dim))
    B[:, :dim] = rng.integers(-L, L + 1, (n2, dim))
    B[:N1:3] = A[::3]
    v = rng.choice([-L, L], dim).astype(np.float32)
    v[0] = -1.0
    B[:, 0] = -1.0
    A[1, :dim] = v
    B[1, :dim] = v
    B[n2 - 2, :dim] = v
    B[n2 - 1] = B[2]
    sq_a, sq_b = (A * A).sum(1, dtype=np.float32), (B * B).sum(1, dtype=np.float32)
    rt = (rng.integers(-16, 17, N1) / 8.0).astype(np.float32)
    rs = (rng.integers(-15, 17, n2) / 8.0).astype(np.float32)
    rs[[1, n2 - 2]] = np.float32(-2.0)
    rs[n2 - 1] = rs[2]
    return A, B, sq_a, sq_b, rt, rs


def _first_chunk(kpad, n2):
    """Columns [0, end) of the sweep's first column chunk; of its first tile when the whole sweep is one chunk."""
    bounds = sc.chunk_bounds(sc.Case("rank", "corner", kpad, kpad - 3, N1, n2))
    return bounds[0][1] if len(bounds) > 1 else sc.bn_for(kpad)


def _nan_cols(scenario, kpad, n2):
    if scenario == "chunk":
        return np.arange(_first_chunk(kpad, n2))
    return np.array(GOLD_NAN if scenario == "gold" else (), dtype=np.int64)


def _best_key(v, col):
    u = int(np.float32(v).view(np.uint32))
    o = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (o << 32) | (0xFFFFFFFF - col)


def _oracle(S, ex):
    """(rank int32, ties int32, best uint64) of the rules in the module docstring."""
    n = S.shape[0]
    gold = S[np.arange(n), np.arange(n)]
    with np.errstate(invalid="ignore"):
        rank = (~np.isnan(S) & (S > gold[:, None])).sum(1).astype(np.int32)
        ties = (S == gold[:, None]).sum(1).astype(np.int32)
        live = ~np.isnan(S) if ex else (S > FLOOR)
    best = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        if live[i].any():
            m = S[i][live[i]].max()
            best[i] = _best_key(m, int(np.flatnonzero(live[i] & (S[i] == m))[0]))
        elif not ex:
            best[i] = _best_key(FLOOR, 0)
    return rank, ties, best


def _check(S, ex, rank, ties, best, scenario):
    want_rank, want_ties, want_best = _oracle(S, ex)
    if scenario == "rows":                               # the oracle's input is what the scenario promises
        assert np.isnan(S[NAN_ROW]).all() and np.isneginf(S[INF_ROW]).all()
        assert want_ties[NAN_ROW] == 0 and want_ties[INF_ROW] == S.shape[1] and want_best[NAN_ROW] == (0 if ex else _best_key(FLOOR, 0))
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    if ties is not None:
        assert np.array_equal(ties.cpu().numpy(), want_ties)
    assert np.array_equal(best.cpu().numpy().view(np.uint64), want_best)


SHAPES = [(kpad, n2) for kpad in (16, 256) for n2 in (150, 1100)]
SCENARIOS = ("rows", "chunk", "gold")


@pytest.mark.parametrize("with_ties", (True, False), ids=("ties", "noties"))
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("kpad,n2", SHAPES)
def test_plain_entry_point(kpad, n2, scenario, with_ties):
    import torch
    from multike_amd import _lib
    A, B = (x.copy() for x in _operands(kpad, n2)[:2])
    if scenario == "rows":
        A[NAN_ROW, :kpad - 3] = np.nan
        A[INF_ROW] = 0.0
        A[INF_ROW, 0] = np.inf                           # against B[:, 0] = -1: every similarity of the row is -inf
    B[_nan_cols(scenario, kpad, n2)] = np.nan
    with np.errstate(invalid="ignore"):
        S = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32)   # finite entries: exact integers
    ad, bd = _dev(A), _dev(B)
    outs = []
    for _ in range(2):
        rank = torch.zeros(N1, dtype=torch.int32, device="cuda")
        ties = torch.zeros(N1, dtype=torch.int32, device="cuda") if with_ties else None
        best = torch.zeros(N1, dtype=torch.int64, device="cuda")
        _lib.align_rank(ad, bd, kpad, N1, n2, rank, best, ties)
        _check(S, False, rank, ties, best, scenario)
        outs.append((rank, best) + ((ties,) if with_ties else ()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


@pytest.mark.parametrize("euclidean", (False, True), ids=("inner", "euclidean"))
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("kpad,n2", SHAPES)
def test_ex_entry_point(kpad, n2, scenario, euclidean):
    import torch
    from multike_amd import _lib
    A, B, sq_a, sq_b, rt, rs = _operands(kpad, n2)
    rt, rs = rt.copy(), rs.copy()
    if scenario == "rows":
        rt[NAN_ROW] = np.nan
        rt[INF_ROW] = np.inf                             # (2 v - inf) - r_S = -inf in every column
    rs[_nan_cols(scenario, kpad, n2)] = np.nan
    dots = sc.int_dots(A, B).astype(np.float32)
    with np.errstate(invalid="ignore"):
        S = sc.rescore32(dots, sq_a, sq_b, rt, rs, euclidean, True)
    ad, bd = _dev(A), _dev(B)
    code = _lib.METRIC_EUCLIDEAN if euclidean else _lib.METRIC_INNER
    sq1, sq2 = (_dev(sq_a), _dev(sq_b)) if euclidean else (None, None)
    rtd, rsd = _dev(rt), _dev(rs)
    outs = []
    for _ in range(2):
        rank = torch.zeros(N1, dtype=torch.int32, device="cuda")
        ties = torch.zeros(N1, dtype=torch.int32, device="cuda")
        best = torch.zeros(N1, dtype=torch.int64, device="cuda")
        _lib.align_rank_ex(ad, bd, kpad, rank, ties, best, code, sq1, sq2, rtd, rsd)
        _check(S, True, rank, ties, best, scenario)
        outs.append((rank, ties, best))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
