"""mke_align_lse (the half-iteration of the Sinkhorn re-scoring, (9d) of include/multike_hip.h) against the float64 oracle of
sinkhorn_oracle.py, within its bound tau (n + 8) 2^-23 + 6 * 2^-24 M.  Operands come from sweep_cases.py: integer rows, so the
similarities the sweep hands to the epilogue are exact (inner) or the float32 values of mke_rescore.h emulated one operation
at a time (euclidean), in NaN-poisoned buffers with guard rows; sub_b carries guard entries that would dominate every sum if a
column past n_b were read.  Every call is made twice and must repeat itself bit for bit; `out` is over-allocated and the rows
behind n_a must keep their sentinel."""
import numpy as np
import pytest

import sinkhorn_oracle as O
import sweep_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
TAUS = (0.75, 8.0)              # exact in float32; the dot products of L = 3 rows spread over about +-4 sqrt(dim)


def _case(tag, kpad, n_a, n_b, mode, L=3, ragged=True):
    dim = kpad - 5 if ragged else kpad
    c = sc.Case("topk_mean", tag, kpad, dim, n_a, n_b, mode=mode, L=L)      # the column split of mke_align_lse is topk_mean's
    assert c.L * c.L * c.dim < 2 ** 24
    return c


def _cases():
    out = []
    for kpad in sc.REGIME_KPADS:
        for mode in sc.MODES[:2]:
            out += [_case("nb", kpad, 33, nb, mode, ragged=nb % 2 == 1) for nb in (1, 31, 32, 33, 63, 64, 65)]
            out += [_case("na", kpad, na, 65, mode) for na in (1, 127, 129)]
    out += [_case("chunks", 80, 130, 2113, mode) for mode in sc.MODES[:2]]      # three column chunks, the last tile one column wide
    out += [_case("width", kpad, 70, 90, sc.MODES[i % 2], L=(3, 40)[i % 3 == 0]) for i, kpad in enumerate(sc.KPADS)]
    return out


CASES = _cases()
ids = lambda c: c.id


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(c, vec):
    return _dev(sc.guarded(vec, sc.bn_for(c.kpad)))[:vec.shape[0]]


def _buffers(c, A, B):
    bn = sc.bn_for(c.kpad)
    return _dev(sc.embed(A, c.kpad, sc.LD_EXTRA_A, bn))[:A.shape[0]], _dev(sc.embed(B, c.kpad, sc.LD_EXTRA_B, bn))[:B.shape[0]]


def _scores32(c, A, B, sq_a, sq_b):
    """float32 [n_a, n_b]: what the epilogue sees (sweep_cases.rescore32: mke_rescore.h one float32 operation at a time)."""
    d = sc.int_dots(A, B)
    assert np.abs(d).max() < 2 ** 24
    return sc.rescore32(d.astype(np.float32), sq_a, sq_b, None, None, c.euclidean, False)


def _run(c, A, B, sq_a, sq_b, sub, tau, extra=7):
    """The call, twice, on poisoned buffers into an over-allocated out; returns float32 [n_a] after the common checks."""
    import torch
    from multike_amd import _lib
    a, b = _buffers(c, A, B)
    code = _lib.METRIC_EUCLIDEAN if c.euclidean else _lib.METRIC_INNER
    qa = _guarded(c, sq_a) if c.euclidean else None
    qb = _guarded(c, sq_b) if c.euclidean else None
    sb = None if sub is None else _guarded(c, sub)
    outs = []
    for _ in range(2):
        out = torch.full((A.shape[0] + extra,), float(SENTINEL), dtype=torch.float32, device="cuda")
        got = _lib.align_lse(a, b, c.kpad, tau, code, qa, qb, sb, out=out)
        assert got.data_ptr() == out.data_ptr()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))           # two runs, the same bits
    assert np.array_equal(outs[0][A.shape[0]:], np.full(extra, SENTINEL))           # rows >= n_a are never written
    return outs[0][:A.shape[0]]


def _check(c, A, B, sq_a, sq_b, sub, tau):
    S = _scores32(c, A, B, sq_a, sq_b)
    got = _run(c, A, B, sq_a, sq_b, sub, tau)
    want = O.lse(S, sub, tau)
    M = float(np.abs(S).max()) + (0.0 if sub is None else float(np.abs(sub).max()))
    bound = O.bound(tau, c.n_b, M)
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{c.id} tau {tau}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (c.id, err, bound)
    return got


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_align_lse_within_the_bound(c):
    ops = sc.operands(c)
    tau = TAUS[CASES.index(c) % 2]
    got = _check(c, ops.A, ops.B, ops.sq_a, ops.sq_b, ops.rs, tau)
    assert got.shape == (c.n_a,)


@pytest.mark.parametrize("c", [x for x in CASES if x.tag in ("chunks", "na") or x.n_b in (1, 65)], ids=ids)
def test_no_sub_b_equals_zeros_bit_for_bit(c):
    ops = sc.operands(c)
    tau = TAUS[(CASES.index(c) + 1) % 2]
    none = _check(c, ops.A, ops.B, ops.sq_a, ops.sq_b, None, tau)
    zeros = _run(c, ops.A, ops.B, ops.sq_a, ops.sq_b, np.zeros(c.n_b, dtype=np.float32), tau)
    assert np.array_equal(none.view(np.int32), zeros.view(np.int32))


@pytest.mark.parametrize("kpad", sc.REGIME_KPADS)
def test_large_arguments_planted_rows(kpad):
    """tau = 1/64, L = 40 integers, inner product: column 0 of every B row is +40; one A row is (-40, +-1, +-1, +-1, 0 ...) — every
    argument (s - b) / tau is below -64 * 1400 — and one is (+40, +-1, +-1, +-1, 0 ...): every argument above +64 * 1400.  A
    raw exp of either is 0 or inf; the results are finite and within the bound."""
    tau = 1.0 / 64
    c = _case("big", kpad, 129, 2 * sc.bn_for(kpad) + 1, "inner", L=40)
    ops = sc.operands(c)
    A, B = ops.A.copy(), ops.B.copy()
    rng = np.random.default_rng(kpad)
    B[:, 0] = 40
    for row, sign in ((3, -40), (100, 40)):
        A[row] = 0
        A[row, 0] = sign
        A[row, 1:4] = rng.choice([-1, 1], 3)
    sq_a, sq_b = (A.astype(np.float64) ** 2).sum(1).astype(np.float32), (B.astype(np.float64) ** 2).sum(1).astype(np.float32)
    S = _scores32(c, A, B, sq_a, sq_b)
    arg = (S.astype(np.float64) - ops.rs.astype(np.float64)[None, :]) / tau
    assert arg[3].max() <= -200 and arg[100].min() >= 200
    got = _check(c, A, B, sq_a, sq_b, ops.rs, tau)
    assert np.isfinite(got[[3, 100]]).all() and got[3] < -1400 and got[100] > 1400


SHIFTS = {"inner": (262144.0, -262144.0), "euclidean": (8.0, -70000.0)}      # |inner product| <= 40^2 * 75; euclidean: -700 < s <= 1


@pytest.mark.parametrize("mode", sc.MODES[:2])
@pytest.mark.parametrize("side", (0, 1), ids=("below", "above"))
def test_large_arguments_every_row(mode, side):
    """tau = 1/64, L = 40 integers, both metrics: a constant added to sub_b pushes EVERY argument of every row below -200 or
    above +200 (the sums s - sub_b stay exact in float32: multiples of 1/8 below 2^19)."""
    tau = 1.0 / 64
    c = _case("shift", 80, 129, 129, mode, L=40)
    ops = sc.operands(c)
    shift = SHIFTS[mode][side]
    sub = (ops.rs + np.float32(shift)).astype(np.float32)
    assert np.array_equal(sub.astype(np.float64), ops.rs.astype(np.float64) + shift)
    S = _scores32(c, ops.A, ops.B, ops.sq_a, ops.sq_b)
    arg = (S.astype(np.float64) - sub.astype(np.float64)[None, :]) / tau
    assert arg.max() <= -200 if shift > 0 else arg.min() >= 200
    _check(c, ops.A, ops.B, ops.sq_a, ops.sq_b, sub, tau)
