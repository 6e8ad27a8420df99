"""The reference-alone half of the exact GEMM tests (gemm_cases.py): for every case of the table, the exactness bound holds
and float32 arithmetic on the case's operands — in two different summation orders — already equals the float64 product, so
`torch.equal` against it is a fair demand on the device kernels.  Also pins the factory itself: layouts, poison, dispatch
predicate.  Runs without a GPU."""
import numpy as np
import pytest

import gemm_cases as gc

MAX_MNK = 1 << 26       # larger cases are checked on a sample of A's rows


def _sampled(c):
    A, B, C0 = gc.operands(c)
    if c.M * c.N * c.K > MAX_MNK:
        rows = np.random.default_rng(c.M).choice(c.M, 48, replace=False)
        A, C0 = A[rows], C0[rows]
    return A, B, C0


def test_table_is_complete():
    names = [c.name for c in gc.ALL_CASES]
    assert len(set(names)) == len(names)
    vec = [c for c in gc.VEC_RAGGED]
    assert {(c.a.trans, c.b.trans) for c in vec} == set(gc.ORIENT)
    for o in gc.ORIENT:     # every orientation sees every K residue, K below a slab, just past one, and split-K
        mine = [c for c in vec if (c.a.trans, c.b.trans) == o]
        assert {c.K % 4 for c in mine} >= {1, 2, 3}
        assert {c.K for c in mine} >= {33, 63, 65} and min(c.K for c in mine) < 32 and any(c.splits > 1 for c in mine)
        assert {c.M for c in mine} >= {1, 63, 64, 65, 129} and {c.N for c in mine} >= {1, 63, 64, 65, 129}
    assert {(c.K, c.splits, c.vec) for c in gc.SPLITK} == {(K, s, v) for K in (1, 17, 32, 33, 1000, 1028) for s in (2, 7, 32, 64)
                                                           for v in (True, False)}
    dw = gc.DWORD_RAGGED
    assert {c.a.offset for c in dw} | {c.b.offset for c in dw} >= {1, 2, 3}
    assert any(c.a.kind == "strided" and c.a.trans for c in dw) and any(c.a.kind == "strided" and not c.a.trans for c in dw)
    assert [(c.M, c.N, c.K, c.a.trans, c.b.trans, c.splits) for c in gc.EXISTING] == gc.EXISTING_SHAPES


@pytest.mark.parametrize("c", gc.ALL_CASES, ids=lambda c: c.id)
def test_case_is_exact_in_float32(c):
    assert c.L * c.L * c.K + gc.C_MAX < 2 ** 24
    assert c.L * c.L * c.K < 2 ** 24
    A, B, C0 = _sampled(c)
    assert np.abs(A).max() <= c.L and np.abs(B).max() <= c.L and np.abs(C0).max() <= gc.C_MAX
    assert np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B))
    ref = gc.reference(A, B)
    assert np.abs(ref).max() + gc.C_MAX < 2 ** 24
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)
    assert np.array_equal(A @ B, ref32)                              # float32 matmul, forward
    assert np.array_equal(A[:, ::-1] @ B[::-1], ref32)               # and with K reversed
    assert np.array_equal(C0 + A @ B, (C0.astype(np.float64) + ref).astype(np.float32))


@pytest.mark.parametrize("c", gc.ALL_CASES, ids=lambda c: c.id)
def test_case_layout_and_dispatch(c):
    """The embedded operands read back as the logical matrices, everything else in the buffers is poison, and the case lands
    on the kernel it was built for."""
    pa, pb, pc = gc.place(c.M, c.K, c.a), gc.place(c.K, c.N, c.b), gc.place(c.M, c.N, c.c)
    assert gc.takes_vec_kernel(c.M, c.N, c.K, pa, pb) == c.vec
    assert pc.cs == 1 and pc.rs >= c.N and pc.offset == 0
    if c.vec and c.a.kind == "pad":        # the 16-byte-load cases over poison: ld = pad4(extent) + {0, 4, 8}
        for p, ext in ((pa, c.M if c.a.trans else c.K), (pb, c.K if c.b.trans else c.N)):
            assert max(p.rs, p.cs) - gc.pad4(ext) in (0, 4, 8)
    if c.M * c.N * c.K > MAX_MNK:
        return
    A, B, C0 = gc.operands(c)
    for mat, lay in ((A, c.a), (B, c.b)):
        buf, p = gc.embed(mat, lay)
        assert np.array_equal(gc.view(buf, *mat.shape, p), mat)
        assert np.isnan(buf).sum() == buf.size - mat.size and np.isnan(buf[-1])
    buf, p = gc.embed(C0, c.c, gc.SENTINEL)
    assert (buf == gc.SENTINEL).sum() == buf.size - C0.size


@pytest.mark.parametrize("M,K,N", [(50, 301, 75), (129, 75, 33), (64, 150, 70)])
def test_dyadic_preactivation_is_exact(M, K, N):
    x, w, b = gc.dyadic_operands(M, K, N, 0)
    p64 = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    assert np.array_equal((x @ w + b).astype(np.float64), p64)
    assert np.array_equal(((x[:, ::-1] @ w[::-1]) + b).astype(np.float64), p64)
    assert np.array_equal(p64 * 512, np.rint(p64 * 512)) and np.abs(p64).max() < 6.0     # on the 2^-9 grid, unsaturated
    assert np.abs(np.tanh(p64)).max() < 1.0 - 1e-5 and np.abs(p64).std() > 0.2
