"""The hand-written f32 MFMA GEMM (mke_gemm_f32) against float64 matmul: every operand orientation the attribute step
uses, ragged sizes, split-K accumulation."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,N,K,ta,tb,splits", [(5000, 75, 300, False, False, 1), (300, 75, 5000, True, False, 32),
                                                (5000, 300, 75, False, True, 1), (1, 1, 1, False, False, 1),
                                                (65, 33, 17, True, True, 1), (128, 64, 64, False, False, 4),
                                                (37, 300, 1024, True, False, 7),
                                                # 16-byte-load kernel (k_gemm_vec), the four operand layouts, ragged M / N / K edges
                                                (5000, 1024, 1500, False, False, 1), (1500, 1024, 5000, True, False, 4),
                                                (5000, 1024, 512, False, True, 1), (516, 260, 1028, True, True, 3),
                                                (68, 72, 36, False, False, 1), (4, 4, 4, True, True, 1)])
def test_matches_float64(M, N, K, ta, tb, splits):
    from multike_amd import _lib
    g = torch.Generator(device="cuda"); g.manual_seed(M + N + K)
    a = torch.randn((K, M) if ta else (M, K), device="cuda", generator=g)
    b = torch.randn((N, K) if tb else (K, N), device="cuda", generator=g)
    out = torch.zeros(M, N, device="cuda")
    _lib.gemm_f32(a, b, out, transpose_a=ta, transpose_b=tb, splits=splits, accumulate=splits > 1)
    ref = (a.t() if ta else a).double() @ (b.t() if tb else b).double()
    scale = float(ref.abs().max()) + 1e-30
    assert float((out.double() - ref).abs().max()) / scale < 5e-6
    # accumulate on top of an existing C
    base = torch.randn(M, N, device="cuda", generator=g)
    out2 = base.clone()
    _lib.gemm_f32(a, b, out2, transpose_a=ta, transpose_b=tb, splits=splits, accumulate=True)
    assert float((out2.double() - (base.double() + ref)).abs().max()) / scale < 5e-6


def test_asymmetric_operand_catches_transposition():
    """A = I check with an ASYMMETRIC B (guide: a symmetric B would hide a row/col swap in the C write)."""
    from multike_amd import _lib
    n = 96
    b = torch.arange(n * n, dtype=torch.float32, device="cuda").reshape(n, n) / 1000.0
    out = torch.empty(n, n, device="cuda")
    _lib.gemm_f32(torch.eye(n, device="cuda"), b, out)
    assert torch.equal(out, b)


# ---------------------------------------------------------------------------------------------------------------------------
# Exact tests (gemm_cases.py): integer operands whose every partial sum is exactly representable, so the device result must
# EQUAL the float64 product; operands embedded in NaN-poisoned buffers, C in a sentinel-filled one.
@functools.lru_cache(maxsize=2)
def _problem(c):
    A, B, C0 = gc.operands(c)
    return A, B, C0, gc.reference(A, B)


def _device_views(c, A, B, c_init):
    """(a view, b view, c buffer, c view): logical [M, K] / [K, N] / [M, N] views of the flat poisoned device buffers."""
    abuf, pa = gc.embed(A, c.a)
    bbuf, pb = gc.embed(B, c.b)
    cbuf, pc = gc.embed(c_init, c.c, gc.SENTINEL)
    dev = lambda x: torch.as_tensor(x, device="cuda")
    abuf, bbuf, cbuf = dev(abuf), dev(bbuf), dev(cbuf)
    assert abuf.data_ptr() % 16 == 0 and bbuf.data_ptr() % 16 == 0      # the dispatch predicate of the table assumes it
    return gc.view(abuf, c.M, c.K, pa), gc.view(bbuf, c.K, c.N, pb), cbuf, gc.view(cbuf, c.M, c.N, pc)


def _run_exact(c, accumulate):
    """One launch; the logical result must equal the float64 one and everything else in C's buffer must be untouched."""
    from multike_amd import _lib
    A, B, C0, ref = _problem(c._replace(name="", splits=1, c=gc.Lay()))   # operands do not depend on these
    start = C0 if accumulate else np.full_like(C0, gc.SENTINEL)        # a plain store must overwrite whatever was there
    a, b, cbuf, out = _device_views(c, A, B, start)
    before = cbuf.clone()
    _lib.gemm_f32(a, b, out, splits=c.splits if accumulate else 1, accumulate=accumulate)
    want = torch.as_tensor(((C0.astype(np.float64) + ref) if accumulate else ref).astype(np.float32), device="cuda")
    assert not bool(torch.isnan(out).any()), "poison reached the result"
    assert torch.equal(out, want), (c.name, int((out != want).sum()), float((out - want).abs().max()))
    out.copy_(before.as_strided(out.shape, out.stride(), out.storage_offset()))
    assert torch.equal(cbuf.view(torch.int32), before.view(torch.int32)), "C was written outside [M, N]"


@pytest.mark.parametrize("c", gc.EXISTING, ids=lambda c: c.id)
def test_existing_shapes_exact(c):
    """The shapes of test_matches_float64 with integer operands: plain store, accumulation onto an integer C, split-K."""
    _run_exact(c, accumulate=False)
    _run_exact(c._replace(splits=1), accumulate=True)
    if c.splits > 1:
        _run_exact(c, accumulate=True)


@pytest.mark.parametrize("c", gc.VEC_RAGGED, ids=lambda c: c.id)
def test_vec_kernel_ragged_over_poison(c):
    """k_gemm_vec, the four operand orientations, with K % 4 != 0, M % 4 != 0, N % 4 != 0: the 16-byte loads that straddle a
    logical edge read NaN, which the K-edge component masks must discard and the M / N clamps must keep out of stored rows."""
    assert c.vec
    if c.splits == 1:
        _run_exact(c, accumulate=False)
    _run_exact(c, accumulate=True)


@pytest.mark.parametrize("c", gc.DWORD_RAGGED, ids=lambda c: c.id)
def test_dword_kernel_forced(c):
    """The same logical problems pushed off the 16-byte path: a base 1-3 floats off, ld % 4 != 0, neither stride 1."""
    assert not c.vec
    if c.splits == 1:
        _run_exact(c, accumulate=False)
    _run_exact(c, accumulate=True)


@pytest.mark.parametrize("c", gc.SPLITK, ids=lambda c: c.id)
def test_split_k_edges(c):
    """splits of 2, 7, 32, 64 on K of 1, 17, 32, 33, 1000, 1028, both kernels: fewer K slices than requested splits, a ragged
    last split, single-slab splits, K below one slab."""
    _run_exact(c, accumulate=True)


@pytest.mark.parametrize("vec", [True, False])
def test_ldc_wider_than_n(vec):
    """ldc > N with rows behind M in the buffer: pad columns and trailing rows keep the sentinel bit for bit."""
    for extra in (1, 4, 37):
        c = gc.make_case(f"ldc+{extra}", 129, 65, 97, gc.Lay("pad", False, 0 if vec else 1), gc.Lay("pad", False, 4),
                     gc.Lay("pad", False, extra), 1)
        assert c.vec == vec and gc.place(c.M, c.N, c.c).rs > c.N
        _run_exact(c, accumulate=False)
        _run_exact(c._replace(splits=3), accumulate=True)


def test_error_contract():
    from multike_amd import _lib
    import ctypes as C
    a = torch.ones(8, 8, device="cuda")
    out = torch.full((8, 8), gc.SENTINEL, device="cuda")
    with pytest.raises(_lib.MultiKEHipError, match="accumulate"):
        _lib.gemm_f32(a, a, out, splits=2, accumulate=False)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda ldc, M, N, K: _lib.lib().mke_gemm_f32(p(a), C.c_int64(8), C.c_int64(1), p(a), C.c_int64(8), C.c_int64(1), p(out),
                                                         C.c_int64(ldc), C.c_int(M), C.c_int(N), C.c_int(K), C.c_int(1), C.c_int(0), None)
    assert call(7, 8, 8, 8) != 0 and b"ldc" in _lib.lib().mke_last_error()
    for M, N, K in ((-1, 8, 8), (8, -1, 8), (8, 8, -1)):
        assert call(8, M, N, K) != 0 and b"negative" in _lib.lib().mke_last_error()
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())                              # a refused call launches nothing
    assert call(8, 0, 8, 8) == 0 and call(8, 8, 8, 8) == 0               # empty is fine; the same call with good sizes runs
    torch.cuda.synchronize()
    assert bool((out == 8.0).all())
