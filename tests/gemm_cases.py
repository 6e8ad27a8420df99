"""Case table and operand factory of the GEMM dispatch tests (test_gemm_cases.py here, test_gemm_gpu.py and
test_gemm_clients_gpu.py on the device).  No GPU code: NumPy only, torch tensors are handled by duck typing.

Exactness.  A and B hold integers in [-L, L] and C (when accumulated onto) integers in [-C_MAX, C_MAX], with
L^2 K + C_MAX < 2^24 for every case.  Every product is an integer of magnitude <= L^2 and every sum of ANY subset of the K
products of one output element, with or without C's entry, is an integer below 2^24 in magnitude — exactly representable in
float32.  So whatever order a kernel adds them in (MFMA chains, the four-wave LDS reduction, split-K atomics) no rounding
happens, and the result must EQUAL the float64 product converted to float32: the tests assert torch.equal, not a tolerance.

Poisoned padding.  An operand is embedded in a larger flat buffer whose every other element is NaN: a kernel that lets a
value from outside the logical matrix reach an accumulator (a wrong K-edge mask of a 16-byte load, a wrong clamp) turns
output elements into NaN.  C is embedded the same way with a finite sentinel that must survive bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

C_MAX = 64
SENTINEL = -12345.0


def pad4(v: int) -> int:
    return (int(v) + 3) // 4 * 4


class Lay(NamedTuple):
    """How one logical [rows, cols] matrix lies in its flat buffer.
    kind 'pad':     row-major (or, trans, column-major) with ld = pad4(contiguous extent) + extra
    kind 'contig':  ld = contiguous extent exactly
    kind 'strided': a `base[::2, ::3]`-style view — neither stride is 1 (trans: of the transposed matrix)
    offset: floats between the (16-byte aligned) buffer start and element (0, 0)."""
    kind: str = "pad"
    trans: bool = False
    extra: int = 0
    offset: int = 0


class Placed(NamedTuple):
    rs: int       # element strides of the LOGICAL matrix: m(i, j) = buf[offset + i rs + j cs]
    cs: int
    offset: int
    size: int     # floats in the flat buffer


def place(rows: int, cols: int, lay: Lay) -> Placed:
    r_s, c_s = (cols, rows) if lay.trans else (rows, cols)      # stored shape
    if lay.kind == "contig":
        s0, s1 = c_s, 1
    elif lay.kind == "pad":
        s0, s1 = pad4(c_s) + lay.extra, 1
    elif lay.kind == "strided":
        s0, s1 = 2 * (3 * c_s + 1), 3
    else:
        raise ValueError(lay.kind)
    size = lay.offset + (r_s + 2) * s0                          # two rows of padding behind the last stored row
    rs, cs = (s1, s0) if lay.trans else (s0, s1)
    return Placed(rs, cs, lay.offset, size)


def view(buf, rows: int, cols: int, p: Placed):
    """The logical [rows, cols] view of a flat buffer (numpy array or torch tensor)."""
    if isinstance(buf, np.ndarray):
        it = buf.itemsize
        return np.lib.stride_tricks.as_strided(buf[p.offset:], (rows, cols), (p.rs * it, p.cs * it))
    return buf.as_strided((rows, cols), (p.rs, p.cs), p.offset)


def embed(mat: np.ndarray, lay: Lay, fill=np.nan):
    """(flat float32 buffer full of `fill` with `mat` at its place, Placed)."""
    rows, cols = mat.shape
    p = place(rows, cols, lay)
    buf = np.full(p.size, fill, dtype=np.float32)
    view(buf, rows, cols, p)[...] = mat
    return buf, p


def takes_vec_kernel(M, N, K, pa: Placed, pb: Placed) -> bool:
    """The host dispatcher's choice (launch_gemm_f32_ex) for 16-byte aligned buffer starts: True = k_gemm_vec."""
    a_kc, b_nc = pa.cs == 1, pb.cs == 1
    a_mc, b_kc = pa.rs == 1 and not a_kc, pb.rs == 1 and not b_nc
    if not ((a_kc or a_mc) and (b_nc or b_kc)) or pa.offset % 4 or pb.offset % 4:
        return False
    ok_a = (pa.rs % 4 == 0 and pad4(K) <= pa.rs) if a_kc else (pa.cs % 4 == 0 and pad4(M) <= pa.cs)
    ok_b = (pb.cs % 4 == 0 and pad4(K) <= pb.cs) if b_kc else (pb.rs % 4 == 0 and pad4(N) <= pb.rs)
    return ok_a and ok_b


class Case(NamedTuple):
    name: str
    M: int
    N: int
    K: int
    a: Lay
    b: Lay
    c: Lay
    splits: int
    L: int
    vec: bool      # the kernel the case is built to reach: k_gemm_vec (True) or the dword kernel k_gemm_f32

    @property
    def id(self):
        return self.name


def magnitude(K: int) -> int:
    return 8 if K <= 2048 else 4


def operands(c: Case):
    """Integer A [M, K], B [K, N], C0 [M, N] as float32 arrays, deterministic per case."""
    rng = np.random.default_rng([c.M, c.N, c.K, int(c.a.trans), int(c.b.trans)])
    A = rng.integers(-c.L, c.L + 1, (c.M, c.K)).astype(np.float32)
    B = rng.integers(-c.L, c.L + 1, (c.K, c.N)).astype(np.float32)
    C0 = rng.integers(-C_MAX, C_MAX + 1, (c.M, c.N)).astype(np.float32)
    return A, B, C0


def reference(A, B) -> np.ndarray:
    return A.astype(np.float64) @ B.astype(np.float64)


def make_case(name, M, N, K, a, b, c=Lay("contig"), splits=1, vec=None):
    pa, pb = place(M, K, a), place(K, N, b)
    return Case(name, M, N, K, a, b, c, splits, magnitude(K), takes_vec_kernel(M, N, K, pa, pb) if vec is None else vec)


# --- the shapes test_gemm_gpu.py::test_matches_float64 has always run, contiguous as there --------------------------------
EXISTING_SHAPES = [(5000, 75, 300, False, False, 1), (300, 75, 5000, True, False, 32), (5000, 300, 75, False, True, 1),
                   (1, 1, 1, False, False, 1), (65, 33, 17, True, True, 1), (128, 64, 64, False, False, 4),
                   (37, 300, 1024, True, False, 7), (5000, 1024, 1500, False, False, 1), (1500, 1024, 5000, True, False, 4),
                   (5000, 1024, 512, False, True, 1), (516, 260, 1028, True, True, 3), (68, 72, 36, False, False, 1),
                   (4, 4, 4, True, True, 1)]
EXISTING = [make_case(f"{M}x{N}x{K}-{'t' if ta else 'n'}{'t' if tb else 'n'}-s{s}", M, N, K, Lay("contig", ta), Lay("contig", tb), splits=s)
            for M, N, K, ta, tb, s in EXISTING_SHAPES]

# --- ragged logical problems: K % 4 in {1, 2, 3}, K below a slab, just past one or two, M / N edges 1, 63, 64, 65, 129 -----
RAGGED = [  # (M, N, K, splits)
    (63, 65, 1, 1), (1, 129, 2, 1), (129, 1, 3, 1), (65, 63, 5, 1), (64, 64, 17, 1), (63, 63, 30, 1), (65, 129, 31, 1),
    (129, 65, 33, 1), (1, 1, 63, 1), (63, 129, 65, 1), (65, 65, 65, 2), (129, 63, 97, 3), (37, 50, 130, 1), (63, 65, 161, 4),
    (129, 129, 255, 2), (70, 75, 301, 1), (65, 33, 1030, 7)]
ORIENT = [(False, False), (False, True), (True, False), (True, True)]
_ot = lambda ta, tb: ("t" if ta else "n") + ("t" if tb else "n")

# 16-byte-load kernel: aligned bases, ld = pad4(extent) + {0, 4, 8}, NaN in every pad
VEC_RAGGED = []
for i, (M, N, K, s) in enumerate(RAGGED):
    for j, (ta, tb) in enumerate(ORIENT):
        ea, eb, ec = (0, 4, 8)[(i + j) % 3], (0, 4, 8)[(i + 2 * j + 1) % 3], (0, 4, 8)[(i + j + 2) % 3]
        VEC_RAGGED.append(make_case(f"vec-{M}x{N}x{K}-{_ot(ta, tb)}-s{s}", M, N, K, Lay("pad", ta, ea), Lay("pad", tb, eb),
                                    Lay("pad", False, ec), s, vec=True))

# the same logical problems forced onto the dword kernel: base offset 1..3 floats / ld % 4 != 0 / neither stride 1
DWORD_RAGGED = []
for i, (M, N, K, s) in enumerate(RAGGED):
    ta, tb = ORIENT[(i // 4 + i) % 4]      # every way of forcing meets every orientation
    how = i % 4
    if how == 0:     # A's base off by 1..3 floats, everything else as the vec kernel wants it
        a, b, tag = Lay("pad", ta, 4, 1 + i % 3), Lay("pad", tb, 0), "offA"
    elif how == 1:   # B's base
        a, b, tag = Lay("pad", ta, 0), Lay("pad", tb, 4, 1 + i % 3), "offB"
    elif how == 2:   # leading dimension not a multiple of 4
        a, b, tag = Lay("pad", ta, 1 + i % 3), Lay("pad", tb, 8), "ldA"
    else:
        a, b, tag = Lay("pad", ta, 4), Lay("pad", tb, 1 + i % 3), "ldB"
    DWORD_RAGGED.append(make_case(f"dw-{tag}-{M}x{N}x{K}-{_ot(ta, tb)}-s{s}", M, N, K, a, b, Lay("pad", False, 4), s, vec=False))
for i, (M, N, K, s) in enumerate(RAGGED[3::3]):
    # general strides: a[::2, ::3]-style views, plain and transposed, against every layout of the other operand
    ta, tb = ORIENT[i % 4]
    DWORD_RAGGED.append(make_case(f"dw-strA-{M}x{N}x{K}-{_ot(ta, tb)}-s{s}", M, N, K, Lay("strided", ta), Lay("pad", tb, 4),
                                  Lay("pad", False, 0), s, vec=False))
    DWORD_RAGGED.append(make_case(f"dw-strAB-{M}x{N}x{K}-{_ot(tb, ta)}-s{s}", M, N, K, Lay("strided", tb, 0, i % 4),
                                  Lay("strided", ta, 0, (i + 1) % 4), Lay("pad", False, 8), s, vec=False))

# --- split-K edges on both kernels: gz < splits, a ragged last split, a split of one slab, K < 32 with splits > 1 -----------
SPLITK = []
for K in (1, 17, 32, 33, 1000, 1028):
    for s in (2, 7, 32, 64):
        ta, tb = ORIENT[(K + s) % 4]
        SPLITK.append(make_case(f"vec-splitk-K{K}-s{s}-{_ot(ta, tb)}", 65, 33, K, Lay("pad", ta, 4), Lay("pad", tb, 0),
                                Lay("pad", False, 4), s, vec=True))
        SPLITK.append(make_case(f"dw-splitk-K{K}-s{s}-{_ot(ta, tb)}", 65, 33, K, Lay("pad", ta, 1), Lay("pad", tb, 0, 2),
                                Lay("pad", False, 4), s, vec=False))

ALL_CASES = EXISTING + VEC_RAGGED + DWORD_RAGGED + SPLITK


# --- dyadic operands for the activation epilogue ---------------------------------------------------------------------------
def dyadic_operands(M: int, K: int, N: int, seed: int):
    """x in multiples of 1/8 within [-1, 1], w in multiples of 1/64 within [-1/8, 1/8], bias in multiples of 1/64 within
    [-1/2, 1/2]: every term of x w + bias is a multiple of 2^-9 and every partial sum stays below 2^6 for K <= 4096 — 15
    significant bits, so the pre-activation is exact in float32 in any order; its spread (~ 0.05 sqrt(K)) keeps tanh and
    the sigmoid away from saturation."""
    assert K <= 4096
    rng = np.random.default_rng([M, K, N, seed])
    x = (rng.integers(-8, 9, (M, K)) / 8.0).astype(np.float32)
    w = (rng.integers(-8, 9, (K, N)) / 64.0).astype(np.float32)
    b = (rng.integers(-32, 33, N) / 64.0).astype(np.float32)
    return x, w, b
