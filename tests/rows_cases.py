"""Case table, operand factories and float64 references of the exact row-kernel tests (test_rows_cases.py here,
test_rows_exact_gpu.py on the device): the kernels of multike_amd/csrc/mke_rows.hip.  No GPU code: NumPy only.

Exactness.  Every entry of an exact case is a multiple of 1/4 in [-L, L] (L = 1; the saturated logistic tier at dim < 15 needs
L = 4, see `glog_ops`), every weight and learning rate a power of two.  All values a kernel forms are then integer multiples of
a power of two, the case's `unit`: differences of entries (1/4), their squares (1/16), weighted gradient rows (2 w / 4).  A sum of
such values is exact in float32 in ANY order if the sum of the ABSOLUTE values of its terms, divided by the unit, stays below
2^24: every partial sum of every order is a multiple of the unit and bounded by that sum.  `Bound.add` records one such
(sum of absolute values, unit) pair per kind of intermediate the kernel forms, for the worst element of the case:

  chain    the per-lane fma chain over the FPL floats of a lane and the 16-lane sum behind it (one row's squared distance:
           non-negative terms, so the row total bounds every partial sum),
  thread   the float accumulation of one thread over the rows of all its grid passes (a grid of G blocks of 16 rows gives row i
           to quarter-wave i mod 16 G),
  atomic   the sum over all duplicates of one gradient row, from both sides where the two sides share the array,
  value    a table entry after an SGD step (mke_align_steps).

`Bound.check()` asserts all of them, so no rounding happens anywhere and the device result must EQUAL the float64 reference
converted to float32.  The block sums (double), the partial sums and the weight factor of the loss are exact as well: sums of
multiples of 2^-k far below 2^53.

Poison.  Dense operands [n, ld] lie in [n + 1, ld] buffers with NaN in columns [dim, ld) and in the tail row; gradient buffers
have the same shape and hold SENTINEL everywhere, so a row that is skipped, a column past dim that is written and a row past n
all show.  Nothing lies outside the buffers: a guard that fails reads NaN from inside them.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

FPLS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 20)          # MKE_DISPATCH_FPL
STRIDES = tuple(16 * f for f in FPLS)
# the dims the dense kernels are held at, and six more: 48, 64, 96 and 112 are the only way to the instantiations FPL = 3, 4, 6, 7
# (dense_fpl never rounds up to them), 240 and 288 need 15 and 18 floats per lane (rounded up to 16 and 20)
DENSE_DIMS = (1, 15, 16, 17, 48, 64, 75, 96, 112, 128, 129, 144, 145, 176, 177, 208, 209, 240, 256, 257, 288, 304, 320)
LD_EXTRA = (0, 3, 16)
COUNTS = (0, 1, 15, 16, 17, 255, 257)
LOSS_BLOCKS = 2048                                            # MKE_LOSS_PARTIALS: grid of the loss kernels
ROW_BLOCKS_MAX = 4096                                         # grid_for_rows: grid cap of gather / probe
SUBS = 16                                                     # rows per block (MKE_BLOCK / 16)
PASS_LOSS = (LOSS_BLOCKS * SUBS, LOSS_BLOCKS * SUBS + 1, 70001)          # 32,768 / 32,769 / a third pass
PASS_ROWS = (ROW_BLOCKS_MAX * SUBS, ROW_BLOCKS_MAX * SUBS + 1, 140001)   # 65,536 / 65,537 / a third pass
SENTINEL = -12345.0
TAG, OLD_TAG = 7, 3
L2_EPS = 1e-12
ALIGN_PATTERNS = ("same", "diff", "dup", "shared", "self", "no_ga", "no_gb", "loss_only")
WEIGHTS = (0.5, 1.0, 2.0, 0.25)
SAT_POS, SAT_NEG = 32, 128                                    # x at and above which softplus / sigmoid are exact (sign +1 / -1)


def dense_fpl(dim: int) -> int:
    need = (dim + 15) // 16
    return [f for f in FPLS if f >= need][0]


def table_dims(stride: int):
    return (stride, stride - 1, stride - 15) + ((75,) if stride == 80 else ())


def passes(n: int, blocks: int) -> int:
    """Rows one quarter-wave visits at most."""
    return max(1, -(-n // (blocks * SUBS)))


class Case(NamedTuple):
    kernel: str          # galign | glog | gather | probe | align | steps
    n: int               # rows of the launch (batch entries)
    dim: int
    width: int           # ld of the dense kernels, stride of the table kernels
    variant: str = ""    # galign: grad / nograd; glog: w / now / nograd_w / nograd_now; gather: copy / norm; probe: a / ab / abc;
    #                      align: one of ALIGN_PATTERNS
    sign: int = 0        # glog
    idx: str = ""        # gather: null / rep
    rows: int = 0        # rows of the table(s)
    weight: float = 1.0  # align
    tag: str = ""

    @property
    def id(self):
        s = f"{self.kernel}-d{self.dim}-w{self.width}-n{self.n}"
        for v in (self.variant, self.idx, f"s{self.sign:+d}" if self.sign else "", f"r{self.rows}" if self.rows else "",
                  f"w{self.weight}" if self.kernel == "align" else "", self.tag):
            if v:
                s += "-" + v
        return s


class Bound:
    """(sum of absolute values, unit) of every kind of intermediate; check() asserts each fits 24 bits."""

    def __init__(self):
        self.items = []

    def add(self, what: str, sum_abs: float, unit: float):
        self.items.append((what, float(sum_abs), float(unit)))

    def check(self):
        assert self.items
        for what, s, u in self.items:
            assert u > 0 and np.log2(u) == np.rint(np.log2(u)), (what, u)
            assert s / u < 2 ** 24, f"{what}: {s} / {u} = 2^{np.log2(max(s / u, 1)):.1f} does not fit 24 bits"


def _rng(c: Case, salt=0):
    name = zlib.crc32((c.kernel + "/" + c.variant + "/" + c.idx + "/" + c.tag).encode())
    return np.random.default_rng([name, c.n, c.dim, c.width, c.sign + 1, c.rows, salt])


def quarters(rng, shape, L=1):
    """float64 multiples of 1/4 in [-L, L]."""
    return rng.integers(-4 * L, 4 * L + 1, shape).astype(np.float64) / 4.0


def is_quarters(a, L=1):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a * 4, np.rint(a * 4)) and (a.size == 0 or np.abs(a).max() <= L))


def poisoned(mat: np.ndarray, ld: int) -> np.ndarray:
    """float32 [n + 1, ld]: mat in [:n, :dim], NaN in the pad columns and in the tail row."""
    n, d = mat.shape
    buf = np.full((n + 1, ld), np.nan, dtype=np.float32)
    buf[:n, :d] = mat
    return buf


def sentinel_buffer(n: int, ld: int) -> np.ndarray:
    return np.full((n + 1, ld), SENTINEL, dtype=np.float32)


def padded_table(mat: np.ndarray, stride: int) -> np.ndarray:
    """float32 [rows, stride]: mat in the first dim columns, zeros behind (the ABI's padding)."""
    buf = np.zeros((mat.shape[0], stride), dtype=np.float32)
    buf[:, :mat.shape[1]] = mat
    return buf


# ----------------------------------------------------------------------------------------------------- float32 in two orders
def rowsum32(M: np.ndarray, order: str) -> np.ndarray:
    """Row sums of a float32 matrix, one float32 addition at a time.  "lanes": the kernels' order (lane j adds its columns
    j, j + 16, ... in turn, then the butterfly over the 16 lanes); "reverse": last column to first."""
    M = np.ascontiguousarray(M, dtype=np.float32)
    n, cols = M.shape
    if order == "reverse":
        s = np.zeros(n, dtype=np.float32)
        for k in range(cols - 1, -1, -1):
            s = s + M[:, k]
        return s
    assert order == "lanes"
    f = (cols + 15) // 16
    P = np.zeros((n, f * 16), dtype=np.float32)
    P[:, :cols] = M
    P = P.reshape(n, f, 16)
    lane = np.zeros((n, 16), dtype=np.float32)
    for k in range(f):
        lane = lane + P[:, k, :]
    for perm in ([1, 0, 3, 2], [2, 3, 0, 1]):                       # quad_perm
        ix = np.arange(16) // 4 * 4 + np.tile(perm, 4)
        lane = lane + lane[:, ix]
    lane = lane + lane[:, np.arange(16) // 8 * 8 + (7 - np.arange(16) % 8)]     # row_half_mirror
    lane = lane + lane[:, 15 - np.arange(16)]                                   # row_mirror
    assert lane.dtype == np.float32
    return lane[:, 0].copy()


def thread_sums32(terms: np.ndarray, blocks: int, order: str, dtype=np.float32) -> np.ndarray:
    """[blocks * SUBS]: what each quarter-wave accumulates over its grid passes (first pass first, or last first), in float32."""
    terms = np.asarray(terms, dtype=dtype)
    nsub = blocks * SUBS
    acc = np.zeros(nsub, dtype=dtype)
    chunks = [terms[lo:lo + nsub] for lo in range(0, len(terms), nsub)]
    for ch in (chunks if order == "lanes" else chunks[::-1]):
        acc[:len(ch)] = acc[:len(ch)] + ch
    return acc


def thread_max(terms: np.ndarray, blocks: int) -> float:
    """Largest float64 sum of the absolute values one quarter-wave accumulates."""
    return float(thread_sums32(np.abs(terms), blocks, "lanes", np.float64).max())


def scatter32(idx, G: np.ndarray, rows: int, order: str, into=None) -> np.ndarray:
    """float32 scatter-add of the rows of G, batch order or reversed (np.add.at adds one entry at a time, in float32)."""
    out = np.zeros((rows, G.shape[1]), dtype=np.float32) if into is None else into
    idx = np.asarray(idx, dtype=np.int64)
    G = np.asarray(G, dtype=np.float32)
    if order == "reverse":
        idx, G = idx[::-1], G[::-1]
    np.add.at(out, idx, G)
    assert out.dtype == np.float32
    return out


def max_scatter_abs(idx_list, G_list, rows: int) -> float:
    """Largest sum of absolute values that lands on one gradient element."""
    tot = np.zeros((rows, G_list[0].shape[1]))
    for idx, G in zip(idx_list, G_list):
        np.add.at(tot, np.asarray(idx, dtype=np.int64), np.abs(G))
    return float(tot.max()) if tot.size else 0.0


# ----------------------------------------------------------------------------------------------------- gathered alignment
class GAlignOps(NamedTuple):
    a: np.ndarray        # float64 [n, dim]
    b: np.ndarray
    loss: float          # float64
    ga: np.ndarray       # float64 [n, dim]; gb == -ga
    bound: Bound


@functools.lru_cache(maxsize=8)
def galign_ops(c: Case) -> GAlignOps:
    rng = _rng(c)
    a, b = quarters(rng, (c.n, c.dim)), quarters(rng, (c.n, c.dim))
    if c.n > 2:
        b[1] = a[1]                                   # a row at distance zero
        a[2], b[2] = 1.0, -1.0                        # the largest distance: 4 dim
    d = a - b
    x = (d * d).sum(1)
    bd = Bound()
    # |d| <= 2 in quarters: d^2 <= 4 in sixteenths; a row's x <= 4 dim; a thread adds `passes` of them; ga = 2 d
    assert c.dim * 4 * 16 * passes(c.n, LOSS_BLOCKS) < 2 ** 24
    bd.add("chain", x.max() if c.n else 0.0, 1 / 16)
    bd.add("thread", thread_max(x, LOSS_BLOCKS), 1 / 16)
    return GAlignOps(a, b, float(x.sum()), 2.0 * d, bd)


# ----------------------------------------------------------------------------------------------------- gathered logistic
class GLogOps(NamedTuple):
    h: np.ndarray        # float64 [n, dim]
    r: np.ndarray
    t: np.ndarray
    w: np.ndarray        # float64 [n] (powers of two), or None
    x: np.ndarray        # float64 [n]: ||h + r - t||^2, integers
    loss: float
    gh: np.ndarray       # float64 [n, dim]; gr == gh, gt == -gh
    L: int
    bound: Bound


def glog_L(dim: int) -> int:
    """Operand range of the saturated tier.  |h + r - t| <= 3 L per column, so x <= 9 L^2 dim; x >= 128 needs L = 1 from
    dim 15 on (135) and L = 4 below (dim 1: 144)."""
    return 1 if 9 * dim >= SAT_NEG else 4


@functools.lru_cache(maxsize=8)
def glog_ops(c: Case) -> GLogOps:
    """Saturated tier: every row has an INTEGER x = ||h + r - t||^2 >= 32 (sign +1) or >= 128 (sign -1).  With
    softplus_f(z) = max(z, 0) + log(1 + exp(-|z|)) and sigmoid_f(z) = rcp(1 + exp(-z)) in float32: exp(-32) < 2^-25, so
    1 + exp(-x) rounds to 1 and the term is w x, the gradient 2 w (h + r - t) (sign +1); exp(128) overflows to infinity, whose
    reciprocal is 0, and the term and the gradient rows are 0 (sign -1)."""
    rng = _rng(c)
    L = glog_L(c.dim)
    thr = SAT_POS if c.sign > 0 else SAT_NEG
    h, r = quarters(rng, (c.n, c.dim), L), quarters(rng, (c.n, c.dim), L)
    t0 = rng.integers(-4 * L + 2, 4 * L - 1, (c.n, c.dim)).astype(np.float64) / 4.0      # |t0| <= L - 1/2
    e = np.rint(h + r - t0)                           # integer differences: |t - t0| <= 1/2 keeps t in [-L, L]
    t = h + r - e
    x = (e * e).sum(1)
    low = x < thr                                     # rows short of the threshold: +-3 L in every column
    if low.any():
        s = rng.choice([-1.0, 1.0], (int(low.sum()), c.dim))
        h[low], r[low], t[low] = L * s, L * s, -L * s
    e = h + r - t
    x = (e * e).sum(1)
    assert np.array_equal(e, np.rint(e)) and (c.n == 0 or x.min() >= thr) and 9 * L * L * c.dim >= thr
    w = None
    if c.variant.endswith("w") and not c.variant.endswith("now"):
        w = 2.0 ** -rng.integers(0, 3, c.n).astype(np.float64)
    wv = np.ones(c.n) if w is None else w
    if c.sign > 0:
        term, gh = wv * x, 2.0 * wv[:, None] * e
    else:
        term, gh = np.zeros(c.n), np.zeros((c.n, c.dim))
    bd = Bound()
    assert 9 * L * L * c.dim * 16 * 4 * passes(c.n, LOSS_BLOCKS) < 2 ** 24    # x in sixteenths, w x in quarters of that
    bd.add("chain", x.max() if c.n else 0.0, 1 / 16)
    bd.add("thread", thread_max(wv * x, LOSS_BLOCKS), 1 / 4)
    bd.add("gradient", np.abs(2.0 * wv[:, None] * e).max() if c.n else 0.0, 1 / 4)
    return GLogOps(h, r, t, w, x, float(term.sum()), gh, L, bd)


class GLogGeneric(NamedTuple):
    h: np.ndarray        # float32 [n, dim]
    r: np.ndarray
    t: np.ndarray
    w: np.ndarray        # float32 [n]
    x: np.ndarray        # float64 [n] of the float32 operands
    terms: np.ndarray    # float64 [n]
    loss: float
    gh: np.ndarray       # float64; gr == gh, gt == -gh
    extreme: np.ndarray  # bool [n]: rows with |z| in [80, 110]
    zero: np.ndarray     # bool [n]: rows with (h + r) - t == 0 in float32 (x below 1e-13 in float64)


def glog_generic(dim: int, sign: int, n: int = 257, n_extreme: int = 0) -> GLogGeneric:
    """Tolerance tier: x spread over [0, 4] (with x = 0 rows: term ln 2, sigmoid 1/2), weights in [0.25, 1]; n_extreme rows
    behind them with |z| in [80, 110], where exp overflows (sign -1: exp(+x)) or goes denormal (sign +1: exp(-x))."""
    rng = np.random.default_rng([dim, sign + 1, n, n_extreme])
    N = n + n_extreme
    x_t = rng.uniform(0.0, 4.0, N)
    x_t[:n:50] = 0.0
    x_t[1:n:50] = 4.0
    x_t[n:] = np.linspace(80.0, 110.0, n_extreme) if n_extreme else []
    u = rng.standard_normal((N, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    e = u * np.sqrt(x_t)[:, None]
    h = (0.5 * rng.standard_normal((N, dim)) / np.sqrt(dim)).astype(np.float32)
    r = (0.5 * rng.standard_normal((N, dim)) / np.sqrt(dim)).astype(np.float32)
    t = ((h + r).astype(np.float64) - e).astype(np.float32)
    zero = x_t == 0.0
    t[zero] = (h + r)[zero]                              # the float32 sum: (h + r) - t is exactly zero on the device too
    w = rng.uniform(0.25, 1.0, N).astype(np.float32)
    d = h.astype(np.float64) + r.astype(np.float64) - t.astype(np.float64)   # the float32 rounding of h + r is the kernel's error
    x = (d * d).sum(1)
    z = sign * x
    terms = w.astype(np.float64) * np.logaddexp(0.0, z)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-z))
    gh = (2.0 * sign * w.astype(np.float64) * sig)[:, None] * d
    extreme = np.arange(N) >= n
    assert np.all(x[zero] < 1e-13) and zero.sum() >= 2 and x[~extreme].max() <= 4.0 + 1e-5
    assert n_extreme == 0 or (np.abs(z[extreme]).min() >= 79.9 and np.abs(z[extreme]).max() <= 110.1)
    return GLogGeneric(h, r, t, w, x, terms, float(terms.sum()), gh, extreme, zero)


# ----------------------------------------------------------------------------------------------------- gather
class GatherOps(NamedTuple):
    table: np.ndarray    # float32 [rows, stride]: pad columns NaN for the copy, zero for the normalised read
    idx: np.ndarray      # int32 [n] or None
    ref: np.ndarray      # copy: float32 [n, dim] (bit pattern); norm: float64 [n, dim]
    special: dict        # norm: name -> output rows that hold the planted table row (names with none are left out)


@functools.lru_cache(maxsize=8)
def gather_ops(c: Case) -> GatherOps:
    rng = _rng(c)
    rows = c.rows
    special = {}
    if c.variant == "copy":
        mat = quarters(rng, (rows, c.dim)).astype(np.float32)
        table = np.full((rows, c.width), np.nan, dtype=np.float32)    # the copy must not look at the pad
        table[:, :c.dim] = mat
    else:
        mat = (0.3 * rng.standard_normal((rows, c.dim))).astype(np.float32)
        assert rows >= 8
        mat[0] = 0.0                                      # all zero: output exactly zero
        mat[1] = np.float32(2.0 ** -30)                   # squared norm dim 2^-60 < eps: v rsqrt(eps)
        mat[2] = np.float32(1e-25)                        # squares underflow to zero
        mat[3] = 0.0
        mat[3, :min(4, c.dim)] = 0.5 if c.dim >= 4 else 0.0
        if c.dim < 4:
            mat[3, 0] = 1.0                               # norm exactly 1 (four halves, or a single one)
        special = {"zero": 0, "tiny": 1, "underflow": 2, "unit": 3}
        table = padded_table(mat, c.width)
    idx = None
    if c.idx == "rep":
        idx = rng.integers(0, rows, c.n).astype(np.int32)         # with replacement
        if c.n >= 8:
            idx[:4] = np.arange(4)
            idx[-1] = idx[4]                                      # at least one repeated id
    else:
        assert rows >= c.n
    src_rows = np.arange(c.n) if idx is None else idx.astype(np.int64)
    src = mat[src_rows]
    if c.variant == "copy":
        ref = src.copy()
    else:
        m = src.astype(np.float64)
        ref = m / np.sqrt(np.maximum((m * m).sum(1, keepdims=True), L2_EPS))
        special = {k: np.nonzero(src_rows == r)[0] for k, r in special.items()}
        special = {k: v for k, v in special.items() if len(v)}
    return GatherOps(table, idx, ref, special)


# ----------------------------------------------------------------------------------------------------- probe
class ProbeOps(NamedTuple):
    a: np.ndarray        # float32 [rows, stride], every column live
    b: np.ndarray        # or None
    c: np.ndarray        # or None
    idx: np.ndarray      # int32 [n]
    ref: np.ndarray      # float64 [n]
    bound: Bound


@functools.lru_cache(maxsize=8)
def probe_ops(c: Case) -> ProbeOps:
    rng = _rng(c)
    mats = [quarters(rng, (c.rows, c.width)) for _ in range(len(c.variant))]
    idx = rng.integers(0, c.rows, c.n).astype(np.int32)
    tot = sum(mats)
    bd = Bound()
    assert 3 * c.width * 4 < 2 ** 24                              # up to three entries per column, in quarters
    bd.add("chain", sum(np.abs(m) for m in mats).sum(1).max(), 1 / 4)
    f32 = [m.astype(np.float32) for m in mats] + [None, None]
    return ProbeOps(f32[0], f32[1], f32[2], idx, tot.sum(1)[idx], bd)


# ----------------------------------------------------------------------------------------------------- fused alignment term
class AlignOps(NamedTuple):
    ta: np.ndarray       # float32 [rows, stride], pad columns zero
    tb: np.ndarray       # the same array as ta for the "self" pattern
    ia: np.ndarray       # int32 [n]
    ib: np.ndarray
    loss: float          # float64: weight * sum ||A[ia] - B[ib]||^2
    ga: np.ndarray       # float64 [rows, stride] (np.add.at); "self": the one shared array, in ga AND gb
    gb: np.ndarray
    hit_a: np.ndarray    # bool [rows]: rows whose flag must become TAG
    hit_b: np.ndarray
    bound: Bound


def align_ids(c: Case, rng):
    n = c.n
    rows = c.rows if c.tag == "heavy" else c.rows - 2        # the last two rows are never named: their flags must survive
    p = c.variant
    if p == "same":                                   # ia == ib, distinct
        ia = rng.permutation(rows)[:n]
        return ia, ia.copy()
    if p in ("diff", "self"):                         # ia != ib as arrays (distinct ids on each side where they fit)
        if n <= rows:
            ia, ib = rng.permutation(rows)[:n], rng.permutation(rows)[:n]
        else:
            ia, ib = rng.integers(0, rows, n), rng.integers(0, rows, n)
        if n >= 1 and rows >= 2 and np.array_equal(ia, ib):
            ib = (ib + 1) % rows
        if p == "self" and n >= 3:
            ib[0] = ia[1]                             # one row on both sides of ONE table: the two atomic streams meet
            ia[2] = ib[2]                             # and a row paired with itself (difference zero)
        return ia, ib
    ia, ib = rng.integers(0, rows, n), rng.integers(0, rows, n)      # with replacement
    if p == "shared" and n >= 2:
        ib[0] = ia[-1]                                # one row id present in ia and in ib
    return ia, ib


@functools.lru_cache(maxsize=8)
def align_ops(c: Case) -> AlignOps:
    rng = _rng(c)
    A = quarters(rng, (c.rows, c.dim))
    B = A if c.variant == "self" else quarters(rng, (c.rows, c.dim))
    ia, ib = (x.astype(np.int32) for x in align_ids(c, rng))
    ta = padded_table(A, c.width)
    tb = ta if c.variant == "self" else padded_table(B, c.width)
    d = ta.astype(np.float64)[ia] - tb.astype(np.float64)[ib]
    x = (d * d).sum(1)
    g = 2.0 * c.weight * d
    ga, gb = np.zeros(ta.shape), np.zeros(ta.shape)
    np.add.at(ga, ia, g)
    np.add.at(gb, ib, -g)
    hit_a, hit_b = np.zeros(c.rows, bool), np.zeros(c.rows, bool)
    hit_a[ia], hit_b[ib] = True, True
    bd = Bound()
    unit_g = 2.0 * c.weight / 4
    hits = np.bincount(ia, minlength=c.rows) + np.bincount(ib, minlength=c.rows)     # both sides may share the array
    assert c.width * 4 * 16 * passes(c.n, LOSS_BLOCKS) < 2 ** 24 and (hits.max() if c.n else 0) * 8 < 2 ** 24
    bd.add("chain", x.max() if c.n else 0.0, 1 / 16)
    bd.add("thread", thread_max(x, LOSS_BLOCKS), 1 / 16)
    if c.variant == "self":
        ga = gb = ga + gb
        hit_a = hit_b = hit_a | hit_b
        bd.add("atomic", max_scatter_abs([ia, ib], [g, g], c.rows), unit_g)
    else:
        bd.add("atomic", max(max_scatter_abs([ia], [g], c.rows), max_scatter_abs([ib], [g], c.rows)), unit_g)
    return AlignOps(ta, tb, ia, ib, float(c.weight * x.sum()), ga, gb, hit_a, hit_b, bd)


def align_f32(c: Case, order: str):
    """(loss, ga, gb) of an align case in float32, one operation at a time, in the kernel's order or the reverse one."""
    o = align_ops(c)
    d = o.ta[o.ia] - o.tb[o.ib]
    x = rowsum32(d * d, order)
    th = thread_sums32(x, LOSS_BLOCKS, order)
    loss = th.astype(np.float64).sum() * c.weight
    g = d * np.float32(2.0 * c.weight)
    if c.variant == "self":
        ga = scatter32(o.ia, g, c.rows, order)
        ga = gb = scatter32(o.ib, -g, c.rows, order, into=ga)
    else:
        ga, gb = scatter32(o.ia, g, c.rows, order), scatter32(o.ib, -g, c.rows, order)
    return loss, ga, gb


# ----------------------------------------------------------------------------------------------------- mke_align_steps (SGD)
STEPS_LR = 2.0 ** -3
STEPS_TERMS = ((0, 1, 1.0), (0, 2, 0.5), (0, 3, 1.0), (2, 3, 0.5))
STEPS_CONSTANT = 1                                   # table 1 has no gradient: it must come back bit-identical


class StepsOps(NamedTuple):
    tables: tuple        # four float32 [rows, stride], pad columns zero
    ia: np.ndarray       # int32, all steps behind each other
    ib: np.ndarray
    off: np.ndarray      # int64 [n_steps + 1]
    losses: np.ndarray   # float64 [n_steps, n_terms]
    final: tuple         # four float64 [rows, stride] after the replay
    bound: Bound


def steps_replay(tables, ia, ib, off, dtype, order="lanes"):
    """The float64 (or, in float32, one-operation-at-a-time) replay: per step the gradient of every term on the tables as they
    stand, then one SGD step per table that has a gradient.  The float64 form is mo.alignment_step_dense(update=False) per
    term (test_rows_cases.py holds the two against each other).  Returns (tables, losses [step, term], record): record holds
    (step, kind, value) with the largest row total ("chain"), the largest sum of absolute values on one gradient element
    ("atomic") and the largest table entry after the step ("value")."""
    T = [np.array(t, dtype=dtype) for t in tables]
    rows = T[0].shape[0]
    live = [k for k in range(len(T)) if k != STEPS_CONSTANT]
    losses = np.zeros((len(off) - 1, len(STEPS_TERMS)))
    record = []
    for s in range(len(off) - 1):
        a, b = ia[off[s]:off[s + 1]].astype(np.int64), ib[off[s]:off[s + 1]].astype(np.int64)
        G = [np.zeros_like(t) for t in T]
        absG = [np.zeros(t.shape) for t in T]
        for k, (p, q, w) in enumerate(STEPS_TERMS):
            d = T[p][a] - T[q][b]
            if dtype == np.float32:
                x = rowsum32(d * d, order)
                losses[s, k] = thread_sums32(x, LOSS_BLOCKS, order).astype(np.float64).sum() * w
            else:
                x = (d * d).sum(1)
                losses[s, k] = w * x.sum()
            g = d * dtype(2.0 * w)
            if dtype == np.float32:
                scatter32(a, g, rows, order, into=G[p])
                scatter32(b, -g, rows, order, into=G[q])
            else:
                np.add.at(G[p], a, g)
                np.add.at(G[q], b, -g)
            np.add.at(absG[p], a, np.abs(g).astype(np.float64))
            np.add.at(absG[q], b, np.abs(g).astype(np.float64))
            record.append((s, "chain", float(x.max()) if len(x) else 0.0))
        record.append((s, "atomic", max(float(absG[k].max()) for k in live)))
        for k in live:
            T[k] = T[k] - dtype(STEPS_LR) * G[k]
        record.append((s, "value", max(float(np.abs(T[k]).max()) for k in live)))
    return T, losses, record


@functools.lru_cache(maxsize=4)
def steps_ops(c: Case) -> StepsOps:
    """Three steps with duplicates and an empty one between them.  Units: entries start as multiples of 2^-2; a gradient entry
    is 2 w (difference) with w >= 1/2, a multiple of the entries' unit u; the SGD step multiplies it by lr = 2^-3, so the
    entries' unit shrinks by 2^-3 per non-empty step (2^-2, 2^-5, 2^-8, 2^-11) and the squared distances of a step come in units
    of u^2.  The bound is taken from the replayed values themselves (sums of absolute values, see the module docstring)."""
    rng = _rng(c)
    rows, B = c.rows, c.n
    # wide rows start in [-1/2, 1/2]: the squared distances of the third step come in units of 2^-16 and must stay below 256
    amp = 4 if c.dim <= 80 else 2
    tables = tuple(padded_table(rng.integers(-amp, amp + 1, (rows, c.dim)).astype(np.float64) / 4.0, c.width) for _ in range(4))
    sizes = (B, 0, B - 7, B // 2)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ia = rng.integers(0, rows, off[-1]).astype(np.int32)
    ib = rng.integers(0, rows, off[-1]).astype(np.int32)
    ia[1], ib[0] = ia[0], ia[0]                       # a duplicate and a row on both sides in the first step
    final, losses, record = steps_replay(tables, ia, ib, off, np.float64)
    assert min(w for _, _, w in STEPS_TERMS) >= 0.5
    bd = Bound()
    for s, kind, v in record:
        if sizes[s] == 0:
            continue
        u = 2.0 ** (-2 - 3 * sum(1 for z in sizes[:s] if z))      # the entries' unit when step s starts
        if kind == "chain":
            bd.add(f"step {s} chain", v, u * u)
            bd.add(f"step {s} thread", v * passes(sizes[s], LOSS_BLOCKS), u * u)
        elif kind == "atomic":
            bd.add(f"step {s} atomic", v, u)
        else:
            bd.add(f"step {s} value", v, u * STEPS_LR)
    return StepsOps(tables, ia, ib, off, losses, tuple(final), bd)


# ----------------------------------------------------------------------------------------------------- the case table
def _build():
    cases = []
    # dense kernels: every dim x ld x row count; the (sign, weights) combinations of the logistic loss rotate over them
    glog_kinds = [(+1, "w"), (-1, "now"), (+1, "now"), (-1, "w")]
    i = 0
    for dim in DENSE_DIMS:
        for extra in LD_EXTRA:
            for n in COUNTS:
                cases.append(Case("galign", n, dim, dim + extra, "grad"))
                sign, var = glog_kinds[i % 4]
                cases.append(Case("glog", n, dim, dim + extra, var, sign=sign))
                i += 1
        i += 1                                                    # 21 cases per dim: shift the rotation between dims
        cases.append(Case("galign", 257, dim, dim, "nograd"))
        cases.append(Case("glog", 257, dim, dim + 3, "nograd_w", sign=+1))
    for dim in (1, 16):                                           # across a grid pass of the 2048-block kernels
        for n in PASS_LOSS:
            cases.append(Case("galign", n, dim, dim, "grad"))
            cases.append(Case("glog", n, dim, dim, "w", sign=+1))
            cases.append(Case("glog", n, dim, dim, "now", sign=-1))
    cases.append(Case("galign", PASS_LOSS[1], 16, 19, "grad"))
    cases.append(Case("galign", PASS_LOSS[1], 16, 16, "nograd"))
    cases.append(Case("glog", PASS_LOSS[1], 15, 31, "w", sign=+1))
    # table kernels: every stride x its dims x row count; id patterns, weights and index modes rotate so that every stride sees all
    for si, stride in enumerate(STRIDES):
        for di, dim in enumerate(table_dims(stride)):
            for ni, n in enumerate(COUNTS):
                pat = ALIGN_PATTERNS[(ni + 5 * di + si) % len(ALIGN_PATTERNS)]
                rows = max(n, 1) + 3 if pat == "same" else max(4, (n * 2) // 3 + 4)
                cases.append(Case("align", n, dim, stride, pat, rows=rows, weight=WEIGHTS[(ni + di) % 4]))
                for var in ("copy", "norm"):
                    im = ("null", "rep")[(ni + di + (var == "norm")) % 2]
                    cases.append(Case("gather", n, dim, stride, var, idx=im, rows=max(n, 8) if im == "null" else max(8, n // 2 + 3)))
        for n in COUNTS:
            for var in ("a", "ab", "abc"):
                cases.append(Case("probe", n, stride, stride, var, rows=max(4, n // 3 + 1)))
    # heavy duplicates, at the model's width and at the narrowest and the widest
    for stride, dim in ((80, 75), (16, 16), (320, 305)):
        cases.append(Case("align", 500, dim, stride, "dup", rows=7, weight=0.5, tag="heavy"))
        cases.append(Case("align", 4000, dim, stride, "dup", rows=3000, weight=2.0, tag="heavy"))
        cases.append(Case("align", 500, dim, stride, "self", rows=7, weight=1.0, tag="heavy"))
    for stride, dim in ((16, 16), (16, 1)):
        for n in PASS_LOSS:                                       # across a grid pass
            cases.append(Case("align", n, dim, stride, "dup", rows=3000, weight=0.5, tag="pass"))
        cases.append(Case("align", PASS_LOSS[1], dim, stride, "self", rows=3000, weight=1.0, tag="pass"))
        cases.append(Case("align", PASS_LOSS[1], dim, stride, "loss_only", rows=3000, weight=2.0, tag="pass"))
        cases.append(Case("align", PASS_LOSS[0], dim, stride, "same", rows=PASS_LOSS[0] + 2, weight=1.0, tag="pass"))
        for n in PASS_ROWS:
            cases.append(Case("gather", n, dim, stride, "copy", idx="null", rows=n, tag="pass"))
            cases.append(Case("gather", n, dim, stride, "copy", idx="rep", rows=1000, tag="pass"))
    for n in PASS_ROWS:
        for var in ("a", "abc"):
            cases.append(Case("probe", n, 16, 16, var, rows=1000, tag="pass"))
    # mke_align_steps (k_align_batch): SGD over three steps with duplicates (n = the first step's batch), at every stride; the
    # dims rotate over stride, stride - 1, stride - 15, and stride 80 also runs the model's 75
    for si, stride in enumerate(STRIDES):
        cases.append(Case("steps", 48, table_dims(stride)[si % 3], stride, rows=40))
    cases.append(Case("steps", 48, 75, 80, rows=40))
    assert len({c.id for c in cases}) == len(cases)
    return cases


ALL_CASES = _build()
EXACT_KERNELS = ("galign", "glog", "gather", "probe", "align", "steps")


def cases_of(kernel, **kw):
    return [c for c in ALL_CASES if c.kernel == kernel and all(getattr(c, k) == v for k, v in kw.items())]


# widths refused before any launch
REFUSED_STRIDE = 144            # a multiple of 16 that is no instantiation: MKE_E_UNSUPPORTED
REFUSED_DIM = 321               # past MKE_MAX_STRIDE: MKE_E_SHAPE
