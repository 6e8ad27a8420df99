"""Case table, operand factories, references and error bounds of the exact optimizer-kernel tests (test_update_cases.py here,
test_update_exact_gpu.py on the device): k_rows_update / k_rows_update_multi (mke_update.hip), k_rows_update_dense /
k_dense_update_opt (mke_dense_opt.hip) and the flat k_dense_update (dense_update_range in mke_common.h).  NumPy only.

Operands follow rows_cases.py.  Table entries and every gradient contribution (rows, privatised copies, hub copies, src_rows
rows) are multiples of 1/4 in [-1, 1], learning rates powers of two (1 and 1/4 among them: the step is as large as the
weight).  Every sum the kernels form is then exact in float32 in any order: the sum over copies, hub copies and ranks,
s = sum w^2 and dot = sum w g.  `Bound.add` records (sum of absolute values, unit) for each of them and the CPU test asserts
`Bound.check()`.

Poison, all of it INSIDE the buffers: every array has one tail row behind its last row (a [copies][n][stride] gradient behind
its last copy, the hub copies before it): NaN in table / acc / slots, SENTINEL in grad and src_rows.  `touched` has 64 extra
entries equal to the tag (only `r < n_rows` stops the kernel there), slot_of a tail row of live-looking slots.  Gradient rows,
copies and hub copies of unvisited rows hold SENTINEL and must still hold it afterwards.  Pad columns: 0 in table and grad
(the ABI), 0.1 in acc (EmbeddingTable.slot), SENTINEL in the Adam / Adadelta slots.

Tier 1 (bit for bit): SGD with normalize = 0 -- table, grad and every copy, hub copies, slot_of, ref_count; Adagrad's
accumulator with normalize = 0 (one fmaf(g, g, a): a single rounding of a sum float64 holds exactly); Adam's m, v and
Adadelta's accum at beta1 = beta2 = rho = 1/2 with normalize = 0.

Tier 2 (float64 with a derived bound): everything else.  The bound is computed by running the kernel's own formula on
(value, error) pairs (class V), charging in units of u = 2^-23 (one ulp, relative):

  +, -, x, fmaf              u/2 on the result (round to nearest); a product with a power of two is free
  rsqrtf, rsq, sqrtf, /      2 u on the result (the project's assumption, NORM_RTOL in test_rows_exact_gpu.py; not measured)
  a sum over a row           nothing where `dyadic_sum_exact` proves it exact in 24 bits (always, for quarter operands), else
                             (FPL + 6) u/2 of the sum of absolute values: each term passes at most FPL fmas and 6 butterflies
  every operation            2^-149 absolute on top (denormal results)

and propagating input errors to first order with the second-order term kept.  A contracted a - b c drops one rounding, so the
count covers both compilations.  Counted out for the normalised SGD row, w' = w - lr (ghat - w coef) inv, coef = dot inv inv:
inv 2 u; coef 2 + 2 + 1/2 + 1/2 = 5 u; w coef 5.5 u; the subtraction u/2 of |ghat| + |w coef|; the product with inv 2.5 u of the
same: 3 u on |ghat| inv and 8.5 u on |w coef| inv (c = 8.5 in the issue's form).  The operation that forms a STORED value is
charged a whole ulp, as the issue's form does (`Arith.stored`):
      |dw| <= u (8.5 lr (|ghat| + |w coef|) inv + |w| + lr |g|).
Adagrad adds a' = fmaf(g, g, a) (2 |g| dg + dg^2 + u/2 a'), rsq(a') (2 u + half the relative error of a') and the two products
(lr g) rsq and w - that (u/2 each).  Adam: two products and a sum for m and for v each, sqrtf, + eps, one product, the division,
the subtraction; Adadelta likewise with sqrtf x rsqrtf x g.  The bounds are never fitted to a device: a ratio above 1 is a finding.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import rows_cases as rc
from rows_cases import FPLS, OLD_TAG, SENTINEL, TAG, Bound, quarters

f32, f64 = np.float32, np.float64
STRIDES = rc.STRIDES
N_CHUNK4 = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257)
N_SMALL_MAX = 16384                                             # chunk_for: at and below, 4 rows per wavefront
N_LARGE = (16385, 16400, 16448, 16449)                          # chunks 16 and 64, by option
N_BY_SIZE = 500001                                              # chunk 64 by size alone (> 500,000 rows)
PATTERNS = ("none", "all", "first", "last", "fifth", "q0", "q1", "q2", "q3", "old", "null")
COPIES = (1, 2, 8)
N_HOT = (1, 5)
HOT_COPIES = (1, 2, 3, 4, 5, 8, 64)
N_RANKS = (1, 3, 16, 17, 64)
LRS = (1.0, 0.25, 2.0 ** -10)
BLOCK = 256
DENSE_ROWS_N = (1, 15, 16, 17, 257)
DENSE_ROWS_PASS = 8192 * 16 + 1                                 # 131,073: one row past the 8192-block grid of k_rows_update_dense
DENSE_OPT_N = (1, 255, 256, 257, 2048 * BLOCK, 2048 * BLOCK + 1)           # 524,288 / 524,289: the 2048-block cap
DENSE_N = (1, 255, 256, 257, 1024 * BLOCK + 1)                  # 262,145: the 1024-block cap of k_dense_update
COUNT_TOTALS = (1, 255, 257, 1024 * BLOCK + 1)                  # n_pos + n_neg; 262,145: the rider blocks stride
L2_EPS32 = float(f32(1e-12))                                    # MKE_L2_EPS as the kernels hold it
U = 2.0 ** -23
TINY = 2.0 ** -149
ACC_PAD = f32(0.1)
STEPS = 3
N_BITS = (1, 15, 16, 17, 31, 32, 33, 255, 257)                  # bitmap tables: chunk 4, the edges of the bitmap's words
N_BITS_LARGE = (16385, 16449)                                   # chunks 16 and 64, by option
N_POS = (0, 1, 3, 4, 5, 8, 9, 15, 16, 17, 33, 300)              # no list blocks; the h / t split inside a wavefront's eight entries; partial last wavefront / block
LIST_WAVE = 8                                                   # entries of pos_h ++ pos_t per wavefront of the list segment
LIST_PATTERNS = ("q0", "q1", "q2", "q3", "all", "none")        # wavefront i holds exactly 4 (i mod 2) + 1 + q entries that name a pair-01 row
LIST_PAD = 64                                                   # entries behind pos_h and pos_t: rows with pair 01 that no entry of the lists names
BIT_MUTANTS = ("chunk_takes_01", "list_takes_11", "list_h_only", "tail_not_rebased", "skip_fifth_entry", "drop_last_wave", "pair_word_r5",
               "list_blocks_as_update", "junk_pairs_honoured")
MUTANTS = ("skip_last_copy", "copies_not_zeroed", "last_hub_twice", "coef_one_inv", "keep_projection", "old_acc", "stale_tag",
           "skip_fifth_bit", "pad_written", "reset_below_16", "route_first_block", "refcount_all", "count_repeats")


class Hyper(NamedTuple):
    lr: float
    b1: float
    b2: float
    eps: float
    rho: float


HYPERS = {"half": Hyper(0.25, 0.5, 0.5, 1e-8, 0.5), "tf": Hyper(2.0 ** -10, 0.9, 0.999, 1e-8, 0.95)}


def chunk_of(n_rows: int, option: int = 0) -> int:
    """chunk_for() of mke_update.hip without a touched-rows hint."""
    if n_rows <= N_SMALL_MAX:
        return 4
    if option in (16, 64):
        return option
    return 64 if n_rows > 500000 else 16


def row_shape(n_rows: int, stride: int, option: int = 0, shard: bool = False) -> str:
    """wave: a whole wavefront per row; quarter64: quarter-waves under a 64-bit flag mask; quarter: 4 or 16 flags."""
    ch = chunk_of(n_rows, option)
    if ch == 64:
        return "wave" if stride % 64 == 0 and not shard else "quarter64"
    return "quarter"


class UCase(NamedTuple):
    kernel: str            # rows | dense_rows | dense_opt | dense
    n: int                 # rows of the table (elements of a flat buffer)
    dim: int = 1
    stride: int = 1
    pattern: str = "all"   # rows: one of PATTERNS, or "sparse"
    chunk: int = 0         # the update_chunk option of the launch
    copies: int = 1
    n_hot: int = 0
    hot_copies: int = 1
    n_ranks: int = 0       # > 0: the gradient comes through slot_of
    opt: str = "sgd"       # sgd | adagrad | adam | adadelta
    normalize: int = 0
    lr: float = 1.0
    refcount: bool = False
    special: bool = False  # tier 2: rows 0..2 are the zero row, the 2^-30 row and the row of norm 1, all visited
    hyper: str = ""        # dense rules: half | tf
    tag: str = ""
    bits: bool = False     # rows: the visited set comes from a bitmap row and the lists pos_h / pos_t (mke_update_table.bits);
    n_pos: int = 0         #   `pattern` then places the pairs 11, `lpat` the list entries that name a pair-01 row
    lpat: str = ""         #   one of LIST_PATTERNS

    @property
    def id(self):
        s = f"{self.kernel}-{self.opt}{'-norm' if self.normalize else ''}-s{self.stride}-d{self.dim}-n{self.n}"
        if self.kernel in ("rows", "dense"):
            s += f"-{self.pattern}-lr{self.lr:g}"
        for v in (f"ch{self.chunk}" if self.chunk else "", f"c{self.copies}" if self.copies > 1 else "",
                  f"hot{self.n_hot}x{self.hot_copies}" if self.n_hot else "", f"ranks{self.n_ranks}" if self.n_ranks else "",
                  "rc" if self.refcount else "", "special" if self.special else "", self.hyper, self.tag,
                  f"bits-p{self.n_pos}-{self.lpat}" if self.bits else ""):
            if v:
                s += "-" + v
        return s

    @property
    def exact_table(self):
        return self.opt == "sgd" and not self.normalize

    @property
    def tier2(self):
        return not self.exact_table


def _rng(c, salt=0):
    return np.random.default_rng([zlib.crc32(c.id.encode()), salt])


# ----------------------------------------------------------------------------------------------------- (value, error) arithmetic
def _pow2(x) -> bool:
    return isinstance(x, float) and (x == 0.0 or np.frexp(abs(x))[0] == 0.5)


def _rnd(val):
    return 0.5 * U * np.abs(val) + TINY


class V:
    """float64 values with an absolute error bound each; every operator charges the rounding of its float32 twin."""

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, dtype=f64)
        err = np.zeros(self.val.shape) + err
        self.err = np.where(np.isnan(err), np.inf, err)         # 0 inf: an operand without a bound leaves none

    @staticmethod
    def lift(x):
        return x if isinstance(x, V) else V(x)

    def __mul__(self, o):
        free = _pow2(o)
        o = V.lift(o)
        val = self.val * o.val
        err = np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err
        return V(val, err if free else err + _rnd(val))

    __rmul__ = __mul__

    def __add__(self, o):
        o = V.lift(o)
        val = self.val + o.val
        return V(val, self.err + o.err + _rnd(val))

    __radd__ = __add__

    def __sub__(self, o):
        o = V.lift(o)
        val = self.val - o.val
        return V(val, self.err + o.err + _rnd(val))


def lowbit(x):
    """The power of two of the lowest set bit of each float64 (inf for zero)."""
    m, e = np.frexp(np.asarray(x, dtype=f64))
    mi = np.abs(np.rint(np.ldexp(m, 53))).astype(np.int64)
    return np.where(mi == 0, np.inf, np.ldexp((mi & -mi).astype(f64), e - 53))


def dyadic_sum_exact(terms):
    """Per row: all terms are multiples of one power of two and the sum of their absolute values fits 24 bits of it, so that
    every partial sum of every order is exact in float32."""
    unit = lowbit(terms).min(axis=1, keepdims=True)
    tot = np.abs(terms).sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(unit), True, tot / unit < 2 ** 24)


class Arith:
    """One formula, three arithmetics: "bound" (V: float64 with error bounds), "f32" (NumPy float32, one rounding per
    operation) and "fma" (the same with a - b c contracted)."""

    def __init__(self, mode):
        assert mode in ("bound", "f32", "fma")
        self.mode, self.bound = mode, mode == "bound"

    def lift(self, x):
        return V(x) if self.bound else np.asarray(x, dtype=f32)

    def k(self, x):
        """A float32 constant of the kernel."""
        return float(f32(x)) if self.bound else f32(x)

    def val(self, x):
        return x.val if self.bound else np.asarray(x, dtype=f64)

    def out(self, x):
        return (x.val, x.err) if self.bound else (np.asarray(x, dtype=f32), None)

    def _unary(self, x, fn, lo_fn):
        if not self.bound:
            return fn(np.asarray(x, dtype=f64)).astype(f32)
        val = fn(x.val)
        return V(val, lo_fn(x) + 2 * U * np.abs(val) + TINY)

    def rsqrt(self, x):
        def spread(x):
            lo = x.val - x.err
            return np.where(lo > 0, 1.0 / np.sqrt(np.where(lo > 0, lo, 1.0)) - 1.0 / np.sqrt(x.val + x.err), np.inf)
        return self._unary(x, lambda v: 1.0 / np.sqrt(v), spread)

    def sqrt(self, x):
        return self._unary(x, np.sqrt, lambda x: np.sqrt(x.val + x.err) - np.sqrt(np.maximum(x.val - x.err, 0.0)))

    def div(self, a, b):
        if not self.bound:
            return (np.asarray(a, dtype=f64) / np.asarray(b, dtype=f64)).astype(f32)
        lo = np.abs(b.val) - b.err                              # <= 0: the divisor is rounding noise, the quotient has no bound
        ok = lo > 0
        lo = np.where(ok, lo, 1.0)
        val = a.val / b.val
        err = a.err / lo + np.abs(a.val) * b.err / (lo * np.abs(b.val)) + 2 * U * np.abs(val) + TINY
        return V(val, np.where(ok, err, np.inf))

    def msub(self, a, b, c):
        """a - b c: where the compiler may contract."""
        if self.mode == "fma":
            return (np.asarray(a, dtype=f64) - np.asarray(b, dtype=f64) * np.asarray(c, dtype=f64)).astype(f32)
        return a - b * c

    def fma(self, a, b, c):
        """fmaf(a, b, c) of the source: fused in every compilation."""
        if not self.bound:
            return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)
        val = a.val * b.val + c.val
        return V(val, np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err + c.err + _rnd(val))

    def dots(self, a, b, depth):
        """[rows, 1]: the row sums of a b (fma chain per lane, then the butterflies)."""
        if not self.bound:
            return rc.rowsum32(a * b, "lanes").reshape(-1, 1)
        P = a.val * b.val
        perr = (np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err).sum(1, keepdims=True)
        exact = dyadic_sum_exact(P) & (perr == 0)
        chain = depth * 0.5 * U * np.abs(P).sum(1, keepdims=True) + TINY
        return V(P.sum(1, keepdims=True), perr + np.where(exact, 0.0, chain))

    def stored(self, x):
        """A value the kernel stores: its last rounding is charged a whole ulp (the issue's form: ... + |w| + lr |g|), which
        also keeps a float32 emulation, whose last rounding alone reaches u/2, within half the bound."""
        return V(x.val, x.err + 0.5 * U * np.abs(x.val)) if self.bound else x

    def maximum(self, x, k):
        return V(np.maximum(x.val, k), x.err) if self.bound else np.maximum(x, f32(k))

    def select(self, mask, x):
        if self.bound:
            return V(np.where(mask, x.val, 0.0), np.where(mask, x.err, 0.0))
        return np.where(mask, x, f32(0))


# ----------------------------------------------------------------------------------------------------- the rules, written once
def jacobian(ar, w, g, depth, mutant=""):
    """(ghat - what (what . ghat)) inv of the normalise-on-read tables (update_one_row*, k_rows_update_dense)."""
    s, dot = ar.dots(w, w, depth), ar.dots(w, g, depth)
    inv = ar.rsqrt(ar.maximum(s, L2_EPS32))
    live = ar.val(s) > L2_EPS32
    if mutant == "keep_projection":
        live = np.ones_like(live)
    coef = ar.select(live, dot * inv if mutant == "coef_one_inv" else dot * inv * inv)
    return ar.msub(g, w, coef) * inv


def rule_sgd(ar, w, g, lr):
    return ar.stored(ar.msub(w, ar.k(lr), g))


def rule_adagrad(ar, w, g, a, lr, mutant=""):
    a2 = ar.fma(g, g, a)
    return ar.stored(ar.msub(w, ar.k(lr) * g, ar.rsqrt(a if mutant == "old_acc" else a2))), ar.stored(a2)


def adam_lr_t(h: Hyper, t: int) -> float:
    """make_hyper(): double arithmetic on the float32 hyper-parameters, rounded to float32."""
    lr, b1, b2 = (float(f32(x)) for x in (h.lr, h.b1, h.b2))
    return float(f32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def rule_adam(ar, w, g, m, v, h: Hyper, t: int):
    b1, b2 = ar.k(h.b1), ar.k(h.b2)
    omb1, omb2 = ar.k(f32(1) - f32(h.b1)), ar.k(f32(1) - f32(h.b2))
    m2 = b1 * m + omb1 * g
    v2 = b2 * v + omb2 * g * g
    return ar.stored(w - ar.div(ar.k(adam_lr_t(h, t)) * m2, ar.sqrt(v2) + ar.k(h.eps))), ar.stored(m2), ar.stored(v2)


def rule_adadelta(ar, w, g, a, b, h: Hyper):
    rho, omr, eps = ar.k(h.rho), ar.k(f32(1) - f32(h.rho)), ar.k(h.eps)
    a2 = rho * a + omr * g * g
    u = ar.sqrt(b + eps) * ar.rsqrt(a2 + eps) * g
    b2 = rho * b + omr * u * u
    return ar.stored(w - ar.k(h.lr) * u), ar.stored(a2), ar.stored(b2)


# ----------------------------------------------------------------------------------------------------- k_rows_update*: operands
class RowsOps(NamedTuple):
    table: np.ndarray       # float32 [n + 1, stride]
    acc: np.ndarray         # float32 [n + 1, stride] (also under SGD: it must come back untouched)
    grad: np.ndarray        # float32 [copies n + hot_copies n_hot + 1, stride], or None (slot_of)
    touched: np.ndarray     # int32 [n + 64], or None
    ref_count: np.ndarray   # int32 [n + 1], or None
    hot_slot: np.ndarray    # int32 [n + 1], or None
    slot_of: np.ndarray     # int32 [n + 1, n_ranks], or None
    src_rows: np.ndarray    # float32 [n_ranks capacity + 1, stride], or None
    capacity: int
    visited: np.ndarray     # bool [n]
    bound: Bound
    bits: np.ndarray = None     # uint32 [(n + 15) // 16 + 2]: two bits per row; junk pairs of the last word 11, two words of ones behind
    pos_h: np.ndarray = None    # int32 [n_pos + LIST_PAD]
    pos_t: np.ndarray = None


def pairs_of(bits, n, mutant=""):
    """code_pair of mke_update.hip for rows [0, n)."""
    r = np.arange(n)
    word = r >> (5 if mutant == "pair_word_r5" else 4)
    return ((bits[word] >> ((r & 15) * 2).astype(np.uint32)) & 3).astype(np.int64)


def _bitmap(c: UCase, rng, base11):
    """(bits, pos_h, pos_t, visited, hub rows) of a bitmap table.  `base11` (from c.pattern) are the rows of the chunk walk.
    The other rows are dealt to: pair 00 named by entries, pair 10 (named or not), pair 01 named by exactly ONE entry (the rows
    of the list walk, as many as c.lpat asks for), pair 01 named by none (finished by the score launch), pair 00 unnamed.
    The bake's invariant holds: a row named twice, or by the head and the tail of one positive, has pair 11 (or is not visited
    at all), so no row is visited twice."""
    n, P = c.n, c.n_pos
    pair = np.zeros(n, dtype=np.int64)
    pair[base11] = 3
    rest = rng.permutation(np.nonzero(~base11)[0])
    if c.special and n >= 3 and P and base11[1]:                 # the 2^-30 row goes through the list
        pair[1] = 0
        base11 = base11.copy()
        base11[1] = False
        rest = np.concatenate([[1], rest])
        forced = 1
    else:
        forced = 0
    n_waves = -(-2 * P // LIST_WAVE)
    want = []
    for i in range(n_waves):
        size = min(LIST_WAVE, 2 * P - i * LIST_WAVE)
        q = {"all": LIST_WAVE, "none": 0}.get(c.lpat, 4 * (i % 2) + 1 + int(c.lpat[1]) if c.lpat[0] == "q" else 0)
        want.append(min(q, size))
    # pools: the entries that must not lead to a visit need a row to name
    k = len(rest) - forced
    n_c = min(k, 2) if (P and k > 1) or not base11.any() else 0          # pair 00, named
    n_f = min(k - n_c, 2)                                                # pair 10: one named, one not
    n_b = min(k - n_c - n_f, max(2, k // 8))                             # pair 01, unnamed
    n_a = min(sum(want), max(k - n_c - n_f - n_b, 0)) + forced           # pair 01, named once
    a_rows = rest[:n_a]
    body = rest[n_a:]
    c_rows, f_rows, b_rows = body[:n_c], body[n_c:n_c + n_f], body[n_c + n_f:n_c + n_f + n_b]
    pair[a_rows], pair[b_rows], pair[f_rows] = 1, 1, 2
    pool = np.concatenate([np.nonzero(base11)[0], c_rows, f_rows[:1]]).astype(np.int64)
    entries = np.zeros(2 * P, dtype=np.int64)
    left = list(a_rows)
    for i in range(n_waves):
        lo = i * LIST_WAVE
        size = min(LIST_WAVE, 2 * P - lo)
        take = min(want[i], len(left))
        at = rng.choice(size, take, replace=False)
        fill = np.ones(size, bool)
        fill[at] = False
        entries[lo + at] = [left.pop() for _ in range(take)]
        if fill.any():
            entries[lo + np.nonzero(fill)[0]] = rng.choice(pool, int(fill.sum()))
    pair[np.array(left, dtype=np.int64)] = 1                            # rows the lists had no room for: pair 01, unnamed
    b_all = np.nonzero(pair == 1)[0]
    named = np.zeros(n, bool)
    named[entries] = True
    unnamed01 = b_all[~named[b_all]]
    pad = rng.choice(unnamed01, LIST_PAD) if len(unnamed01) else np.zeros(LIST_PAD, dtype=np.int64)
    pos_h = np.concatenate([entries[:P], pad]).astype(np.int32)
    pos_t = np.concatenate([entries[P:], pad[::-1]]).astype(np.int32)
    words = (n + 15) // 16
    bits = np.zeros(words + 2, dtype=np.uint32)
    full = np.full(words * 16, 3, dtype=np.int64)                        # the junk pairs of the last word: 11
    full[:n] = pair
    r = np.arange(words * 16)
    np.bitwise_or.at(bits, r >> 4, (full << ((r & 15) * 2)).astype(np.uint32))
    bits[words:] = 0xFFFFFFFF
    visited = (pair == 3) | ((pair == 1) & named)
    return bits, pos_h, pos_t, visited, (a_rows if P else a_rows[:0]), np.nonzero(base11)[0]


def _flags(c: UCase, rng):
    """(touched or None, visited)."""
    n, ch = c.n, chunk_of(c.n, c.chunk)
    p = c.pattern
    if p == "null":
        return None, np.ones(n, bool)
    t = np.zeros(n + 64, dtype=np.int32)
    r = np.arange(n)
    if p == "all":
        t[:n] = TAG
    elif p == "first":
        t[:min(n, 1)] = TAG
    elif p == "last":
        t[max(n - 1, 0):n] = TAG
    elif p == "fifth":
        t[:n][r % 5 == 2] = TAG
    elif p == "old":
        t[:n] = rng.choice(np.array([TAG, TAG, OLD_TAG, TAG + 1, 0], dtype=np.int32), n)
    elif p == "sparse":
        t[rng.choice(n, min(n, 300), replace=False)] = TAG
        t[[0, n - 1]] = TAG
    elif p.startswith("q"):                                     # chunk i holds exactly 4 k + 1 + q set bits, k = i mod (chunk / 4)
        q = int(p[1])
        for i, base in enumerate(range(0, n, ch)):
            size = min(ch, n - base)
            want = min(4 * (i % max(ch // 4, 1)) + 1 + q, size)
            t[base + rng.choice(size, want, replace=False)] = TAG
    else:
        assert p == "none", p
    if c.special and n >= 3 and p != "none":
        t[:3] = TAG
    t[n:] = TAG
    return t, t[:n] == TAG


def _hot_rows(c: UCase, rng, touched, visited):
    """hot_slot [n + 1] and the hub rows; hub row 0 is visited, hub row 1 (n_hot = 1: hub row 0 at even copies) is not."""
    slot = np.full(c.n + 1, -1, dtype=np.int32)
    rows = rng.choice(c.n, c.n_hot, replace=False)
    slot[rows] = np.arange(c.n_hot, dtype=np.int32)
    if touched is not None:
        on = rows[:1] if (c.n_hot > 1 or c.hot_copies % 2) else rows[:0]
        off = rows[1:2] if c.n_hot > 1 else (rows[:1] if not len(on) else rows[:0])
        touched[on], touched[off] = TAG, OLD_TAG
        visited[on], visited[off] = True, False
    return slot, rows


@functools.lru_cache(maxsize=4)
def rows_ops(c: UCase) -> RowsOps:
    assert c.kernel == "rows" and c.lr in LRS and not (c.n_hot and c.copies > 1) and not (c.n_ranks and (c.n_hot or c.copies > 1))
    rng = _rng(c)
    n, st, d = c.n, c.stride, c.dim
    table = np.zeros((n + 1, st), dtype=f32)
    table[:n, :d] = quarters(rng, (n, d))
    table[n] = np.nan
    if c.special and n >= 3:
        table[0] = 0.0
        table[1, :d] = 2.0 ** -30
        table[2] = 0.0
        table[2, :min(4, d)] = 0.5 if d >= 4 else 0.0
        if d < 4:
            table[2, 0] = 1.0
    acc = np.full((n + 1, st), ACC_PAD, dtype=f32)
    acc[:n, :d] = (0.1 + np.abs(quarters(rng, (n, d)))).astype(f32)
    acc[n] = np.nan
    bd = Bound()
    touched = hot_slot = slot_of = src_rows = grad = ref_count = None
    capacity = 0
    if c.n_ranks:
        R = c.n_ranks
        kind = rng.integers(0, 3, n)                            # rows with no slot, one slot, several
        if n >= 3:
            kind[:3] = (0, 1, 2) if not c.special else (2, 2, 2)
        has = np.zeros((n, R), bool)
        one = np.nonzero(kind == 1)[0]
        has[one, rng.integers(0, R, len(one))] = True
        many = kind == 2
        has[many] = rng.random((int(many.sum()), R)) < 0.6
        if R > 16 and n >= 3:
            has[2, R - 1] = True                                # a consumed slot past rank 16
        if many.any():
            has[np.nonzero(many)[0], 0] |= ~has[many].any(1)
        visited = has.any(1)
        per_rank = has.sum(0)
        capacity = int(per_rank.max()) + 2 if n else 1
        slot_of = np.full((n + 1, R), -1, dtype=np.int32)
        src_rows = np.full((R * capacity + 1, st), SENTINEL, dtype=f32)
        for r in range(R):
            rows = np.nonzero(has[:, r])[0]
            slots = rng.permutation(capacity)[:len(rows)]
            slot_of[rows, r] = slots
            src_rows[r * capacity + slots] = 0.0
            src_rows[r * capacity + slots, :d] = quarters(rng, (len(rows), d))
        slot_of[n] = 0                                          # the tail row looks live: only r < n_rows keeps the kernel off it
        contrib = has.sum(1).max() if n else 0
    else:
        touched, visited = _flags(c, rng)
        hub = np.zeros(0, dtype=np.int64)
        bitmap = pos_h = pos_t = None
        if c.bits:
            assert c.copies == 1 and c.pattern not in ("null", "old") and c.lpat in LIST_PATTERNS
            bitmap, pos_h, pos_t, visited, by_list, by_chunk = _bitmap(c, rng, visited)
            touched = np.full(n + 64, TAG, dtype=np.int32) if n % 2 else None      # not read (it may be NULL)
            if c.n_hot:                                         # one hub row in the list walk, one in the chunk walk
                placed = by_list[visited[by_list]]
                first = placed[:1] if (c.n_hot > 1 or c.hot_copies % 2) and len(placed) else by_chunk[:1]
                second = by_chunk[:1] if len(first) and first[0] not in by_chunk else by_chunk[1:2]
                others = np.setdiff1d(np.arange(n), np.concatenate([first, second]))
                hub = np.concatenate([first, second, rng.permutation(others)])[:c.n_hot].astype(np.int64)
                hot_slot = np.full(n + 1, -1, dtype=np.int32)
                hot_slot[hub] = np.arange(c.n_hot, dtype=np.int32)
        elif c.n_hot:
            hot_slot, hub = _hot_rows(c, rng, touched, visited)
        n_grad = c.copies * n + (c.hot_copies * c.n_hot if c.n_hot else 0)
        grad = np.full((n_grad + 1, st), SENTINEL, dtype=f32)
        vis = np.nonzero(visited)[0]
        for k in range(c.copies):
            grad[k * n + vis] = 0.0
            grad[k * n + vis, :d] = quarters(rng, (len(vis), d))
            if c.special and n >= 3 and visited[1]:
                grad[k * n + 1, :d] = 1.0                       # sum g = copies dim on the 2^-30 row: a projection kept there shows
        for k in range(c.hot_copies if c.n_hot else 0):
            hv = hub[visited[hub]]
            at = n * c.copies + k * c.n_hot + hot_slot[hv]
            grad[at] = 0.0
            grad[at, :d] = quarters(rng, (len(hv), d))
        contrib = c.copies + (c.hot_copies if c.n_hot else 0)
    if c.refcount:
        ref_count = (1 + rng.integers(0, 5, n + 1)).astype(np.int32)
    bd.add("gradient", max(contrib, 1), 1 / 4)                  # |entries| <= 1: the sum of absolute values per element
    bd.add("s", d, 1 / 16)
    bd.add("dot", d * max(contrib, 1), 1 / 16)
    if c.special:
        bd.add("s of the 2^-30 row", d * 2.0 ** -60, 2.0 ** -60)
        bd.add("dot of the 2^-30 row", d * max(contrib, 1) * 2.0 ** -30, 2.0 ** -32)
    if c.exact_table:
        bd.add("value", 1 + c.lr * max(contrib, 1), c.lr / 4)
    assert (1 + contrib) ** 2 * 2 ** 27 < 2 ** 52               # g g + a is exact in float64: g g in 1/16, a in [0.1, 1.1] at 2^-27
    if not c.n_ranks and c.bits:
        return RowsOps(table, acc, grad, touched, ref_count, hot_slot, slot_of, src_rows, capacity, visited, bd, bitmap, pos_h, pos_t)
    return RowsOps(table, acc, grad, touched, ref_count, hot_slot, slot_of, src_rows, capacity, visited, bd)


# ----------------------------------------------------------------------------------------------------- k_rows_update*: reference
def list_visits(c: UCase, o: RowsOps, mutant=""):
    """walk_list of mke_update.hip, entry by entry: the rows the list segment visits, and the rows it visits although the chunk
    walk has them (a mutant's second visit)."""
    P, n = c.n_pos, c.n
    pair = pairs_of(o.bits, n, mutant)
    i = np.arange(2 * P)
    if mutant == "list_h_only":
        rows = o.pos_h[np.where(i < P, i, i - P)]
    elif mutant == "tail_not_rebased":                           # pos_t[i] for i >= n_pos: the pad behind the list, then nothing
        rows = np.where(i < P, o.pos_h[np.minimum(i, P + LIST_PAD - 1)], np.where(i < P + LIST_PAD, o.pos_t[np.minimum(i, P + LIST_PAD - 1)], -1))
    else:
        rows = np.where(i < P, o.pos_h[np.minimum(i, max(P - 1, 0))], o.pos_t[np.maximum(i - P, 0)]) if P else np.zeros(0, dtype=np.int64)
    rows = rows.astype(np.int64)
    ok = (rows >= 0) & (rows < n)
    p = np.where(ok, pair[np.where(ok, rows, 0)], 0)
    take = p == 1
    twice = (p == 3) if mutant == "list_takes_11" else np.zeros(2 * P, bool)
    if mutant == "skip_fifth_entry":
        rank = np.zeros(2 * P, dtype=np.int64)
        for lo in range(0, 2 * P, LIST_WAVE):
            rank[lo:lo + LIST_WAVE] = np.cumsum(take[lo:lo + LIST_WAVE]) - 1
        take &= rank != 4
    if mutant == "drop_last_wave" and (2 * P) % LIST_WAVE:
        take[2 * P - (2 * P) % LIST_WAVE:] = False
    return rows[take], rows[twice]


def _visited(c: UCase, o: RowsOps, mutant, skip_block=False, skip_rows=0):
    """(visited rows, rows whose gradient a mutant applies twice)."""
    if c.bits:                                                   # pair 11, and pair 01 where an entry of pos_h ++ pos_t names the row
        pair = pairs_of(o.bits, c.n, mutant)
        vis = (pair == 3) | ((pair == 1) if mutant == "chunk_takes_01" else False)
        vis[:skip_rows] = False
        by_list, twice = list_visits(c, o, mutant)
        twice = np.concatenate([twice, by_list[vis[by_list]]])
        vis[by_list] = True
        return np.nonzero(vis)[0], np.unique(twice)
    vis = o.visited.copy()
    if mutant == "stale_tag" and o.touched is not None:
        vis |= o.touched[:c.n] == OLD_TAG
    ch = chunk_of(c.n, c.chunk)
    if mutant == "skip_fifth_bit":
        idx = np.nonzero(vis)[0]
        chunk_id = idx // ch
        first = np.searchsorted(chunk_id, chunk_id, side="left")          # position of the chunk's first set bit
        vis[idx[np.arange(len(idx)) - first == 4]] = False
    if skip_block:
        vis[:(BLOCK // 64) * ch] = False
    vis[:skip_rows] = False
    return np.nonzero(vis)[0], np.zeros(0, dtype=np.int64)


def rows_rule(c: UCase, W0, A0, G, mode="bound", mutant="", G_err=None) -> dict:
    """The update of rows "given their gradient": float64 operands W0 (table rows), A0 (accumulator rows) and G (the summed
    gradient rows, exact inputs) -> {"table": (values, error bound or None = bit for bit), "acc": ...}.  G_err: an error bound on
    G (a sum of copies the caller could not form exactly); with it nothing is held bit for bit."""
    ar = Arith(mode)
    st, d = c.stride, c.dim
    out = {}
    exact = G_err is None
    w, g = ar.lift(W0), (ar.lift(G) if exact or not ar.bound else V(G, G_err))
    if c.normalize:
        g = jacobian(ar, w, g, st // 16 + 6, mutant)
    a2 = None
    if c.opt == "adagrad":
        w2, a2 = rule_adagrad(ar, w, g, ar.lift(A0), c.lr, mutant)
    else:
        w2 = rule_sgd(ar, w, g, c.lr)
    wv, we = ar.out(w2)
    wv = np.array(wv)
    if mutant == "pad_written":
        wv[:, d:] = 2.0 ** -20
    elif mode == "bound" and not mutant:
        assert not wv[:, d:].any()                              # pad columns: 0 - lr 0 rsq(0.1) stays exactly zero
    if mode == "bound":
        we = np.array(we)
        we[:, d:] = 0.0
        if c.exact_table and exact:
            wv, we = wv.astype(f32), None                       # exact in float64, and (Bound) a float32 value
    out["table"] = (wv, we)
    if a2 is not None:
        av, ae = ar.out(a2)
        if mode == "bound":
            assert mutant or np.array_equal(av[:, d:], A0[:, d:])
            ae = np.array(ae)
            ae[:, d:] = 0.0
            if not c.normalize and exact:
                av, ae = av.astype(f32), None                   # one rounding of an exact float64 sum
        out["acc"] = (av, ae)
    return out


def rows_reference(c: UCase, mode="bound", mutant="", skip_block=False, skip_rows=0) -> dict:
    """What one table of a k_rows_update / k_rows_update_multi launch must hold afterwards: "rows" (the visited rows),
    "table" / "acc" as (values of those rows, error bound or None = bit for bit), and the whole grad / slot_of / ref_count."""
    o = rows_ops(c)
    n, st, d = c.n, c.stride, c.dim
    v, twice = _visited(c, o, mutant, skip_block, skip_rows)
    out = {"rows": v}
    G = np.zeros((len(v), st))
    if c.n_ranks:
        so = o.slot_of.copy()
        for r in range(c.n_ranks):
            s = so[v, r]
            G[s >= 0] += o.src_rows[r * o.capacity + s[s >= 0]]
        so[v, :16 if mutant == "reset_below_16" else c.n_ranks] = -1
        out["slot_of"] = so
    else:
        grad = o.grad.copy()
        last = c.copies - 1 if mutant == "skip_last_copy" else c.copies
        for k in range(last):
            G += grad[k * n + v]
            if k == 0 or mutant != "copies_not_zeroed":
                grad[k * n + v] = 0.0
        if c.n_hot:
            hs = o.hot_slot[v]
            hv = hs >= 0
            for k in list(range(c.hot_copies)) + ([c.hot_copies - 1] if mutant == "last_hub_twice" else []):
                at = n * c.copies + k * c.n_hot + hs[hv]
                G[hv] += o.grad[at]
                grad[at] = 0.0
        out["grad"] = grad
    if c.refcount:
        rcnt = o.ref_count.copy()
        rcnt[:n if mutant == "refcount_all" else 0] = 0
        rcnt[v] = 0
        out["ref_count"] = rcnt
    if len(twice):                                               # two visits that both read the gradient before either zeroes it
        G[np.isin(v, twice)] *= 2.0
    if mutant == "junk_pairs_honoured" and c.bits and n % 16:    # the pairs behind the table's last row are 11: a visit of row n
        out["grad"][n] = 0.0
    out.update(rows_rule(c, o.table[v].astype(f64), o.acc[v].astype(f64), G, mode, mutant))
    return out


BUFFERS = ("table", "acc", "grad", "touched", "ref_count", "hot_slot", "slot_of", "src_rows", "bits", "pos_h", "pos_t")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def check_rows(o: RowsOps, got: dict, want: dict):
    """(problems, ratios): `got` holds the buffers after the launch (any of BUFFERS; "table" required).  Rows outside
    want["rows"] and every buffer the kernel only reads must be bit-identical to the operands."""
    problems, ratios = [], {}
    v = want["rows"]
    rest = np.ones(len(o.table), bool)
    rest[v] = False
    for name in ("table", "acc"):
        if name not in got or got[name] is None:
            continue
        g, init = got[name], getattr(o, name)
        if not np.array_equal(bits(g[rest]), bits(init[rest])):
            problems.append(f"{name}: a row outside the visited ones changed")
        if name not in want:
            if not np.array_equal(bits(g), bits(init)):
                problems.append(f"{name}: changed though the rule does not use it")
            continue
        val, err = want[name]
        if err is None:
            if not np.array_equal(bits(g[v]), bits(val)):
                problems.append(f"{name}: visited rows differ from the exact reference")
            continue
        diff = np.abs(g[v].astype(f64) - val)
        if not np.isfinite(g[v]).all() or (diff[err == 0] != 0).any():
            problems.append(f"{name}: not finite, or an element with bound 0 differs")
            continue
        r = float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
        ratios[name] = r
        if r > 1:
            problems.append(f"{name}: error / bound = {r:.3g}")
    for name in ("grad", "slot_of", "ref_count"):
        if name in want and not np.array_equal(bits(got[name]), bits(want[name])):
            problems.append(f"{name}: differs from the reference")
    for name in ("touched", "hot_slot", "src_rows", "bits", "pos_h", "pos_t"):
        if got.get(name) is not None and not np.array_equal(bits(got[name]), bits(getattr(o, name))):
            problems.append(f"{name}: a read-only buffer changed")
    return problems, ratios


def apply_reference(o: RowsOps, ref: dict) -> dict:
    """The buffers a kernel that computes `ref` leaves behind (float32)."""
    got = {k: (None if getattr(o, k) is None else getattr(o, k).copy()) for k in BUFFERS}
    for name in ("table", "acc"):
        if name in ref:
            got[name][ref["rows"]] = np.asarray(ref[name][0], dtype=f32)
    for name in ("grad", "slot_of", "ref_count"):
        if name in ref:
            got[name] = ref[name].copy()
    return got


# ----------------------------------------------------------------------------------------------------- launches of several tables
class CountCase(NamedTuple):
    n_pos: int
    neg_per_pos: int
    n_ent: int = 1000

    @property
    def total(self):
        return self.n_pos * (1 + self.neg_per_pos)


class CountOps(NamedTuple):
    pos_h: np.ndarray
    pos_t: np.ndarray
    neg_h: np.ndarray       # int32 [n_neg] (one element where n_neg = 0: never read)
    neg_t: np.ndarray
    ref_count: np.ndarray   # int32 [n_ent + 1], small counts on entry: the rider ADDS


@functools.lru_cache(maxsize=4)
def count_ops(cc: CountCase) -> CountOps:
    rng = np.random.default_rng([cc.n_pos, cc.neg_per_pos, cc.n_ent])
    ph, pt = (rng.integers(0, cc.n_ent, cc.n_pos).astype(np.int32) for _ in range(2))
    n_neg = cc.n_pos * cc.neg_per_pos
    nh, nt = (rng.integers(0, cc.n_ent, max(n_neg, 1)).astype(np.int32) for _ in range(2))
    if n_neg:
        g = np.arange(n_neg) // cc.neg_per_pos
        side = rng.integers(0, 3, n_neg)                        # a corrupted tail keeps the head, a corrupted head keeps the tail
        nh[:n_neg][side == 0] = ph[g][side == 0]
        nt[:n_neg][side == 1] = pt[g][side == 1]
    return CountOps(ph, pt, nh, nt, rng.integers(0, 3, cc.n_ent + 1).astype(np.int32))


def count_reference(cc: CountCase, mutant="") -> np.ndarray:
    """mke_count_entity_refs of the header: occurrences in (pos_h, pos_t, neg_h, neg_t), not counting a negative's entry that
    repeats its own positive's entity on that side."""
    o = count_ops(cc)
    out = o.ref_count.astype(np.int64)
    n_neg = cc.n_pos * cc.neg_per_pos
    np.add.at(out, o.pos_h, 1)
    np.add.at(out, o.pos_t, 1)
    g = np.arange(n_neg) // max(cc.neg_per_pos, 1)
    for neg, pos in ((o.neg_h[:n_neg], o.pos_h), (o.neg_t[:n_neg], o.pos_t)):
        keep = np.ones(n_neg, bool) if mutant == "count_repeats" else neg != pos[g]
        np.add.at(out, neg[keep], 1)
    return out.astype(np.int32)


class Launch(NamedTuple):
    name: str
    tables: tuple           # UCases of one stride / dim / optimizer / lr / chunk option
    count: CountCase = None

    @property
    def id(self):
        return self.name


def launch_blocks(L: Launch):
    """Update blocks per table (launch_rows_update_multi)."""
    return [-(-t.n // ((BLOCK // 64) * chunk_of(t.n, t.chunk))) for t in L.tables]


def list_blocks(L: Launch) -> int:
    """Blocks of the list segment, ahead of the rider and the update blocks: LIST_WAVE entries per wavefront."""
    return sum(-(-2 * t.n_pos // ((BLOCK // 64) * LIST_WAVE)) for t in L.tables if t.bits)


def launch_reference(L: Launch, mode="bound", mutant=""):
    """Every table comes out as it does alone.  (The mutant that routes the second table's first block to the first table
    leaves that block's rows unvisited.)"""
    second = [k for k, b in enumerate(launch_blocks(L)) if b][1:2]
    skip = [0] * len(L.tables)
    if mutant == "list_blocks_as_update":                       # the first list_blocks update blocks take the list's place: their rows are lost
        left = list_blocks(L)
        for k, (t, b) in enumerate(zip(L.tables, launch_blocks(L))):
            skip[k] = min(left, b) * (BLOCK // 64) * chunk_of(t.n, t.chunk)
            left -= min(left, b)
    return [rows_reference(t, mode, mutant, skip_block=(mutant == "route_first_block" and [k] == second), skip_rows=skip[k])
            for k, t in enumerate(L.tables)]


# ----------------------------------------------------------------------------------------------------- dense rules
class DenseOps(NamedTuple):
    table: np.ndarray       # float32 [n + 1, stride] (flat buffers: [n + 1, 1])
    s1: np.ndarray          # Adam m / Adadelta accum / Adagrad acc; None for SGD
    s2: np.ndarray          # Adam v / Adadelta accum_update; None for Adagrad, SGD
    grads: tuple            # STEPS float32 [n + 1, stride]: the gradient of each step (tail row SENTINEL)
    bound: Bound


@functools.lru_cache(maxsize=4)
def dense_ops(c: UCase) -> DenseOps:
    rng = _rng(c)
    n, st, d = c.n, c.stride, c.dim
    flat = c.kernel != "dense_rows"
    table = np.zeros((n + 1, st), dtype=f32)
    table[:n, :d] = quarters(rng, (n, d))
    table[n] = np.nan
    if c.kernel == "dense_rows" and n >= 3:
        table[0] = 0.0                                          # a zero row: s <= eps
    steps = 1 if c.kernel == "dense" else STEPS
    grads = []
    for _ in range(steps):
        g = np.zeros((n + 1, st), dtype=f32)
        g[:n, :d] = quarters(rng, (n, d))
        g[:n][np.arange(n) % 5 == 3] = 0.0                      # rows without a gradient: Adam and Adadelta move them all the same
        g[n] = SENTINEL
        grads.append(g)
    s1 = s2 = None
    if c.opt == "adagrad":
        s1 = np.full((n + 1, st), ACC_PAD, dtype=f32)
        s1[:n, :d] = (0.1 + np.abs(quarters(rng, (n, d)))).astype(f32)
        s1[n] = np.nan
    elif c.opt in ("adam", "adadelta"):
        s1, s2 = (np.full((n + 1, st), 0.0 if flat else SENTINEL, dtype=f32) for _ in range(2))
        s1[:n, :d], s2[:n, :d] = 0.0, 0.0                       # TF's zero slots
        s1[n], s2[n] = np.nan, np.nan
    bd = Bound()
    bd.add("s", d, 1 / 16)
    bd.add("dot", d, 1 / 16)
    if c.opt == "sgd":
        bd.add("value", 1 + c.lr, c.lr / 4)
    if c.hyper == "half":                                       # m: g / 2 per step on top of m / 2; v and accum: g g / 2
        bd.add("m", 1, 2.0 ** -(2 + STEPS))
        bd.add("v", 1, 2.0 ** -(4 + STEPS))
    return DenseOps(table, s1, s2, tuple(grads), bd)


def dense_exact(c: UCase):
    """Names of the outputs held bit for bit."""
    if c.opt == "sgd":
        return {"table"}
    if c.opt == "adagrad":
        return {"s1"}
    if c.hyper == "half" and not c.normalize:
        return {"s1", "s2"} if c.opt == "adam" else {"s1"}
    return set()


def dense_reference(c: UCase, mode="bound") -> list:
    with np.errstate(invalid="ignore", over="ignore"):          # bounds of inf times values of 0
        return _dense_reference(c, mode)


def _dense_reference(c: UCase, mode) -> list:
    """Per step: {"table": (values [n, stride], bound or None), "s1": ..., "s2": ...}.  Errors of a step are carried into the
    next one, so from the second normalised step on s and dot are charged as rounded sums."""
    o = dense_ops(c)
    ar = Arith(mode)
    n, d = c.n, c.dim
    live = np.arange(c.stride) < d
    w = ar.lift(o.table[:n].astype(f64))
    s1 = None if o.s1 is None else ar.lift(np.where(live, o.s1[:n].astype(f64), 0.0))
    s2 = None if o.s2 is None else ar.lift(np.where(live, o.s2[:n].astype(f64), 0.0))
    h = HYPERS.get(c.hyper)
    exact = dense_exact(c)
    steps = []
    for t, g0 in enumerate(o.grads, start=1):
        g = ar.lift(g0[:n].astype(f64))
        if c.normalize:
            g = jacobian(ar, w, g, c.stride // 16 + 6)
        if c.opt == "sgd":
            w = rule_sgd(ar, w, g, c.lr)
        elif c.opt == "adagrad":
            w, s1 = rule_adagrad(ar, w, g, s1, c.lr)
        elif c.opt == "adam":
            w, s1, s2 = rule_adam(ar, w, g, s1, s2, h, t)
        else:
            w, s1, s2 = rule_adadelta(ar, w, g, s1, s2, h)
        step = {}
        for name, x, init in (("table", w, o.table), ("s1", s1, o.s1), ("s2", s2, o.s2)):
            if x is None:
                continue
            val, err = ar.out(x)
            val = np.where(live, val, init[:n])                 # pad columns are not written (table: 0, slots: SENTINEL)
            if mode == "bound":
                err = np.where(live, err, 0.0)
                if name in exact:
                    assert np.array_equal(val.astype(f32).astype(f64), val) or c.opt == "adagrad"
                    val, err = val.astype(f32), None
            else:
                val = val.astype(f32)
            step[name] = (val, err)
        if mode == "bound" and c.opt == "adagrad":              # the next operation reads the ROUNDED accumulator
            s1 = V(step["s1"][0].astype(f64))
        steps.append(step)
    return steps


def check_dense(o: DenseOps, got: dict, want: dict, n: int):
    """(problems, ratios) of one step: got[name] = the whole [n + 1, stride] buffer."""
    problems, ratios = [], {}
    for name, (val, err) in want.items():
        g, init = got[name], getattr(o, name)
        if not np.array_equal(bits(g[n:]), bits(init[n:])):
            problems.append(f"{name}: tail row written")
        if err is None:
            if not np.array_equal(bits(g[:n]), bits(val)):
                problems.append(f"{name}: differs from the exact reference")
            continue
        diff = np.abs(g[:n].astype(f64) - val)
        if not np.isfinite(g[:n][err > 0]).all() or (diff[err == 0] != 0).any():
            problems.append(f"{name}: not finite, or an element with bound 0 (a pad column) differs")
            continue
        r = float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
        ratios[name] = r
        if r > 1:
            problems.append(f"{name}: error / bound = {r:.3g}")
    return problems, ratios


def unbounded(steps) -> float:
    """Share of the elements of a dense reference without a finite bound."""
    errs = [e for s in steps for _, e in s.values() if e is not None]
    return float(np.mean([np.isinf(e).mean() for e in errs])) if errs else 0.0


# ----------------------------------------------------------------------------------------------------- the case table
def _build():
    cases, launches = [], []
    R = lambda **kw: cases.append(UCase("rows", **kw))
    for si, stride in enumerate(STRIDES):
        dims = rc.table_dims(stride)
        for di, dim in enumerate(dims):
            # tier 1, chunk 4: every row count, the flag patterns rotating so that every stride sees them all
            for ni, n in enumerate(N_CHUNK4):
                R(n=n, dim=dim, stride=stride, pattern=PATTERNS[(ni + 5 * di + si) % len(PATTERNS)], lr=LRS[(ni + di) % 2],
                  refcount=ni % 2 == 0, opt=("sgd", "adagrad")[(ni + si) % 4 == 3])
            # tier 2: the three arithmetic forms with the planted rows
            for k, (opt, norm) in enumerate((("sgd", 1), ("adagrad", 0), ("adagrad", 1))):
                R(n=17, dim=dim, stride=stride, pattern=("fifth", "null", "all")[(k + di) % 3], lr=LRS[(k + di + si) % 3], opt=opt,
                  normalize=norm, special=True)
        R(n=N_SMALL_MAX, dim=dims[si % 3], stride=stride, pattern=PATTERNS[si % len(PATTERNS)], lr=LRS[si % 2])
        # chunks 16 and 64 by option: whole-wave visits at the strides divisible by 64, a 64-bit mask over quarter-waves at the others
        for ci, ch in enumerate((16, 64)):
            for ni, n in enumerate(N_LARGE):
                R(n=n, dim=dims[(ni + ci) % 3], stride=stride, chunk=ch, pattern=PATTERNS[(3 * ni + 5 * ci + si) % len(PATTERNS)],
                  lr=LRS[ni % 2], refcount=ni == 1)
            R(n=16400, dim=dims[ci], stride=stride, chunk=ch, copies=2, pattern=("q1", "fifth")[ci], lr=0.25)
        for ci, copies in enumerate((2, 8)):
            R(n=65, dim=dims[ci], stride=stride, copies=copies, pattern=PATTERNS[(si + 4 * ci) % len(PATTERNS)], lr=LRS[ci])
    for stride, ch in ((16, 16), (64, 64), (80, 64), (80, 16), (128, 64)):
        R(n=16400, dim=stride - 1, stride=stride, chunk=ch, copies=8, pattern="q2", lr=1.0)
    for stride in (64, 80, 128, 192, 256, 320):                  # tier 2 on the large shapes: one reference serves both row shapes
        for k, (opt, norm) in enumerate((("sgd", 1), ("adagrad", 0), ("adagrad", 1))):
            R(n=16400, dim=stride - (5 if stride == 80 else 1), stride=stride, chunk=64 if stride != 80 else 16,
              pattern=("q3", "fifth", "old")[k], lr=LRS[k], opt=opt, normalize=norm, special=True)
    R(n=N_BY_SIZE, dim=64, stride=64, pattern="sparse", lr=0.25, tag="bysize")
    # hub rows: HB = 4 up to FPL 5, 2 beyond; quarter, 64-bit mask and whole-wave shapes
    for stride, n, ch in ((16, 65, 0), (80, 65, 0), (96, 65, 0), (320, 65, 0), (64, 16400, 64), (128, 16400, 64), (80, 16400, 16),
                          (96, 16400, 64)):
        for hi, n_hot in enumerate(N_HOT):
            for ki, hc in enumerate(HOT_COPIES):
                R(n=n, dim=stride - (5 if stride == 80 else ki % 2), stride=stride, chunk=ch, n_hot=n_hot, hot_copies=hc,
                  pattern=("fifth", "q0", "old", "all")[(hi + ki) % 4], lr=LRS[ki % 2], refcount=ki == 2)
    # the owner path: gradient through slot_of
    for stride, n, ch in ((16, 65, 0), (80, 65, 0), (96, 65, 0), (256, 65, 0), (64, 16400, 64), (64, 16400, 16)):
        for ri, ranks in enumerate(N_RANKS):
            R(n=n, dim=stride - (5 if stride == 80 else ri % 2), stride=stride, chunk=ch, n_ranks=ranks, lr=LRS[ri % 2],
              refcount=ri == 1)
    R(n=65, dim=75, stride=80, n_ranks=17, lr=0.25, opt="adagrad", normalize=1)
    # launches of several tables
    T = lambda n, **kw: UCase("rows", n=n, **{"dim": 75, "stride": 80, "pattern": "fifth", "lr": 0.25, **kw})
    L = lambda name, *tables, count=None: launches.append(Launch(name, tuple(tables), count))
    L("chunks-4-16-4", T(20, chunk=16, tag="t0"), T(16400, chunk=16, pattern="q1", normalize=1, tag="t1"), T(4, chunk=16, pattern="all", tag="t2"))
    L("chunks-4-64-4-wave", T(20, dim=64, stride=64, chunk=64, tag="t0"), T(16400, dim=64, stride=64, chunk=64, pattern="q2", tag="t1"),
      T(4, dim=64, stride=64, chunk=64, pattern="all", normalize=1, tag="t2"))
    L("adagrad-chunks", T(20, chunk=16, opt="adagrad", tag="t0"), T(16400, chunk=16, opt="adagrad", normalize=1, pattern="old", tag="t1"),
      T(4, chunk=16, opt="adagrad", pattern="null", tag="t2"))
    L("empty-first", T(0, tag="e0"), T(20, tag="t1"), T(65, pattern="all", normalize=1, tag="t2"))
    L("empty-middle", T(20, tag="t0"), T(0, tag="e1"), T(65, pattern="all", tag="t2"))
    L("empty-last", T(20, tag="t0"), T(65, pattern="q3", tag="t1"), T(0, tag="e2"))
    L("four-tables", T(5, pattern="all", tag="t0"), T(0, tag="e1"), T(17, pattern="null", normalize=1, tag="t2"), T(300, refcount=True, tag="t3"))
    L("all-empty", T(0, tag="e0"), T(0, tag="e1"))
    L("slot-and-copies", T(65, n_ranks=3, tag="t0"), T(65, copies=8, pattern="q1", tag="t1"))
    L("copies-then-slot-64", T(16400, dim=64, stride=64, chunk=64, copies=8, pattern="fifth", tag="t0"),
      T(300, dim=64, stride=64, chunk=64, n_ranks=17, tag="t1"))
    L("hub-and-plain", T(65, n_hot=5, hot_copies=3, refcount=True, tag="t0"), T(20, pattern="all", tag="t1"))
    for total in COUNT_TOTALS:
        cc = {1: CountCase(1, 0), 255: CountCase(85, 2), 257: CountCase(1, 256)}.get(total, CountCase(-(-total // 5), 4))
        assert cc.total == total or (total > 257 and cc.total >= total)
        L(f"count-{total}", T(20, dim=31, stride=32, tag="t0"), T(300, dim=31, stride=32, pattern="q1", refcount=True, tag="t1"), count=cc)
    # the dense rules
    combos = [(opt, hy, nm) for opt in ("adam", "adadelta") for hy in ("half", "tf") for nm in (0, 1)]
    for si, stride in enumerate(STRIDES):
        for di, dim in enumerate(rc.table_dims(stride)):
            for ni, n in enumerate(DENSE_ROWS_N):
                opt, hy, nm = combos[(ni + 3 * di + si) % len(combos)]
                cases.append(UCase("dense_rows", n, dim, stride, opt=opt, hyper=hy, normalize=nm, lr=HYPERS[hy].lr))
    for dim, (opt, hy, nm) in ((16, ("adam", "half", 0)), (1, ("adadelta", "tf", 1))):
        cases.append(UCase("dense_rows", DENSE_ROWS_PASS, dim, 16, opt=opt, hyper=hy, normalize=nm, lr=HYPERS[hy].lr, tag="pass"))
    for n in DENSE_OPT_N:
        for opt in ("adam", "adadelta"):
            for hy in ("half", "tf"):
                cases.append(UCase("dense_opt", n, opt=opt, hyper=hy, lr=HYPERS[hy].lr))
    for n in DENSE_N:
        for opt in ("sgd", "adagrad"):
            for lr in LRS[:2]:
                cases.append(UCase("dense", n, opt=opt, lr=lr))
    assert len({c.id for c in cases}) == len(cases)
    for Ln in launches:
        assert len({(t.stride, t.dim, t.opt, t.lr, t.chunk) for t in Ln.tables}) == 1 and 1 <= len(Ln.tables) <= 4, Ln.name
        assert len({t.id for t in Ln.tables}) == len(Ln.tables)
    return cases, launches


ALL_CASES, LAUNCHES = _build()


def _build_bits():
    """Bitmap tables (beside ALL_CASES and LAUNCHES, which they leave as they are): (cases run alone, launches)."""
    cases, launches = [], []
    B = lambda **kw: cases.append(UCase("rows", bits=True, **kw))
    PAT = ("q0", "q1", "q2", "q3", "all", "none", "fifth", "first", "last")
    for si, stride in enumerate(STRIDES):
        dims = rc.table_dims(stride)
        ragged = [d for d in dims if d != stride]
        # tier 1, chunk 4: every row count; the list lengths, list patterns and pair-11 patterns rotate through the widths
        for ni, n in enumerate(N_BITS):
            k = ni + 4 * si
            B(n=n, dim=dims[k % len(dims)], stride=stride, pattern=PAT[(ni + 2 * si) % len(PAT)], n_pos=N_POS[k % len(N_POS)],
              lpat=LIST_PATTERNS[(ni + si) % 6], lr=LRS[k % 2], refcount=k % 2 == 0, opt=("sgd", "adagrad")[k % 4 == 3])
        # the deal to the quarter-waves: every q of the list with both k at a ragged dim (25 wavefronts; at chunk 4 the chunk walk's q3
        # is every row, which leaves the list none: its own q patterns run at chunks 16 and 64 below)
        for qi in range(4):
            B(n=1023, dim=ragged[qi % len(ragged)], stride=stride, pattern=f"q{(qi + si) % 3}", n_pos=100, lpat=f"q{qi}", lr=LRS[qi % 2])
        # tier 2: the three arithmetic forms with the planted rows, the 2^-30 row through the list
        for k, (opt, norm) in enumerate((("sgd", 1), ("adagrad", 0), ("adagrad", 1))):
            B(n=33, dim=dims[(k + si) % len(dims)], stride=stride, pattern=("fifth", "all", "q1")[k], n_pos=17, lpat=("all", "q2", "q0")[k],
              lr=LRS[(k + si) % 3], opt=opt, normalize=norm, special=True)
        # chunks 16 and 64 by option: whole-wave rows at the strides divisible by 64, the 64-bit mask over quarter-waves at the others
        for ci, ch in enumerate((16, 64)):
            for ni, n in enumerate(N_BITS_LARGE):
                k = 2 * ci + ni
                B(n=n, dim=ragged[(ni + ci) % len(ragged)], stride=stride, chunk=ch, pattern=f"q{(k + si) % 4}", n_pos=(300, 33, 16, 9)[(k + si) % 4],
                  lpat=f"q{(k + 2 * si + 1) % 4}", lr=LRS[ni % 2], refcount=ni == 1, opt=("sgd", "adagrad")[(k + si) % 5 == 0])
    # hub rows: one in the list, one in the chunk walk; HB = 4 up to FPL 5, 2 beyond; the three row shapes
    for stride, n, ch in ((16, 65, 0), (80, 65, 0), (320, 65, 0), (64, 16449, 64), (80, 16449, 64), (80, 16449, 16)):
        for hi, n_hot in enumerate(N_HOT):
            for ki, hc in enumerate(HOT_COPIES):
                if (ki + hi) % 2 == 0 or n == 65:
                    B(n=n, dim=stride - (5 if stride == 80 else 1), stride=stride, chunk=ch, n_hot=n_hot, hot_copies=hc, pattern=("fifth", "q0")[ki % 2],
                      n_pos=(33, 17)[hi], lpat=("q1", "all")[ki % 2], lr=LRS[ki % 2], refcount=ki == 2)
    T = lambda n, **kw: UCase("rows", n=n, **{"dim": 75, "stride": 80, "pattern": "fifth", "lr": 0.25, **kw})
    L = lambda name, *tables, count=None: launches.append(Launch(name, tuple(tables), count))
    for stride, dim in ((16, 15), (80, 75), (256, 255)):
        for copies in (2, 8):                                    # the production launch: flagged relation table, then the bitmap table
            L(f"production-s{stride}-c{copies}", T(65, dim=dim, stride=stride, copies=copies, pattern="q1", tag="rel"),
              T(300, dim=dim, stride=stride, bits=True, n_pos=33, lpat="q2", pattern="q3", refcount=True, tag="ent"))
    for total in COUNT_TOTALS:                                   # ... with the count rider: list blocks, rider blocks, update blocks
        cc = {1: CountCase(1, 0), 255: CountCase(85, 2), 257: CountCase(1, 256)}.get(total, CountCase(-(-total // 5), 4))
        L(f"production-count-{total}", T(20, dim=31, stride=32, copies=(2, 8)[total % 2], tag="rel"),
          T(300, dim=31, stride=32, bits=True, n_pos=(5, 300)[total % 2], lpat="q1", pattern="q0", refcount=True, tag="ent"), count=cc)
    L("production-adagrad-64", T(65, dim=64, stride=64, chunk=64, copies=2, opt="adagrad", pattern="q1", tag="rel"),
      T(16449, dim=64, stride=64, chunk=64, bits=True, n_pos=300, lpat="q3", pattern="q2", opt="adagrad", normalize=1, tag="ent"))
    L("production-hub", T(65, copies=8, pattern="all", tag="rel"), T(300, bits=True, n_pos=17, lpat="all", n_hot=5, hot_copies=3, tag="ent"))
    L("bitmap-alone", T(300, bits=True, n_pos=33, lpat="q0", tag="ent"))
    L("bitmap-no-positives", T(65, copies=2, pattern="all", tag="rel"), T(300, bits=True, n_pos=0, lpat="none", pattern="q1", tag="ent"))
    L("bitmap-first", T(300, bits=True, n_pos=9, lpat="q3", tag="ent"), T(65, copies=2, pattern="all", tag="rel"), T(20, tag="t2"))
    assert len({c.id for c in cases}) == len(cases)
    for Ln in launches:
        assert len({(t.stride, t.dim, t.opt, t.lr, t.chunk) for t in Ln.tables}) == 1 and sum(t.bits for t in Ln.tables) == 1, Ln.name
        assert len({t.id for t in Ln.tables}) == len(Ln.tables)
    return cases, launches


BIT_CASES, BIT_LAUNCHES = _build_bits()


def cases_of(kernel, **kw):
    return [c for c in ALL_CASES if c.kernel == kernel and all(getattr(c, k) == v for k, v in kw.items())]


def launch_tables():
    return [t for L in LAUNCHES for t in L.tables]
