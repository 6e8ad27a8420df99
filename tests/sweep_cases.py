"""Case table, operand factory and oracles of the exact similarity-sweep tests (test_sweep_cases.py here,
test_sweep_exact_gpu.py on the device).  No GPU code: NumPy only.

Exactness.  Rows hold integers in [-L, L] with L^2 dim < 2^24 (L = 3: many exact ties; L = 40: both signs, many
exponents, negative keys).  Every dot product, and every partial sum of it in any order, is an integer exactly representable
in float32: what the MFMA chains of mke_simtile.h return must EQUAL the integer product.  The euclidean epilogue then sees
exact integer arguments (sq_i + sq_j - 2 dot <= 4 L^2 dim < 2^24, so a contracted fma changes nothing) and a correctly
rounded sqrtf; the CSLS epilogue (2 v - r_T) - r_S is evaluated in float32 in the order of mke_rescore.h (2 v is exact, so a
contracted fma changes nothing there either).  r_T / r_S are GIVEN inputs, multiples of 1/8.  Assertions are equality of
integers and of float32 bit patterns.

Poisoned padding.  An operand [n, dim] lies in a NaN-filled [n + BN, kpad + extra] buffer: columns [dim, kpad) are zero
(the ABI), columns [kpad, ld) and the BN rows behind the last logical row are NaN.  A wrong K extent, column guard or row
clamp turns results into NaN or changes counts; nothing lies outside the tensor's own allocation.  The per-row inputs (squared
norms, CSLS terms) carry BN guard entries of -1e30 behind them, which would win every comparison if read (see `guarded`).

Planted structure (every case, as far as its shape has room): a zero row in A; one vector of +-L entries at columns 1, BN - 1,
BN, the last column and on both sides of the first and the last chunk / segment boundary of the client's own column split, and
copied into one row of A — that row's maximum (inner: L^2 dim; euclidean: distance 0; CSLS: these columns get the lowest r_S)
lies in the first AND the last chunk, the lowest column must win; a copy of one gold column at another column (raw ties >= 2 in
every mode); B[i] == A[i] for i % 3 == 0, A[i] perturbed in three coordinates for i % 3 == 1, unrelated otherwise.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

KPADS = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)
REGIME_KPADS = (80, 128, 320)            # double-buffered / one buffer, 64 columns / one buffer, 32 columns
CLIENTS = ("rank", "rank_ex", "topk_mean", "sim_select", "sim_sample", "knn", "stable")
SELF_CLIENTS = ("sim_select", "knn")     # rows and columns are rows of ONE matrix
MODES = ("inner", "euclidean", "inner+csls", "euclidean+csls")
BM = 128                                 # SIMT_BM
LD_EXTRA_A, LD_EXTRA_B = 4, 12
TAU_ALL = -3.0e38                        # below every similarity; what k_sim_select gives its padding columns


def bn_for(kpad: int) -> int:
    return 64 if kpad <= 208 else 32


def regime(kpad: int) -> str:
    return "double" if kpad <= 112 else ("single64" if kpad <= 208 else "single32")


class Case(NamedTuple):
    client: str
    tag: str
    kpad: int
    dim: int
    n_a: int            # rows swept (row_hi - row_lo for the self clients and sim_sample)
    n_b: int            # columns (rows of the one matrix for the self clients; n_samp for sim_sample)
    row_lo: int = 0
    n_rows: int = 0     # rows of the matrix the swept rows come from (self clients: n_b; sim_sample: its own)
    n_seg: int = 1
    seg_cap: int = 0
    k: int = 0          # k of the top-k clients, cut of the stable lists
    mode: str = "inner"
    L: int = 3
    variant: str = ""   # rank: ties / noties; stable: sweep / sample / whole / simmat

    @property
    def row_hi(self):
        return self.row_lo + self.n_a

    @property
    def id(self):
        v = (f"-k{self.k}" if self.k else "") + (f"-r{self.row_lo}" if self.row_lo else "") + \
            (f"-s{self.n_seg}x{self.seg_cap}" if self.seg_cap else "") + (f"-{self.variant}" if self.variant else "")
        return f"{self.client}-{self.tag}-kp{self.kpad}-d{self.dim}-{self.n_a}x{self.n_b}-{self.mode}-L{self.L}{v}"

    @property
    def euclidean(self):
        return self.mode.startswith("euclidean")

    @property
    def csls(self):
        return self.mode.endswith("+csls")


# ----------------------------------------------------------------------------------------------------- the hosts' column splits
def _sweep_chunks(rows, ntiles, target, cap, min_tiles):
    row_blocks = (rows + BM - 1) // BM
    chunks = min((target + row_blocks - 1) // row_blocks, (ntiles + min_tiles - 1) // min_tiles, cap)
    return max(chunks, 1)


def tiles_per_chunk(c: Case, n_cols=None) -> int:
    """Tiles per column chunk / segment of the sweep launched for this case (the host code's arithmetic: mke_align_rank,
    sweep_chunks of mke_csls.hip, mke_sim_sample, mke_sim_select, mke_stable_lists)."""
    n_cols = c.n_b if n_cols is None else n_cols
    nt = (n_cols + bn_for(c.kpad) - 1) // bn_for(c.kpad)
    whole = c.client == "sim_sample" or (c.client == "topk_mean" and c.k > 32) or \
        (c.client == "stable" and (c.variant == "whole" or c.k > 128))
    if whole:                                        # mke_sim_sample: chunks of >= 8 tiles
        chunks = _sweep_chunks(c.n_a, nt, 4096, 1 << 30, 8)
    elif c.client in ("rank", "rank_ex"):
        chunks = _sweep_chunks(c.n_a, nt, 6144, 1 << 16, 16)
    elif c.client == "topk_mean":
        chunks = _sweep_chunks(c.n_a, nt, 6144, 64, 16)
    elif c.client == "stable":
        chunks = 8
    else:                                            # sim_select (and the k-NN chain's main pass)
        chunks = c.n_seg
    return max((nt + chunks - 1) // chunks, 1)


def chunk_bounds(c: Case, n_cols=None):
    """[(first column, one past the last)] per chunk / segment, empty segments included for sim_select."""
    n_cols = c.n_b if n_cols is None else n_cols
    per = tiles_per_chunk(c, n_cols) * bn_for(c.kpad)
    n_chunks = c.n_seg if c.client in SELF_CLIENTS else (n_cols + per - 1) // per
    return [(min(s * per, n_cols), min((s + 1) * per, n_cols)) for s in range(n_chunks)]


# ----------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    A: np.ndarray            # float32 [n_rows_a, dim] (self clients: the same array as B)
    B: np.ndarray            # float32 [n_b, dim]
    sq_a: np.ndarray         # float32 exact squared norms
    sq_b: np.ndarray
    rt: np.ndarray           # float32 [rows of A] multiples of 1/8 (the CSLS row term)
    rs: np.ndarray           # float32 [n_b]
    zero_row: int            # index into A, or -1
    max_row: int             # the row whose maximum is planted twice, or -1
    max_cols: tuple          # (lower, higher) column of the planted maximum, or ()
    dup_cols: tuple          # columns holding the duplicated vector
    tie: tuple               # (row, column != row holding a copy of the row's gold column), or ()


def _seed(c: Case):
    return [CLIENTS.index(c.client), c.kpad, c.dim, c.n_a, c.n_b, c.row_lo, c.n_rows, c.L, c.n_seg]


@functools.lru_cache(maxsize=4)
def operands(c: Case) -> Operands:
    rng = np.random.default_rng(_seed(c))
    L, bn, self_ = c.L, bn_for(c.kpad), c.client in SELF_CLIENTS
    n_cols = c.n_b
    rows_a = c.n_rows if (self_ or c.client == "sim_sample") else c.n_a
    B = rng.integers(-L, L + 1, (n_cols, c.dim))
    if self_:
        A = B
    else:
        A = rng.integers(-L, L + 1, (rows_a, c.dim))
        if c.client != "sim_sample":
            for i in range(min(rows_a, n_cols)):
                if i % 3 == 0:
                    B[i] = A[i]
                elif i % 3 == 1:
                    B[i] = A[i]
                    at = rng.integers(0, c.dim, 3)
                    B[i, at] = rng.integers(-L, L + 1, 3)
    bounds = chunk_bounds(c)
    edges = sorted({b for (a, b) in bounds if 0 < b < n_cols})
    dups = {1, bn - 1, bn, n_cols - 1}
    for e in (edges[:1] + edges[-1:]):
        dups |= {e - 1, e}
    dups = sorted(x for x in dups if 0 <= x < n_cols)
    if len(dups) < 2 or len(dups) > n_cols // 2:   # tiny shapes keep their random rows
        dups = []
    lo, hi = c.row_lo, c.row_lo + c.n_a
    rows = [r for r in range(lo, hi) if not (self_ and r in dups)]
    zero_row = rows[2] if len(rows) > 2 else rows[-1]
    max_row = (rows[5] if len(rows) > 5 else rows[0]) if (dups and len(rows) > 1) else -1
    max_cols = ()
    if dups:
        # the duplicated vector is +-L everywhere: its copy in A has its maximum (inner: L^2 dim; euclidean: distance 0) at
        # every duplicate, i.e. in the first and in the last chunk — the lowest column must win
        v = rng.choice([-L, L], c.dim)
        B[dups] = v
        if max_row >= 0:
            A[max_row] = v
            max_cols = (dups[0], dups[-1])
    A[zero_row] = 0                             # self clients: a zero column as well
    tie = ()
    if not self_ and c.client != "sim_sample":  # a gold column duplicated elsewhere: ties >= 2 in every mode
        tie_row = 7 if c.n_a > 7 else c.n_a - 1
        spare = [x for x in range(n_cols) if x not in dups and x != tie_row]
        if len(spare) > 4:
            tie = (tie_row, spare[len(spare) // 2])
            B[tie[1]] = B[tie_row]
    A32, B32 = A.astype(np.float32), (A if self_ else B).astype(np.float32)
    if self_:
        A32 = B32
    sq_a = (A.astype(np.int64) ** 2).sum(1).astype(np.float32)
    sq_b = (B.astype(np.int64) ** 2).sum(1).astype(np.float32)
    rt = (rng.integers(-16, 17, A.shape[0]) / 8.0).astype(np.float32)
    rs = (rng.integers(-15, 17, n_cols) / 8.0).astype(np.float32)
    if dups:
        rs[dups] = np.float32(-2.0)             # below every other r_S: the planted maximum stays the maximum under CSLS
    if tie:
        rs[tie[1]] = rs[tie[0]]
    return Operands(A32, B32, sq_a, sq_b, rt, rs, zero_row, max_row, max_cols, tuple(dups), tie)


def embed(mat: np.ndarray, kpad: int, extra: int, tail_rows: int) -> np.ndarray:
    """[n + tail_rows, kpad + extra] float32: mat in [:n, :dim], zeros up to kpad, NaN everywhere else."""
    n, d = mat.shape
    buf = np.full((n + tail_rows, kpad + extra), np.nan, dtype=np.float32)
    buf[:n, :kpad] = 0.0
    buf[:n, :d] = mat
    return buf


GUARD = np.float32(-1.0e30)


def guarded(vec: np.ndarray, tail_rows: int) -> np.ndarray:
    """A per-row / per-column input (squared norms, CSLS terms) with `tail_rows` guard entries behind it.  NaN would hide a read
    past the end (every comparison with it is false); -1e30 WINS instead: as a squared norm it clamps the distance to 0
    (similarity 1, the maximum), as a CSLS term it lifts the re-scored value above everything — a column or row past the end
    that reaches an epilogue becomes the best column and a member of every list."""
    buf = np.full(vec.shape[0] + tail_rows, GUARD, dtype=np.float32)
    buf[:vec.shape[0]] = vec
    return buf


def buffers(c: Case):
    """(A buffer, B buffer) poisoned; for the self clients one buffer twice."""
    ops, bn = operands(c), bn_for(c.kpad)
    bb = embed(ops.B, c.kpad, LD_EXTRA_B, bn)
    if c.client in SELF_CLIENTS:
        return bb, bb
    return embed(ops.A, c.kpad, LD_EXTRA_A, bn), bb


# ----------------------------------------------------------------------------------------------------- oracles
def int_dots(A, B) -> np.ndarray:
    """The exact integer products (float64 holds them exactly: |dot| < 2^24)."""
    d = A.astype(np.float64) @ B.astype(np.float64).T
    assert np.array_equal(d, np.rint(d))
    return d


def rescore32(dot32, sq_i, sq_j, rt, rs, euclidean, csls):
    """mke_rescore.h, one float32 operation at a time (dot32 [r, c]; sq_i, rt [r]; sq_j, rs [c])."""
    v = dot32
    assert v.dtype == np.float32
    if euclidean:
        t = sq_i[:, None] + sq_j[None, :]
        w = t - np.float32(2.0) * v
        v = np.float32(1.0) - np.sqrt(np.maximum(w, np.float32(0.0)))
    if csls:
        v = (np.float32(2.0) * v - rt[:, None]) - rs[None, :]
    assert v.dtype == np.float32
    return v


@functools.lru_cache(maxsize=4)
def scores(c: Case) -> np.ndarray:
    """float32 [n_a, n_b]: what the client's epilogue sees for the swept rows (metric and CSLS as the case's mode says)."""
    ops = operands(c)
    r = slice(c.row_lo, c.row_lo + c.n_a)
    d = int_dots(ops.A[r], ops.B)
    assert np.abs(d).max() < 2 ** 24
    return rescore32(d.astype(np.float32), ops.sq_a[r], ops.sq_b, ops.rt[r], ops.rs, c.euclidean, c.csls)


def scores64(c: Case) -> np.ndarray:
    """The inner modes by brute force in float64."""
    assert not c.euclidean
    ops = operands(c)
    r = slice(c.row_lo, c.row_lo + c.n_a)
    v = ops.A[r].astype(np.float64) @ ops.B.astype(np.float64).T
    if c.csls:
        v = (2.0 * v - ops.rt[r].astype(np.float64)[:, None]) - ops.rs.astype(np.float64)[None, :]
    return v


def rank_oracle(S):
    """(greater, raw ties, best column with the lowest column winning, best value) for gold column = row index."""
    n = S.shape[0]
    gold = S[np.arange(n), np.arange(n)]
    greater = (S > gold[:, None]).sum(1).astype(np.int32)
    ties = (S == gold[:, None]).sum(1).astype(np.int32)
    best = np.argmax(S, axis=1).astype(np.int64)
    return greater, ties, best, S[np.arange(n), best]


def select_oracle(S, tau, bounds, seg_cap, strict=True):
    """(count int32 [rows, n_seg] — the TRUE count even past seg_cap, stored: per (row, segment) the first seg_cap
    columns in ascending order)."""
    hit = (S > tau[:, None]) if strict else (S >= tau[:, None])
    cnt = np.zeros((S.shape[0], len(bounds)), dtype=np.int32)
    stored = []
    for r in range(S.shape[0]):
        row = []
        for s, (a, b) in enumerate(bounds):
            cols = np.nonzero(hit[r, a:b])[0] + a
            cnt[r, s] = len(cols)
            row.append(cols[:seg_cap].astype(np.int32))
        stored.append(row)
    return cnt, stored


def order_desc(S):
    """Per row the columns by value descending, then column ascending."""
    return np.argsort(-S, axis=1, kind="stable")


def topk_sets(S, k):
    """int32 [rows, k]: the columns above the k-th largest value plus the first ties in column order, in column order."""
    return np.sort(order_desc(S)[:, :k], axis=1).astype(np.int32)


def kth_largest(S, k):
    return -np.sort(-S, axis=1)[:, k - 1]


def topk_means(S, k):
    top = -np.sort(-S, axis=1)[:, :k]
    return (top.astype(np.float64).sum(1) / float(k)).astype(np.float32)


def stable_lists_oracle(S, cut):
    """(val float32 [rows, cut], col int32 [rows, cut]); NaN entries never enter a list, short lists end in (-inf, -1)."""
    key = np.where(np.isnan(S), -np.inf, S).astype(np.float32)
    o = order_desc(key)[:, :cut]
    val = np.take_along_axis(key, o, axis=1)
    dead = np.take_along_axis(np.isnan(S), o, axis=1)
    col = np.where(dead, -1, o).astype(np.int32)
    return np.where(dead, np.float32(-np.inf), val).astype(np.float32), col


def stable_plan(c: Case, sample_cols: int):
    """(thresholded, column step of the sample, m) as mke_stable_lists computes them for the sweep path."""
    thresholded = sample_cols > 0 or c.n_b > 1024
    step = (c.n_b + 4095) // 4096
    if sample_cols > 0 and c.n_b // sample_cols > step:
        step = c.n_b // sample_cols
    n_samp = (c.n_b + step - 1) // step
    m = min(max((n_samp * (2 * c.k + 32) + c.n_b // 2) // c.n_b, 1), n_samp)
    return thresholded, step, m


def stable_flags_oracle(c: Case, S, sample_cols: int):
    """bool [rows]: the rows the sweep path must flag (a segment past its 128 slots, or fewer than `cut` candidates)."""
    thresholded, step, m = stable_plan(c, sample_cols)
    if not thresholded:
        tau = np.full(S.shape[0], -np.inf, dtype=np.float32)
    else:
        tau = kth_largest(S[:, ::step], m)
    cnt, _ = select_oracle(S, tau, chunk_bounds(c), 128, strict=False)
    return (cnt > 128).any(1) | (thresholded & (cnt.sum(1) < c.k))


def sample_cols_of(c: Case) -> int:
    return c.seg_cap if (c.client == "stable" and c.variant == "sample") else 0


def select_taus(c: Case, S):
    """Thresholds of a sim_select case: row r % 4 == 0 between attained values (integer + 0.5), r % 4 == 1 equal to an attained
    value (strictness), r % 4 == 2 equal to the row's maximum (nothing passes), r % 4 == 3 below everything (every segment
    counts all its columns: overflow past seg_cap)."""
    n = S.shape[1]
    live = sum(1 for a, b in chunk_bounds(c) if a < b)          # segments that hold columns
    q = max(1, min(n, c.seg_cap * live // 2))
    kth = kth_largest(S, q)
    tau = kth.copy()
    r = np.arange(S.shape[0])
    tau[r % 4 == 0] = np.floor(kth[r % 4 == 0]) - np.float32(0.5)
    tau[r % 4 == 2] = S.max(1)[r % 4 == 2]
    tau[r % 4 == 3] = np.float32(TAU_ALL)
    return tau.astype(np.float32)


def knn_plan(c: Case):
    """(sample row indices, m) of a k-NN chain case: the threshold of a row is the m-th largest of its similarities to the
    sample rows, m as base.batch.neighbour_table chooses it."""
    n = c.n_b
    n_samp = min(n, 4 * bn_for(c.kpad) + 1)
    samp = np.random.default_rng([n, c.kpad, 7]).permutation(n)[:n_samp]
    m = min(n_samp, int(np.ceil(1.4 * c.k * n_samp / n)) + 8)
    return samp, m


def knn_status_oracle(c: Case, S, tau):
    """int32 [rows]: 2 a segment overflowed, 1 fewer than k candidates, 0 the candidate list holds the top k."""
    cnt, _ = select_oracle(S, tau, chunk_bounds(c), c.seg_cap)
    over = (cnt > c.seg_cap).any(1)
    return np.where(over, 2, np.where(cnt.sum(1) < c.k, 1, 0)).astype(np.int32)


# ----------------------------------------------------------------------------------------------------- the case table
def _dims(kpad, ragged):
    return kpad - 5 if ragged else kpad


def _shape_pair(kpad):
    bn = bn_for(kpad)
    return [("s1", 33, 16 * bn + 1, True), ("s2", 129, 2 * bn + bn // 2 + 1, False)]   # (tag, n_a, n_b, ragged dim)


def _edges(kpad):
    """(tag, n_a, n_b): the n_b edges at n_a = 33 (or n_b, where smaller), the n_a edges at n_b = 16 BN + 1."""
    bn = bn_for(kpad)
    out = [(f"nb{nb}", min(33, nb), nb) for nb in (20, bn - 1, bn, bn + 1, 16 * bn, 16 * bn + 1, 33 * bn + 31)]
    out += [(f"na{na}", na, 16 * bn + 1) for na in (1, 32, 33, 128, 129, 257)]
    return out


def _make(client, tag, kpad, n_a, n_b, ragged, **kw) -> Case:
    if client in ("rank", "rank_ex") or client in SELF_CLIENTS:
        n_a = min(n_a, n_b)             # gold column = row index / rows of the one matrix: n_b >= n_a (129 x 81 becomes 81 x 81)
    kw.setdefault("dim", _dims(kpad, ragged))
    if client in SELF_CLIENTS:
        kw.setdefault("n_rows", n_b)
        kw.setdefault("row_lo", (n_b - n_a) // 2 if n_b > n_a else 0)     # a row window inside the matrix
    c = Case(client, tag, kpad, n_a=n_a, n_b=n_b, **kw)
    assert c.L * c.L * c.dim < 2 ** 24 and 0 < c.dim <= c.kpad and c.n_a <= 300
    return c


def _client_defaults(client, kpad, n_a, n_b, i):
    """Per-client parameters of a generic (shape pair / edge) case; i varies the modes over the table."""
    j = i // 2 + i                      # the shapes alternate: keep modes and variants from alternating with them
    if client == "rank":
        return dict(variant=("ties", "noties")[j % 2])
    if client == "rank_ex":
        return dict(mode=MODES[j % 4])
    if client == "topk_mean":
        k = (1, 7, 32)[i % 3]
        return dict(k=min(k, n_b - 2), mode=MODES[j % 2])
    if client == "sim_select":
        n_seg = (1, 3, 16)[i % 3]
        return dict(n_seg=n_seg, seg_cap=max(3, min(48, n_b // 2) // n_seg))
    if client == "sim_sample":
        return dict(n_rows=n_a + 37, row_lo=(5, 32, 37)[i % 3])
    if client == "knn":
        n_seg = (1, 2, 4)[i % 3]
        return dict(n_seg=n_seg, seg_cap=64 // n_seg, k=max(1, min(20, n_b // 3)))
    if client == "stable":
        return dict(k=min((100, 1, 128)[i % 3], n_b), mode=MODES[j % 4], variant="sweep")
    raise ValueError(client)


def _build():
    cases = []
    for client in CLIENTS:
        i = 0
        for kpad in KPADS:                              # every instantiation at the two shapes
            for tag, n_a, n_b, ragged in _shape_pair(kpad):
                cases.append(_make(client, tag, kpad, n_a, n_b, ragged, **_client_defaults(client, kpad, n_a, n_b, i)))
                i += 1
        for kpad in REGIME_KPADS:                       # the full edge list for one width of each regime
            for j, (tag, n_a, n_b) in enumerate(_edges(kpad)):
                cases.append(_make(client, tag, kpad, n_a, n_b, j % 2 == 1, **_client_defaults(client, kpad, n_a, n_b, i)))
                i += 1
    for kpad in REGIME_KPADS:
        bn = bn_for(kpad)
        nb = 16 * bn + 1
        # both TIES instantiations, all four modes, and L = 40 (negative keys) for every client
        for v in ("ties", "noties"):
            cases.append(_make("rank", "L40", kpad, 129, nb, True, variant=v, L=40))
        for mode in MODES:
            cases.append(_make("rank_ex", "modes", kpad, 129, nb, True, mode=mode, L=40))
            cases.append(_make("rank_ex", "modes", kpad, 33, 2 * bn + 1, False, mode=mode))
            for variant, cut, n_b in (("sweep", 100, 1024), ("sweep", 128, 16 * bn), ("sweep", 1, 2 * bn + 1),
                                      ("sample", 20, nb if bn == 64 else 33 * bn + 31), ("whole", 50, nb), ("whole", 200, nb), ("simmat", 60, 2 * bn + 9)):
                cases.append(_make("stable", "modes", kpad, 129, n_b, variant != "sweep", k=cut, mode=mode, variant=variant,
                                   L=40 if variant in ("sample", "whole") and cut != 200 else 3,
                                   seg_cap=256 if variant == "sample" else 0))       # seg_cap = sample_cols of the forced sample
        # sim_select: row windows x segment counts (n_seg > ntiles: empty segments), overflowing seg_cap, both threshold kinds
        n = 263                                         # 5 / 9 tiles, the last holding 7 columns
        for lo, hi in ((0, n), (1, 34), (100, 229)):
            for n_seg in (1, 3, 16):
                cases.append(_make("sim_select", "win", kpad, hi - lo, n, n_seg == 3, row_lo=lo, n_seg=n_seg, seg_cap=max(3, 40 // n_seg),
                                   L=40 if n_seg == 16 else 3))
        # sim_sample: n_samp edges (8 BN + 1: two chunks of 5 and 4 tiles), ld_samp != ld, row_lo not a multiple of 32
        for n_samp in (1, bn + 1, 8 * bn + 1):
            cases.append(_make("sim_sample", "samp", kpad, 129, n_samp, n_samp == 1, n_rows=200, row_lo=37, L=40 if n_samp > bn + 1 else 3))
        # the k-NN chain: thresholds from a sample, main pass, exact selection, long rows for the flagged
        for n_seg, L in ((1, 3), (2, 40), (4, 40)):
            cases.append(_make("knn", "chain", kpad, 129, nb, n_seg == 2, row_lo=100, n_seg=n_seg, seg_cap=64 // n_seg, k=20, L=L))
        # top-k means: the partial sweep (k <= 32) and whole rows (k > 32), both metrics
        for k in (1, 7, 32, 33, 300):
            for mode in MODES[:2]:
                cases.append(_make("topk_mean", "k", kpad, 129, nb, k % 2 == 1, k=k, mode=mode, L=40 if k in (7, 300) else 3))
    # a chunk with fewer than k columns: the host's split keeps chunks at >= 16 tiles until 16 chunks are reached, so the
    # smallest such sweep is 241 tiles of 32 columns = 16 chunks of 16, 16, ..., 1 tiles, the last tile holding 5 columns
    for mode in MODES[:2]:
        cases.append(_make("topk_mean", "short-chunk", 256, 33, 240 * 32 + 5, True, k=32, mode=mode))
    return list(dict.fromkeys(cases))          # a shape named by two lists appears once


ALL_CASES = _build()


def cases_of(client):
    return [c for c in ALL_CASES if c.client == client]
