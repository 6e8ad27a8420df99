"""Case table, staging, reference, routing layer, bounds and mutants of the exact tests of the owner-computes (sharded) relation
step (test_oc_cases.py here, test_oc_exact_gpu.py on the device): k_oc_bases, k_oc_count, k_oc_score / k_oc_score_q in their five
forms, k_oc_apply, k_oc_gv_sum (multike_amd/csrc/mke_oc.hip), k_oc_em_pass2 and k_oc_em_combine (mke_oc_em.hip).  NumPy only.

One global step is STAGED for G virtual ranks (`stage`): positives, negatives as codes with the MKE_OC_NEED_* flags on each group's
first code, slots, owned-slot lists, `per`, the code buffer with `code_off` per home rank (three live-looking gap codes between
the shares, so that an offset taken from the wrong share reads the wrong codes, not the right ones by accident), hub rows, and the
entity-major reference lists — all from the definitions of include/multike_hip.h section 13.  `Ref` is the reference: ONE formula
for a negative's and a positive's loss term and coefficient over `SArith` of score_cases.py ("bound" mode: float64 values with
an error bound each), and a ROUTING layer written from the kernels' work-item structure: who owns a negative (id % G, row id / G),
who scores the own term, which g_all / inbox slot, scratch row, hub copy, relation copy or em_coef entry takes what, which rows
are finished in place, which references a row's second-pass list holds and in which order, how it is cut into segments.  The
collectives are the test's: all-gather = the send blocks side by side, reduce-scatter / all-reduce = float32 sums in rank order.

`staged=True`: between two phases the reference hands on its values ROUNDED TO float32 as exact inputs — what a test of one phase
alone writes into the buffers (the vectors may then be scaled per positive, `vec="sat"`: saturated negatives, sigmoid 1).
`staged=False`: values and bounds are carried through the whole step (the chained test).

Charges (u = 2^-23), all from the table of score_cases.py / update_cases.py: u/2 per rounded operation, 2 u for rsqrtf / rsq /
rcp / exp / log, |a| u/2 + 2^-126 for __expf(a), u/2 for the ln 2 product of __logf, a whole ulp on a stored value, 2^-149 per
operation, the row-sum rule, and k / (1 - k) of the sum of absolute values for a sum of m terms, k = (m - 1) u/2, whatever its
order (the fma chains and butterflies of a gradient vector, the atomics of a row, the rank-ordered sums of the collectives, a
second-pass list with its segments and the combine).  An fma is charged as a product and an addition.  Nothing is fitted.

Bit for bit (quarters, rows_cases.quarters; coefficients powers of two): mke_oc_gv_sum, mke_oc_apply on staged gradient vectors,
the relation rows, the long rows' partial slots and the combined relation partials of mke_oc_pass2, and every structural output.

Poison: a NaN tail row behind tables and accumulators, SENTINEL in every g_all / inbox / mirror / em_coef / em_partials /
rel_grad entry that must not be written, NaN loss partials, extra touched entries; rows that receive atomic adds start at zero.
The accumulators' pad columns hold 0.1 (EmbeddingTable.slot: rsq(0) would turn the pad columns of a row into NaN) and must keep it;
the pad columns of tables, scratch and every vector are exactly 0.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import rows_cases as rc
import score_cases as sc
import update_cases as uc
from rows_cases import FPLS, OLD_TAG, SENTINEL, STRIDES, TAG, quarters, table_dims
from update_cases import ACC_PAD, L2_EPS32, TINY, U, V

f32, f64 = np.float32, np.float64
LOSS_PARTIALS = 2048
NEED_HR, NEED_RT, CODE_MASK = 0x40000000, 0x80000000, 0x3FFFFFFF
LOC_GV, LOC_PLUS, LOC_RT = 0x80000000, 1 << 24, 1 << 23
FORMS = ("atm", "em", "mir", "own", "mirown")
GROUPS = (0, 1, 3, 4, 5, 15, 16, 17, 25, 32, 33, 63, 64)
RANKS = (1, 2, 3, 5, 8, 16)
N_POS = (1, 4, 5, 70)
REL_COPIES = (1, 2, 8, 64)
HOT_COPIES = (1, 3, 64)
LONG_LISTS = (33, 64, 65, 200)
MUTANTS = ("owner_row_swapped", "own_other_owner", "own_both_owners", "slot_m1_as_0", "rt_offset_dropped", "home_mod_g",
           "code_off_last", "flags_unmasked", "equal_as_head", "drop_17th", "wave_last_round", "tail_gv_sign", "rel_tail_sign",
           "rc1_scattered", "rc2_in_place", "hub_in_place", "pos_w_ignored", "scale_twice", "coef_no_plus1", "chunk_ignored",
           "last_segment_dropped", "odd_partial_dropped", "rel_added", "gv_skip_writer0", "old_acc_stored", "no_projection")
# A mutant that provably changes no output: a positive WITHOUT a travelling RT vector (slot_t == -1) whose RT registers are
# nevertheless added to its negatives — they hold zeros (the kernel clears HR / RT / gHR / gRT per positive), and no negative of
# such a positive corrupts the head (the need flag would be set).  test_oc_cases.py asserts the premise on every case.
SILENT_MUTANTS = ("rt_registers_used_without_slot",)


class OCase(NamedTuple):
    stride: int
    dim: int
    G: int
    rank: int               # the rank under test of the phase tests
    N: int
    n_pos: int
    chunks: int = 1
    opt: str = "adagrad"
    scale: float = 1.0
    pos_w: bool = False
    hot: int = 0            # hub rows declared per rank
    hot_copies: int = 3
    rel_copies: int = 1
    refcount: bool = True
    vec: str = "chain"      # "sat": the staged vectors of every third positive are scaled by 8
    long: bool = False      # rows with second-pass lists of 33, 64, 65 and 200 references
    share: int = 0          # negatives of positives 7, 8, ... that corrupt into ONE entity of `rank`: a second-pass list of `share` references
    n_ent: int = 97
    n_rel: int = 6
    lr: float = 0.0625
    tag: str = ""

    @property
    def id(self):
        s = f"s{self.stride}-d{self.dim}-G{self.G}r{self.rank}-N{self.N}-p{self.n_pos}"
        for v in (f"ch{self.chunks}" if self.chunks > 1 else "", self.opt if self.opt != "adagrad" else "",
                  f"sc{self.scale:g}" if self.scale != 1 else "", "pw" if self.pos_w else "",
                  f"hot{self.hot}x{self.hot_copies}" if self.hot else "", f"c{self.rel_copies}" if self.rel_copies > 1 else "",
                  "" if self.refcount else "norc", self.vec if self.vec != "chain" else "", "long" if self.long else "", f"sh{self.share}" if self.share else "",
                  f"e{self.n_ent}" if self.n_ent != 97 else "", self.tag):
            if v:
                s += "-" + v
        return s

    @property
    def fpl(self):
        return self.stride // 16

    @property
    def n_local(self):
        return -(-self.n_ent // self.G)


class Run(NamedTuple):
    case: OCase
    form: str               # one of FORMS
    quarter: int            # mke_tuning.oc_score_quarter: 0, 1 or -1 (by shape)

    @property
    def id(self):
        return f"{self.case.id}/{self.form}-q{self.quarter}"


def quarter_of(c: OCase, oq: int) -> bool:
    """mke_oc_score's choice of kernel."""
    return (c.G >= 4 and c.N <= 8 * c.G and c.stride <= 128) if oq < 0 else bool(oq)


def instantiation(r: Run):
    """(kernel, FPL, mirror, owned, entity-major, power-of-two divisor)."""
    return ("q" if quarter_of(r.case, r.quarter) else "w", r.case.fpl, r.form in ("mir", "mirown"), r.form in ("own", "mirown"),
            r.form != "atm", r.case.G & (r.case.G - 1) == 0)


def all_instantiations():
    forms = ((False, False, False), (False, False, True), (True, False, True), (False, True, True), (True, True, True))
    return {(k, fpl) + f + (p2,) for k in "qw" for fpl in FPLS for f in forms for p2 in (False, True)}


# ----------------------------------------------------------------------------------------------------- staging
class Stage:
    pass


def _table(rng, n, c: OCase):
    """Xavier-like rows with norms in [0.5, 2]: nothing that is compared is ill-conditioned."""
    x = rng.standard_normal((n, c.dim))
    x *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(x, axis=1, keepdims=True)
    t = np.zeros((n, c.stride), dtype=f32)
    t[:, :c.dim] = x
    return t


def _acc(rng, n, c: OCase):
    a = np.full((n, c.stride), ACC_PAD, dtype=f32)
    a[:, :c.dim] = (0.1 + np.abs(quarters(rng, (n, c.dim)))).astype(f32)
    return a


@functools.lru_cache(maxsize=32)
def stage(c: OCase) -> Stage:
    rng = np.random.default_rng([zlib.crc32(c.id.encode())])
    S = Stage()
    G, r, N, P, n_ent = c.G, c.rank, c.N, c.n_pos, c.n_ent
    assert 0 <= r < G and r + 3 * G < n_ent and c.scale in (1.0, 0.5) and N <= 64
    S.ent, S.rel, S.acc_e, S.acc_r = _table(rng, n_ent, c), _table(rng, c.n_rel, c), _acc(rng, n_ent, c), _acc(rng, c.n_rel, c)
    X, Y, Hb = r + G, r + 2 * G, r + 3 * G          # referenced once / twice as a corrupt row; the shared (hub) head
    special = (X, Y, Hb) + ((r + 4 * G,) if c.share else ())
    assert not c.share or (r + 4 * G < n_ent and (P - 7) * N >= c.share and not c.long)
    span = n_ent // G * G

    def draw(n, residue=None):
        e = rng.integers(0, n_ent, n)
        if residue is not None:
            e = e // G * G % span + residue
        for k in range(n):
            while int(e[k]) in special:
                e[k] = (e[k] + (G if residue is not None else 1)) % (span if residue is not None else n_ent)
        return e

    ph, pt, pr = draw(P), draw(P), rng.integers(0, c.n_rel, P)
    cent = np.zeros((P, N), dtype=np.int64)
    cside = np.repeat(rng.integers(0, 2, P)[:, None], N, 1)          # one coin per positive
    for p in range(P):
        cent[p] = draw(N)
    equal = np.zeros((P, N), dtype=bool)
    if c.long:                                                        # lists of 33 / 64 / 65 / 200 references on rank r
        assert P >= sum(LONG_LISTS) and G > 1
        heads = [r + (4 + k) * G for k in range(len(LONG_LISTS))]
        other = lambda a: np.where(np.isin(a, heads), (a + 1) % n_ent, a)     # (a head + 1 belongs to another rank: no head)
        ph, pt, cent = other(ph), other(pt), other(cent)               # a head is the head of its n positives and nothing else:
        at = 0                                                        # its row's list is their n gradient vectors (HR travels)
        for k, n in enumerate(LONG_LISTS):
            ph[at:at + n] = heads[k]
            cside[at:at + n] = 0
            at += n
    elif P >= 5:
        pt[4] = ph[4]                                                 # head == tail
        ph[3], pr[4] = ph[0], pr[2]                                   # a shared head, a shared relation
        if P >= 7:
            ph[5] = ph[6] = Hb
            pr[6] = pr[5]
        if N:
            cent[0] = draw(N, r)                                      # all negatives owned by the rank under test
            cent[0, 0] = X                                            # ... the first a row nothing else references
            if G > 1:
                cent[1] = draw(N, (r + 1) % G)                        # none owned by it
            cside[2] = np.arange(N) % 2                               # both sides: both vectors travel, two slots
            cent[2, 0] = cent[4, 0] = Y                               # a row referenced twice
            if N >= 2 and P >= 7:
                cent[2, 1] = Hb                                       # the hub head, once as a corrupt row
            cent[3, N - 1], cside[3, N - 1] = pt[3], 0                # the negative equals its positive: a corrupted tail
            equal[3, N - 1] = True
        if c.share:                                                   # the first `share` negatives from positive 7 on corrupt into one
            flat = cent[7:].reshape(-1)                               # entity of rank r that nothing else names: its row's list
            flat[:c.share] = r + 4 * G
            cent[7:] = flat.reshape(-1, N)
    S.ph, S.pr, S.pt, S.cent, S.cside, S.equal = ph, pr, pt, cent, cside, equal
    S.X, S.Y, S.Hb = special[:3]
    S.pw = rng.choice(np.array(rc.WEIGHTS, dtype=f32), P) if c.pos_w else None
    S.need_rt = cside.astype(bool).any(1) if N else np.zeros(P, bool)
    S.need_hr = (~S.need_rt | (cside == 0).any(1)) if N else np.ones(P, bool)
    size = -(-P // c.chunks)
    S.parts = [(a, min(P, a + size)) for a in range(0, P, size)]
    S.part_of = np.concatenate([np.full(hi - lo, k) for k, (lo, hi) in enumerate(S.parts)])
    S.sh, S.st = np.full(P, -1), np.full(P, -1)
    S.own_h, S.own_t, S.per = [], [], []
    most = 0
    for lo, hi in S.parts:
        oh, ot = [[] for _ in range(G)], [[] for _ in range(G)]
        for p in range(lo, hi):
            if S.need_hr[p]:
                S.sh[p] = len(oh[ph[p] % G])
                oh[ph[p] % G].append(p - lo)
            if S.need_rt[p]:
                S.st[p] = len(ot[pt[p] % G])
                ot[pt[p] % G].append(p - lo)
        S.own_h.append([np.asarray(v, dtype=np.int32) for v in oh])
        S.own_t.append([np.asarray(v, dtype=np.int32) for v in ot])
        S.per.append(max(1, -(-(hi - lo) // G)))
        most = max([most] + [len(v) for v in oh + ot])
    S.C = most + 2                                                    # two slots per half that nothing may write
    # the code buffer: every home rank's share of every part, three gap codes (a valid entity, corrupted head) behind each
    code = (cent << 1) | cside
    if N:
        code[:, 0] |= S.need_hr * NEED_HR + S.need_rt * NEED_RT
    buf, S.code_off = [], []
    for k, (lo, hi) in enumerate(S.parts):
        off = []
        for g in range(G):
            off.append(len(buf))
            a, b = min(hi, lo + g * S.per[k]), min(hi, lo + (g + 1) * S.per[k])
            if b > a and N:
                buf += code[a:b].ravel().tolist() + [(r << 1) | 1] * 3
        S.code_off.append(off)
    S.codes = np.asarray(buf + [(r << 1) | 1], dtype=np.int64)
    # hub rows per rank: the shared head first, then the heads / tails it owns in position order
    S.hot_slot = None
    if c.hot:
        S.hot_slot = []
        for g in range(G):
            rows = [int(e) // G for e in [Hb] + np.stack([ph, pt], 1).ravel().tolist() if int(e) % G == g]
            rows = list(dict.fromkeys(rows + list(range(c.n_local))))[:c.hot]
            slot = np.full(c.n_local + 1, -1, dtype=np.int32)
            slot[rows] = np.arange(len(rows), dtype=np.int32)
            slot[c.n_local] = 0
            S.hot_slot.append(slot)
    return S


def local_rows(c: OCase, table, g, fill=np.nan):
    """Rank g's shard [n_local + 1, stride]: rows g, g + G, ...; rows past the table are zero rows, the tail row is `fill`."""
    out = np.zeros((c.n_local + 1, c.stride), dtype=f32)
    rows = table[g::c.G]
    out[:len(rows)] = rows
    out[c.n_local] = fill
    return out


def ref_counts(c: OCase, S: Stage, k: int, g: int) -> np.ndarray:
    """mke_oc_count of part k on rank g, by enumeration: the negatives of every home rank, the heads and tails it owns; hub rows
    are not counted as heads / tails.  [n_local + 1], 9 in the tail entry."""
    lo, hi = S.parts[k]
    out = np.zeros(c.n_local + 1, dtype=np.int32)
    out[c.n_local] = 9
    e = S.cent[lo:hi].ravel()
    np.add.at(out, e[e % c.G == g] // c.G, 1)
    for ids in (S.ph[lo:hi], S.pt[lo:hi]):
        rows = ids[ids % c.G == g] // c.G
        if S.hot_slot is not None:
            rows = rows[S.hot_slot[g][rows] < 0]
        np.add.at(out, rows, 1)
    return out


def em_lists(c: OCase, S: Stage, g: int):
    """The second pass's references on rank g, in list order: arrays (row, kind, p, n, locator, cidx) sorted by row, a row's
    negatives by (position, n) first, then own term / gradient vectors by (position, kind) — mke_oc_em_plan's element order under
    a stable sort by row.  Rows >= n_local are relation rows.  kind: 0 negative, 1 own term, 2 + gv (head), 3 - gv (tail),
    4 relation + gv of HR, 5 relation + gv of RT."""
    G, N, nl = c.G, c.N, c.n_local
    recs = []
    P = c.n_pos
    for p in range(P):
        ch = int(S.part_of[p])
        for n in range(N):
            e, rt = int(S.cent[p, n]), int(S.cside[p, n])
            if e % G == g:
                src, slot = (S.pt[p], S.st[p]) if rt else (S.ph[p], S.sh[p])
                recs.append((e // G, 0, p, n, (ch << 28) | (int(src) % G << 24) | (rt << 23) | int(slot), p * (N + 1) + n))
    for p in range(P):
        ch = int(S.part_of[p])
        hr = S.sh[p] >= 0
        own, rt = (S.pt[p], 0) if hr else (S.ph[p], 1)
        src, slot = (S.pt[p], S.st[p]) if rt else (S.ph[p], S.sh[p])
        if own % G == g:
            recs.append((int(own) // G, 1, p, N, (ch << 28) | (int(src) % G << 24) | (rt << 23) | int(slot), p * (N + 1) + N))
        if S.sh[p] >= 0 and S.ph[p] % G == g:
            recs.append((int(S.ph[p]) // G, 2, p, N, (ch << 28) | LOC_GV | int(S.sh[p]), 0))
        if S.st[p] >= 0 and S.pt[p] % G == g:
            recs.append((int(S.pt[p]) // G, 3, p, N, (ch << 28) | LOC_GV | LOC_RT | int(S.st[p]), 0))
        if S.sh[p] >= 0 and S.ph[p] % G == g:
            recs.append((nl + int(S.pr[p]), 4, p, N, (ch << 28) | LOC_GV | LOC_PLUS | int(S.sh[p]), 0))
        if S.st[p] >= 0 and S.pt[p] % G == g:
            recs.append((nl + int(S.pr[p]), 5, p, N, (ch << 28) | LOC_GV | LOC_PLUS | LOC_RT | int(S.st[p]), 0))
    a = np.asarray(recs, dtype=np.int64).reshape(-1, 6)
    a = a[np.argsort(a[:, 0], kind="stable")]
    return a


def em_items(rows: np.ndarray):
    """(first reference, end, row, partial slot or -1) per work item, and (row, first slot, end slot) per long row."""
    items, longs, part = [], [], 0
    if len(rows):
        cut = np.flatnonzero(np.diff(rows)) + 1
        for lo, hi in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(rows)]])):
            nseg = -(-(hi - lo) // 32)
            if nseg > 1:
                longs.append((int(rows[lo]), part, part + nseg))
            for s in range(nseg):
                items.append((lo + 32 * s, min(hi, lo + 32 * s + 32), int(rows[lo]), part + s if nseg > 1 else -1))
            part += nseg if nseg > 1 else 0
    return items, longs, part


# ----------------------------------------------------------------------------------------------------- sums with their charge
def _sum(dest, n_dest, val, err, sign=None):
    """Sums of the rows `val` per destination, in any order: (values, bounds, terms per destination)."""
    st = val.shape[1]
    sv, se, tot = (np.zeros((n_dest, st)) for _ in range(3))
    sg = np.ones(len(dest)) if sign is None else np.asarray(sign, dtype=f64)
    np.add.at(sv, dest, sg.reshape(-1, 1) * val)
    np.add.at(se, dest, err)
    np.add.at(tot, dest, np.abs(val))
    m = np.bincount(dest, minlength=n_dest).reshape(-1, 1)
    k = np.maximum(m - 1, 0) * 0.5 * U
    se += k / (1 - k) * tot + np.where(m > 1, TINY, 0.0)
    return sv, se, m[:, 0]


def _f32(v):
    return np.asarray(v, dtype=f32).astype(f64)


class Ref:
    """The reference of one case for every rank and phase."""

    def __init__(self, c: OCase, quarter=0, mutant="", staged=True):
        assert mutant in ("",) + MUTANTS + SILENT_MUTANTS, mutant
        self.c, self.S, self.mut, self.staged = c, stage(c), mutant, staged
        self.quarter = quarter_of(c, quarter)
        self.ar = sc.SArith("bound")
        self.depth = c.fpl + 6
        self.live = np.arange(c.stride) < c.dim
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            self._bases()
        self._have_terms = False

    def _ensure(self):
        if not self._have_terms:
            with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
                self._terms()
            self._have_terms = True

    # ---- helpers
    def _norm(self, W):
        ar = self.ar
        inv = ar.rsqrt(ar.maximum(ar.dots(W, W, self.depth), L2_EPS32))
        return W * inv, inv

    def _relay(self, val, err, fac=1.0):
        """What the next phase reads: the float32 buffer itself (staged), or the value with its bound (chained)."""
        return (_f32(val) * fac, np.zeros_like(err)) if self.staged else (val, err)

    def _buf(self, n_rows, rows, val, err, fill=SENTINEL):
        """[n_rows + 1, stride] with `fill` in the rows that are not written and in the tail row; bound 0 in the pad columns."""
        v, e = np.full((n_rows + 1, val.shape[1]), fill, dtype=f64), np.zeros((n_rows + 1, val.shape[1]))
        v[rows], e[rows] = val, np.where(self.live[:val.shape[1]] if val.shape[1] == self.c.stride else True, err, 0.0)
        return v, e

    # ---- phase 1: the bases
    def _bases(self):
        c, S, ar = self.c, self.S, self.ar
        En, _ = self._norm(ar.lift(S.ent.astype(f64)))
        Rn, _ = self._norm(ar.lift(S.rel.astype(f64)))
        HR = ar.take(En, S.ph) + ar.take(Rn, S.pr)
        RT = ar.take(Rn, S.pr) - ar.take(En, S.pt)
        self.HR, self.RT = HR, RT
        fac = np.where(np.arange(c.n_pos) % 3 == 1, 8.0, 1.0).reshape(-1, 1) if (c.vec == "sat" and self.staged) else 1.0
        self.HRv, self.RTv = V(*self._relay(HR.val, HR.err, fac)), V(*self._relay(RT.val, RT.err, fac))

    def send(self, k, g):
        """Rank g's send block of part k: (values, bounds) [2 C + 1, stride], SENTINEL where nothing is written."""
        c, S = self.c, self.S
        lo, _ = S.parts[k]
        ph_, pt_ = lo + S.own_h[k][g], lo + S.own_t[k][g]
        rows = np.concatenate([np.arange(len(ph_)), S.C + np.arange(len(pt_))]).astype(np.int64)
        val = np.concatenate([self.HR.val[ph_], self.RT.val[pt_]]).reshape(-1, c.stride)
        err = np.concatenate([self.HR.err[ph_], self.RT.err[pt_]]).reshape(-1, c.stride)
        return self._buf(2 * S.C, rows, val, err)

    def vall64(self, k):
        """The all-gathered vectors of part k with their bounds: [G, 2 C, stride] each, SENTINEL in unused slots."""
        c, S = self.c, self.S
        v, e = np.full((c.G, 2 * S.C, c.stride), SENTINEL, dtype=f64), np.zeros((c.G, 2 * S.C, c.stride))
        lo, hi = S.parts[k]
        for p in range(lo, hi):
            if S.sh[p] >= 0:
                v[S.ph[p] % c.G, S.sh[p]], e[S.ph[p] % c.G, S.sh[p]] = self.HRv.val[p], self.HRv.err[p]
            if S.st[p] >= 0:
                v[S.pt[p] % c.G, S.C + S.st[p]], e[S.pt[p] % c.G, S.C + S.st[p]] = self.RTv.val[p], self.RTv.err[p]
        return v, e

    def vall(self, k):
        """... as the float32 buffer a staged score launch reads (and a peer-direct one leaves in its mirror)."""
        return self.vall64(k)[0].astype(f32)

    # ---- the codes as the kernels read them
    def _codes_seen(self):
        """[P, N] raw codes: position i of part k reads codes[code_off[home] + (i - home per) N + n], home = i / per."""
        c, S = self.c, self.S
        out = np.zeros((c.n_pos, c.N), dtype=np.int64)
        for k, (lo, hi) in enumerate(S.parts):
            i = np.arange(hi - lo)
            home = i % c.G if self.mut == "home_mod_g" else i // S.per[k]
            off = np.asarray(S.code_off[k], dtype=np.int64)
            if self.mut == "code_off_last":                       # the last share that holds positives, taken as if no gap preceded it
                last = int((hi - lo - 1) // S.per[k])
                off[last] -= 3 * last
            at = off[home] + (i - home * S.per[k]) * c.N
            idx = np.clip(at[:, None] + np.arange(c.N)[None, :], 0, len(S.codes) - 1)
            out[lo:hi] = S.codes[idx]
        return out

    # ---- the formula, written once
    def _terms(self):
        c, S, ar = self.c, self.S, self.ar
        P, N = c.n_pos, c.N
        raw = self._codes_seen()
        code = raw if self.mut == "flags_unmasked" else raw & CODE_MASK
        self.n_ent_id = (code >> 1).ravel()                          # the corrupt entity the kernel computes with
        e = np.minimum(self.n_ent_id, c.n_ent - 1)
        side = (code & 1).ravel().astype(bool)
        if self.mut == "equal_as_head":
            side = side | S.equal.ravel()
        self.n_side, self.n_p, self.n_n = side, np.repeat(np.arange(P), N), np.tile(np.arange(N), P)
        sideH = side.reshape(-1, 1)
        C = ar.lift(S.ent[e].astype(f64))
        base = ar.where(sideH, ar.take(self.RTv, self.n_p), ar.take(self.HRv, self.n_p))
        cinv = ar.rsqrt(ar.maximum(ar.dots(C, C, self.depth), L2_EPS32))
        d = ar.fma(ar.free(cinv, np.where(sideH, 1.0, -1.0)), C, base)
        y = ar.dots(d, d, self.depth)
        t = ar.exp(ar.neg(y))
        s1 = ar.const(1.0, y) + t
        self.n_c = ar.free(t * ar.rcp(s1), -2.0 * c.scale)
        self.n_loss, self.n_d, self.n_C, self.n_cinv, self.n_y = ar.log(s1), d, C, cinv, y
        self.n_cd = d * self.n_c
        # the positives' own terms
        use_hr = S.sh >= 0
        self.o_hr = use_hr
        self.o_ent = np.where(use_hr, S.pt, S.ph)
        pw = np.ones((P, 1)) if (S.pw is None or self.mut == "pos_w_ignored") else S.pw.astype(f64).reshape(-1, 1)
        En, _ = self._norm(ar.lift(S.ent[self.o_ent].astype(f64)))
        Vv = ar.where(use_hr.reshape(-1, 1), self.HRv, self.RTv)
        d = ar.fma(ar.free(ar.const(1.0, En), np.where(use_hr, -1.0, 1.0).reshape(-1, 1)), En, Vv)
        x = ar.dots(d, d, self.depth)
        ex = ar.exp(ar.neg(x))
        s1 = ar.const(1.0, x) + ex
        self.o_c = ar.free(ar.rcp(s1), 2.0 * c.scale * pw)
        self.o_loss, self.o_x = ar.free(x + ar.log(s1), pw), x
        self.o_d = d
        self.o_cd = d * self.o_c

    # ---- routing of the score launch
    def _scored(self, k, g):
        """(indices of the negatives rank g scores in part k, positions whose own term it scores)."""
        c, S = self.c, self.S
        lo, hi = S.parts[k]
        inpart = (self.n_p >= lo) & (self.n_p < hi)
        e = self.n_ent_id
        mine = ((e // c.G == g) if self.mut == "owner_row_swapped" else (e % c.G == g)) & inpart
        if self.mut == "drop_17th" and self.quarter:
            mine &= self.n_n != 16
        if self.mut == "wave_last_round" and not self.quarter:
            per_round = 4 * (2 if c.fpl <= 5 else 1)
            for p in range(lo, hi):
                own = np.flatnonzero(mine & (self.n_p == p))
                if len(own) % per_round:
                    mine[own[len(own) // per_round * per_round:]] = False
        pos = np.arange(lo, hi)
        a, b = np.where(self.o_hr, S.pt, S.ph)[pos] % c.G == g, np.where(self.o_hr, S.ph, S.pt)[pos] % c.G == g
        own = {"own_other_owner": b, "own_both_owners": a | b}.get(self.mut, a)
        return np.flatnonzero(mine), pos[own]

    def _hub(self, g, rows, k):
        c, S = self.c, self.S
        if S.hot_slot is None:
            return rows
        hs = S.hot_slot[g][rows]
        return np.where(hs >= 0, c.n_local + (k % c.hot_copies) * c.hot + hs, rows)

    def score(self, k, g, form="em"):
        """What mke_oc_score of rank g leaves behind for part k."""
        self._ensure()
        c, S = self.c, self.S
        G, N, C2, st = c.G, c.N, 2 * S.C, c.stride
        lo, hi = S.parts[k]
        ni, oi = self._scored(k, g)
        out = {}
        rt_off = 0 if self.mut == "rt_offset_dropped" else S.C
        # the gradient-vector slots: every live slot of the part is written (zeros without a term)
        pos = np.arange(lo, hi)
        slot_h = (S.ph % G) * C2 + S.sh
        slot_t = (S.pt % G) * C2 + rt_off + S.st
        dest = np.concatenate([np.where(self.n_side[ni], slot_t[self.n_p[ni]], slot_h[self.n_p[ni]]), np.where(self.o_hr[oi], slot_h[oi], slot_t[oi])])
        val = np.concatenate([self.n_cd.val[ni], self.o_cd.val[oi]]).reshape(-1, st)
        err = np.concatenate([self.n_cd.err[ni], self.o_cd.err[oi]]).reshape(-1, st)
        sv, se, _ = _sum(dest.astype(np.int64), G * C2, val, err)
        written = np.unique(np.concatenate([slot_h[pos][S.sh[pos] >= 0], slot_t[pos][S.st[pos] >= 0]])).astype(np.int64)
        if self.mut == "slot_m1_as_0":                              # a vector that does not travel written to slot 0 of its half
            extra = np.concatenate([(S.ph[pos] % G * C2)[S.sh[pos] < 0], (S.pt[pos] % G * C2 + S.C)[S.st[pos] < 0]])
            sv[extra], se[extra] = 0.0, 0.0
            written = np.unique(np.concatenate([written, extra])).astype(np.int64)
        out["g_all"] = self._buf(G * C2, written, sv[written], se[written])
        # the coefficients (entity-major) and the loss
        step = N if self.mut == "coef_no_plus1" else N + 1
        coef_v, coef_e = np.full(c.n_pos * (N + 1) + 1, SENTINEL), np.zeros(c.n_pos * (N + 1) + 1)
        ci = np.concatenate([self.n_p[ni] * step + self.n_n[ni], oi * step + N]).astype(np.int64)
        coef_v[ci] = np.concatenate([self.n_c.val[ni, 0], self.o_c.val[oi, 0]])
        coef_e[ci] = np.concatenate([self.n_c.err[ni, 0], self.o_c.err[oi, 0]])
        out["coef"] = (coef_v, coef_e)
        lv = np.concatenate([self.n_loss.val[ni, 0], self.o_loss.val[oi, 0]])
        le = np.concatenate([self.n_loss.err[ni, 0], self.o_loss.err[oi, 0]])
        waves = LOSS_PARTIALS * (16 if self.quarter else 4)
        m_thread = (N + 1) * (1 + (hi - lo) // waves)
        sc2 = c.scale * (c.scale if self.mut == "scale_twice" else 1.0)
        out["loss"] = (float(lv.sum() * sc2), float(c.scale * (le.sum() + m_thread * 0.5 * U * np.abs(lv).sum()) + TINY))
        out["mirror"] = self.vall(k)
        if form != "atm":
            return out
        # atomics form: scratch rows, flags, rows finished in place, reference counts
        hot = S.hot_slot[g] if S.hot_slot is not None else None
        rcnt = ref_counts(c, S, k, g)
        rows_n = self.n_ent_id[ni] % G if self.mut == "owner_row_swapped" else self.n_ent_id[ni] // G
        ok = rows_n < c.n_local
        ni, rows_n = ni[ok], rows_n[ok]
        is_hot = hot[rows_n] >= 0 if hot is not None else np.zeros(len(ni), bool)
        cnt = np.where(is_hot & (self.mut != "hub_in_place"), 2, rcnt[rows_n])
        ip = (cnt == 1) if c.refcount else np.zeros(len(ni), bool)
        if self.mut == "rc1_scattered":
            ip[:] = False
        if self.mut == "rc2_in_place" and c.refcount:
            ip |= cnt == 2
        a, b = ~ip, ip
        n_grad = c.n_local + (c.hot * c.hot_copies if hot is not None else 0)
        o_rows = self.o_ent[oi] // G
        dest = np.concatenate([rows_n[a], self._hub(g, o_rows, oi - lo)]).astype(np.int64)
        sign = np.concatenate([np.where(self.n_side[ni[a]], 1.0, -1.0), np.where(self.o_hr[oi], -1.0, 1.0)])
        val = np.concatenate([self.n_cd.val[ni[a]], self.o_cd.val[oi]]).reshape(-1, st)
        err = np.concatenate([self.n_cd.err[ni[a]], self.o_cd.err[oi]]).reshape(-1, st)
        out["grad_entries"] = (dest, sign, val, err, np.concatenate([rows_n[a], o_rows]).astype(np.int64))
        touched = np.full(c.n_local + 64, OLD_TAG, dtype=np.int32)
        touched[np.concatenate([rows_n[a], o_rows]).astype(np.int64)] = TAG
        touched[c.n_local:] = TAG
        out["touched_ent"] = touched
        ent, acc = local_rows(c, S.ent, g).astype(f64), local_rows(c, S.acc_e, g).astype(f64)
        ent_e, acc_e = np.zeros_like(ent), np.zeros_like(acc)
        if b.any():
            ar = self.ar
            cfg = sc.SCase(c.stride, c.dim, 0, ent_norm=1, opt=c.opt, lr=c.lr)
            nb = ni[b]
            w2, a2 = sc.in_place(ar, cfg, ar.take(self.n_C, nb), ar.lift(acc[rows_n[b]]), ar.take(self.n_cd, nb), ar.take(self.n_cinv, nb),
                                 self.n_side[nb].reshape(-1, 1), self.mut)
            ent[rows_n[b]], ent_e[rows_n[b]] = np.where(self.live, w2.val, 0.0), np.where(self.live, w2.err, 0.0)
            if a2 is not None:
                acc[rows_n[b]], acc_e[rows_n[b]] = np.where(self.live, a2.val, float(ACC_PAD)), np.where(self.live, a2.err, 0.0)
            rcnt[rows_n[b]] = 0
        out["ent"], out["acc"], out["ref_count"], out["in_place_rows"] = (ent, ent_e), (acc, acc_e), rcnt, rows_n[b]
        sv, se, m = _sum(dest, n_grad, val, err, sign)
        out["ent_grad"] = self._buf(n_grad, np.flatnonzero(m > 0), sv[m > 0], se[m > 0])
        return out

    # ---- the collectives, done by the test in float32 in rank order
    def gv(self, k, g, scores=None):
        """Rank g's reduce-scattered block of part k: sum over the writers, in rank order, of their g_all slice — [2 C + 1, stride]
        values and bounds, SENTINEL where nobody writes."""
        c, S = self.c, self.S
        C2 = 2 * S.C
        scores = scores or [self.score(k, w, "em") for w in range(c.G)]
        first = 1 if self.mut == "gv_skip_writer0" else 0
        vals, errs = [], []
        for w in range(first, c.G):
            v, e = scores[w]["g_all"]
            v, e = self._relay(v[g * C2:(g + 1) * C2], e[g * C2:(g + 1) * C2])
            vals.append(v)
            errs.append(e)
        rows = np.concatenate([np.arange(len(S.own_h[k][g])), S.C + np.arange(len(S.own_t[k][g]))]).astype(np.int64)
        if not vals:
            return self._buf(C2, rows, np.zeros((len(rows), c.stride)), np.zeros((len(rows), c.stride)))
        n = len(vals)
        val, err = np.concatenate([v[rows] for v in vals]), np.concatenate([e[rows] for e in errs])
        sv, se, _ = _sum(np.tile(np.arange(len(rows)), n), len(rows), val, err)
        return self._buf(C2, rows, sv, se)

    # ---- phase 4: apply (atomics form), on any gradient vectors
    def apply_entries(self, k, g, gv_val, gv_err):
        """(scratch rows, signs, relation rows with their copy, values, bounds) of mke_oc_apply."""
        c, S = self.c, self.S
        lo, _ = S.parts[k]
        nh, nt = len(S.own_h[k][g]), len(S.own_t[k][g])
        sub = np.arange(nh + nt)
        pos = lo + np.concatenate([S.own_h[k][g], S.own_t[k][g]]).astype(np.int64)
        rows = np.concatenate([S.ph[pos[:nh]], S.pt[pos[nh:]]]) // c.G
        slot = np.concatenate([np.arange(nh), S.C + np.arange(nt)]).astype(np.int64)
        sign = np.concatenate([np.ones(nh), -np.ones(nt) if self.mut != "tail_gv_sign" else np.ones(nt)])
        rsign = np.concatenate([np.ones(nh), np.ones(nt) if self.mut != "rel_tail_sign" else -np.ones(nt)])
        rel = (sub % c.rel_copies) * c.n_rel + S.pr[pos]
        return self._hub(g, rows, sub).astype(np.int64), sign, rel.astype(np.int64), rsign, rows, S.pr[pos], gv_val[slot], gv_err[slot]

    def apply(self, k, g, gv_val, gv_err, base=None):
        """ent_grad (on top of the score launch's entries `base`), rel_grad with its copies, both flag arrays."""
        c = self.c
        dest, sign, rel, rsign, rows, rrows, val, err = self.apply_entries(k, g, gv_val, gv_err)
        n_grad = c.n_local + (c.hot * c.hot_copies if self.S.hot_slot is not None else 0)
        te, tr = np.full(c.n_local + 64, OLD_TAG, dtype=np.int32), np.full(c.n_rel + 64, OLD_TAG, dtype=np.int32)
        te[c.n_local:], tr[c.n_rel:] = TAG, TAG
        brow = rows.astype(np.int64)
        if base is not None:
            bd, bs, bv, be, bb = base["grad_entries"]
            dest, sign, val, err = np.concatenate([bd, dest]), np.concatenate([bs, sign]), np.concatenate([bv, val]), np.concatenate([be, err])
            brow = np.concatenate([bb, brow])
            te = base["touched_ent"].copy()
        te[rows], tr[rrows] = TAG, TAG
        sv, se, m = _sum(dest, n_grad, val, err, sign)
        out = {"ent_grad": self._buf(n_grad, np.flatnonzero(m > 0), sv[m > 0], se[m > 0]), "touched_ent": te, "touched_rel": tr,
               "row_sums": _sum(brow, c.n_local, val, err, sign)}     # a row's scratch row and hub copies together (the update's sum)
        n = len(rel)
        sv, se, m = _sum(rel, c.rel_copies * c.n_rel, val[len(val) - n:], err[len(err) - n:], rsign)
        out["rel_grad"] = self._buf(c.rel_copies * c.n_rel, np.flatnonzero(m > 0), sv[m > 0], se[m > 0])
        return out

    # ---- phase 6: the second pass, on any coefficients / vectors / gradient vectors
    def pass2(self, g, coef, vall, gvs, start=None):
        """mke_oc_pass2 (+ combine) of rank g.  coef: (values, bounds) [P (N + 1) + 1]; vall[k]: (values, bounds) [G, 2 C, stride] of
        part k; gvs[k]: (values, bounds) [2 C (+ 1), stride].  -> ent, acc (local, with bounds), rel_grad copy 0 [n_rel + 1, stride]
        (SENTINEL where not stored), partials [slots + 1, stride + 16] (SENTINEL where not written), written coefficient mask."""
        c, S, ar = self.c, self.S, self.ar
        st, nl = c.stride, c.n_local
        L = em_lists(c, S, g)
        items, longs, n_part = em_items(L[:, 0])
        n = len(L)
        val, err, cval, cerr = np.zeros((n, st)), np.zeros((n, st)), np.zeros(n), np.zeros(n)
        for x in range(n):
            row, kind, p, _, loc, cidx = (int(v) for v in L[x])
            ch = 0 if self.mut == "chunk_ignored" else (loc >> 28) & 7
            slot = (loc & 0x7FFFFF) + (S.C if loc & LOC_RT else 0)
            if kind >= 2:
                sg = -1.0 if kind == 3 else 1.0
                if (kind == 3 and self.mut == "tail_gv_sign") or (kind == 5 and self.mut == "rel_tail_sign"):
                    sg = -sg
                val[x], err[x] = sg * gvs[ch][0][slot], gvs[ch][1][slot]
            else:
                v = V(vall[ch][0][(loc >> 24) & 15, slot], vall[ch][1][(loc >> 24) & 15, slot])
                cf = V(np.asarray(coef[0][cidx]), np.asarray(coef[1][cidx]))
                t = v * cf
                sg = 1.0 if loc & LOC_RT else -1.0
                val[x], err[x], cval[x], cerr[x] = sg * t.val, t.err, cf.val, cf.err
        # segments, then rows
        seg_of = np.zeros(n, dtype=np.int64)
        keep = np.ones(n, bool)
        for w, (lo, hi, row, part) in enumerate(items):
            seg_of[lo:hi] = w
        parts_v = np.full((n_part + 1, st + 16), SENTINEL)
        if n:
            pv, pe, _ = _sum(seg_of, len(items), val, err)
            cv, ce, _ = _sum(seg_of, len(items), cval.reshape(-1, 1), cerr.reshape(-1, 1))
        for w, (lo, hi, row, part) in enumerate(items):
            if part >= 0:
                parts_v[part, :st], parts_v[part, st:] = pv[w], cv[w, 0]
        for row, p0, p1 in longs:
            last = [w for w, it in enumerate(items) if it[3] == p1 - 1][0]
            if self.mut == "last_segment_dropped" or (self.mut == "odd_partial_dropped" and (p1 - p0) % 2):
                keep[items[last][0]:items[last][1]] = False
        urows, inv_ = np.unique(L[:, 0], return_inverse=True) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        gv_, ge_, _ = _sum(inv_[keep], len(urows), val[keep], err[keep]) if n else (np.zeros((0, st)),) * 3
        cs_, ce_, _ = _sum(inv_[keep], len(urows), cval[keep].reshape(-1, 1), cerr[keep].reshape(-1, 1)) if n else (np.zeros((0, 1)),) * 3
        is_rel = urows >= nl
        rel_v = np.full((c.n_rel + 1, st), SENTINEL) if start is None else start.astype(f64).copy()
        rel_e = np.zeros_like(rel_v)
        rr = urows[is_rel] - nl
        rel_v[rr] = (rel_v[rr] if self.mut == "rel_added" else 0.0) + gv_[is_rel]
        rel_e[rr] = np.where(self.live, ge_[is_rel], 0.0)
        ent, acc = local_rows(c, self._ent_now, g).astype(f64), local_rows(c, S.acc_e, g).astype(f64)
        ent_e, acc_e = np.zeros_like(ent), np.zeros_like(acc)
        er = urows[~is_rel]
        if len(er):
            w = ar.lift(ent[er])
            ghat = V(gv_[~is_rel], ge_[~is_rel])
            csum = V(cs_[~is_rel], ce_[~is_rel])
            s = ar.dots(w, w, self.depth)
            inv = ar.rsqrt(ar.maximum(s, L2_EPS32))
            g2 = ar.fma(csum * inv, w, ghat)
            dot = ar.dots(w, g2, self.depth)
            live = (ar.val(s) > L2_EPS32) & (self.mut != "no_projection")
            g3 = ar.msub(g2, w, ar.select(live, dot * inv * inv)) * inv
            if c.opt == "adagrad":
                w2, a2 = uc.rule_adagrad(ar, w, g3, ar.lift(acc[er]), c.lr)
                if self.mut == "old_acc_stored":
                    a2 = ar.lift(acc[er])
                acc[er], acc_e[er] = np.where(self.live, a2.val, float(ACC_PAD)), np.where(self.live, a2.err, 0.0)
            else:
                w2 = uc.rule_sgd(ar, w, g3, c.lr)
            ent[er], ent_e[er] = np.where(self.live, w2.val, 0.0), np.where(self.live, w2.err, 0.0)
        return {"ent": (ent, ent_e), "acc": (acc, acc_e), "rel_grad": (rel_v, rel_e), "partials": (parts_v, None),
                "lists": L, "items": items, "longs": longs}

    @property
    def _ent_now(self):
        return self.S.ent

    # ---- the relation table's update from the all-reduced gradient (mke_rows_update_multi: every row, the copies summed)
    def rel_update(self, entries):
        """entries: (relation row, values, bounds) of everything the step added to the relation gradient on any rank and copy."""
        c, S, ar = self.c, self.S, self.ar
        row, val, err = entries
        sv, se, _ = _sum(row, c.n_rel, val, err)
        w = ar.lift(S.rel.astype(f64))
        g = uc.jacobian(ar, w, V(sv, se), self.depth)
        if c.opt == "adagrad":
            w2, a2 = uc.rule_adagrad(ar, w, g, ar.lift(S.acc_r.astype(f64)), c.lr)
        else:
            w2, a2 = uc.rule_sgd(ar, w, g, c.lr), ar.lift(S.acc_r.astype(f64))
        fin = lambda x, pad: (np.concatenate([np.where(self.live, x.val, pad), np.full((1, c.stride), np.nan)]),
                              np.concatenate([np.where(self.live, x.err, 0.0), np.zeros((1, c.stride))]))
        return fin(w2, 0.0), fin(a2, float(ACC_PAD))

    # ---- the whole step
    def step(self, form="em"):
        """Every rank's tables after the step, the relation table, the loss: {"ent": [per rank (values, bounds)], "acc": [...],
        "rel": (values, bounds), "rel_acc": ..., "loss": (value, bound)}."""
        c, S, ar = self.c, self.S, self.ar
        G = c.G
        K = len(S.parts)
        f = "atm" if form == "atm" else "em"
        assert f == "em" or K == 1
        scores = [[self.score(k, g, f) for g in range(G)] for k in range(K)]
        gvs = [[self.gv(k, g, scores[k]) for g in range(G)] for k in range(K)]
        loss = (sum(scores[k][g]["loss"][0] for k in range(K) for g in range(G)), sum(scores[k][g]["loss"][1] for k in range(K) for g in range(G)))
        out = {"ent": [], "acc": [], "loss": loss, "touched_ent": [], "touched_rel": []}
        te0, tr0 = np.full(c.n_local + 64, OLD_TAG, dtype=np.int32), np.full(c.n_rel + 64, OLD_TAG, dtype=np.int32)
        te0[c.n_local:], tr0[c.n_rel:] = TAG, TAG                     # (the update launch compares the flags, it does not clear them)
        rel_rows, rel_val, rel_err = [], [], []
        for g in range(G):
            if f == "em":
                coef = (np.full(c.n_pos * (c.N + 1) + 1, SENTINEL), np.zeros(c.n_pos * (c.N + 1) + 1))
                for k in range(K):
                    m = scores[k][g]["coef"][0] != SENTINEL
                    coef[0][m], coef[1][m] = scores[k][g]["coef"][0][m], scores[k][g]["coef"][1][m]
                coef = self._relay(*coef)
                vall = [self.vall64(k) for k in range(K)]
                p2 = self.pass2(g, coef, vall, [self._relay(*gvs[k][g]) for k in range(K)])
                out["ent"].append(p2["ent"])
                out["acc"].append(p2["acc"])
                out["touched_ent"].append(te0)                        # entity-major: no flag is written
                out["touched_rel"].append(tr0)
                rv, re_ = p2["rel_grad"]
                rows = np.unique(p2["lists"][:, 0][p2["lists"][:, 0] >= c.n_local] - c.n_local)
                rel_rows.append(rows)
                rel_val.append(rv[rows])
                rel_err.append(re_[rows])
            else:
                gvv, gve = self._relay(*gvs[0][g])
                ap = self.apply(0, g, gvv, gve, scores[0][g])
                dest, sign, rel, rsign, rows, rrows, val, err = self.apply_entries(0, g, gvv, gve)
                rel_rows.append(rrows)
                rel_val.append(rsign.reshape(-1, 1) * val)
                rel_err.append(err)
                out["touched_ent"].append(ap["touched_ent"])
                out["touched_rel"].append(ap["touched_rel"])
                out["ent"].append(self._ent_update(g, scores[0][g], ap))
                out["acc"].append(out["ent"][-1][2:])
                out["ent"][-1] = out["ent"][-1][:2]
        out["rel"], out["rel_acc"] = self.rel_update((np.concatenate(rel_rows).astype(np.int64), np.concatenate(rel_val).reshape(-1, c.stride),
                                                      np.concatenate(rel_err).reshape(-1, c.stride)))
        return out

    def _ent_update(self, g, score, ap):
        """The shard after mke_rows_update_multi on the touched rows: the scratch row + the hub copies, Jacobian, rule."""
        c, S, ar = self.c, self.S, self.ar
        (ent, ent_e), (acc, acc_e) = (a.copy() for a in score["ent"]), (a.copy() for a in score["acc"])
        tot, tote, _ = ap["row_sums"]
        rows = np.flatnonzero(ap["touched_ent"][:c.n_local] == TAG)
        if len(rows):
            w = ar.lift(ent[rows])
            gg = uc.jacobian(ar, w, V(tot[rows], tote[rows]), self.depth)
            if c.opt == "adagrad":
                w2, a2 = uc.rule_adagrad(ar, w, gg, ar.lift(acc[rows]), c.lr)
                acc[rows], acc_e[rows] = np.where(self.live, a2.val, float(ACC_PAD)), np.where(self.live, a2.err, 0.0)
            else:
                w2 = uc.rule_sgd(ar, w, gg, c.lr)
            ent[rows], ent_e[rows] = np.where(self.live, w2.val, 0.0), np.where(self.live, w2.err, 0.0)
        return ent, ent_e, acc, acc_e


# ----------------------------------------------------------------------------------------------------- comparison
canon = sc.canon


def compare(named):
    """named: [(name, got, (values, bounds or None))] -> (problems, ratios); bounds None = bit for bit (sign of zero aside)."""
    problems, ratios = [], {}
    for name, got, want in named:
        if isinstance(want, tuple):
            if want[1] is None:
                sc._cmp(name, np.asarray(got), (np.asarray(want[0], dtype=f32), None), problems, ratios)
            elif np.ndim(want[0]) == 0:
                r = abs(float(got) - want[0]) / want[1]
                ratios[name] = r
                if not (np.isfinite(got) and r <= 1):
                    problems.append(f"{name}: error / bound = {r:.3g}")
            else:
                sc._cmp(name, np.asarray(got), want, problems, ratios)
        elif not np.array_equal(got, want):
            problems.append(f"{name}: differs from the reference")
    return problems, ratios


def moved(a, b, factor=4.0) -> bool:
    """Does output b (a mutant's) differ from a (the reference's, with its bounds) by more than `factor` bounds, or structurally?"""
    if not isinstance(a, tuple):
        return not np.array_equal(a, b)
    av, ae = a
    bv = b[0]
    if np.ndim(av) == 0:
        return abs(av - bv) > factor * ae
    av, bv = np.asarray(av, dtype=f64), np.asarray(bv, dtype=f64)
    if av.shape != bv.shape:
        return True
    nan = np.isnan(av)
    if not np.array_equal(nan, np.isnan(bv)):
        return True
    ae = np.zeros_like(av) if ae is None else ae
    with np.errstate(invalid="ignore"):
        return bool((np.abs(np.where(nan, 0.0, av - bv)) > factor * ae).any())


def pass2_inputs(c: OCase):
    """Quarters for one rank's second pass alone: coefficients +-2^-k, vectors and gradient vectors multiples of 1/4 (pad columns 0):
    every sum of a list of up to 200 references is exact in float32 in any order (|term| <= 1, unit 2^-5, 200 x 32 < 2^24)."""
    S = stage(c)
    rng = np.random.default_rng([zlib.crc32(c.id.encode()), 7])
    n = c.n_pos * (c.N + 1) + 1
    coef = (rng.choice([-1.0, 1.0], n) * 2.0 ** -rng.integers(0, 4, n)).astype(f32)
    live = np.arange(c.stride) < c.dim
    q = lambda shape: np.where(live, quarters(rng, shape), 0.0).astype(f32)
    vall = [q((c.G, 2 * S.C, c.stride)) for _ in S.parts]
    gvs = [q((2 * S.C + 1, c.stride)) for _ in S.parts]
    return coef, vall, gvs


# ----------------------------------------------------------------------------------------------------- the case table
def _build():
    runs = []
    add = lambda case, form, quarter=0: runs.append(Run(case, form, quarter))
    # widths: every stride and dim at one mid shape, G = 3 (general divisor) and 4 (power of two), every form, both kernels
    for si, stride in enumerate(STRIDES):
        for di, dim in enumerate(table_dims(stride)):
            for G in (3, 4):
                k = si + di + G
                share = (33, 65)[G - 3]                                   # two partials at G = 3, three at G = 4: the combine's even and odd count
                case = OCase(stride, dim, G, (0, G // 2, G - 1)[k % 3], 5, 23, opt=("adagrad", "sgd")[k % 2], pos_w=bool(k % 3 == 0),
                             scale=(1.0, 0.5)[(k // 2) % 2], rel_copies=REL_COPIES[k % 4], share=share, tag="width")
                for form in FORMS:
                    for quarter in (0, 1):
                        add(case, form, quarter)
    # group sizes at stride 80 / dim 75, and once each at strides 16 and 320
    for ni, N in enumerate(GROUPS):
        for stride, dim in ((80, 75),) + (((16, 16), (320, 319)) if N in (17, 33, 64) else ()):
            G = (1, 3, 4)[ni % 3]
            case = OCase(stride, dim, G, G - 1, N, 9, pos_w=bool(ni % 2), tag="group")
            for form in ("atm", "em", "mirown"):
                for quarter in (0, 1):
                    add(case, form, quarter)
    # ranks, ragged home slices, two parts
    for G in RANKS:
        for rank in sorted({0, G // 2, G - 1}):
            for n_pos in N_POS:
                add(OCase(80, 75, G, rank, 5, n_pos, tag="ranks"), "atm", (n_pos + rank) % 2)
                form = ("em", "mir", "own", "mirown")[(G + rank + n_pos) % 4]          # (a peer-direct step has one part: the header)
                add(OCase(80, 75, G, rank, 5, n_pos, chunks=2 if (n_pos >= 4 and form in ("em", "own")) else 1, tag="ranks"), form, (n_pos + rank + 1) % 2)
    # the rule of oc_score_quarter = -1, on each side
    for G, N, stride in ((4, 32, 128), (4, 33, 128), (3, 5, 80), (4, 5, 160)):
        add(OCase(stride, stride - 1, G, 1, N, 9, tag="rule"), "em", -1)
        add(OCase(stride, stride - 1, G, 1, N, 9, tag="rule"), "atm", -1)
    # options
    for ki, copies in enumerate(REL_COPIES):
        add(OCase(80, 75, 3, 1, 5, 23, rel_copies=copies, opt=("adagrad", "sgd")[ki % 2], tag="opt"), "atm", ki % 2)
    for ki, hc in enumerate(HOT_COPIES):
        add(OCase(80, 75, (3, 4, 1)[ki], 0, 5, 23, hot=2, hot_copies=hc, pos_w=True, tag="opt"), "atm", ki % 2)
    add(OCase(80, 75, 3, 1, 5, 23, refcount=False, tag="opt"), "atm", 0)
    add(OCase(80, 75, 4, 1, 5, 23, refcount=False, scale=0.5, tag="opt"), "atm", 1)
    for form in FORMS:
        for quarter in (0, 1):
            add(OCase(80, 75, 3, 1, 17, 23, vec="sat", pos_w=True, scale=0.5, tag="sat"), form, quarter)
    # long second-pass lists, one to four parts
    for chunks, opt in ((1, "adagrad"), (2, "sgd"), (4, "adagrad")):
        add(OCase(32, 31, 2, 1, 1, 370, chunks=chunks, opt=opt, long=True, n_ent=400, tag="long"), "em", 0)
    # a second trip of the grid-stride loops
    add(OCase(16, 16, 2, 1, 1, 8192 + 3, n_ent=4096, tag="trip"), "em", 0)
    add(OCase(16, 16, 4, 1, 15, 32768 + 5, n_ent=4096, tag="trip"), "atm", 1)
    assert len({r.id for r in runs}) == len(runs)
    return runs


RUNS = _build()
CASES = list({r.case.id: r.case for r in RUNS}.values())
