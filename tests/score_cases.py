"""Case table, operand factories, reference, float32 model, bounds and mutants of the exact tests of the relation score kernel
(test_score_cases.py here, test_score_exact_gpu.py on the device): k_triple_score in its twelve instantiations per row width,
k_stage_reduce and k_count_refs (multike_amd/csrc/mke_score.hip).  NumPy only.

One formula, written once over `Arith` of update_cases.py, gives every triple's loss term and gradient row c d: in "bound"
mode as float64 values with an error bound each (the reference), in "f32" mode as NumPy float32 (the model of the kernel's
arithmetic at contribution level).  A routing layer, written from the kernel's work-item structure, turns triples into
ENTRIES (destination, triple, sign): which scratch row, privatised relation copy, hub copy or staging slot takes a triple's
row, which rows are finished in place, which flags are set.  The mutants are switches of that layer and of the formula.

Tier 1 (bit for bit).  Both normalise flags off, entity entries multiples of 1/4 in [-1, 1], relation entries +-R + quarters
(R = 16 below dim 15, else 6), weights, scale and lr powers of two.  Every |d_k| >= R - 2, so EVERY triple has
||h + r - t||^2 >= SAT_NEG = 128 (>= SAT_POS): softplus(x) = x, sigmoid(x) = 1 and c = 2 w scale for a positive; exp(-y) = 0,
loss term 0 and gradient +-0 for a negative (either path).  All sums are then exact in any order (`Bound.check()`), and the
loss, every gradient row, relation copy, hub copy, staging slot, flag, in-place row and reference count must EQUAL the float64
reference rounded to float32.  The sign of a zero is not compared (`canon`).  A negative's row is a zero here: its routing shows
in the flags, the slot keys, the reference counts and the SENTINEL -> 0 change of a slot, not in a sum.

Tier E compares device runs with each other (test_score_exact_gpu.py); here it only has its collision-free batches ("unique").

Tier 2 (float64 within a derived bound): normalised or scaled tables with y in [0, 16], collisions, slices, the in-place
Jacobian + SGD / Adagrad.  Charges, in u = 2^-23: u/2 per rounded operation, 2 u for rsqrtf / rsq / rcp and for the hardware
exp and log, |a| u/2 more on __expf(a) for the scaling of its argument and 2^-126 absolute for its flush to zero, u/2 for the
ln 2 product of __logf, a whole ulp on a stored value, 2^-149 absolute per operation, the row-sum rule of update_cases.py, and
for a sum of m terms in free order (the fma chain of a flush, its butterflies, the atomics of a row) k / (1 - k) of the sum of
absolute values, k = (m - 1) u/2 (the m - 1 additions of a summation tree, second order kept; nothing for a row that receives one
add), with the positive's term counted three times in gR = (gH + gT) - gP.  Nothing is fitted to a device.

Poison, inside the buffers: a NaN tail row behind tables and accumulator, SENTINEL in every gradient row, relation copy, hub copy
and staging slot that must not be written (rows that receive adds start at zero, the ABI's invariant), NaN in all loss
partials, 64 extra `touched` entries, 0x7F bytes in the slot keys.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import rows_cases as rc
import update_cases as uc
from rows_cases import FPLS, OLD_TAG, SAT_NEG, SAT_POS, SENTINEL, STRIDES, TAG, Bound, quarters, table_dims
from update_cases import ACC_PAD, L2_EPS32, TINY, U, Arith, V

f32, f64 = np.float32, np.float64
LOSS_PARTIALS = 2048
WAVES = LOSS_PARTIALS * 4                                       # wavefronts of a launch
KEY_FILL = 0x7F7F7F7F7F7F7F7F
STAGE_REL = 1 << 40
FLUSH_TINY = 2.0 ** -126
NPPS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 130)
REL_COPIES = (1, 2, 8, 64)
HOT_COPIES = (1, 2, 3, 8, 64)
COUNT_TOTALS = (1, 255, 257, 512 * 4 * 256 + 1)                 # 524,289: one past the 512 rider blocks of 4 x 256 entries
REDUCE_SLOTS = (1, 15, 16, 17, 4096 * 16 + 1)
MUTANTS = ("gR_keeps_gP", "cH_cT_swapped", "skip_fourth", "skip_past_first_block", "drop_last_odd_group", "slow_as_fast",
           "equal_as_fast", "ragged_guard", "hub_mod_n_hot", "rel_copy_0", "inplace_at_2", "refcount_not_reset",
           "neg_weight_ignored", "scale_twice", "no_projection", "old_acc_stored", "rider_scores")
# Two of the issue's mutants change no output and are therefore not in the list: a flush by an EMPTY slice adds the zeros
# gH = gT = gP = 0 to rows the group's first slice has flagged already (x + 0 = x, SENTINEL + 0 = SENTINEL), and a pad column
# that is ADDED adds c * 0 (the tables' pad columns are 0 by the ABI).  test_score_cases.py asserts both equalities;
# "ragged_guard" is the guard failing the other way (the last live column of a ragged dim skipped).
SILENT_MUTANTS = ("empty_slice_flushes", "pad_added")
# The code-word forms (section (1c) of the header).  Mutants of the routing by words; the last one is a mutant of the REFERENCE
# (it lists entity flags although touched_ent is NULL) and must fail against the unmutated model.
CODE_ENT_BITS = 26
CODE_HEAD, CODE_FAST, CODE_EXCL = 1 << 26, 1 << 27, 1 << 28
CODE_ENT_MASK = (1 << CODE_ENT_BITS) - 1
CW_MUTANTS = ("cw_excl_ignored", "cw_excl_without_fast", "cw_head_inverted", "cw_slow_skipped", "cw_slow_entity_head", "cw_mask16",
              "cw_flags_listed")


class Form(NamedTuple):
    """How one call selects its instantiation: staging and ref_count given or not, and the mke_tuning of the call."""
    det: int = 0
    x: int = 0
    o32: int = 1
    lid: int = 1
    half: int = -1          # score_half_groups
    splits: int = 0         # score_splits (0 = auto)
    cw: int = 0             # neg_code given and no ref_count: the code-word instantiation (only det=0, x=1, o32=1, lid=1, npp > 0)
    ids: int = 1            # cw: neg_h / neg_r / neg_t given (0: all three NULL, "own" batches only)
    flags: int = 1          # cw: touched_ent given (0: NULL)

    @property
    def id(self):
        s = f"{'det' if self.det else 'atm'}-x{self.x}-o{self.o32}-l{self.lid}-h{self.half}-s{self.splits}"
        return s + (f"-cw-i{self.ids}-f{self.flags}" if self.cw else "")

    @property
    def legal(self):
        return not self.cw and self.ids == 1 and self.flags == 1 or bool(self.cw and not self.det and self.x and self.o32 and self.lid)


def forms12(npp_max=1000):
    """The twelve instantiations of a width, two and one group per wavefront (splits forced to 1 for the former)."""
    out = []
    for half, splits in ((npp_max, 1), (0, 1)):
        out += [Form(1, 0, 1, 1, half, splits), Form(1, 1, 1, 1, half, splits), Form(0, 1, 1, 1, half, splits),
                Form(0, 1, 1, 0, half, splits), Form(0, 1, 0, 1, half, splits), Form(0, 0, 1, 1, half, splits)]
    return out


def forms_cw(npp_max=1000):
    """The code-word forms of a width: two and one group per wavefront, with and without id arrays, with and without entity flags."""
    return [Form(0, 1, 1, 1, half, 1, 1, ids, flags) for half in (npp_max, 0) for ids in (1, 0) for flags in (1, 0)]


class SCase(NamedTuple):
    stride: int
    dim: int
    n_pos: int
    npp: int = 0            # negatives per positive; 0: ungrouped
    n_neg0: int = 0         # ungrouped negatives
    tier: int = 1
    kinds: str = "fast"     # fast | mixed | slow2nd | unique | dup | own (the sampler's shape of a batch: see own_positions)
    weights: str = "none"   # none | pos | both
    scale: float = 1.0
    copies: int = 1
    n_hot: int = 0
    hot_copies: int = 1
    ent_norm: int = 0
    rel_norm: int = 0
    opt: str = "sgd"
    lr: float = 0.25
    special: bool = False
    fwd_only: bool = False
    rider: int = 0          # total of the count rider's job
    n_ent: int = 150
    n_rel: int = 5
    tag: str = ""

    @property
    def id(self):
        s = f"t{self.tier}-s{self.stride}-d{self.dim}-p{self.n_pos}-n{self.npp or self.n_neg0}{'' if self.npp else 'u'}-{self.kinds}-w{self.weights}"
        for v in (f"sc{self.scale:g}" if self.scale != 1 else "", f"c{self.copies}" if self.copies > 1 else "",
                  f"hot{self.n_hot}x{self.hot_copies}" if self.n_hot else "", "en" if self.ent_norm else "", "rn" if self.rel_norm else "",
                  self.opt if self.opt != "sgd" else "", "special" if self.special else "", "fwd" if self.fwd_only else "",
                  f"rider{self.rider}" if self.rider else "", self.tag):
            if v:
                s += "-" + v
        return s

    @property
    def n_neg(self):
        return self.n_pos * self.npp if self.npp else self.n_neg0

    @property
    def fpl(self):
        return self.stride // 16


class Run(NamedTuple):
    case: SCase
    form: Form

    @property
    def id(self):
        return self.case.id + "/" + self.form.id


# ----------------------------------------------------------------------------------------------------- the launcher's decisions
def splits_of(c: SCase, f: Form) -> int:
    if not c.npp or not c.n_pos or f.det:
        return 1
    s = min(WAVES // c.n_pos, (c.npp + 3) // 4)
    s = max(s, 1)
    if f.splits > 0:
        s = f.splits
    return min(s, c.npp)


def qpg_of(c: SCase, f: Form) -> int:
    half_max = f.half if f.half >= 0 else (64 if c.fpl <= 8 else 31)
    return 2 if (c.npp > 0 and c.npp <= half_max and splits_of(c, f) == 1) else 4


def excl_of(c: SCase, f: Form) -> bool:
    return bool(f.x) and c.npp > 0 and not c.fwd_only


def instantiation(c: SCase, f: Form):
    """(FPL, family, flag, QPG): the template arguments launch_score() picks; (FPL, "cw", QPG) for the code-word instantiation."""
    x = excl_of(c, f)
    if f.cw:
        assert f.legal and x
        return (c.fpl, "cw", qpg_of(c, f))
    if f.det:
        fam = ("det", x)
    elif x and f.o32:
        fam = ("o32", bool(f.lid))
    else:
        fam = ("plain", x)
    return (c.fpl,) + fam + (qpg_of(c, f),)


def all_instantiations():
    return {(fpl, fam, flag, q) for fpl in FPLS for fam in ("det", "o32", "plain") for flag in (False, True) for q in (2, 4)}


def cw_instantiations():
    return {(fpl, "cw", q) for fpl in FPLS for q in (2, 4)}


def count_blocks(c: SCase) -> int:
    return min(-(-c.rider // 1024), LOSS_PARTIALS // 4) if c.rider else 0


def count_case(total: int) -> uc.CountCase:
    cc = {1: uc.CountCase(1, 0), 255: uc.CountCase(85, 2), 257: uc.CountCase(1, 256), 524289: uc.CountCase(174763, 2)}[total]
    assert cc.total == total
    return cc


# ----------------------------------------------------------------------------------------------------- operands
class SOps(NamedTuple):
    ent: np.ndarray         # float32 [n_ent + 1, stride], NaN tail row
    rel: np.ndarray         # float32 [n_rel + 1, stride]
    acc: np.ndarray         # float32 [n_ent + 1, stride]
    ph: np.ndarray
    pr: np.ndarray
    pt: np.ndarray
    pw: np.ndarray          # or None
    nh: np.ndarray          # int32 [max(n_neg, 1)]
    nr: np.ndarray
    nt: np.ndarray
    nw: np.ndarray          # or None
    ref_count: np.ndarray   # int32 [n_ent + 1]: the step's own counts (mke_count_entity_refs rule), 9 in the tail entry
    hot_slot: np.ndarray    # int32 [n_ent + 1] or None
    bound: Bound


def _rng(c: SCase, salt=0):
    return np.random.default_rng([zlib.crc32(c._replace(rider=0).id.encode()), salt])      # the rider changes no operand


def sizes(c: SCase):
    """(n_ent, n_rel): a collision-free batch needs a row of its own for every id."""
    if collision_free(c):
        return c.n_pos * (2 + c.npp) + 3, c.n_pos
    return c.n_ent, c.n_rel


def collision_free(c: SCase) -> bool:
    """Every id names a row of its own ("own" with the tag "free": the positive drawn as its own negative apart, which gives its
    three rows a second add -- two adds to a zero row commute, so device runs still agree bit for bit)."""
    return c.kinds == "unique" or (c.kinds == "own" and c.tag == "free")


def own_positions(npp: int, n_neg: int):
    """The negatives of an "own" batch that equal their positive (mke_neg_sample keeps the positive when the last round draws
    the replaced id): the last of an even group (with slices: not slice 0; npp = 1: the group's only negative), the first of an
    odd group (the first id block) and negative 70 of every group that has one (the second id block, 32 or 64 lanes long)."""
    g, n = np.arange(n_neg) // npp, np.arange(n_neg) % npp
    return ((g % 2 == 0) & (n == npp - 1)) | ((g % 2 == 1) & (n == 0) & (npp > 1)) | (n == 70)


def _ids(c: SCase, rng, n_ent, n_rel):
    P, N = c.n_pos, c.n_neg
    if collision_free(c):
        perm = rng.permutation(n_ent - 3) + 3 if c.special else rng.permutation(n_ent)
        ph, pt, e = perm[:P], perm[P:2 * P], perm[2 * P:2 * P + N]
        if c.special and N >= 3:
            e[:3] = (0, 1, 2)
        pr = rng.permutation(n_rel)[:P]
        g = np.arange(N) // max(c.npp, 1)
        head = rng.integers(0, 2, N).astype(bool)
        own = own_positions(c.npp, N) if c.kinds == "own" else np.zeros(N, bool)
        nh, nt = np.where(head & ~own, e, ph[g]), np.where(head | own, pt[g], e)
        return ph, pr, pt, nh, pr[g].copy(), nt
    ph, pt = rng.integers(0, n_ent, P), rng.integers(0, n_ent, P)
    pr = rng.integers(0, n_rel, P)
    nh, nr, nt = (np.zeros(max(N, 1), dtype=np.int64) for _ in range(3))
    if not c.npp:
        if N:
            nh[:], nr[:], nt[:] = rng.integers(0, n_ent, N), rng.integers(0, n_rel, N), rng.integers(0, n_ent, N)
        return ph, pr, pt, nh, nr, nt
    g = np.arange(N) // c.npp
    n = np.arange(N) % c.npp
    if c.kinds == "own":                                             # one side replaced by a draw that differs from it, or the positive itself
        lo = 65536 if n_ent > 65536 else 0                           # a table past 2^16 rows: every draw needs more than 16 bits
        draw = lambda a: lo + (a - lo + 1 + rng.integers(0, n_ent - lo - 1, len(a))) % (n_ent - lo)
        head, own = (n + g) % 2 == 0, own_positions(c.npp, N)
        return ph, pr, pt, np.where(head & ~own, draw(ph[g]), ph[g]), pr[g].copy(), np.where(~head & ~own, draw(pt[g]), pt[g])
    other = lambda a: (a + 1 + rng.integers(0, n_ent - 1, len(a))) % n_ent          # an entity different from a
    kind = np.where((n + g) % 2 == 0, 0, 1)                          # fast: corrupted head / tail in turn
    if c.kinds == "mixed":
        kind = (n + 3 * g) % 10
    elif c.kinds == "slow2nd":                                       # one slow negative, in the second id block of its group
        lpg = 32 if c.npp <= 64 else 64
        kind = np.where(n == min(c.npp - 1, lpg + 6), 2, kind)
    elif c.kinds == "dup":
        kind = np.full(N, 6)
    nh[:], nr[:], nt[:] = ph[g], pr[g], pt[g]
    xg = other(ph)                                                   # the entity kinds 0 and 6 of a group share
    for k in range(10):
        m = kind == k
        if k in (0, 6):      # corrupted head; 6 repeats the entity of 0 in its group
            nh[m] = xg[g[m]] if c.kinds in ("mixed", "dup") else other(ph[g[m]])
        elif k in (1, 9):    # corrupted tail
            nt[m] = other(pt[g[m]])
        elif k == 2:         # both sides differ
            nh[m], nt[m] = other(ph[g[m]]), other(pt[g[m]])
        elif k == 3:         # the relation and one side
            nr[m], nh[m] = (pr[g[m]] + 1) % n_rel, other(ph[g[m]])
        elif k == 4:         # the relation alone
            nr[m] = (pr[g[m]] + 1) % n_rel
        elif k == 7:         # another group's head (its own: the negative equals the positive)
            nh[m] = ph[(g[m] + 1) % P]
        elif k == 8:         # the corrupted head is the group's own tail
            nh[m] = pt[g[m]]
    return ph, pr, pt, nh, nr, nt


def count_refs(ph, pt, nh, nt, npp, n_neg, n_ent):
    """mke_count_entity_refs of the header."""
    out = np.zeros(n_ent, dtype=np.int64)
    np.add.at(out, ph, 1)
    np.add.at(out, pt, 1)
    if n_neg and npp:
        g = np.arange(n_neg) // npp
        np.add.at(out, nh[:n_neg][nh[:n_neg] != ph[g]], 1)
        np.add.at(out, nt[:n_neg][nt[:n_neg] != pt[g]], 1)
    return out


def step_counts(ph, pt, nh, nt, npp, n_ent):
    """mke_count_entity_refs of one step."""
    cnt = np.zeros(n_ent, dtype=np.int64)
    np.add.at(cnt, ph, 1)
    np.add.at(cnt, pt, 1)
    g = np.arange(len(nh)) // npp
    np.add.at(cnt, nh[nh != ph[g]], 1)
    np.add.at(cnt, nt[nt != pt[g]], 1)
    return cnt


def define(pos, neg, off, s0, s1, npp, n_ent):
    """Section (1c) of the header in NumPy: (codes of the negatives of steps [s0, s1), bitmap rows [s1 - s0, row_words])."""
    ph, pr, pt = pos
    nh, nr, nt = neg                                   # laid out from off[s0]
    words = (n_ent + 15) // 16
    codes = np.zeros((off[s1] - off[s0]) * npp, dtype=np.int64)
    bits = np.zeros((s1 - s0, words), dtype=np.uint32)
    for s in range(s0, s1):
        lo, hi = off[s], off[s + 1]
        a, b = (lo - off[s0]) * npp, (hi - off[s0]) * npp
        cnt = step_counts(ph[lo:hi], pt[lo:hi], nh[a:b], nt[a:b], npp, n_ent)
        g = lo + np.arange(b - a) // npp
        dh, dt = nh[a:b] != ph[g], nt[a:b] != pt[g]
        e = np.where(dh, nh[a:b], nt[a:b]).astype(np.int64)
        fast = (nr[a:b] == pr[g]) & (dh != dt)
        codes[a:b] = e | np.where(dh, CODE_HEAD, 0) | np.where(fast, CODE_FAST, 0) | np.where(cnt[e] == 1, CODE_EXCL, 0)
        two = np.where(cnt == 0, 0, np.where(cnt == 1, 1, 3)).astype(np.uint32)
        ent = np.arange(n_ent)
        np.bitwise_or.at(bits[s - s0], ent >> 4, two << ((ent & 15) * 2).astype(np.uint32))
    return codes.astype(np.int32), bits


def codes_of(c: SCase) -> np.ndarray:
    """The baked code words of the case's one step."""
    return step_codes(c)[0]


def step_codes(c: SCase):
    """(words [n_neg], bitmap row [(n_ent + 15) // 16]) of the case's one step; `sampler_words` are the words before the bake."""
    o = ops(c)
    n_ent, _ = sizes(c)
    codes, bits = define((o.ph, o.pr, o.pt), (o.nh[:c.n_neg], o.nr[:c.n_neg], o.nt[:c.n_neg]), np.array([0, c.n_pos]), 0, 1, c.npp, n_ent)
    return codes, bits[0]


def sampler_words(c: SCase) -> np.ndarray:
    """What mke_neg_sample writes for an "own" batch: draw | HEAD | FAST, or pos_t without flags for the positive itself."""
    assert c.kinds == "own"
    return codes_of(c) & ~np.int32(CODE_EXCL)


def tier2_shift(dim: int) -> int:
    """Entries of an unnormalised tier-2 table are quarters times 2^-k with dim 4^-k <= 1: rows of norm <= 1, y <= 9."""
    k = 0
    while dim > 4 ** k:
        k += 1
    return k


@functools.lru_cache(maxsize=8)
def ops(c: SCase) -> SOps:
    rng = _rng(c)
    n_ent, n_rel = sizes(c)
    st, d = c.stride, c.dim
    ent, rel = np.zeros((n_ent + 1, st), dtype=f32), np.zeros((n_rel + 1, st), dtype=f32)
    bd = Bound()
    if c.tier == 1:
        assert not (c.ent_norm or c.rel_norm)
        R = 16 if d < 15 else 6
        ent[:n_ent, :d] = quarters(rng, (n_ent, d))
        rel[:n_rel, :d] = rng.choice((-R, R), (n_rel, d)) + quarters(rng, (n_rel, d))
    else:
        ent[:n_ent, :d] = quarters(rng, (n_ent, d)) * (1.0 if c.ent_norm else 2.0 ** -tier2_shift(d))
        rel[:n_rel, :d] = quarters(rng, (n_rel, d)) * (1.0 if c.rel_norm else 2.0 ** -tier2_shift(d))
        if c.special:                                                 # the three rows of update_cases.py
            ent[0] = 0.0
            ent[1] = 0.0
            ent[1, :d] = 2.0 ** -30
            ent[2] = 0.0
            ent[2, :min(4, d)] = 0.5 if d >= 4 else 0.0
            if d < 4:
                ent[2, 0] = 1.0
    ent[n_ent], rel[n_rel] = np.nan, np.nan
    acc = np.full((n_ent + 1, st), ACC_PAD, dtype=f32)
    acc[:n_ent, :d] = (0.1 + np.abs(quarters(rng, (n_ent, d)))).astype(f32)
    acc[n_ent] = np.nan
    ph, pr, pt, nh, nr, nt = (np.ascontiguousarray(a, dtype=np.int32) for a in _ids(c, rng, n_ent, n_rel))
    pw = nw = None
    if c.weights in ("pos", "both"):
        pw = rng.choice(np.array(rc.WEIGHTS, dtype=f32), c.n_pos)
    if c.weights == "both":
        nw = rng.choice(np.array(rc.WEIGHTS, dtype=f32), max(c.n_neg, 1))
    rcnt = np.full(n_ent + 1, 9, dtype=np.int32)
    rcnt[:n_ent] = count_refs(ph, pt, nh, nt, c.npp, c.n_neg, n_ent)
    hot_slot = None
    if c.n_hot:
        rows = np.unique(np.concatenate([ph, pt]))
        rows = np.concatenate([rows, np.setdiff1d(np.arange(n_ent), rows)])[:c.n_hot]
        hot_slot = np.full(n_ent + 1, -1, dtype=np.int32)
        hot_slot[rng.permutation(rows)] = np.arange(c.n_hot, dtype=np.int32)
        hot_slot[n_ent] = 0
    if c.tier == 1:
        R = 16 if d < 15 else 6
        wmax = 2.0 if c.weights != "none" else 1.0
        wmin = 0.25 if c.weights != "none" else 1.0
        dmax = R + 3
        n_tr = c.n_pos + c.n_neg
        bd.add("chain", d * dmax ** 2, 1 / 16)
        passes = 1 + (c.n_pos // WAVES if c.npp else n_tr // (WAVES * 4))     # a negative's term is an exact 0: one positive per pass
        bd.add("loss of a thread", passes * wmax * d * dmax ** 2, wmin / 16)
        per_row = max(np.bincount(np.concatenate([ph, pt, pr]), minlength=1).max(), 1) if c.n_pos else 1
        bd.add("gradient row", 3 * per_row * 2 * wmax * c.scale * dmax, 2 * wmin * c.scale / 4)
        bd.add("value", 1 + c.lr * 2 * wmax * c.scale * dmax, min(c.lr * 2 * wmin * c.scale / 4, 1 / 4))
    return SOps(ent, rel, acc, ph, pr, pt, pw, nh, nr, nt, nw, rcnt, hot_slot, bd)


# ----------------------------------------------------------------------------------------------------- the formula, written once
class SArith(Arith):
    """Arith with the kernel's transcendentals and a few structural helpers."""

    def take(self, x, idx):
        return V(x.val[idx], x.err[idx]) if self.bound else x[idx]

    def neg(self, x):
        return V(-x.val, x.err) if self.bound else -x

    def free(self, x, k):
        """x times an array of powers of two (signed): exact."""
        k = np.asarray(k, dtype=f64)
        return V(x.val * k, x.err * np.abs(k)) if self.bound else (x.astype(f64) * k).astype(f32)

    def where(self, m, a, b):
        return V(np.where(m, a.val, b.val), np.where(m, a.err, b.err)) if self.bound else np.where(m, a, b)

    def const(self, val, like):
        return V(np.full(self.val(like).shape, val)) if self.bound else np.full(like.shape, val, dtype=f32)

    def exp(self, a):
        """__expf(a), a <= 16."""
        with np.errstate(under="ignore", over="ignore"):
            if not self.bound:
                return np.exp(np.asarray(a, dtype=f64)).astype(f32)
            val = np.exp(a.val)
            return V(val, val * np.expm1(a.err) + (2 * U + 0.5 * U * np.abs(a.val)) * val + FLUSH_TINY + TINY)

    def log(self, x):
        """__logf(x), x >= 1."""
        if not self.bound:
            return np.log(np.asarray(x, dtype=f64)).astype(f32)
        val = np.log(x.val)
        return V(val, x.err / (x.val - x.err) + 2.5 * U * np.abs(val) + TINY)

    def rcp(self, x):
        """__builtin_amdgcn_rcpf(x), x >= 1 (inf: 0)."""
        with np.errstate(over="ignore"):
            if not self.bound:
                return (1.0 / np.asarray(x, dtype=f64)).astype(f32)
            val = 1.0 / x.val
            lo = x.val - x.err
            return V(val, np.where(np.isinf(x.val), 0.0, x.err / (lo * x.val)) + 2 * U * val + TINY)


def read_rows(ar, table, idx, norm, depth):
    """(rows as the kernel uses them, raw rows, inv or None)."""
    W = ar.lift(table[idx].astype(f64))
    if not norm:
        return W, W, None
    s = ar.dots(W, W, depth)
    inv = ar.rsqrt(ar.maximum(s, L2_EPS32))
    return W * inv, W, inv


def independent(ar, H, R, T, sign, w, scale):
    """independent_triple, and the positive of a group (the same arithmetic): (loss terms [n, 1], rows c d [n, stride])."""
    depth = ar.val(H).shape[1] // 16 + 6
    d = (H + R) - T
    x = ar.dots(d, d, depth)
    one = ar.const(1.0, x)
    e = ar.exp(ar.neg(x))                                            # exp(-|z|)
    lg = ar.log(one + e)
    if sign > 0:
        sp, sig = x + lg, ar.rcp(one + e)
    else:
        sp, sig = lg, ar.rcp(one + ar.exp(x))
    return ar.free(sp, w), d * ar.free(sig, 2.0 * sign * w * scale)


def fast_negative(ar, C, base, side_h, w, scale, ent_norm):
    """A negative that replaces one entity of its positive: (loss terms, rows c d, cinv or None)."""
    depth = ar.val(C).shape[1] // 16 + 6
    cinv = None
    sgn = np.where(side_h, 1.0, -1.0)
    if ent_norm:
        cinv = ar.rsqrt(ar.maximum(ar.dots(C, C, depth), L2_EPS32))
        d = ar.fma(ar.free(cinv, sgn), C, base)
    else:
        d = ar.fma(ar.free(ar.const(1.0, C), sgn), C, base)          # cinv = 1.0f
    y = ar.dots(d, d, depth)
    t = ar.exp(ar.neg(y))
    s1 = ar.const(1.0, y) + t
    c = ar.free(t * ar.rcp(s1), -2.0 * w * scale)
    return ar.free(ar.log(s1), w), d * c, cinv


def in_place(ar, c: SCase, C, A, D, cinv, side_h, mutant=""):
    """The row finished by the quarter-wave that scored its only reference: (w', acc' or None)."""
    depth = c.fpl + 6
    sg = np.where(side_h, 1.0, -1.0)
    if c.ent_norm:
        a1 = ar.free(cinv, sg)
        dot = ar.dots(C, D, depth) * a1
        live = ar.val(ar.dots(C, C, depth)) > L2_EPS32
        if mutant == "no_projection":
            live = np.zeros_like(live)
        a2 = ar.select(live, ar.neg(dot) * cinv * cinv)
        g = ar.fma(a2, C, a1 * D)
    else:
        g = ar.free(D, sg)
    if c.opt == "adagrad":
        a2_ = ar.fma(g, g, A)
        w2 = ar.stored(ar.msub(C, ar.k(c.lr) * g, ar.rsqrt(a2_)))
        return w2, ar.stored(A if mutant == "old_acc_stored" else a2_)
    return ar.stored(ar.msub(C, ar.k(c.lr), g)), None


# ----------------------------------------------------------------------------------------------------- routing
def stage_slot(g, npp, n, k):
    return (g * (npp + 1) + n) * 3 + k


class Entries:
    """(destination table, scratch row, entity / relation row, staging slot, triple, sign, weight in the sum of absolute values)."""

    def __init__(self):
        self.cols = [[] for _ in range(7)]

    def add(self, table, dest, row, slot, triple, sign, absw=1):
        n = len(np.atleast_1d(dest))
        for col, v in zip(self.cols, (table, dest, row, slot, triple, sign, absw)):
            col.append(np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)))

    def arrays(self):
        return [np.concatenate(col) if col else np.zeros(0, dtype=np.int64) for col in self.cols]


def reference(c: SCase, f: Form, mode="bound", mutant="") -> dict:
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return _reference(c, f, mode, mutant)


def _reference(c, f, mode, mutant):
    """What the launch must leave behind.  Values come as (val, err): err None = bit for bit (tier 1, where val is float32)."""
    o = ops(c)
    ar = SArith(mode)
    n_ent, n_rel = sizes(c)
    st, d, P, N, npp = c.stride, c.dim, c.n_pos, c.n_neg, c.npp
    depth = c.fpl + 6
    det, excl, bwd = bool(f.det), excl_of(c, f), not c.fwd_only
    S, qpg = splits_of(c, f), qpg_of(c, f)
    K = 1 if det else c.copies
    hot = c.n_hot > 0 and not det and bwd
    hc = c.hot_copies
    pw = np.ones((P, 1)) if o.pw is None else o.pw.astype(f64).reshape(-1, 1)
    nw = np.ones((max(N, 1), 1)) if (o.nw is None or mutant == "neg_weight_ignored") else o.nw.astype(f64).reshape(-1, 1)
    nw = nw[:N]
    nh, nr, nt = o.nh[:N], o.nr[:N], o.nt[:N]
    zero = P + N                                                     # index of the zero row behind the triples' rows
    Dval, Derr = np.zeros((P + N + 1, st)), np.zeros((P + N + 1, st))
    Lval, Lerr = np.zeros(P + N), np.zeros(P + N)

    def put(idx, loss, rows):
        lv, le = ar.out(loss)
        rv, re = ar.out(rows)
        Lval[idx], Dval[idx] = np.asarray(lv, f64).ravel(), rv
        if le is not None:
            Lerr[idx], Derr[idx] = le.ravel(), re

    Hn, _, _ = read_rows(ar, o.ent, o.ph, c.ent_norm, depth)
    Rn, _, _ = read_rows(ar, o.rel, o.pr, c.rel_norm, depth)
    Tn, _, _ = read_rows(ar, o.ent, o.pt, c.ent_norm, depth)
    if P:
        put(np.arange(P), *independent(ar, Hn, Rn, Tn, 1.0, pw, c.scale))
    E = Entries()
    inpl = {"rows": np.zeros(0, dtype=np.int64)}
    live_neg = np.ones(N, bool)
    hub = lambda rows, k: np.where(o.hot_slot[rows] >= 0, n_ent + (k % hc) * c.n_hot + o.hot_slot[rows], rows) if hot else rows
    if mutant == "hub_mod_n_hot" and hot:
        hub = lambda rows, k: np.where(o.hot_slot[rows] >= 0, n_ent + np.minimum(k % c.n_hot, hc - 1) * c.n_hot + o.hot_slot[rows], rows)
    relcopy = (lambda wk: np.zeros_like(wk)) if mutant == "rel_copy_0" else (lambda wk: wk % K)
    if npp:
        g, n = np.arange(N) // npp, np.arange(N) % npp
        per = -(-npp // S)
        s = n // per
        dh, dt = nh != o.ph[g], nt != o.pt[g]
        fast = (nr == o.pr[g]) & (dh != dt)
        if mutant == "slow_as_fast":
            fast = fast | (nr != o.pr[g]) | (dh & dt)
        if mutant == "equal_as_fast":
            fast = fast | ((nr == o.pr[g]) & ~dh & ~dt)
        e = np.where(dh, nh, nt)
        xbit = o.ref_count[:n_ent][e] == 1                           # MKE_CODE_EXCL of the negative's word
        if f.cw:
            # the kernel sees the WORD (entity, HEAD, FAST, EXCL) and, for a word without FAST, the id arrays or -- without
            # them -- the positive's own triple; only the sampler's shape of a batch may come without ids
            assert f.legal and (f.ids or c.kinds == "own") and not c.fwd_only, (c.id, f.id)
            w = codes_of(c)                                          # the routing below is the NumPy statement of section (1c)
            assert np.array_equal(w & CODE_ENT_MASK, e) and np.array_equal((w & CODE_HEAD) != 0, dh), c.id
            assert np.array_equal((w & CODE_FAST) != 0, fast) and np.array_equal((w & CODE_EXCL) != 0, xbit), c.id
            if mutant == "cw_head_inverted":
                dh = np.where(fast, ~dh, dh)
            if mutant == "cw_mask16":
                e = e & 0xFFFF
            sh, sr, st_ = (nh, nr, nt) if f.ids else (o.ph[g], o.pr[g], o.pt[g])
            if mutant == "cw_slow_entity_head" and not f.ids:
                sh = e
            nh, nr, nt = np.where(fast, np.where(dh, e, o.ph[g]), sh), np.where(fast, o.pr[g], sr), np.where(fast, np.where(dh, o.pt[g], e), st_)
            if mutant == "cw_slow_skipped" and not f.ids:
                live_neg &= fast
        lpg = 64 if qpg == 4 else 32
        if mutant == "skip_fourth":
            live_neg &= (n - s * per) % 4 != 3
        if mutant == "skip_past_first_block":
            live_neg &= (n - s * per) < lpg
        groups = np.ones(P, bool)
        if mutant == "drop_last_odd_group" and qpg == 2 and P % 2:
            groups[P - 1] = False
            live_neg &= g != P - 1
            Lval[P - 1] = Lerr[P - 1] = 0.0
        fi, si = np.nonzero(fast & live_neg)[0], np.nonzero(~fast & live_neg)[0]
        gone = np.nonzero(~live_neg)[0]
        Lval[P + gone] = 0.0
        # arithmetic of the negatives
        if len(si):
            Hs, _, _ = read_rows(ar, o.ent, nh[si], c.ent_norm, depth)
            Rs, _, _ = read_rows(ar, o.rel, nr[si], c.rel_norm, depth)
            Ts, _, _ = read_rows(ar, o.ent, nt[si], c.ent_norm, depth)
            put(P + si, *independent(ar, Hs, Rs, Ts, -1.0, nw[si], c.scale))
        cinv = Craw = None
        if len(fi):
            side = dh[fi].reshape(-1, 1)
            Craw = ar.lift(o.ent[e[fi]].astype(f64))
            base = ar.where(side, ar.take(Rn - Tn, g[fi]), ar.take(Hn + Rn, g[fi]))
            lo, rows, cinv = fast_negative(ar, Craw, base, side, nw[fi], c.scale, c.ent_norm)
            put(P + fi, lo, rows)
        if bwd:
            cnt = o.ref_count[:n_ent]
            ip = np.zeros(N, bool)
            if excl:
                ip[fi] = (cnt[e[fi]] == 1) | ((cnt[e[fi]] == 2) if mutant == "inplace_at_2" else False)
            if f.cw:                                                  # in-place rows are exactly the words with FAST and EXCL
                ip[fi] = xbit[fi] & (mutant != "cw_excl_ignored")
            a, b = fi[~ip[fi]], fi[ip[fi]]
            # a fast negative's own row, then its share of the flush of its work item (group g, slice s)
            swap = mutant == "cH_cT_swapped"
            E.add(0, e[a], e[a], stage_slot(g[a], npp, n[a], np.where(dh[a], 0, 2)), P + a, np.where(dh[a], 1, -1))
            to_tail = dh[fi] != swap
            ft, fh = fi[to_tail], fi[~to_tail]
            E.add(0, hub(o.pt[g[ft]], g[ft]), o.pt[g[ft]], stage_slot(g[ft], npp, npp, 2), P + ft, -1)
            E.add(0, hub(o.ph[g[fh]], g[fh]), o.ph[g[fh]], stage_slot(g[fh], npp, npp, 0), P + fh, 1)
            E.add(1, relcopy(s[fi] * P + g[fi]) * n_rel + o.pr[g[fi]], o.pr[g[fi]], stage_slot(g[fi], npp, npp, 1), P + fi, 1)
            # slow negatives: three rows each
            gs, ns = g[si], n[si]
            k3 = gs * (npp + 1) + ns
            kh = kt = np.ones(len(si), bool)
            if mutant == "cw_excl_without_fast" and f.cw:             # the word's entity row left to an in-place update that never comes
                kh, kt = ~(xbit[si] & dh[si]), ~(xbit[si] & ~dh[si])
            E.add(0, hub(nh[si], k3)[kh], nh[si][kh], stage_slot(gs, npp, ns, 0)[kh], P + si[kh], 1)
            E.add(1, relcopy(s[si] * P + gs) * n_rel + nr[si], nr[si], stage_slot(gs, npp, ns, 1), P + si, 1)
            E.add(0, hub(nt[si], k3)[kt], nt[si][kt], stage_slot(gs, npp, ns, 2)[kt], P + si[kt], -1)
            # the positive (slice 0), and the zero every flushing work item adds to its three rows
            gg = np.nonzero(groups)[0]
            E.add(0, hub(o.ph[gg], gg), o.ph[gg], stage_slot(gg, npp, npp, 0), gg, 1)
            E.add(1, relcopy(gg) * n_rel + o.pr[gg], o.pr[gg], stage_slot(gg, npp, npp, 1), gg, 2 if mutant == "gR_keeps_gP" else 1, 3)
            E.add(0, hub(o.pt[gg], gg), o.pt[gg], stage_slot(gg, npp, npp, 2), gg, -1)
            for sl in range(1, S):
                if sl * per < npp or mutant == "empty_slice_flushes":
                    aw = 1 if sl * per < npp else 0                 # the mutant's add of 0.0 leaves whatever the row holds, SENTINEL too
                    E.add(0, hub(o.ph[gg], gg), o.ph[gg], -1, zero, 1, aw)
                    E.add(1, relcopy(sl * P + gg) * n_rel + o.pr[gg], o.pr[gg], -1, zero, 1, aw)
                    E.add(0, hub(o.pt[gg], gg), o.pt[gg], -1, zero, 1, aw)
            if mutant == "rider_scores" and c.rider:                  # block 0 of the grid scores its four work items as well
                g4 = gg[:4 * (4 // qpg)]
                E.add(0, hub(o.ph[g4], g4), o.ph[g4], -1, g4, 1)
                Lval[g4] *= 2
            if len(b):
                pos_of = {int(v): k for k, v in enumerate(fi)}
                bi = np.array([pos_of[int(v)] for v in b], dtype=np.int64)
                Db = V(Dval[P + b], Derr[P + b]) if ar.bound else ar.lift(Dval[P + b])
                w2, a2 = in_place(ar, c, ar.take(Craw, bi), ar.lift(o.acc[e[b]].astype(f64)),
                                  Db, None if cinv is None else ar.take(cinv, bi), dh[b].reshape(-1, 1), mutant)
                inpl = {"rows": e[b], "w": ar.out(w2), "acc": None if a2 is None else ar.out(a2)}
    else:
        if N:
            Hs, _, _ = read_rows(ar, o.ent, nh, c.ent_norm, depth)
            Rs, _, _ = read_rows(ar, o.rel, nr, c.rel_norm, depth)
            Ts, _, _ = read_rows(ar, o.ent, nt, c.ent_norm, depth)
            put(P + np.arange(N), *independent(ar, Hs, Rs, Ts, -1.0, nw, c.scale))
        if bwd:
            i = np.arange(P + N)
            hh, rr, tt = (np.concatenate([a, b_]) for a, b_ in ((o.ph, nh), (o.pr, nr), (o.pt, nt)))
            E.add(0, hub(hh, i), hh, 3 * i, i, 1)
            E.add(1, relcopy(i) * n_rel + rr, rr, 3 * i + 1, i, 1)
            E.add(0, hub(tt, i), tt, 3 * i + 2, i, -1)
    return _assemble(c, f, o, ar, E, Dval, Derr, Lval, Lerr, inpl, mutant, K, det, excl, bwd)


def _sum(dest, n_dest, triple, sign, absw, Dval, Derr):
    """Row sums of the entries per destination: (values, error bounds, written mask)."""
    st = Dval.shape[1]
    val, err, tot = (np.zeros((n_dest, st)) for _ in range(3))
    np.add.at(val, dest, sign.reshape(-1, 1) * Dval[triple])
    np.add.at(err, dest, absw.reshape(-1, 1) * Derr[triple])
    np.add.at(tot, dest, absw.reshape(-1, 1) * np.abs(Dval[triple]))
    m = np.bincount(dest, weights=absw, minlength=n_dest).reshape(-1, 1)
    k = np.maximum(m - 1, 0) * 0.5 * U                               # a summation tree of m leaves has m - 1 additions, whatever its
    err += k / (1 - k) * tot + np.where(m > 1, TINY, 0.0)            # order: fma chain, butterflies and atomics are among them
    return val, err, m[:, 0] > 0


def _assemble(c, f, o, ar, E, Dval, Derr, Lval, Lerr, inpl, mutant, K, det, excl, bwd):
    n_ent, n_rel = sizes(c)
    st, d = c.stride, c.dim
    exact = c.tier == 1
    table, dest, row, slot, triple, sign, absw = E.arrays()
    out = {"tier": c.tier}
    m_thread = (max(c.npp, 0) + 1) * (1 + (c.n_pos + c.n_neg) // (WAVES * 4))
    lsum = Lval.sum() * c.scale * (c.scale if mutant == "scale_twice" else 1.0)
    out["loss"] = (lsum, None if exact else c.scale * (Lerr.sum() + m_thread * 0.5 * U * np.abs(Lval).sum()))
    cb = count_blocks(c)
    partials = np.zeros(LOSS_PARTIALS)
    partials[cb] = lsum
    if mutant == "rider_scores" and cb:
        partials[0] = Lval[0] * c.scale
    out["partials"], out["count_blocks"] = partials, cb
    live_col = np.arange(st) < d

    def finish(val, err, written, n_rows):
        buf = np.full((n_rows + 1, st), SENTINEL, dtype=f64)
        buf[:n_rows][written] = val[written]
        if mutant == "ragged_guard" and d % 16:
            buf[:n_rows][written, d - 1] = 0.0
        if mutant == "pad_added":
            buf[:n_rows][written] += 0.0 * np.where(live_col, 0.0, 1.0)
        e = np.zeros((n_rows + 1, st))
        e[:n_rows][written] = np.where(live_col, err[written], 0.0)
        return (buf.astype(f32), None) if (exact or not ar.bound) else (buf, e)

    n_gent = n_ent + (c.hot_copies * c.n_hot if c.n_hot else 0)
    n_grel = c.copies * n_rel
    t_ent, t_rel = np.full(n_ent + 64, OLD_TAG, dtype=np.int32), np.full(n_rel + 64, OLD_TAG, dtype=np.int32)
    if bwd and not det:
        for tb, nd, name in ((0, n_gent, "grad_ent"), (1, n_grel, "grad_rel")):
            m = table == tb
            val, err, written = _sum(dest[m], nd, triple[m], sign[m], absw[m], Dval, Derr)
            out[name] = finish(val, err, written, nd)
            (t_ent if tb == 0 else t_rel)[row[m]] = TAG
    elif bwd:
        n_slots = 3 * (c.n_pos * (c.npp + 1) if c.npp else c.n_pos + c.n_neg)
        m = slot >= 0
        val, err, written = _sum(slot[m], n_slots, triple[m], sign[m], absw[m], Dval, Derr)
        out["stage_rows"] = finish(val, err, written, n_slots)
        keys = np.full(n_slots + 1, KEY_FILL, dtype=np.int64)
        keys[slot[m]] = table[m] * STAGE_REL + row[m]
        out["stage_keys"] = keys
        # what mke_stage_reduce makes of the slots: every row's sum, one copy, no hub copies
        for tb, nd, name in ((0, n_gent, "reduced_ent"), (1, n_grel, "reduced_rel")):
            mm = table == tb
            val, err, written = _sum(row[mm], nd, triple[mm], sign[mm], absw[mm], Dval, Derr)
            out[name] = finish(val, err, written, nd)
            (t_ent if tb == 0 else t_rel)[row[mm]] = TAG
        out["reduced_touched"] = (t_ent.copy(), t_rel.copy())
        t_ent[:], t_rel[:] = OLD_TAG, OLD_TAG
    out["touched_ent"], out["touched_rel"] = t_ent, t_rel
    # tables, accumulator, reference counts
    rows = inpl["rows"]
    ent, acc, rcnt = o.ent.astype(f64), o.acc.astype(f64), o.ref_count.copy()
    ent_err, acc_err = np.zeros_like(ent), np.zeros_like(acc)
    if len(rows):
        wv, we = inpl["w"]
        ent[rows] = np.where(live_col, wv, 0.0)
        if we is not None:
            ent_err[rows] = np.where(live_col, we, 0.0)
        if inpl["acc"] is not None:
            av, ae = inpl["acc"]
            acc[rows] = np.where(live_col, av, float(ACC_PAD))
            if ae is not None:
                acc_err[rows] = np.where(live_col, ae, 0.0)
        if mutant != "refcount_not_reset":
            rcnt[rows] = 0
    lossless = exact or not ar.bound
    out["ent"] = (ent.astype(f32), None) if lossless else (ent, ent_err)
    out["acc"] = (acc.astype(f32), None) if lossless else (acc, acc_err)
    out["ref_count"] = rcnt
    out["in_place_rows"] = rows
    if f.cw:                                                         # neither reads nor resets ref_count; no entity flag without touched_ent
        out["cw"] = True
        del out["ref_count"]
        if not f.flags and mutant != "cw_flags_listed":
            del out["touched_ent"]
    return out


def two_kernel_reference(c: SCase, rows):
    """The rows `rows` of table and accumulator after the step WITHOUT ref_count followed by mke_rows_update: the gradient rows of
    `reference` (value, error) through the row kernel's own formula and bound (update_cases.py)."""
    gval, gerr = reference(c, Form(0, 0, 1, 1, 0, 1))["grad_ent"]
    o, ar = ops(c), Arith("bound")
    live_col = np.arange(c.stride) < c.dim
    with np.errstate(invalid="ignore", over="ignore"):
        w, g = ar.lift(o.ent[rows].astype(f64)), V(gval[rows], gerr[rows])
        if c.ent_norm:
            g = uc.jacobian(ar, w, g, c.fpl + 6)
        if c.opt == "adagrad":
            w2, a2 = uc.rule_adagrad(ar, w, g, ar.lift(o.acc[rows].astype(f64)), c.lr)
        else:
            w2, a2 = uc.rule_sgd(ar, w, g, c.lr), None
    fin = lambda x: None if x is None else (x.val, np.where(live_col, x.err, 0.0))
    return fin(w2), fin(a2)


# ----------------------------------------------------------------------------------------------------- comparison
def canon(a):
    """Bit patterns with -0 folded into +0 (the sign of a zero is not compared)."""
    a = np.ascontiguousarray(a, dtype=f32)
    return np.where(a == 0, f32(0), a).view(np.int32)


def _cmp(name, got, want, problems, ratios):
    val, err = want
    if err is None:
        if not np.array_equal(canon(got), canon(val)):
            bad = np.argwhere(canon(got) != canon(val))
            problems.append(f"{name}: differs from the exact reference at {bad[:3].tolist()} ({len(bad)} elements)")
        return
    nan = np.isnan(val)
    if not np.array_equal(np.isnan(got), nan):
        problems.append(f"{name}: NaN rows moved")
        return
    diff = np.where(nan, 0.0, np.abs(got.astype(f64) - np.where(nan, 0.0, val)))
    err = np.where(nan, 0.0, err)
    if (diff[err == 0] != 0).any():
        problems.append(f"{name}: an element with bound 0 (poison, a pad column, an untouched row) differs")
        return
    r = float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
    ratios[name] = r
    if not r <= 1:
        problems.append(f"{name}: error / bound = {r:.3g}")


def compare(got: dict, want: dict):
    """(problems, ratios).  got: the buffers after the launch -- "partials" [2048], the float buffers named as in `want`,
    "touched_ent", "touched_rel", "ref_count", "stage_keys"; a buffer the launch was not given is absent."""
    problems, ratios = [], {}
    p = got["partials"]
    cb = want["count_blocks"]
    if not np.isfinite(p).all():
        problems.append("loss: a partial was not written or is not finite")
    else:
        if p[:cb].any():
            problems.append("loss: a rider block's partial is not 0")
        lv, le = want["loss"]
        if le is None:
            if float(p.sum()) != lv:
                problems.append(f"loss: {float(p.sum())!r} != {lv!r}")
        else:
            ratios["loss"] = abs(float(p.sum()) - lv) / le if le > 0 else 0.0
            if not ratios["loss"] <= 1:
                problems.append(f"loss: error / bound = {ratios['loss']:.3g}")
    for name in ("grad_ent", "grad_rel", "stage_rows", "ent", "acc"):
        if name in got and name in want:
            _cmp(name, got[name], want[name], problems, ratios)
    for name in ("touched_ent", "touched_rel", "ref_count", "stage_keys"):
        if name in got and name in want and not np.array_equal(got[name], want[name]):
            problems.append(f"{name}: differs from the reference")
    if want.get("cw") and "touched_ent" in want and "touched_ent" not in got:
        problems.append("touched_ent: the reference lists entity flags, the launch had no flag array")
    return problems, ratios


def buffers_of(ref: dict) -> dict:
    """The buffers a kernel that computes `ref` leaves behind (float32)."""
    got = {"partials": ref["partials"].copy()}
    for name in ("grad_ent", "grad_rel", "stage_rows", "ent", "acc"):
        if name in ref:
            got[name] = np.asarray(ref[name][0], dtype=f32)
    for name in ("touched_ent", "touched_rel", "ref_count", "stage_keys"):
        if name in ref:
            got[name] = ref[name].copy()
    return got


def initial(name: str, want: dict):
    """What a scratch buffer holds before the launch: SENTINEL, and zeros in the rows that will receive an add or a store."""
    val = np.asarray(want[name][0])
    if name == "stage_rows":
        return np.full(val.shape, SENTINEL, dtype=f32)
    return np.where(val == SENTINEL, f32(SENTINEL), f32(0)).astype(f32)


# ----------------------------------------------------------------------------------------------------- mke_stage_reduce alone
class ReduceCase(NamedTuple):
    n_slots: int
    seg: int                # slots per row (the last segment may be shorter)
    stride: int = 32
    n_rows: int = 40


@functools.lru_cache(maxsize=4)
def reduce_ops(rcase: ReduceCase):
    """(stage_rows [n + 1, stride], sorted keys [n + 1], order [n + 1], expected grad_ent, grad_rel, touched_ent, touched_rel).
    A third of the slots is unused (0x7F keys, sorted last, SENTINEL rows that must not be read into a sum); relation and
    entity keys share row numbers; slot order is a permutation."""
    rng = np.random.default_rng([rcase.n_slots, rcase.seg, rcase.stride])
    n, st, R = rcase.n_slots, rcase.stride, rcase.n_rows
    used = n - n // 3
    seg_id = np.arange(used) // rcase.seg
    n_seg = int(seg_id.max()) + 1 if used else 0
    R = max(R, (n_seg + 1) // 2)
    key_of_seg = np.sort(np.concatenate([np.arange((n_seg + 1) // 2), STAGE_REL + np.arange(n_seg // 2)]))
    keys = np.full(n + 1, KEY_FILL, dtype=np.int64)
    keys[:used] = key_of_seg[seg_id]
    order = np.zeros(n + 1, dtype=np.int64)
    order[:n] = rng.permutation(n)
    rows = np.full((n + 1, st), SENTINEL, dtype=f32)
    rows[order[:used]] = quarters(rng, (used, st))
    ge, gr = np.full((R + 1, st), SENTINEL, dtype=f32), np.full((R + 1, st), SENTINEL, dtype=f32)
    te, tr = np.full(R + 64, OLD_TAG, dtype=np.int32), np.full(R + 64, OLD_TAG, dtype=np.int32)
    sums = np.zeros((n_seg, st))
    np.add.at(sums, seg_id, rows[order[:used]].astype(f64))
    bd = Bound()
    bd.add("segment", rcase.seg, 1 / 4)
    for k, key in enumerate(key_of_seg):
        (gr if key >= STAGE_REL else ge)[key % STAGE_REL] = sums[k].astype(f32)
        (tr if key >= STAGE_REL else te)[key % STAGE_REL] = TAG
    return rows, keys, order, ge, gr, te, tr, R, bd


REDUCE_CASES = [ReduceCase(n, seg) for n in REDUCE_SLOTS for seg in (1, 2, 300) if seg <= max(n, 1)] + [ReduceCase(17, 2, 320), ReduceCase(65, 3, 16)]


# ----------------------------------------------------------------------------------------------------- the case table
def _build():
    runs = []
    add = lambda case, form: runs.append(Run(case, form))
    for si, stride in enumerate(STRIDES):
        dims = table_dims(stride)
        big = stride > 128
        # tier 1: every group length, the twelve forms, the kinds and the weights in rotation
        for di, dim in enumerate(dims):
            for ni, npp in enumerate(NPPS):
                k = ni + 5 * di + si
                kinds = ("mixed", "fast", "mixed", "slow2nd" if npp >= 40 else "dup")[k % 4]
                n_pos = (3, 2, 1, 64)[k % 4] if npp <= 9 else (3, 2, 1)[k % 3]
                add(SCase(stride, dim, n_pos, npp, kinds=kinds, weights=("none", "pos", "both")[k % 3], scale=(1.0, 0.25)[k % 2],
                          copies=REL_COPIES[k % 4], opt=("sgd", "adagrad")[(k // 2) % 2]), forms12()[k % 12])
        dim = dims[si % len(dims)]
        for k, form in enumerate(forms12()):                         # all twelve at one shape, for the comparison among them
            add(SCase(stride, dim, 3, 9, kinds="mixed", weights="both", copies=2, tag="twelve"), form)
        # the default boundary of two groups per wavefront, and the option at 0 and 64
        for npp in ((31, 32) if big else (64, 65)):
            for half in (-1, 0, 64):
                add(SCase(stride, dim, 3, npp, kinds="mixed", tag="half"), Form(0, 1, 1, 1, half, 1))
        # a slow negative in the second id block only, in the two instantiations that fetch ids one per lane (__any must see it)
        for npp, half in ((100, 0), (40, 1000)):
            add(SCase(stride, dim, 3, npp, kinds="slow2nd", weights="both", tag="lanes"), Form(0, 1, 1, 1, half, 1))
        # slices: auto, forced, clamped, uneven, empty
        for npp, S in ((10, 0), (10, 1), (10, 2), (10, 3), (10, 10), (10, 15), (10, 4), (9, 4), (5, 4)):
            for x in (0, 1):
                add(SCase(stride, dim, 2, npp, kinds="mixed", weights="both", copies=(8, 2)[x], tag="slices"), Form(0, x, 1, 1, 0, S))
        # ungrouped, with and without negatives
        for n_neg0 in (0, 7):
            add(SCase(stride, dim, 5, 0, n_neg0, weights="both", copies=8, n_hot=5, hot_copies=3, tag="ungrouped"), Form())
            add(SCase(stride, dim, 5, 0, n_neg0, weights="pos", tag="ungrouped"), Form(det=1))
        # hub rows
        for hi, n_hot in enumerate((1, 5)):
            for ki, hcop in enumerate(HOT_COPIES):
                add(SCase(stride, dim, 64 if ki == 4 else 9, (2, 9)[ki % 2], kinds="mixed", n_hot=n_hot, hot_copies=hcop, n_ent=40, tag="hub"),
                    forms12()[(2 + 3 * (ki + hi)) % 12])
        add(SCase(stride, dim, 9, 2, kinds="mixed", n_hot=5, hot_copies=3, n_ent=40, tag="hub"), Form(det=1))
        # forward only
        add(SCase(stride, dim, 3, 9, kinds="mixed", weights="both", scale=0.25, fwd_only=True), Form(half=0))
        add(SCase(stride, dim, 3, 9, kinds="mixed", fwd_only=True), Form())
        add(SCase(stride, dim, 4, 0, 3, fwd_only=True), Form())
        # tier E / in place against two kernels: collision-free tier-2 batches (every form runs them, see the GPU test)
        for en, rn, opt in ((1, 1, "adagrad"), (0, 0, "sgd"), (1, 0, "sgd"), (0, 1, "adagrad")):
            add(SCase(stride, dim, 3, 9, tier=2, kinds="unique", weights="both", ent_norm=en, rel_norm=rn, opt=opt, special=bool(en)), Form(x=1, splits=1))
        # tier 2: collisions, slices, normalised tables
        for k, (en, rn) in enumerate(((1, 1), (0, 0), (1, 0))):
            for form in forms12() + [Form(0, 0, 1, 1, 0, 0), Form(0, 1, 0, 0, 0, 3)]:
                add(SCase(stride, dims[k % len(dims)], 3, (9, 33, 5)[k], tier=2, kinds="mixed", weights="both", copies=2, ent_norm=en, rel_norm=rn,
                          opt=("adagrad", "sgd")[k % 2], n_ent=60), form)
        # tier 2 across the boundary of the second id block: the flush sum of a group of 65, ids per lane and per round, staged
        for form in (Form(0, 1, 1, 1, 0, 1), Form(0, 1, 1, 1, 1000, 1), Form(0, 0, 1, 1, 0, 1), Form(1, 0, 1, 1, 0, 1)):
            add(SCase(stride, dim, 2, 65, tier=2, kinds="mixed", weights="both", ent_norm=1, rel_norm=1, opt="adagrad", tag="blocks"), form)
    # second grid pass, the count rider: one width is enough
    for n_pos, form in ((8193, Form(0, 1, 1, 1, 0, 1)), (16385, Form(0, 1, 1, 1, 64, 1)), (8193, Form(1, 0, 1, 1, 0, 1))):
        add(SCase(16, 16, n_pos, 1, kinds="fast", weights="pos", copies=8, n_ent=3000, tag="pass"), form)
    add(SCase(16, 15, 32769, 0, 0, weights="pos", copies=64, n_ent=3000, tag="pass"), Form())
    for total in COUNT_TOTALS:
        add(SCase(32, 31, 3, 9, kinds="mixed", weights="both", rider=total, tag="rider"), Form(x=1, splits=1))
        add(SCase(32, 31, 5, 0, 4, rider=total, tag="rider"), Form())
    assert len({r.id for r in runs}) == len(runs)
    return runs


RUNS = _build()


def _build_cw():
    """The runs of the code-word forms (beside RUNS, which they leave as it is).  Per width: every group length on "own" batches in
    tier 1, the eight forms in rotation; in tier 2 all eight forms on "own" batches with collisions (normalised tables, hub rows,
    a second id block), the forms with ids on "mixed" batches, slices, and the collision-free batches of tier E."""
    runs = []
    add = lambda case, form: runs.append(Run(case, form))
    F = forms_cw()
    for si, stride in enumerate(STRIDES):
        dims = table_dims(stride)
        for ni, npp in enumerate(NPPS):
            k = ni + si
            add(SCase(stride, dims[k % len(dims)], (3, 4, 2)[k % 3], npp, kinds="own", weights=("none", "pos", "both")[k % 3], scale=(1.0, 0.25)[k % 2],
                      copies=REL_COPIES[k % 4], opt=("sgd", "adagrad")[(k // 2) % 2], n_ent=40), F[k % 8])
        dim = dims[si % len(dims)]
        t2 = (SCase(stride, dim, 4, 9, tier=2, kinds="own", weights="both", copies=2, ent_norm=1, rel_norm=1, opt="adagrad", n_ent=40),
              SCase(stride, dims[(si + 1) % len(dims)], 3, 65, tier=2, kinds="own", weights="both", copies=8, opt="sgd", n_hot=5, hot_copies=3, n_ent=60),
              SCase(stride, dim, 5, 1, tier=2, kinds="own", weights="pos", ent_norm=1, opt="sgd", n_hot=1, hot_copies=2, n_ent=12))
        for c in t2:
            for form in F:
                add(c, form)
        for form in F:
            if form.ids:                                             # words without FAST that stand for other ids than the positive's
                add(SCase(stride, dim, 3, 9, tier=2, kinds="mixed", weights="both", copies=2, ent_norm=1, rel_norm=1, opt="adagrad", n_ent=60), form)
            if form.half == 0:                                       # slices: the positive as its own negative outside slice 0
                add(SCase(stride, dim, 2, 10, tier=2, kinds="own", weights="both", copies=2, ent_norm=1, opt="adagrad", n_ent=40, tag="slices"),
                    form._replace(splits=3))
        for en, opt in ((1, "adagrad"), (0, "sgd")):                 # tier E (every form runs them, see the GPU test)
            add(SCase(stride, dim, 4, 9, tier=2, kinds="own", weights="both", ent_norm=en, rel_norm=en, opt=opt, special=bool(en), tag="free"), F[0])
    for form in F:                                                   # entities past 2^16: a 16-bit entity mask shows
        add(SCase(16, 16, 3, 9, tier=2, kinds="own", weights="both", n_ent=70000, tag="mask"), form)
    assert len({r.id for r in runs}) == len(runs) and all(r.form.legal and r.case.npp > 0 for r in runs)
    assert all(r.form.ids or r.case.kinds == "own" for r in runs)
    return runs


CW_RUNS = _build_cw()


def runs_of(**kw):
    return [r for r in RUNS if all(getattr(r.case, k) == v for k, v in kw.items())]
