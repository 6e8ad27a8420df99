"""Case tables, operand factories, kernel-by-kernel float64 references, scratch layouts, error bounds and mutants of the exact
tests of the dense steps' tails (test_tail_cases.py here, test_tail_exact_gpu.py on the device).  NumPy only.

Covered: the space-mapping step (mke_mapping.hip: gathers, P = V M with its sum-of-squares epilogue, k_map_tail1, k_map_tail2,
gM += V^T dP, k_map_ortho, k_scatter_dense_rows, the SGD update) phase by phase through mke_mapping_step_phases; the attribute
step's loss tail (mke_attr_cnn.hip: k_attr_tail_z, k_attr_tail_loss, k_attr_tail_bwd with k_colsum_add, and W^T / the backward on
planted sums through mke_attr_step_phases); the literal auto-encoder (mke_autoenc.hip and gemm_epilogue_ext, section C below:
bit for bit without activation, against float64 with tanh / sigmoid and for the wide, deep and ragged plans).  Every kernel is checked ALONE: the reference of a phase starts from what the device left in the scratch after
the phase before (float32 values, exact in float64), so no error is carried from one kernel into the bound of the next.

Operands follow rows_cases.py / update_cases.py: tables, F, GF and gradients are multiples of 1/4 in [-1, 1], the mapping
matrices multiples of 1/8 in [-1/2, 1/2], weights and learning rates powers of two.

Tier 1 (bit for bit; `Bound.check()` proves every sum exact in float32 in any order): P = V M of a view that is not read
through the row normalisation; k_map_ortho's gradient and loss; k_scatter_dense_rows and the atomic row scatter of
k_attr_tail_loss's touched tags; the SGD update of the matrices and the touched rows; gathers without normalisation; every
"this memory keeps its poison" check.

Tier 2 (float64 with a derived bound): everything behind rsqrtf, i.e. behind the batch-wide normalisation.  The kernel's own
formula runs through update_cases.Arith("bound") with the charges stated there (u/2 per rounding, 2 u for rsqrtf -- the
project's assumption, not measured --, a whole ulp for a stored value).  On top of that:

  (float) of a double scalar      u/2
  a per-thread fmaf chain         E u/2 of the sum of absolute values, E = the elements one thread adds (the grids are known)
  block_sum_double and the        2^-40 relative: at most 2048 + 256 double additions of 2^-53 each
    2048 partial slots
  an MFMA product of depth K      K u of sum |a b| per element: one rounding per accumulated term, charged a whole ulp since
    (+ S atomic split-K adds)     the rounding inside v_mfma_f32_* is not specified to be to nearest; + S u for the atomics
  tanhf                           4 x the error of the CPU's float32 tanh against float64 on the pre-activations the cases can
                                  form (the rule of test_gemm_clients_gpu.py::test_dense_layer_fwd_activation), `tanh_charge`
  softplus_f, sigmoid_f           exact for saturated rows (x >= rows_cases.SAT_POS: softplus_f(x) = x, sigmoid_f(x) = 1), else
                                  3 u + u softplus / 3 u sigmoid, counted out in `logistic_charges`

Nothing is fitted to a device; a ratio error / bound above 1 is a finding.

Poison: the scratch, G / GF and every partials array hold NaN on entry to the kernel that must rewrite them; tables have a NaN
tail row and zero pad columns (the ABI: the row kernels load whole strides); outputs have SENTINEL behind the logical region;
gradient pad columns hold SENTINEL where no update follows.
"""
from __future__ import annotations

import zlib
from typing import NamedTuple

import numpy as np

import rows_cases as rc
from rows_cases import OLD_TAG, SENTINEL, TAG, Bound, quarters
from update_cases import L2_EPS32, TINY, U, Arith, V, bits, lowbit

f32, f64 = np.float32, np.float64
BLOCK = 256
SLOTS = 2048                                                    # MKE_LOSS_PARTIALS
MAX_VIEWS = 3                                                   # MKE_MAPPING_MAX_VIEWS
MAP_MAX_DIM = 88                                                # MKE_MAP_MAX_DIM: 2 d (d + 1) floats of LDS
MAP_FWD, MAP_TAIL, MAP_BWD, MAP_UPD, MAP_ALL = 1, 2, 4, 8, 15
E_SHAPE = -2
DSUM = 2.0 ** -40                                               # block_sum_double + the slots, relative
ORTHO_W, NORM_W = 0.25, 0.125                                   # powers of two: every product with them is exact
MAP_LR = 0.25
FLOOR_SCALE = 2.0 ** -25                                        # view entries of the floor cases
S_FLOOR_PLANTED = 2.0 ** -42                                    # a planted total below MKE_L2_EPS = 1e-12 (2^-39.9)
MAP_WIDTHS = (1, 5, 16, 17, 64, 75, 80, 81, 88)
MAP_ROWS = (1, 15, 16, 17, 63, 65, 257)
MAP_ROWS_TALL = (1024, 1039)                                    # k_gemm_tall at d <= 80
MAP_BIG = (64, 32785)                                           # n d = 2048 x 1024 + 1088: the tail grids' second pass, 513 GEMM blocks
MAP_MUTANTS = ("slots_not_cleared", "floor_keeps_projection", "coef_one_inv", "first_view_adds", "later_view_overwrites",
               "ortho_keeps_identity", "scatter_last_wins")
ATTR_MUTANTS = ("bias_by_stride", "second_pass_row", "weights_dropped_in_gradient", "scale_twice", "wt_not_transposed")
MUTANTS = MAP_MUTANTS + ATTR_MUTANTS


def _rng(name: str, salt=0):
    return np.random.default_rng([zlib.crc32(name.encode()), salt])


def nan32(*shape):
    return np.full(shape, np.nan, dtype=f32)


# ----------------------------------------------------------------------------------------------------- shared arithmetic
def scalar32(ar: Arith, x: float):
    """(float)x of a double the kernel added up from the partial slots."""
    return V(x, 0.5 * U * abs(x) + TINY) if ar.bound else f32(x)


def live32(S: float) -> bool:
    """(float)S > MKE_L2_EPS as the kernels decide it."""
    return bool(f32(S) > f32(L2_EPS32))


def thread_elems(total: int, blocks: int) -> int:
    """Elements the busiest thread of a grid-stride loop over `total` elements visits."""
    return max(1, -(-total // (blocks * BLOCK)))


def chain_sum(ar: Arith, a, b, total_threads: int, depth: int):
    """sum a b the way a grid-stride kernel forms it: an fmaf chain of `depth` links per thread (the last one charged a whole
    ulp, as a stored value is), then doubles.  -> (per-thread values in f32 mode | None, (value, error))."""
    if ar.bound:
        t = a * b
        val = float(t.val.sum())
        err = float((t.err - (0.5 * U * np.abs(t.val) + TINY)).sum())          # the product inside an fmaf is not rounded
        return None, (val, err + (depth + 1) * 0.5 * U * float(np.abs(t.val).sum()) + DSUM * abs(val) + TINY)
    a, b = np.asarray(a, f32).ravel(), np.asarray(b, f32).ravel()
    n = a.size
    rounds = max(1, -(-n // total_threads))
    pa = np.zeros(rounds * total_threads, f32)
    pb = np.zeros(rounds * total_threads, f32)
    pa[:n], pb[:n] = a, b
    acc = np.zeros(total_threads, f32)
    for j in range(rounds):
        s = slice(j * total_threads, (j + 1) * total_threads)
        acc = (pa[s].astype(f64) * pb[s].astype(f64) + acc.astype(f64)).astype(f32)
    return acc, (float(acc.astype(f64).sum()), None)


def slots_of(thread_sums, blocks: int, stale=None):
    """The partials array a kernel with `blocks` blocks leaves: its block sums, zeros in the slots no block owns (`stale`: what
    a kernel that does not clear them leaves there)."""
    out = np.zeros(SLOTS, f64) if stale is None else np.array(stale, f64)
    out[:blocks] = thread_sums.astype(f64).reshape(blocks, BLOCK).sum(1)
    return out


def check_slots(name, got, want, problems, ratios):
    """All MKE_LOSS_PARTIALS slots finite, their sum against (value, error)."""
    val, err = want
    if got.shape != (SLOTS,) or not np.isfinite(got).all():
        problems.append(f"{name}: a partial slot is not finite")
        return
    diff = abs(float(got.sum()) - val)
    if err == 0:
        if diff != 0:
            problems.append(f"{name}: differs from the exact reference")
        return
    ratios[name] = diff / err
    if diff > err:
        problems.append(f"{name}: error / bound = {diff / err:.3g}")


def check_tier2(name, got, want, problems, ratios):
    val, err = want
    got = np.asarray(got)
    if got.shape != val.shape:
        problems.append(f"{name}: shape {got.shape}")
        return
    diff = np.abs(got.astype(f64) - val)
    if not np.isfinite(got).all() or (diff[err == 0] != 0).any():
        problems.append(f"{name}: not finite, or an element with bound 0 differs")
        return
    pos = err > 0
    r = float((diff[pos] / err[pos]).max()) if pos.any() else 0.0
    ratios[name] = r
    if r > 1:
        problems.append(f"{name}: error / bound = {r:.3g}")


def check_exact(name, got, want, problems):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(bits(got.astype(want.dtype, copy=False)), bits(want)):
        problems.append(f"{name}: differs from the reference")


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ===================================================================================================== A. the space-mapping step
class MCase(NamedTuple):
    d: int
    n: int
    views: tuple           # the `normalize` flag of each view table
    idx: str = "perm"      # perm: distinct rows | rep: rows hit several times
    ent_norm: int = 0
    plant: str = "own"     # what TAIL / BWD find in the partials: own (the device's) | total ([t, 0, ...]) | split (slots 0 and 2047)
    floor: str = ""        # "" | view (a view of 2^-25 entries: S < 1e-12 by itself) | planted (S = 2^-42 planted)
    sgd: bool = False      # UPD runs a second time with update = 1 (SGD, lr 1/4)

    @property
    def id(self):
        s = f"map-d{self.d}-n{self.n}-v{''.join(str(v) for v in self.views)}-{self.idx}-{self.plant}"
        return s + ("-entnorm" if self.ent_norm else "") + (f"-floor_{self.floor}" if self.floor else "") + ("-sgd" if self.sgd else "")

    @property
    def stride(self):
        return 16 * ((self.d + 15) // 16)

    @property
    def total(self):
        return self.n * self.d

    @property
    def blocks(self):
        """eb of mapping_step_impl: the grid of k_map_tail1 / k_map_tail2 / k_scatter_dense_rows."""
        return max(1, min(-(-self.total // (4 * BLOCK)), SLOTS))

    @property
    def tall(self):
        return self.d <= 80 and self.n >= 1024 and (self.n + 15) // 16 <= SLOTS

    @property
    def gemm_blocks(self):
        return (self.n + 15) // 16 if self.tall else -(-self.d // 64) * -(-self.n // 64)


def mapping_scratch_floats(n: int, d: int) -> int:
    return n * d * (2 + 3 * MAX_VIEWS)


def mapping_layout(n: int, d: int) -> dict:
    """name -> float offset into the scratch: F | GF | per view k: V_k, P_k, G_k, each [n][d] dense."""
    t = n * d
    lay = {"F": 0, "GF": t}
    for k in range(MAX_VIEWS):
        lay[f"V{k}"], lay[f"P{k}"], lay[f"G{k}"] = (2 + 3 * k) * t, (3 + 3 * k) * t, (4 + 3 * k) * t
    return lay


def map_region(scratch, c: MCase, name: str):
    o = mapping_layout(c.n, c.d)[name]
    return scratch[o:o + c.total].reshape(c.n, c.d)


class MOps(NamedTuple):
    n_ent: int
    ent: np.ndarray        # [n_ent + 1][stride] float32, zero pads, NaN tail row
    views: list            # the same, one per view
    M: np.ndarray          # [3][d][d] float32 in eighths, SENTINEL behind
    gM0: np.ndarray        # [3][d][d] quarters, SENTINEL behind
    idx: np.ndarray        # int32 [n]
    grad0: np.ndarray      # [n_ent + 1][stride]: quarters, SENTINEL pads and tail (zero pads where the SGD update follows)
    touched0: np.ndarray   # int32 [n_ent + 64] of OLD_TAG
    GF: np.ndarray         # [n][d] quarters: planted before UPD


def _table(mat, stride):
    buf = rc.padded_table(mat, stride)
    return np.concatenate([buf, nan32(1, stride)])


def _packed(mats, tail=64):
    return np.concatenate([np.asarray(mats, f32).ravel(), np.full(tail, SENTINEL, f32)])


def map_ops(c: MCase) -> MOps:
    rng = _rng(c.id)
    d, n = c.d, c.n
    n_ent = n + 3
    ent = _table(quarters(rng, (n_ent, d)), c.stride)
    views = []
    for k, _ in enumerate(c.views):
        m = quarters(rng, (n_ent, d))
        if c.floor == "view" and k == 0:
            m = m * FLOOR_SCALE
        views.append(_table(m, c.stride))
    M = rng.integers(-4, 5, (MAX_VIEWS, d, d)).astype(f64) / 8.0
    gM0 = quarters(rng, (MAX_VIEWS, d, d))
    if c.idx == "perm":
        idx = rng.permutation(n_ent)[:n]
    else:
        idx = rng.integers(0, max(1, n // 4) + 1, n)
    grad0 = np.full((n_ent + 1, c.stride), 0.0 if c.sgd else SENTINEL, f32)
    grad0[:n_ent, :d] = quarters(rng, (n_ent, d))
    grad0[n_ent] = SENTINEL
    touched0 = np.full(n_ent + 64, OLD_TAG, np.int32)
    return MOps(n_ent, ent, views, _packed(M), _packed(gM0), idx.astype(np.int32), grad0, touched0, quarters(rng, (n, d)).astype(f32))


def gather_reference(ar: Arith, table, stride, d, idx, normalize):
    """mke_gather_rows: whole strides are loaded (zero pads), the first d columns stored."""
    rows = np.asarray(table, f64)[idx]
    if not normalize:
        return (rows[:, :d], np.zeros((len(idx), d))) if ar.bound else (rows[:, :d].astype(f32), None)
    w = ar.lift(rows)
    inv = ar.rsqrt(ar.maximum(ar.dots(w, w, stride // 16 + 6), L2_EPS32))
    val, err = ar.out(ar.stored(w * inv))
    return val[:, :d], (None if err is None else err[:, :d])


def product_reference(A, B, depth, splits=0, add=None):
    """float64 A B (+ add) and the MFMA bound of the module docstring; the bound is 0 where the sum is exact in 24 bits."""
    A, B = np.asarray(A, f64), np.asarray(B, f64)
    val = A @ B
    mag = np.abs(A) @ np.abs(B)
    if add is not None:
        val, mag = val + add, mag + np.abs(add)
    unit = min(float(lowbit(A).min()), 1.0) * min(float(lowbit(B).min()), 1.0) if A.size and B.size else 1.0
    if add is not None and np.asarray(add).size:
        unit = min(unit, float(lowbit(add).min()))
    exact = np.isfinite(unit) and unit > 0 and mag.max(initial=0.0) / unit < 2 ** 24
    err = np.zeros_like(val) if exact else (depth + splits) * U * mag + TINY
    return val, err


def fwd_ssq_reference(P_dev):
    """sum P^2 of the device's own P: per-thread chains of at most 16 fmafs (16 accumulator registers in k_gemm_f32, two
    column tiles of four in k_gemm_tall)."""
    p = np.asarray(P_dev, f64)
    s = float((p * p).sum())
    return s, 17 * 0.5 * U * s + DSUM * s + TINY


def tail1_reference(ar: Arith, c: MCase, Ps, F, Ss, mutant="", poison=np.nan):
    """k_map_tail1 over the views of a TAIL phase -> {"G": [per view], "GF", "loss": [...], "dot": [...]} as (value, error)
    pairs, in f32 mode also "lossp" / "dotp": the partial arrays."""
    depth, threads = thread_elems(c.total, c.blocks), c.blocks * BLOCK
    Fl = ar.lift(F)
    out = {"G": [], "loss": [], "dot": [], "lossp": [], "dotp": []}
    gf = None
    for k, (P, S) in enumerate(zip(Ps, Ss)):
        inv = ar.rsqrt(ar.maximum(scalar32(ar, S), L2_EPS32))
        Pl = ar.lift(P)
        o = Pl * inv
        diff = ar.stored(ar.msub(Fl, Pl, inv))                  # G = -2 diff and the first GF = 2 diff are stored: exact scalings of it
        g = diff * -2.0
        two = diff * 2.0
        first = (k == 0) != (mutant == "first_view_adds" and k == 0)
        if mutant == "later_view_overwrites":
            first = True
        if first:
            gf = two
        else:                                                   # GF goes through memory between the views
            gf = ar.stored((ar.lift(np.full(np.shape(F), poison)) if gf is None else gf) + two)
        out["G"].append(ar.out(g))
        lt, loss = chain_sum(ar, diff, diff, threads, depth)
        dt, dot = chain_sum(ar, g, o, threads, depth)
        out["loss"].append(loss)
        out["dot"].append(dot)
        if not ar.bound:
            stale = np.full(SLOTS, poison) if mutant == "slots_not_cleared" else None
            out["lossp"].append(slots_of(lt, c.blocks, stale))
            out["dotp"].append(slots_of(dt, c.blocks, stale))
    out["GF"] = ar.out(gf)
    return out


def tail2_reference(ar: Arith, P, G, S, T, mutant=""):
    """k_map_tail2: dP = inv G - P coef, coef = S > eps ? T inv^2 : 0."""
    inv = ar.rsqrt(ar.maximum(scalar32(ar, S), L2_EPS32))
    Tf = scalar32(ar, T)
    live = live32(S) or mutant == "floor_keeps_projection"
    coef = ar.select(np.array(live), Tf * inv if mutant == "coef_one_inv" else Tf * inv * inv)
    return ar.out(ar.stored(ar.msub(ar.lift(G) * inv, ar.lift(P), coef)))


def ortho_reference(M, gM0, d, mutant=""):
    """k_map_ortho for one matrix, exact in float64: (gM, loss)."""
    M, gM0 = np.asarray(M, f64).reshape(d, d), np.asarray(gM0, f64).reshape(d, d)
    Q = M @ M.T - (0.0 if mutant == "ortho_keeps_identity" else np.eye(d))
    return gM0 + 4.0 * ORTHO_W * (Q @ M) + 2.0 * NORM_W * M, ORTHO_W * float((Q * Q).sum()) + NORM_W * float((M * M).sum())


def ortho_bound(b: Bound, M, gM0, d, what):
    """Every sum k_map_ortho forms, for Bound.check()."""
    M, gM0 = np.asarray(M, f64).reshape(d, d), np.asarray(gM0, f64).reshape(d, d)
    A = np.abs(M)
    Q = M @ M.T - np.eye(d)
    b.add(f"{what}: M M^T", (A @ A.T).max() + 1.0, 2.0 ** -6)
    b.add(f"{what}: Q M", (np.abs(Q) @ A).max(), 2.0 ** -9)
    b.add(f"{what}: gM", (np.abs(gM0) + 4 * ORTHO_W * (np.abs(Q) @ A) + 2 * NORM_W * A).max(), min(2.0 ** -9 * 4 * ORTHO_W, 2 * NORM_W / 8, 0.25))
    pad = (-(d * d)) % BLOCK
    q2 = np.concatenate([(Q * Q).ravel(), np.zeros(pad)]).reshape(-1, BLOCK).sum(0)      # thread t: elements t, t + 256, ...
    m2 = np.concatenate([(M * M).ravel(), np.zeros(pad)]).reshape(-1, BLOCK).sum(0)
    b.add(f"{what}: sum Q^2 per thread", q2.max(), 2.0 ** -12)
    b.add(f"{what}: sum M^2 per thread", m2.max(), 2.0 ** -6)
    b.add(f"{what}: w orth + nw nrm", (ORTHO_W * q2 + NORM_W * m2).max(), min(ORTHO_W * 2.0 ** -12, NORM_W * 2.0 ** -6))


def scatter_reference(grad0, touched0, idx, rows, d, mutant=""):
    """k_scatter_dense_rows: grad[idx[i]][:d] += rows[i], touched[idx[i]] = TAG."""
    grad, touched = np.asarray(grad0, f64).copy(), touched0.copy()
    if mutant == "scatter_last_wins":
        grad[idx, :d] = grad[idx, :d] + rows
    else:
        np.add.at(grad, (idx[:, None], np.arange(d)[None, :]), np.asarray(rows, f64))
    touched[idx] = TAG
    return grad.astype(f32), touched


def scatter_bound(b: Bound, grad0, idx, rows, d):
    mag = np.abs(np.asarray(grad0, f64)[:-1, :d])
    np.add.at(mag, (idx[:, None], np.arange(d)[None, :]), np.abs(np.asarray(rows, f64)))
    b.add("scatter", mag.max(), 0.25)


def sgd_reference(o: MOps, c: MCase, gM, grad, touched):
    """update = 1, SGD, no row normalisation: M -= lr gM, touched rows -= lr grad; both gradients consumed."""
    V_ = len(c.views)
    M = o.M.astype(f64).copy()
    k = V_ * c.d * c.d
    M[:k] -= MAP_LR * np.asarray(gM, f64)[:k]
    gM_after = np.asarray(gM, f32).copy()
    gM_after[:k] = 0
    ent, grad_after = o.ent.astype(f64).copy(), np.asarray(grad, f32).copy()
    rows = np.flatnonzero(touched[:o.n_ent] == TAG)
    ent[rows] -= MAP_LR * np.asarray(grad, f64)[rows]
    grad_after[rows] = 0
    return M.astype(f32), gM_after, ent.astype(f32), grad_after


def map_plant(c: MCase, own: float, what: str):
    """The partials block the host leaves in front of TAIL (what = S) / BWD (what = T): (array | None = keep, total)."""
    if c.floor == "planted" and what == "S":
        total = S_FLOOR_PLANTED
    elif c.plant == "own":
        return None, own
    else:
        total = 4.0 * own if what == "S" else 2.0 * own         # not the device's own sum: a kernel that ignored the plant would show
    arr = np.zeros(SLOTS, f64)
    if c.plant == "split":
        arr[0], arr[SLOTS - 1] = total / 2, total / 2
    else:
        arr[0] = total
    return arr, float(arr.sum())


def _map_cases():
    cases = []
    view_sets = ((0,), (1, 0), (0, 1, 1), (1,), (0, 0, 0), (0, 1))
    plants = ("own", "total", "split")
    i = 0
    for d in MAP_WIDTHS:
        for n in MAP_ROWS:
            cases.append(MCase(d, n, view_sets[i % len(view_sets)], "rep" if i % 2 else "perm", ent_norm=(i // 2) % 2, plant=plants[i % 3]))
            i += 1
        for n in MAP_ROWS_TALL:
            if d <= 80:
                cases.append(MCase(d, n, view_sets[i % len(view_sets)], "rep" if i % 2 else "perm", plant=plants[i % 3]))
                i += 1
    for d, n in ((5, 17), (16, 15)):
        cases.append(MCase(d, n, (0, 0), "perm", plant="own", floor="view"))
    for d, n, plant in ((17, 65, "total"), (88, 257, "split"), (75, 1039, "total")):
        cases.append(MCase(d, n, (0, 1, 0), "rep", plant=plant, floor="planted"))
    for d, n in ((17, 63), (88, 16), (64, 257)):
        cases.append(MCase(d, n, (0, 1, 0), "rep", plant="own", sgd=True))
    cases.append(MCase(MAP_BIG[0], MAP_BIG[1], (0,), "rep", plant="split"))
    assert len({c.id for c in cases}) == len(cases)
    return cases


MAP_CASES = _map_cases()


def gm_depth(n: int):
    """(k per split, splits) of the split-K product gM += V^T dP (launch_gemm_f32 with 16 splits over K = n)."""
    kps = (-(-n // 16) + 3) // 4 * 4
    return kps, -(-n // kps)


def emulate_map(c: MCase, mode: str, mutant="") -> dict:
    """The whole step on the case's operands in float32 NumPy ("f32", or "fma" with a - b c contracted), phase by phase, in the
    shape the device test reads back (see check_map).  `mutant` plants one kernel mistake."""
    ar = Arith(mode)
    o = map_ops(c)
    d, nv = c.d, len(c.views)
    M = o.M[:MAX_VIEWS * d * d].astype(f64).reshape(MAX_VIEWS, d, d)
    got = {"F": gather_reference(ar, o.ent[:-1], c.stride, d, o.idx, c.ent_norm)[0], "V": [], "P": [], "ssq": [], "S": [], "T": [], "dP": []}
    for k in range(nv):
        Vk = gather_reference(ar, o.views[k][:-1], c.stride, d, o.idx, c.views[k])[0]
        Pk = (Vk.astype(f64) @ M[k]).astype(f32)
        ssq = np.zeros(SLOTS)
        ssq[0] = float((Pk.astype(f64) ** 2).sum())
        got["V"].append(Vk), got["P"].append(Pk), got["ssq"].append(ssq)
        got["S"].append(map_plant(c, ssq[0], "S")[1])
    t1 = tail1_reference(ar, c, got["P"], got["F"], got["S"], mutant)
    got["G"], got["GF"] = [g[0] for g in t1["G"]], t1["GF"][0]
    got["lossp"], got["dotp"] = t1["lossp"], t1["dotp"]
    gM = o.gM0.copy()
    for k in range(nv):
        own = float(np.nansum(got["dotp"][k]))
        got["T"].append(map_plant(c, own, "T")[1])
        dP = tail2_reference(ar, got["P"][k], got["G"][k], got["S"][k], got["T"][k], mutant)[0]
        got["dP"].append(dP)
        blk = slice(k * d * d, (k + 1) * d * d)
        gM[blk] = (got["V"][k].astype(f64).T @ dP.astype(f64) + o.gM0[blk].astype(f64).reshape(d, d)).astype(f32).ravel()
    got["gM"] = gM
    upd, slots = o.gM0.copy(), np.zeros(SLOTS)
    for k in range(nv):
        blk = slice(k * d * d, (k + 1) * d * d)
        g, slots[k] = ortho_reference(M[k], o.gM0[blk], d, mutant)
        upd[blk] = g.astype(f32).ravel()
    got["gM_upd"], got["ortho"] = upd, slots
    got["grad"], got["touched"] = scatter_reference(o.grad0, o.touched0, o.idx, o.GF, d, mutant)
    return got


def check_map(c: MCase, o: MOps, got: dict):
    """(problems, ratios) of what a step left behind, kernel by kernel: every reference starts from the inputs that kernel
    itself found (`got` of the phase before).  Used on the device's read-backs and on the emulations alike."""
    problems, ratios = [], {}
    ar = Arith("bound")
    d, nv = c.d, len(c.views)
    M = o.M[:MAX_VIEWS * d * d].astype(f64).reshape(MAX_VIEWS, d, d)

    def gathered(name, g, table, normalize):
        val, err = gather_reference(ar, table[:-1], c.stride, d, o.idx, normalize)
        if normalize:
            check_tier2(name, g, (val, err), problems, ratios)
        else:
            check_exact(name, g, val.astype(f32), problems)
    gathered("F", got["F"], o.ent, c.ent_norm)
    for k in range(nv):
        gathered(f"V{k}", got["V"][k], o.views[k], c.views[k])
        check_tier2(f"P{k}", got["P"][k], product_reference(got["V"][k], M[k], d), problems, ratios)
        check_slots(f"ssq{k}", got["ssq"][k], fwd_ssq_reference(got["P"][k]), problems, ratios)
    t1 = tail1_reference(ar, c, got["P"], got["F"], got["S"])
    check_tier2("GF", got["GF"], t1["GF"], problems, ratios)
    kps, nz = gm_depth(c.n)
    for k in range(nv):
        check_tier2(f"G{k}", got["G"][k], t1["G"][k], problems, ratios)
        check_slots(f"loss{k}", got["lossp"][k], t1["loss"][k], problems, ratios)
        check_slots(f"dot{k}", got["dotp"][k], t1["dot"][k], problems, ratios)
        check_tier2(f"dP{k}", got["dP"][k], tail2_reference(ar, got["P"][k], got["G"][k], got["S"][k], got["T"][k]), problems, ratios)
        blk = slice(k * d * d, (k + 1) * d * d)
        want = product_reference(np.asarray(got["V"][k], f64).T, got["dP"][k], kps, nz, add=o.gM0[blk].astype(f64).reshape(d, d))
        check_tier2(f"gM{k}", got["gM"][blk].reshape(d, d), want, problems, ratios)
        g, loss = ortho_reference(M[k], o.gM0[blk], d)
        check_exact(f"ortho gM{k}", got["gM_upd"][blk], g.astype(f32).ravel(), problems)
        if got["ortho"][k] != loss:
            problems.append(f"ortho loss{k}: differs from the exact reference")
    if not (np.isfinite(got["ortho"]).all() and not got["ortho"][nv:].any()):
        problems.append("ortho loss: a slot no block owns is not zero")
    rest = slice(nv * d * d, None)
    if not (same_bits(got["gM"][rest], o.gM0[rest]) and same_bits(got["gM_upd"][rest], o.gM0[rest])):
        problems.append("gM: written outside the views' matrices")
    grad, touched = scatter_reference(o.grad0, o.touched0, o.idx, o.GF, d)
    check_exact("grad", got["grad"], grad, problems)
    check_exact("touched", got["touched"], touched, problems)
    return problems, ratios


def map_bound(c: MCase) -> Bound:
    """Every tier-1 sum of the case, for Bound.check()."""
    o = map_ops(c)
    d = c.d
    b = Bound()
    M = o.M[:MAX_VIEWS * d * d].astype(f64).reshape(MAX_VIEWS, d, d)
    for k, nz in enumerate(c.views):
        blk = slice(k * d * d, (k + 1) * d * d)
        ortho_bound(b, M[k], o.gM0[blk], d, f"view {k}")
        if not nz:
            Vk = o.views[k][:-1].astype(f64)[o.idx][:, :d]
            unit = float(min(lowbit(Vk).min(), 1.0)) / 8.0
            b.add(f"view {k}: P = V M", (np.abs(Vk) @ np.abs(M[k])).max(), unit)
        if c.sgd:
            g, _ = ortho_reference(M[k], o.gM0[blk], d)
            b.add(f"view {k}: M - lr gM", (np.abs(M[k]) + MAP_LR * np.abs(g)).max(), 2.0 ** -16)
    scatter_bound(b, o.grad0, o.idx, o.GF, d)
    if c.sgd:
        grad, _ = scatter_reference(o.grad0, o.touched0, o.idx, o.GF, d)
        b.add("w - lr g", (np.abs(o.ent[:-1].astype(f64)) + MAP_LR * np.abs(grad[:-1].astype(f64))).max(), 2.0 ** -4)
    return b


# ===================================================================================================== B. the attribute tail
class ZCase(NamedTuple):
    n: int
    dim: int
    bias: bool

    @property
    def id(self):
        return f"tailz-n{self.n}-d{self.dim}-{'bias' if self.bias else 'nobias'}"


Z_CASES = [ZCase(n, d, b) for n, d in ((1, 1), (37, 75), (16, 80), (2049, 256)) for b in (True, False)]


def tanh_charge() -> float:
    """4 x the largest error of the float32 CPU tanh against float64 over every pre-activation the cases can form (the
    multiples of 1/4 in [-3, 3]: z in [-2, 2] plus a bias in [-1, 1], exact in float32)."""
    x = np.arange(-12, 13) / 4.0
    return 4.0 * float(np.abs(np.tanh(x.astype(f32)).astype(f64) - np.tanh(x)).max())


def tailz_ops(c: ZCase):
    rng = _rng(c.id)
    z = np.concatenate([quarters(rng, c.n * c.dim, 2).astype(f32), np.full(64, SENTINEL, f32)])
    bias = np.concatenate([quarters(rng, c.dim).astype(f32), nan32(16)]) if c.bias else None
    return z, bias


def tailz_reference(c: ZCase, z, bias, mutant="", stride=16):
    """k_attr_tail_z: z = tanh(z + bias[i % dim]) in place, partials[b] = the block's sum z^2 for ALL 2048 blocks."""
    total = c.n * c.dim
    pre = np.asarray(z[:total], f64)                            # quarters: z + bias is exact in float32
    if bias is not None:
        i = np.arange(total)
        pre = pre + np.asarray(bias, f64)[i % (stride if mutant == "bias_by_stride" else c.dim)]
    val = np.tanh(pre)
    return (val, np.full(total, tanh_charge())), pre


def tailz_ssq_reference(c: ZCase, z_dev):
    """sum z^2 of the device's own z; 2048 x 256 threads, chains of ceil(total / 524288) fmafs."""
    p = np.asarray(z_dev, f64)
    s = float((p * p).sum())
    return s, (thread_elems(c.n * c.dim, SLOTS) + 1) * 0.5 * U * s + DSUM * s + TINY


class BCase(NamedTuple):
    """mke_attr_tail_bwd"""
    n: int
    dim: int
    grad_bias: bool = False
    floor: bool = False
    plant: str = "total"

    @property
    def id(self):
        return f"tailbwd-n{self.n}-d{self.dim}-{self.plant}" + ("-gbias" if self.grad_bias else "") + ("-floor" if self.floor else "")

    @property
    def blocks(self):
        return max(1, min(-(-(self.n * self.dim) // (4 * BLOCK)), 1024))


B_CASES = [BCase(1, 1), BCase(1, 1, floor=True), BCase(33, 31, plant="split"), BCase(33, 31, grad_bias=True), BCase(1024, 1),
           BCase(64, 16, grad_bias=True, plant="split"), BCase(205, 5, grad_bias=True), BCase(41, 25, floor=True, grad_bias=True),
           BCase(32785, 33, grad_bias=True, plant="split"), BCase(32785, 33, floor=True)]


def tailbwd_ops(c: BCase):
    """z in (-1, 1) as multiples of 1/8, g quarters, S / T planted as the host does; grad_bias a running sum of quarters."""
    rng = _rng(c.id)
    total = c.n * c.dim
    z = np.concatenate([(rng.integers(-7, 8, total) / 8.0).astype(f32), nan32(64)])
    g = np.concatenate([quarters(rng, total).astype(f32), np.full(64, SENTINEL, f32)])
    S = S_FLOOR_PLANTED if c.floor else float(np.asarray(z[:total], f64) @ np.asarray(z[:total], f64)) + 0.5
    T = float(np.asarray(z[:total], f64) @ np.asarray(g[:total], f64)) + 0.25
    sp, tp = np.zeros(SLOTS), np.zeros(SLOTS)
    if c.plant == "split":
        sp[0], sp[SLOTS - 1], tp[0], tp[SLOTS - 1] = S / 2, S / 2, T / 2, T / 2
    else:
        sp[0], tp[0] = S, T
    gb = np.concatenate([quarters(rng, c.dim, 4).astype(f32), np.full(16, SENTINEL, f32)]) if c.grad_bias else None
    return z, g, sp, tp, gb


def tailbwd_reference(ar: Arith, c: BCase, z, g, S, T, mutant=""):
    """k_attr_tail_bwd: g = inv (g - z coef) (1 - z z)."""
    total = c.n * c.dim
    zl, gl = ar.lift(np.asarray(z[:total], f64)), ar.lift(np.asarray(g[:total], f64))
    inv = ar.rsqrt(ar.maximum(scalar32(ar, S), L2_EPS32))
    Tf = scalar32(ar, T)
    live = live32(S) or mutant == "floor_keeps_projection"
    coef = ar.select(np.array(live), Tf * inv if mutant == "coef_one_inv" else Tf * inv * inv)
    one = ar.lift(np.ones(total))
    return ar.out(ar.stored(ar.msub(gl, zl, coef) * inv * ar.msub(one, zl, zl)))


def colsum_reference(c: BCase, g_dev, gb0):
    """k_colsum_add on the device's own g: 64 blocks, each a chain over ceil(n / 64) rows, then 64 atomic additions."""
    G = np.asarray(g_dev, f64).reshape(c.n, c.dim)
    val = G.sum(0) + np.asarray(gb0, f64)[:c.dim]
    mag = np.abs(G).sum(0) + np.abs(np.asarray(gb0, f64)[:c.dim])
    return val, (-(-c.n // 64) + 65) * 0.5 * U * mag + TINY


class LCase(NamedTuple):
    """mke_attr_tail_loss"""
    stride: int
    dim: int
    n: int
    weights: bool = True
    grad_ent: bool = True
    ent_norm: int = 0
    scale: float = 0.5
    plant: str = "total"

    @property
    def id(self):
        return (f"tailloss-s{self.stride}-d{self.dim}-n{self.n}-{self.plant}" + ("" if self.weights else "-nows") + ("" if self.grad_ent else "-nogent") +
                ("-entnorm" if self.ent_norm else "") + f"-sc{self.scale:g}")

    @property
    def blocks(self):
        return max(1, min(-(-self.n // 16), SLOTS))


L_STRIDES = (16, 32, 80, 128, 320)
L_ROWS = (0, 1, 15, 16, 17, 255, 257)
L_PASS = (16, 5, 32785)                                         # the second pass of the 2048 x 16-row loop, one row in it


def _l_cases():
    cases, i = [], 0
    for s in L_STRIDES:
        for dim in (s, s - 1, s - 15):
            for n in L_ROWS:
                cases.append(LCase(s, dim, n, weights=i % 3 != 0, grad_ent=i % 4 != 1, ent_norm=(i // 2) % 2, scale=(0.5, 2.0)[i % 2],
                                   plant=("total", "split")[i % 2]))
                i += 1
    for w, ge in ((True, True), (False, False)):
        cases.append(LCase(L_PASS[0], L_PASS[1], L_PASS[2], weights=w, grad_ent=ge, ent_norm=0, scale=0.5, plant="split"))
    assert len({c.id for c in cases}) == len(cases)
    return cases


L_CASES = _l_cases()


class LOps(NamedTuple):
    n_ent: int
    z: np.ndarray          # [n][dim] dense + NaN tail
    ent: np.ndarray        # [n_ent + 1][stride], zero pads, NaN tail row
    ih: np.ndarray         # int32 [n]: heads, repeated
    ws: np.ndarray         # float32 [n] powers of two + NaN tail | None
    S: float
    sumsq: np.ndarray      # planted
    gent0: np.ndarray      # quarters, SENTINEL pads and tail | None
    touched0: np.ndarray


def tailloss_ops(c: LCase) -> LOps:
    rng = _rng(c.id)
    n, dim = c.n, c.dim
    n_ent = max(2, n // 3 + 2)
    z = np.concatenate([(rng.integers(-7, 8, n * dim) / 8.0).astype(f32), nan32(64)])
    rows = quarters(rng, (n_ent, dim))
    if not c.ent_norm:                                          # |h| in [7, 8], |z inv| < 1: x >= 36 in every row, the saturated tier
        rows = np.where(rows < 0, rows - 7.0, rows + 7.0)
    ent = _table(rows, c.stride)
    ih = rng.integers(0, n_ent - 1, n).astype(np.int32)         # the last row is never a head: its gradient and tag must stay
    ws = np.concatenate([(2.0 ** rng.integers(-2, 2, n)).astype(f32), nan32(16)]) if c.weights else None
    S = float(4 ** np.ceil(np.log2(max(1.0, n * dim * 0.3)) / 2))               # near sum z^2, a power of 4
    sumsq = np.zeros(SLOTS)
    if c.plant == "split":
        sumsq[0], sumsq[SLOTS - 1] = S / 2, S / 2
    else:
        sumsq[0] = S
    gent0 = None
    if c.grad_ent:
        gent0 = np.full((n_ent + 1, c.stride), SENTINEL, f32)
        gent0[:n_ent, :dim] = quarters(rng, (n_ent, dim))
    return LOps(n_ent, z, ent, ih, ws, S, sumsq, gent0, np.full(n_ent + 64, OLD_TAG, np.int32))


def softplus64(x):
    return np.logaddexp(0.0, x)


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def logistic_charges(x: V):
    """(softplus, its error, sigmoid, its error) of softplus_f / sigmoid_f (mke_common.h) on the hardware transcendentals, which
    the ISA documents as 1 ulp each.  Rows with x >= SAT_POS are exact: exp(-x) < 2^-25 vanishes against 1, log(1) = 0,
    rcp(1) = 1 (test_rows_exact_gpu.py holds the device to these identities), so softplus_f(x) = x and sigmoid_f(x) = 1.
    Else, with e = exp(-|x|) <= 1 and s = 1 + e in [1, 2]: e carries u e, s that plus u/2 s <= 2 u, log(s) then 2 u / s + u log s
    <= 2.7 u, and the final addition u/2 of the result: 3 u + u softplus(x) absolute.  sigmoid: s carries 1.5 u relative, rcp
    1 u: 3 u relative.  The argument's own error passes through |softplus'| <= 1 and |sigmoid'| <= 1/4."""
    sat = x.val - x.err >= rc.SAT_POS
    sp, sg = softplus64(x.val), sigmoid64(x.val)
    sp_err = np.where(sat, x.err, 3 * U + U * sp + x.err)
    sg_err = np.where(sat, 0.0, 3 * U * sg + 0.25 * x.err)
    return np.where(sat, x.val, sp), sp_err, np.where(sat, 1.0, sg), sg_err


def tailloss_reference(ar: Arith, c: LCase, o: LOps, mutant=""):
    """k_attr_tail_loss: per row  diff = h - z inv, x = |diff|^2, loss += w softplus(x), cf = 2 scale w sigmoid(x), g_h = cf diff,
    gout = -g_h, dot += gout . z; lossp holds scale x the block sums.
    -> {"gout", "gh" (per row, before the scatter), "loss", "dot"} as (value, error | None)."""
    n, dim = c.n, c.dim
    if n == 0:
        z = np.zeros((0, dim))
        return {"gout": (z, z), "gh": (z, z), "loss": (0.0, 0.0), "dot": (0.0, 0.0)}
    Z = np.asarray(o.z[:n * dim], f64).reshape(n, dim)
    ih = o.ih.astype(np.int64)
    if mutant == "second_pass_row":                             # rows of the second pass reuse the row id requested in the first
        span = c.blocks * 16
        ih = np.where(np.arange(n) >= span, ih[np.arange(n) % span], ih)
    H, herr = gather_reference(ar, o.ent[:-1], c.stride, dim, ih, c.ent_norm)
    Hl = V(H, herr) if ar.bound else H
    Zl = ar.lift(Z)
    inv = ar.rsqrt(ar.maximum(scalar32(ar, o.S), L2_EPS32))
    diff = ar.msub(Hl, Zl, inv)
    depth = c.stride // 16 + 4                                  # fmaf chain per lane + the four butterflies of sub16_sum
    x = ar.dots(diff, diff, depth)
    w = np.asarray(o.ws[:n], f64).reshape(n, 1) if c.weights else np.ones((n, 1))
    scale = c.scale * (c.scale if mutant == "scale_twice" else 1.0)
    wg = np.ones((n, 1)) if mutant == "weights_dropped_in_gradient" else w
    rows_per_lane = -(-n // (c.blocks * 16))
    if ar.bound:
        sp, sp_err, sg, sg_err = logistic_charges(x)
        gh = ar.stored(diff * (V(sg, sg_err) * (2.0 * scale) * V(wg)))       # powers of two: exact, charged u/2 all the same
        dotrow = ar.dots(gh, Zl, depth)
        lt = V(sp, sp_err) * V(w)
        loss_val = float(lt.val.sum()) * c.scale
        loss_err = (float(lt.err.sum()) + (rows_per_lane + 1) * 0.5 * U * float(np.abs(lt.val).sum())) * c.scale + DSUM * abs(loss_val) + TINY
        dot_val = -float(dotrow.val.sum())
        dot_err = float(dotrow.err.sum()) + (rows_per_lane + 1) * 0.5 * U * float(np.abs(gh.val * Z).sum()) + DSUM * abs(dot_val) + TINY
        return {"gout": (-gh.val, gh.err), "gh": (gh.val, gh.err), "loss": (loss_val, loss_err), "dot": (dot_val, dot_err)}
    x64 = x.astype(f64)
    sat = x64 >= rc.SAT_POS
    sp = np.where(sat, x64, softplus64(x64)).astype(f32)
    sg = np.where(sat, 1.0, sigmoid64(x64)).astype(f32)
    gh = diff * (sg * f32(2.0 * scale) * wg.astype(f32))
    dot = -float(ar.dots(gh, Zl, depth).astype(f64).sum())
    return {"gout": (-gh, None), "gh": (gh, None), "loss": (float((sp * w.astype(f32)).astype(f64).sum()) * c.scale, None), "dot": (dot, None)}


def tailloss_gent_reference(c: LCase, o: LOps, gh):
    """grad_ent after the atomic row scatter of g_h onto gent0: (value, error) over [n_ent][dim]; an atomic addition rounds,
    the last one charged a whole ulp."""
    val, err = gh
    g = np.asarray(o.gent0, f64)[:o.n_ent, :c.dim].copy()
    mag, e = np.abs(g), np.zeros_like(g)
    cols = np.arange(c.dim)[None, :]
    np.add.at(g, (o.ih[:, None], cols), val)
    np.add.at(mag, (o.ih[:, None], cols), np.abs(val))
    np.add.at(e, (o.ih[:, None], cols), err)
    hits = np.bincount(o.ih, minlength=o.n_ent).reshape(-1, 1)
    return g, e + (hits + 1) * 0.5 * U * mag * (hits > 0) + TINY * (hits > 0)


# ----------------------------------------------------------------------------------------------------- B: emulations and checks
def emulate_tailz(c: ZCase, mutant=""):
    z, bias = tailz_ops(c)
    total = c.n * c.dim
    (val, _), _ = tailz_reference(c, z, bias, mutant)
    out = z.copy()
    out[:total] = val.astype(f32)
    acc, _ = chain_sum(Arith("f32"), out[:total], out[:total], SLOTS * BLOCK, 0)
    return out, slots_of(acc, SLOTS)


def check_tailz(c: ZCase, z0, bias, got_z, got_partials):
    problems, ratios = [], {}
    total = c.n * c.dim
    want, _ = tailz_reference(c, z0, bias)
    check_tier2("z", got_z[:total], want, problems, ratios)
    if not same_bits(got_z[total:], z0[total:]):
        problems.append("z: written behind n x dim")
    if np.isfinite(got_z[:total]).all():
        check_slots("ssq", got_partials, tailz_ssq_reference(c, got_z[:total]), problems, ratios)
    return problems, ratios


def emulate_tailbwd(c: BCase, mode="f32", mutant=""):
    z, g, sp, tp, gb = tailbwd_ops(c)
    total = c.n * c.dim
    out = g.copy()
    out[:total] = tailbwd_reference(Arith(mode), c, z, g, float(sp.sum()), float(tp.sum()), mutant)[0]
    if gb is not None:
        gb = gb.copy()
        gb[:c.dim] = (out[:total].astype(f64).reshape(c.n, c.dim).sum(0) + gb[:c.dim].astype(f64)).astype(f32)
    return out, gb


def check_tailbwd(c: BCase, got_g, got_gb):
    problems, ratios = [], {}
    z, g, sp, tp, gb = tailbwd_ops(c)
    total = c.n * c.dim
    check_tier2("dz", got_g[:total], tailbwd_reference(Arith("bound"), c, z, g, float(sp.sum()), float(tp.sum())), problems, ratios)
    if not same_bits(got_g[total:], g[total:]):
        problems.append("dz: written behind n x dim")
    if gb is not None and np.isfinite(got_g[:total]).all():
        check_tier2("grad_bias", got_gb[:c.dim], colsum_reference(c, got_g[:total], gb), problems, ratios)
        if not same_bits(got_gb[c.dim:], gb[c.dim:]):
            problems.append("grad_bias: written behind dim")
    return problems, ratios


def emulate_tailloss(c: LCase, mode="f32", mutant=""):
    o = tailloss_ops(c)
    r = tailloss_reference(Arith(mode), c, o, mutant)
    n, dim = c.n, c.dim
    gout = np.full(n * dim + 64, SENTINEL, f32)
    gout[:n * dim] = np.asarray(r["gout"][0], f32).ravel()
    lossp, dotp = np.zeros(SLOTS), np.zeros(SLOTS)
    lossp[0], dotp[0] = r["loss"][0], r["dot"][0]
    gent = touched = None
    if c.grad_ent:
        gent, touched = o.gent0.copy(), o.touched0.copy()
        acc = gent[:o.n_ent, :dim].astype(f64)
        np.add.at(acc, (o.ih[:, None], np.arange(dim)[None, :]), np.asarray(r["gh"][0], f64))
        gent[:o.n_ent, :dim] = acc.astype(f32)
        touched[o.ih] = TAG
    return {"gout": gout, "lossp": lossp, "dotp": dotp, "gent": gent, "touched": touched}


def check_tailloss(c: LCase, o: LOps, got: dict):
    problems, ratios = [], {}
    n, dim = c.n, c.dim
    want = tailloss_reference(Arith("bound"), c, o)
    check_tier2("gout", got["gout"][:n * dim].reshape(n, dim), want["gout"], problems, ratios)
    if not (got["gout"][n * dim:] == f32(SENTINEL)).all():
        problems.append("gout: written behind row n")
    check_slots("loss", got["lossp"], want["loss"], problems, ratios)
    check_slots("dot", got["dotp"], want["dot"], problems, ratios)
    if c.grad_ent:
        check_tier2("grad_ent", got["gent"][:o.n_ent, :dim], tailloss_gent_reference(c, o, want["gh"]), problems, ratios)
        keep = got["gent"].copy()
        keep[:o.n_ent, :dim] = o.gent0[:o.n_ent, :dim]
        if not same_bits(keep, o.gent0):
            problems.append("grad_ent: a pad column or the tail row changed")
        touched = o.touched0.copy()
        touched[o.ih] = TAG
        check_exact("touched", got["touched"], touched, problems)
    return problems, ratios


# ----------------------------------------------------------------------------------------------------- B: through mke_attr_step_phases
STEP_SHAPES = ((16, 37), (75, 80), (80, 81), (75, 37))          # (dim, n); the last has n < dim: no fused backward, no W^T


def attr_scratch_floats(n: int, d: int) -> int:
    return n * (10 * d + 4)


def attr_layout(n: int, d: int) -> dict:
    """name -> (float offset, rows, row length): flat [n][4d + 4] | dflat [n][4d] | z [n][d] | gout [n][d]."""
    fs = 4 * d + 4
    return {"flat": (0, n, fs), "dflat": (n * fs, n, 4 * d), "z": (n * fs + 4 * n * d, n, d), "gout": (n * fs + 5 * n * d, n, d)}


def fused_tail(n: int, d: int, option: int) -> bool:
    """c.fused_tail of attr_step_impl: the loss tail leaves W^T in the dflat scratch."""
    return bool(option) and d <= 80 and n >= d


def wt_reference(W, mutant=""):
    """The side job of k_attr_tail_loss: wt[k][f] = w[f][k], f < 4 dim, k < dim, as the first 4 dim^2 floats of dflat."""
    W = np.asarray(W, f32)
    return np.ascontiguousarray(W if mutant == "wt_not_transposed" else W.T).ravel()


def dz_reference(z, g, S: float, T: float):
    """dL/dzpre in float64 from the planted batch-wide scalars (the epsilon as the kernels hold it)."""
    z, g = np.asarray(z, f64), np.asarray(g, f64)
    inv = 1.0 / np.sqrt(max(float(f32(S)), L2_EPS32))
    coef = float(f32(T)) * inv * inv if live32(S) else 0.0
    return inv * (g - z * coef) * (1.0 - z * z)


def planted(total: float, form: str):
    arr = np.zeros(SLOTS)
    if form == "split":
        arr[0], arr[SLOTS - 1] = total / 2, total / 2
    else:
        arr[0] = total
    return arr


# ===================================================================================================== C. the literal auto-encoder
# Tier 1, act = none on sparse dyadic weights: every product of mke_ae_step_phases (forward with bias / alpha, the loss tail with target /
# target_scale / sumsq / colsum, dH = dZ W^T with colsum and dot_with / dot, dW = H^T dZ split over K with atomics) on dyadic
# operands, k_ae_scalar with planted totals and k_ae_norm_bwd.  Weights hold two entries of +-1/2 per column, biases 0 or +-1/2,
# x quarters: every activation stays below 8 and loses one bit of unit per layer; target_scale = 2 / (global_rows dims[0]) is a
# power of two.  Tanh, sigmoid and the plans whose sums cannot stay within 24 bits follow in the tier-2 section below.
AE_ENC, AE_DEC, AE_BWD, AE_UPD = 1, 2, 4, 8
AE_MUTANTS = ("colsum_one_half", "colsum_dead_rows", "target_ld", "mean_over_local_rows", "partials_not_rezeroed", "dact_dropped")
MUTANTS = MUTANTS + AE_MUTANTS


def pad4(x: int) -> int:
    return (x + 3) // 4 * 4


AE_ROWS = (1, 7, 8, 9, 15, 16, 17, 63, 65, 130)
AE_PLANS = (((16, 8), 16), ((64, 33, 9), 64), ((20, 12), 23), ((150, 140, 130), 150), ((32, 24, 16, 12, 8), 32))


class ACase(NamedTuple):
    dims: tuple
    rows: int
    global_rows: int
    ldx: int
    normalize: int
    form: str = "total"
    floor: bool = False
    shift: int = 0         # floats between a 16-byte boundary and the scratch: 1 sends every product that reads it to k_gemm_f32
    act: str = "none"      # none | tanh | sigmoid
    dense: bool = False    # dense dyadic weights, held in tier 2 whatever the activation

    @property
    def id(self):
        return (f"ae-{'x'.join(map(str, self.dims))}-m{self.rows}of{self.global_rows}-ldx{self.ldx}-{'norm' if self.normalize else 'plain'}-{self.form}" +
                ("-floor" if self.floor else "") + (f"-shift{self.shift}" if self.shift else "") + (f"-{self.act}" if self.tier2 else ""))

    @property
    def tier2(self):
        return self.dense or self.act != "none"

    @property
    def n(self):
        return len(self.dims) - 1


def _ae_cases():
    cases, i = [], 0
    for dims, ldx in (((16, 8), 16), ((64, 33, 9), 64), ((32, 12), 35)):
        for m in AE_ROWS:
            g = 1 << max(0, int(np.ceil(np.log2(m))))
            cases.append(ACase(dims, m, g, ldx, i % 2, ("total", "split")[(i // 2) % 2]))
            i += 1
    cases.append(ACase((16, 8), 37, 64, 16, 1, "split"))
    cases.append(ACase((64, 33, 9), 37, 64, 64, 0))
    cases.append(ACase((32, 12), 37, 64, 35, 1))
    cases.append(ACase((64, 33, 9), 65, 128, 64, 1, "split", floor=True))
    cases.append(ACase((16, 8), 9, 16, 16, 1, "total", floor=True))
    cases.append(ACase((16, 8), 17, 32, 16, 1, "split", shift=1))
    cases.append(ACase((64, 33, 9), 65, 128, 64, 1, "total", shift=1))
    cases.append(ACase((64, 33, 9), 9, 16, 64, 0, shift=1))
    cases.append(ACase((32, 12), 63, 64, 35, 1, "split", shift=1))
    # tier 2: every plan of the issue at every row count, the activations in turn (the two plans held bit for bit above at
    # act = none get tanh and sigmoid only); 37 of 64 rows; the scratch misaligned for the dword kernel
    i = 0
    for dims, ldx in AE_PLANS:
        acts = ("tanh", "sigmoid") if dims in ((16, 8), (64, 33, 9)) else ("none", "tanh", "sigmoid")
        for m in AE_ROWS + (37,):
            g = 64 if m == 37 else 1 << max(0, int(np.ceil(np.log2(m))))
            cases.append(ACase(dims, m, g, ldx, (i // 3) % 2, ("total", "split")[i % 2], act=acts[i % len(acts)], dense=True))
            i += 1
    for dims, ldx, m, act in (((64, 33, 9), 64, 65, "tanh"), ((32, 24, 16, 12, 8), 32, 17, "sigmoid"), ((150, 140, 130), 150, 130, "tanh"), ((20, 12), 23, 9, "sigmoid")):
        cases.append(ACase(dims, m, 256, ldx, 1, "split", shift=1, act=act, dense=True))
    assert len({c.id for c in cases}) == len(cases)
    return cases


A_CASES = _ae_cases()


def ae_offsets(dims):
    """(w_off, b_off, n_params) of the packed parameters: encoder layers, then decoder layers; a weight is [in][pad4(out)]."""
    n = len(dims) - 1
    shapes = [(dims[i], dims[i + 1]) for i in range(n)] + [(dims[n - j], dims[n - j - 1]) for j in range(n)]
    w_off, b_off, o = [], [], 0
    for din, dout in shapes:
        w_off.append(o)
        o += din * pad4(dout)
        b_off.append(o)
        o += pad4(dout)
    return w_off, b_off, o, shapes


def ae_layout(dims, rows: int) -> dict:
    """name -> (float offset, row stride): H1..Hn | D1..Dn | G0 | G1 | dcn | dz, the carve-up of ae_batch."""
    n = len(dims) - 1
    lay, o = {}, 0
    for name, w in ([(f"H{i}", dims[i]) for i in range(1, n + 1)] + [(f"D{j}", dims[n - j]) for j in range(1, n + 1)] +
                    [("G0", max(dims)), ("G1", max(dims)), ("dcn", dims[n]), ("dz", dims[n])]):
        lay[name] = (o, pad4(w))
        o += rows * pad4(w)
    lay["end"] = (o, 0)
    return lay


def ae_scratch_floats(dims, rows: int) -> int:
    return rows * sum(pad4(d) for d in dims) * 4 + 64


def ae_products(c: ACase):
    """Every launch_gemm_f32_ex of one step as (the GemmEpilogue fields it sets, True = k_gemm_vec), by the dispatcher's rule
    (gemm_cases.takes_vec_kernel); x and the packed parameters start 16-byte aligned, the scratch `shift` floats behind."""
    import gemm_cases as gc
    n, d, M = c.n, c.dims, c.rows
    w_off, b_off, _, shapes = ae_offsets(d)
    lay = ae_layout(d, M)

    def act(name):                                              # an activation matrix [M][width] as operand
        if name == "x":
            return gc.Placed(c.ldx, 1, 0, 0)
        return gc.Placed(lay[name][1], 1, lay[name][0] + c.shift, 0)

    def tr(p):
        return gc.Placed(p.cs, p.rs, p.offset, 0)

    def w(k, transposed=False):
        p = gc.Placed(pad4(shapes[k][1]), 1, w_off[k], 0)
        return tr(p) if transposed else p
    Hn = [("x" if i == 0 else f"H{i}") for i in range(n + 1)]
    Dn = [Hn[n]] + [f"D{j}" for j in range(1, n + 1)]
    out = []
    for i in range(n):
        f = {"bias"} | ({"sumsq"} if i == n - 1 and c.normalize else set())
        out.append((f, gc.takes_vec_kernel(M, d[i + 1], d[i], act(Hn[i]), w(i))))
    dz = Dn[n]
    for j in range(n):
        f = {"bias"} | ({"alpha"} if j == 0 and c.normalize else set()) | ({"target", "target_scale", "sumsq", "colsum"} if j == n - 1 else set())
        out.append((f, gc.takes_vec_kernel(M, d[n - j - 1], d[n - j], act(Dn[j]), w(n + j))))
    for j in range(n - 1, -1, -1):
        din, dout = d[n - j], d[n - j - 1]
        out.append(({"alpha"} if j == 0 and c.normalize else set(), gc.takes_vec_kernel(din, dout, M, tr(act(Dn[j])), act(dz))))
        f = {"dact_y", "colsum"} if j > 0 else ({"dot_with", "dot"} if c.normalize else set())
        out.append((f, gc.takes_vec_kernel(M, din, dout, act(dz), w(n + j, True))))
        dz = ("G0", "G1")[(n - 1 - j) % 2] if j > 0 else "dcn"
    dz = "dz"
    for i in range(n - 1, -1, -1):
        out.append((set(), gc.takes_vec_kernel(d[i], d[i + 1], M, tr(act(Hn[i])), act(dz))))
        if i > 0:
            out.append(({"dact_y", "colsum"}, gc.takes_vec_kernel(M, d[i], d[i + 1], act(dz), w(i, True))))
            dz = ("G0", "G1")[(n - 1 - i) % 2]
    return out


EPILOGUE_FIELDS = {"alpha", "bias", "target", "target_scale", "dact_y", "dot_with", "dot", "colsum", "sumsq"}


ACT64 = {"none": lambda v: v, "tanh": np.tanh, "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v))}
ACT_CODE = {"none": 0, "tanh": 1, "sigmoid": 2}


class AOps(NamedTuple):
    x: np.ndarray          # [rows + 1][ldx] float32, NaN pads and tail row
    params: np.ndarray     # packed, NaN in the pad entries, SENTINEL behind
    W: list                # float64 matrices, encoder then decoder
    b: list
    S: float               # planted sum code^2 (a power of 4, or 2^-42)
    D: float               # planted sum dcn . code (a power of two)


def ae_ops(c: ACase) -> AOps:
    rng = _rng(c.id)
    w_off, b_off, total, shapes = ae_offsets(c.dims)
    params = np.concatenate([nan32(total), np.full(64, SENTINEL, f32)])
    W, b = [], []
    for (din, dout), wo, bo in zip(shapes, w_off, b_off):
        if c.dense:                                             # multiples of 1/64 in [-1/4, 1/4]: pre-activations of spread ~ 0.1 sqrt(din)
            w, bias = rng.integers(-16, 17, (din, dout)) / 64.0, rng.integers(-16, 17, dout) / 64.0
        else:
            w = np.zeros((din, dout))
            for col in range(dout):
                rows = rng.choice(din, size=min(2, din), replace=False)
                w[rows, col] = rng.choice([-0.5, 0.5], size=len(rows))
            bias = rng.integers(-1, 2, dout) / 2.0
        params[wo:wo + din * pad4(dout)].reshape(din, pad4(dout))[:, :dout] = w
        params[bo:bo + dout] = bias
        W.append(w), b.append(bias)
    x = rc.poisoned(quarters(rng, (c.rows, c.dims[0])), c.ldx)
    ts = 2.0 / (c.global_rows * c.dims[0])                      # D of the size of sum dcn . code: dcn carries target_scale
    S = 16.0
    if c.tier2:                                                 # twice the batch's own sum: not what the device adds up itself
        h = x[:c.rows, :c.dims[0]].astype(f64)
        for i in range(c.n):
            h = ACT64[c.act](h @ W[i] + b[i])
        S = 2.0 * float((h * h).sum())
    return AOps(x, params, W, b, S_FLOOR_PLANTED if c.floor else S, -4.0 * ts)


def _colsum(v, mutant, tail_form=None):
    """Column sums over the live rows of a GEMM output, the way the 32-row tiles of gemm_epilogue_ext form them."""
    M = v.shape[0]
    s = v.sum(0)
    if mutant == "colsum_one_half" and M % 32:                  # the ragged tile: lanes 0-31 counted twice, lanes 32-63 dropped
        r = np.arange(M - M % 32, M)
        first = (r % 8) < 4
        s = s + v[r[first]].sum(0) - v[r[~first]].sum(0)
    if mutant == "colsum_dead_rows" and M % 32 and tail_form is not None:
        s = s + (32 - M % 32) * tail_form                       # what a dead row holds: the epilogue of a zero accumulator
    return s


def ae_reference(c: ACase, o: AOps, mutant="", bound: Bound = None):
    """The whole step in float64, exact.  -> dict of H, D (lists), dZ, loss, S_own, dcn, dot_own, dzc, grads (packed float64),
    scal.  `bound` collects every product for Bound.check()."""
    n, d, M = c.n, c.dims, c.rows
    w_off, b_off, total, shapes = ae_offsets(d)
    We, be, Wd, bd = o.W[:n], o.b[:n], o.W[n:], o.b[n:]
    X = o.x[:M, :d[0]].astype(f64)

    def prod(what, A, B, add=None):
        if bound is not None and A.size and B.size and not (c.floor and what != "H1" and not what.startswith("H")):
            unit = float(min(lowbit(A).min(), 1.0) * min(lowbit(B).min(), 1.0))
            mag = np.abs(A) @ np.abs(B)
            if add is not None:
                unit, mag = min(unit, float(min(lowbit(add).min(), 1.0))), mag + np.abs(add)
            bound.add(f"{c.id}: {what}", float(mag.max()), unit)
        return A @ B + (0.0 if add is None else add)
    H = [X]
    for i in range(n):
        H.append(prod(f"H{i + 1}", H[i], We[i], be[i]))
    code = H[n]
    live = live32(o.S)
    inv = float(f32(1.0 / np.sqrt(o.S if o.S > L2_EPS32 else L2_EPS32))) if c.normalize else 1.0
    D = [code]
    for j in range(n):
        a = prod(f"D{j + 1}", D[j], Wd[j])
        D.append((a * inv if j == 0 else a) + bd[j])
    target = X
    if mutant == "target_ld":
        target = o.x.ravel()[:M * d[0]].astype(f64).reshape(M, d[0])
    g_rows = M if mutant == "mean_over_local_rows" else c.global_rows
    ts = float(f32(2.0) / (f32(g_rows) * f32(d[0])))
    e = D[n] - target
    loss = float((e * e).sum()) / (g_rows * d[0])
    dZ = ts * e
    grads = np.zeros(total)

    def put_w(k, g):
        din, dout = shapes[k]
        grads[w_off[k]:w_off[k] + din * pad4(dout)].reshape(din, pad4(dout))[:, :dout] = g
    grads[b_off[2 * n - 1]:][:d[0]] = _colsum(dZ, mutant, ts * (bd[n - 1] - 0.0))
    dz = dZ
    for j in range(n - 1, -1, -1):
        put_w(n + j, prod(f"dW dec {j}", (D[j] * (inv if j == 0 else 1.0)).T, dz))
        dz = prod(f"dH dec {j}", dz, Wd[j].T)
        if j > 0:
            grads[b_off[n + j - 1]:][:d[n - j]] = _colsum(dz, mutant)
    dcn = dz
    out = {"H": H, "D": D, "dZ": dZ, "loss": loss, "S_own": float((code * code).sum()), "dcn": dcn, "dot_own": float((dcn * code).sum()),
           "grads_dec": grads.copy(), "live": live, "inv": inv, "ts": ts}
    if c.floor:                                                 # behind the floor nothing is dyadic: only H, the scalars and dz
        return out                                              # (from the device's own dcn) are held
    coef = inv ** 3 * o.D if (c.normalize and live) else 0.0
    dzc = inv * dcn - coef * code
    if bound is not None:
        bound.add(f"{c.id}: dz", float((np.abs(inv * dcn) + np.abs(coef * code)).max()), float(min(lowbit(inv * dcn).min(), lowbit(coef * code).min(), 1.0)))
    grads[b_off[n - 1]:][:d[n]] = _colsum(dzc, mutant)
    dz = dzc
    for i in range(n - 1, -1, -1):
        put_w(i, prod(f"dW enc {i}", H[i].T, dz))
        if i > 0:
            dz = prod(f"dH enc {i}", dz, We[i].T)
            grads[b_off[i - 1]:][:d[i]] = _colsum(dz, mutant)
    out.update(dzc=dzc, grads=grads)
    return out


def ae_emulate(c: ACase, mutant=""):
    """What a device that computes ae_reference(mutant) leaves behind, in the shape check_ae takes."""
    o = ae_ops(c)
    r = ae_reference(c, o, mutant)
    n = c.n
    got = {"H": [h.astype(f32) for h in r["H"][1:]], "D": [x.astype(f32) for x in r["D"][1:n]], "dZ": r["dZ"].astype(f32), "loss": r["loss"],
           "dcn": r["dcn"].astype(f32), "grads_dec": r["grads_dec"].astype(f32), "scal_dec": (f32(r["inv"]), f32(o.S)) if c.normalize else None,
           "ssq_own": r["S_own"] if c.normalize else 0.0, "dot_own": r["dot_own"] if c.normalize else 0.0,
           "partials_after_dec": np.zeros((3, SLOTS)), "partials_after_bwd": np.zeros((3, SLOTS))}
    if mutant == "partials_not_rezeroed" and c.normalize:
        got["partials_after_dec"][0] = planted(o.S, c.form)
    if not c.floor:
        got.update(dzc=r["dzc"].astype(f32), grads=r["grads"].astype(f32), scal_bwd=f32(o.D) if c.normalize else None)
    else:
        keep = r["inv"] ** 3 * o.D * r["H"][n] if mutant == "floor_keeps_projection" else 0.0
        got.update(dzc=(r["inv"] * got["dcn"].astype(f64) - keep).astype(f32), scal_bwd=f32(o.D))
    return got


def check_ae(c: ACase, o: AOps, got: dict):
    """problems of a step's read-backs against the exact reference (bit patterns; the three sums within 17 u/2)."""
    problems, ratios = [], {}
    r = ae_reference(c, o)
    n = c.n
    for i in range(n):
        check_exact(f"H{i + 1}", got["H"][i], r["H"][i + 1].astype(f32), problems)
    if not c.floor:
        for j in range(1, n):
            check_exact(f"D{j}", got["D"][j - 1], r["D"][j].astype(f32), problems)
        check_exact("dZ", got["dZ"], r["dZ"].astype(f32), problems)
        check_exact("dcn", got["dcn"], r["dcn"].astype(f32), problems)
        check_exact("decoder gradients", got["grads_dec"], r["grads_dec"].astype(f32), problems)
    sums = [("ssq_own", r["S_own"] if c.normalize else 0.0, r["S_own"])]
    if not c.floor:
        sums += [("loss", r["loss"], r["loss"]), ("dot_own", r["dot_own"] if c.normalize else 0.0, float(np.abs(r["dcn"] * r["H"][n]).sum()))]
    for name, val, mag in sums:
        err = 17 * 0.5 * U * mag + DSUM * mag + TINY
        diff = abs(got[name] - val)
        ratios[name] = diff / err
        if not np.isfinite(got[name]) or diff > err:
            problems.append(f"{name}: error / bound = {diff / err:.3g}")
    if c.normalize and not (same_bits(np.asarray(got["scal_dec"][0], f32), np.asarray(r["inv"], f32)) and got["scal_dec"][1] == f32(o.S)):
        problems.append("scal[0..1]: differs from the reference")
    if got["partials_after_dec"].any():
        problems.append("partials: not all zero after DEC")
    if not c.floor:
        check_exact("dz", got["dzc"], r["dzc"].astype(f32), problems)
        check_exact("gradients", got["grads"], r["grads"].astype(f32), problems)
    else:                                                       # on the floor: coef = 0, dz = inv dcn of the device's own dcn, one rounding
        check_exact("dz", got["dzc"], (r["inv"] * got["dcn"].astype(f64)).astype(f32), problems)
    if c.normalize and got["scal_bwd"] != f32(o.D):
        problems.append("scal[2]: differs from the reference")
    if got["partials_after_bwd"].any():
        problems.append("partials: not all zero after BWD")
    return problems, ratios



# ----------------------------------------------------------------------------------------------------- C, tier 2: activations, dense plans
# The same step with tanh / sigmoid (and the plans whose sums cannot stay within 24 bits) against float64 within a counted bound.
# Every kernel whose operands can be read back starts from the device's own operands; the gradient chain of a backward pass
# lives in the two ping-pong buffers and cannot all be read, so it starts at the device's dZ (decoder) and dz (encoder) and
# carries its error forward.  Charges: an MFMA product K u of sum |a b| (+ u per atomic pass); tanhf and the expf sigmoid of
# act_fwd 4 x the largest error of the CPU's float32 function on the case's own pre-activations; act' in plain operations; a
# column sum (chain + 1) u/2 of sum |v| with the chain counted per kernel; (float) of a double u/2.
def vT(x):
    return V(x.val.T, x.err.T) if isinstance(x, V) else np.asarray(x).T


def mm(ar: Arith, A, B, depth: int, passes: int = 0):
    """A B on the matrix cores: K u of sum |a b| per element, + u per atomic pass onto the output."""
    if not ar.bound:
        return (np.asarray(A, f64) @ np.asarray(B, f64)).astype(f32)
    A, B = V.lift(A), V.lift(B)
    mag = np.abs(A.val) @ np.abs(B.val)
    return V(A.val @ B.val, np.abs(A.val) @ B.err + A.err @ np.abs(B.val) + A.err @ B.err + (depth + passes) * U * mag + TINY)


def act32(kind, x32):
    x32 = np.asarray(x32, f32)
    return np.tanh(x32) if kind == "tanh" else (f32(1) / (f32(1) + np.exp(-x32))).astype(f32)


def act_fwd(ar: Arith, x, kind: str):
    if kind == "none":
        return x
    if not ar.bound:
        return act32(kind, x)
    x32 = x.val.astype(f32)
    charge = 4.0 * float(np.abs(act32(kind, x32).astype(f64) - ACT64[kind](x32.astype(f64))).max(initial=0.0))
    return V(ACT64[kind](x.val), (1.0 if kind == "tanh" else 0.25) * x.err + charge + TINY)


def act_grad(ar: Arith, y, kind: str):
    """act'(y) from the activation's output, as act_grad_from_output forms it.  Each operation is charged a whole ulp (`stored`):
    several roundings of the same size meet in one element here, and the float32 emulations must stay within half the bound."""
    one = ar.lift(np.ones(np.shape(ar.val(y))))
    return ar.stored(ar.msub(one, y, y)) if kind == "tanh" else ar.stored(y * ar.stored(one - y))


def vsum(ar: Arith, t, depth: int):
    """A batch-wide sum: fmaf chains of `depth` links per thread (+ 1), then doubles."""
    if not ar.bound:
        return float(np.asarray(t, f64).sum()), None
    val = float(t.val.sum())
    return val, float(t.err.sum()) + (depth + 1) * 0.5 * U * float(np.abs(t.val).sum()) + DSUM * abs(val) + TINY


def vcolsum(ar: Arith, v, depth: int):
    if not ar.bound:
        return np.asarray(v, f64).sum(0).astype(f32), None
    return v.val.sum(0), v.err.sum(0) + (depth + 1) * 0.5 * U * np.abs(v.val).sum(0) + TINY


def ae2_eval(ar: Arith, c: ACase, o: AOps, src=None, mutant=""):
    """Every output of ENC | DEC | BWD as (value, error | None).  src: the device's read-backs (each kernel then starts from
    them); None: the arithmetic's own results feed the next kernel (the emulation)."""
    n, d, M, kind = c.n, c.dims, c.rows, c.act
    We, be, Wd, bd = o.W[:n], o.b[:n], o.W[n:], o.b[n:]
    X = o.x[:M, :d[0]].astype(f64)
    tile_sum = 16 + 1 + -(-M // 32)                             # 16 registers, the half-wave exchange, an atomic per 32-row tile

    def take(key, own, idx=None):
        if src is None:
            return own                                          # bound mode: the composition in float64
        return ar.lift(np.asarray(src[key] if idx is None else src[key][idx], f64))

    def dense(A, W, b, K, alpha=None):
        acc = mm(ar, A, W, K)
        return (acc * alpha if alpha is not None else acc) + ar.lift(b)
    out = {"H": [], "D": []}
    Hs = [ar.lift(X)]
    for i in range(n):
        h = ar.stored(act_fwd(ar, dense(Hs[i], We[i], be[i], d[i]), kind))
        out["H"].append(ar.out(h))
        Hs.append(take("H", h, i))
    code = Hs[n]
    out["ssq_own"] = vsum(ar, code * code, 16) if c.normalize else (0.0, 0.0 if ar.bound else None)
    inv = None
    if c.normalize:
        t = 1.0 / np.sqrt(max(o.S, L2_EPS32))
        inv = V(t, U * t) if ar.bound else f32(t)               # (float) of a double, stored: a whole ulp
        out["inv"] = ar.out(inv) if ar.bound else (np.asarray(inv, f32), None)
    Ds = [code]
    for j in range(n - 1):
        dn = ar.stored(act_fwd(ar, dense(Ds[j], Wd[j], bd[j], d[n - j], inv if j == 0 else None), kind))
        out["D"].append(ar.out(dn))
        Ds.append(take("D", dn, j))
    v = act_fwd(ar, dense(Ds[n - 1], Wd[n - 1], bd[n - 1], d[1], inv if n == 1 else None), kind)
    e = ar.stored(v - ar.lift(X))
    ts = float(f32(2.0) / (f32(c.global_rows) * f32(d[0])))
    dZ = ar.stored(e * ar.k(ts))
    if kind != "none":
        dZ = dZ * act_grad(ar, v, kind)
    dZ = ar.stored(dZ)
    out["dZ"] = ar.out(dZ)
    lv, le = vsum(ar, e * e, 16)
    out["loss"] = (lv / (c.global_rows * d[0]), None if le is None else le / (c.global_rows * d[0]))
    g = {}
    dz = take("dZ", dZ)
    g[f"b{2 * n - 1}"] = vcolsum(ar, dz, tile_sum)
    for j in range(n - 1, -1, -1):
        dW = mm(ar, vT(Ds[j]), dz, M, 1)
        g[f"W{n + j}"] = ar.out(ar.stored(dW * inv if (j == 0 and inv is not None) else dW))
        nxt = mm(ar, dz, Wd[j].T, d[n - j - 1])
        if j > 0:
            if kind != "none" and mutant != "dact_dropped":
                nxt = nxt * act_grad(ar, Ds[j], kind)
            dz = ar.stored(nxt)
            g[f"b{n + j - 1}"] = vcolsum(ar, dz, tile_sum)
        else:
            dcn = ar.stored(nxt)
    out["dcn"] = ar.out(dcn)
    out["dot_own"] = vsum(ar, dcn * code, 16) if c.normalize else (0.0, 0.0 if ar.bound else None)
    dcn = take("dcn", dcn)
    if c.normalize:
        coef = ar.select(np.array(live32(o.S)), inv * inv * inv * scalar32(ar, o.D))
        vz = ar.stored(ar.msub(dcn * inv, code, coef))          # under cancellation this rounding is the element's whole error: a whole ulp
    else:
        vz = dcn
    if kind != "none":
        vz = vz * act_grad(ar, code, kind)
    vz = ar.stored(vz)
    out["dzc"] = ar.out(vz)
    dz = take("dzc", vz)
    g[f"b{n - 1}"] = vcolsum(ar, dz, 8 + 2 * -(-M // 16))       # an 8-row strip per thread, an atomic per strip
    for i in range(n - 1, -1, -1):
        g[f"W{i}"] = ar.out(ar.stored(mm(ar, vT(Hs[i]), dz, M, 1)))
        if i > 0:
            nxt = mm(ar, dz, We[i].T, d[i + 1])
            if kind != "none" and mutant != "dact_dropped":
                nxt = nxt * act_grad(ar, Hs[i], kind)
            dz = ar.stored(nxt)
            g[f"b{i - 1}"] = vcolsum(ar, dz, tile_sum)
    out["g"] = g
    return out


def ae_unpack(c: ACase, grads):
    """name -> the logical part of a packed gradient buffer; and whether every pad entry is zero."""
    w_off, b_off, total, shapes = ae_offsets(c.dims)
    parts, pads = {}, np.ones(total, bool)
    for k, (din, dout) in enumerate(shapes):
        m = np.asarray(grads[w_off[k]:w_off[k] + din * pad4(dout)]).reshape(din, pad4(dout))
        parts[f"W{k}"], parts[f"b{k}"] = m[:, :dout], np.asarray(grads[b_off[k]:b_off[k] + dout])
        mask = pads[w_off[k]:w_off[k] + din * pad4(dout)].reshape(din, pad4(dout))
        mask[:, :dout] = False
        pads[b_off[k]:b_off[k] + dout] = False
    return parts, not np.asarray(grads[:total])[pads].any()


def ae2_emulate(c: ACase, mode="f32", mutant=""):
    o = ae_ops(c)
    r = ae2_eval(Arith(mode), c, o, None, mutant)
    w_off, b_off, total, shapes = ae_offsets(c.dims)
    grads = np.zeros(total, f32)
    for k, (din, dout) in enumerate(shapes):
        grads[w_off[k]:w_off[k] + din * pad4(dout)].reshape(din, pad4(dout))[:, :dout] = r["g"][f"W{k}"][0]
        grads[b_off[k]:b_off[k] + dout] = r["g"][f"b{k}"][0]
    dec = grads.copy()
    dec[:w_off[c.n]] = 0
    return {"H": [h[0] for h in r["H"]], "D": [x[0] for x in r["D"]], "dZ": r["dZ"][0], "dcn": r["dcn"][0], "loss": r["loss"][0],
            "ssq_own": r["ssq_own"][0], "dot_own": r["dot_own"][0], "grads_dec": dec, "grads": grads, "dzc": r["dzc"][0],
            "scal_dec": (r["inv"][0], f32(o.S)) if c.normalize else None, "scal_bwd": f32(o.D) if c.normalize else None,
            "partials_after_dec": np.zeros((3, SLOTS)), "partials_after_bwd": np.zeros((3, SLOTS))}


def check_ae2(c: ACase, o: AOps, got: dict):
    problems, ratios = [], {}
    r = ae2_eval(Arith("bound"), c, o, got)
    n = c.n
    w_off = ae_offsets(c.dims)[0]
    for i in range(n):
        check_tier2(f"H{i + 1}", got["H"][i], r["H"][i], problems, ratios)
    for j in range(n - 1):
        check_tier2(f"D{j + 1}", got["D"][j], r["D"][j], problems, ratios)
    for name in ("dZ", "dcn", "dzc"):
        check_tier2(name, got[name], r[name], problems, ratios)
    for name in ("loss", "ssq_own", "dot_own"):
        val, err = r[name]
        diff = abs(got[name] - val)
        if err == 0:
            ok = diff == 0
        else:
            ratios[name] = diff / err
            ok = diff <= err
        if not np.isfinite(got[name]) or not ok:
            problems.append(f"{name}: error / bound = {diff / err if err else np.inf:.3g}")
    parts, pads_zero = ae_unpack(c, got["grads"])
    for name, want in r["g"].items():
        check_tier2("g" + name, parts[name], want, problems, ratios)
    if not pads_zero:
        problems.append("gradients: a pad entry of the packed buffer is not zero")
    if got["grads_dec"][:w_off[n]].any() or not same_bits(np.asarray(got["grads_dec"][w_off[n]:], f32), np.asarray(got["grads"][w_off[n]:], f32)):
        problems.append("gradients: DEC wrote an encoder gradient, or BWD a decoder one")
    if c.normalize:
        check_tier2("scal0", np.asarray(got["scal_dec"][0], f32), r["inv"], problems, ratios)
        if got["scal_dec"][1] != f32(o.S) or got["scal_bwd"] != f32(o.D):
            problems.append("scal[1..2]: differs from the reference")
    if got["partials_after_dec"].any() or got["partials_after_bwd"].any():
        problems.append("partials: not all zero after the phase that consumes them")
    return problems, ratios


def check_wt(got_wt, W):
    """The device test's comparison of the W^T copy."""
    problems = []
    check_exact("W^T", np.asarray(got_wt, f32), wt_reference(W), problems)
    return problems
