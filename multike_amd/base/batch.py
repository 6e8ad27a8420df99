"""base/batch.py surface of the reference (code/base/batch.py) over Python lists, backed by the device sampler.

These functions keep the reference's names and argument orders so that code written against `bat.*` runs
unchanged; each call converts its list arguments to device tensors (cached per list object), runs
`mke_neg_sample` and converts back.  The training loops in `MultiKE_model.py` do NOT go through this list
interface (it would put Python back on the critical path) — they use `sampling.RelationBatcher` directly.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from ..sampling import KGSide, KnownTripleSet, kg_batch_split, sample_negatives

_cache: dict = {}
_CACHE_MAX = 16
_call_counter = [0]


def _cached(objs, extra, build):
    """Device-side mirror of host containers, cached per container OBJECT: the entry holds the objects, so an id() cannot
    be recycled for another container while the entry lives; bounded, oldest entry out."""
    key = tuple(id(o) for o in objs) + tuple(extra)
    hit = _cache.get(key)
    if hit is None or any(a is not b for a, b in zip(hit[0], objs)):
        hit = (tuple(objs), build())
        _cache.pop(key, None)
        _cache[key] = hit
        while len(_cache) > _CACHE_MAX:
            _cache.pop(next(iter(_cache)))
    return hit[1]


def _known(triples_set, device):
    def build():
        arr = np.array(list(triples_set), dtype=np.int32).reshape(-1, 3)
        t = torch.as_tensor(arr, device=device)
        return KnownTripleSet(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous())
    return _cached((triples_set,), ("known", len(triples_set)), build)


def _side(entities_list, triples_set, neighbor, device):
    def build():
        side = KGSide(entities_list, _known(triples_set, device) if triples_set is not None else None, device=device)
        if neighbor:
            n_total = max(max(entities_list), max(neighbor)) + 1
            k = min(len(v) for v in neighbor.values())
            table = np.zeros((n_total, k), dtype=np.int32)
            valid = np.zeros(n_total, dtype=np.uint8)
            for e, lst in neighbor.items():
                table[e] = np.asarray(lst[:k], dtype=np.int32)
                valid[e] = 1
            side.set_neighbours(torch.as_tensor(table, device=device), torch.as_tensor(valid, device=device))
        return side
    return _cached((entities_list, triples_set, neighbor), ("side", len(entities_list)), build)


def generate_pos_triples(triples, batch_size, step, is_fixed_size=False):
    """code/base/batch.py:45-54."""
    lo = step * batch_size
    chunk = triples[lo:min(lo + batch_size, len(triples))]
    if is_fixed_size and len(chunk) < batch_size:
        chunk = chunk + triples[:batch_size - len(chunk)]
    return chunk


def generate_neg_triples_fast(pos_batch, all_triples_set, entities_list, neg_triples_num, neighbor=None, max_try=10,
                              seed=None, device="cuda"):
    """code/base/batch.py:86-116 on the device: same distribution, Philox stream (`seed` defaults to a per-call
    counter, as the reference draws from an unseeded global RNG)."""
    if len(pos_batch) == 0 or neg_triples_num == 0:
        return []
    side = _side(entities_list, all_triples_set, neighbor, device)
    arr = torch.as_tensor(np.asarray(pos_batch, dtype=np.int32).reshape(-1, 3), device=device)
    pos = (arr[:, 0].contiguous(), arr[:, 1].contiguous(), arr[:, 2].contiguous())
    if seed is None:
        _call_counter[0] += 1
        seed = (0x5EED, _call_counter[0])
    nh, nr, nt = sample_negatives(pos, side, neg_triples_num, seed=seed, max_try=max_try)
    out = torch.stack([nh, nr, nt], 1).cpu().numpy()
    return [tuple(int(v) for v in row) for row in out]


def generate_relation_triple_batch(triple_list1, triple_list2, triple_set1, triple_set2, entity_list1, entity_list2,
                                   batch_size, step, neighbor1, neighbor2, neg_triples_num):
    """code/base/batch.py:33-42."""
    b1, b2 = kg_batch_split(len(triple_list1), len(triple_list2), batch_size)
    pos1 = generate_pos_triples(triple_list1, b1, step)
    pos2 = generate_pos_triples(triple_list2, b2, step)
    neg1 = generate_neg_triples_fast(pos1, triple_set1, entity_list1, neg_triples_num, neighbor=neighbor1)
    neg2 = generate_neg_triples_fast(pos2, triple_set2, entity_list2, neg_triples_num, neighbor=neighbor2)
    return pos1 + pos2, neg1 + neg2


def generate_relation_triple_batch_queue(triple_list1, triple_list2, triple_set1, triple_set2, entity_list1, entity_list2,
                                         batch_size, steps, out_queue, neighbor1, neighbor2, neg_triples_num):
    """code/base/batch.py:22-30 (without the producer process's exit(0): there is no forked producer here)."""
    for step in steps:
        out_queue.put(generate_relation_triple_batch(triple_list1, triple_list2, triple_set1, triple_set2, entity_list1,
                                                     entity_list2, batch_size, step, neighbor1, neighbor2,
                                                     neg_triples_num))


def neighbour_table(entity_embeds, entity_list, neighbors_num, n_ent_total, device="cuda", block_rows=4096,
                    rows_per_launch=None, part=None, *, cap=None, seed=0, round_floats=None, keyed=None, keyed_params=None,
                    stats=None):
    """Truncated-sampling k-NN refresh on the device (code/base/batch.py:119-150): inner product of the (already
    row-normalised) relation-view rows of one KG's useful entities, top `neighbors_num` per row INCLUDING the entity
    itself, unordered.  Returns (cand_table [n_ent_total, k] int32 — [n_ent_total, cap] when capped, below —, cand_valid
    [n_ent_total] uint8) for `KGSide.set_neighbours`.

    When k is a small share of a long row the n x n similarity matrix is never built: a per-row threshold a bit below
    the k-th largest value is estimated from a fixed column sample (`mke_sim_sample` + `mke_topk_rows`),
    `mke_sim_select` computes the similarities tile by tile on the matrix cores and keeps only the ~1.4 k columns above
    the threshold, `mke_topk_rows` takes the exact top k of that short list.  The few rows whose estimate came out too
    tight (fewer than k hits) or too loose (a segment overflowed) are redone at full width (`mke_sim_sample` + `mke_topk_long`,
    which is also the path of short rows).  The result is the exact top-k set.

    part = (r, G): compute only the r-th of G contiguous slices of the rows (in the function's own working order) — the
    multi-GPU refresh: every rank holds all rows, ranks the slice it is given against all columns and the slices are
    all-gathered.  Returns (table, valid, ids_of_the_slice) with only those rows filled.

    cap (keyword only; None or >= k: off, today's table): the table is [n_ent_total, cap] — row e holds a uniform random
    cap-subset of e's exact top-k set, `mke_idlist_thin` of the list the uncapped call would have written, keyed by (seed, e)
    and applied to every block's [rows, k] list before it is scattered, so that no k-wide array outlives one launch or one
    round.  The kept set is a function of (seed, e, the top-k set) alone: the same whatever the path, the blocking or the
    slice.  round_floats (keyword only; default 2^28 floats = 1 GiB): the whole-row path ranks at most
    max(1, round_floats // n) rows at a time instead of `block_rows` — only when cap or round_floats is given; results
    never depend on it.

    keyed (keyword only): the matrix-free exact selection of a capped table at large k (include/multike_keyed.h).  Row e of a
    capped table is the cap members of e's top-k set with the smallest key(seed, e, neighbour), and a neighbour's key does not
    depend on its similarity: `mke_sim_select_keyed` sweeps the columns once with two thresholds per row taken from a keyed
    column sample (the `floor(s - z sqrt(s))`-th and `(ceil(s + z sqrt(s)) + 1)`-th largest of the row's n_samp sample
    similarities, s = k n_samp / n: `keyed_sample_ranks`), only COUNTS the hits above the upper one whose key is not below
    `keyed_key_below(cap, k)`, and keeps the others and every hit between the two; `mke_keyed_finish` takes the exact
    (k - sure)-th largest of the band, the members, and the cap smallest keys among them.  A row whose thresholds or key
    margin came out wrong (its status is not 0) is redone through the whole-row path; both paths write a row as the thinned
    list in ascending working-column order, so a table does not show which rows were redone.  The path works in the keyed
    working order `keyed_perm(n, 0x3C6EF372, device)`, in which `part` slices are defined, as on the thresholded path;
    `rows_per_launch` bounds a launch there too, and `round_floats` its candidate buffer (8 bytes a slot: by default a launch
    holds 1 GiB of candidates, what a whole-row round holds in similarities).  True forces the path (it needs cap < k, and a
    sample and a list the library takes: an error otherwise), False forbids it, None (default) takes it only when cap < k, the
    thresholded sweep does not apply and n >= 262,144 — every smaller call keeps its path and its bytes — and never raises: at
    large k / n it shrinks the sample to the largest one whose ranks fit, and a list too wide to pay stays on the whole-row
    path (`keyed_plan`, the whole decision on the host).  keyed_params = dict(n_samp=, z=) overrides the defaults
    min(65,536, n // 8) and 3.  stats: a dict the keyed path fills with `rows`, `redone` and `redone_by_status`
    ({status: rows}) from the statuses it reads back anyway."""
    from .. import _lib
    k = int(neighbors_num)
    if keyed and not (cap is not None and 1 <= int(cap) < k):       # before a device is touched
        raise _lib.MultiKEHipError(f"neighbour_table: keyed=True needs a capped table, 1 <= cap < k (cap {cap}, k {k})")
    if cap is not None and int(cap) < 1:
        raise _lib.MultiKEHipError(f"neighbour_table: cap must be >= 1 (or None = uncapped), got {cap}")
    if round_floats is not None and int(round_floats) < 1:
        raise _lib.MultiKEHipError(f"neighbour_table: round_floats must be >= 1, got {round_floats}")
    bounded = cap is not None or round_floats is not None     # whole-row rounds sized by round_floats, not block_rows
    width = int(cap) if cap is not None and int(cap) < k else k
    e = (entity_embeds.to(device).float() if isinstance(entity_embeds, torch.Tensor)
         else torch.as_tensor(np.asarray(entity_embeds), dtype=torch.float32, device=device))
    ids = torch.as_tensor(np.asarray(entity_list), dtype=torch.int64, device=device)
    n, d = e.shape
    table = torch.zeros(n_ent_total, width, dtype=torch.int32, device=device)
    valid = torch.zeros(n_ent_total, dtype=torch.uint8, device=device)
    n_samp, slots = 4096, _pow2_at_least(int(1.4 * k) + 64)
    short = n >= 8 * n_samp and slots * 4 <= n and slots <= 4096
    if bounded:
        block_rows = max(1, int(2 ** 28 if round_floats is None else round_floats) // max(n, 1))
    if d > _lib.SIM_SELECT_KPADS[-1]:     # wider than the widest table the package supports (MKE_MAX_STRIDE): no second backend
        raise _lib.MultiKEHipError(f"neighbour_table: rows of {d} floats exceed the widest k_sim_select instantiation "
                                   f"({_lib.SIM_SELECT_KPADS[-1]} = MKE_MAX_STRIDE)")
    kpad = min(x for x in _lib.SIM_SELECT_KPADS if x >= d)

    def full_width(rows):
        """top k of whole similarity rows (short KGs; rows whose threshold estimate was off).  The similarities come from the
        same sweep as the main pass (`mke_sim_sample` against ALL columns: identical fma chains) — a library GEMM here was
        the refresh's only library call and cost its 170 ms initialisation at the first refresh of a run."""
        cols = ep if ep is not None else _padded(e)
        src = cols[rows].contiguous()
        sim = _lib.sim_sample(src, kpad, 0, int(src.shape[0]), cols)
        return _lib.topk_long(sim, k).long()          # exact top k of whole rows: radix select in the package's own kernel

    def put(rows, lists=None):
        """scatter the [rows, k] entity-id lists of the working rows `rows` into the table — through the thinning kernel, keyed
        by the rows' entity ids, when the table is capped.  lists None: whole-row top k of those rows."""
        if lists is None:
            lists = ids[full_width(rows)].to(torch.int32)
        if width < k:
            lists = _lib.idlist_thin(lists, width, seed, row_ids=ids[rows].to(torch.int32))
        table[ids[rows]] = lists

    def _padded(x):
        out = torch.zeros(x.shape[0], kpad, dtype=torch.float32, device=device)
        out[:, :d] = x
        return out
    ep = None

    p_lo, p_hi = (0, n) if part is None else (n * part[0] // part[1], n * (part[0] + 1) // part[1])
    plan = keyed_plan(n, k, cap, short, keyed, keyed_params, round_floats)
    if plan is not None:
        # working order as on the thresholded path below: a row's hits are spread evenly over the column segments
        perm = keyed_perm(n, 0x3C6EF372, device)
        e, ids = e[perm], ids[perm]
        ep = _padded(e)
        ids32 = ids.to(torch.int32)
        n_samp, r_hi, r_lo, top = plan["n_samp"], plan["r_hi"], plan["r_lo"], plan["top"]
        key_below, slots, chunk = plan["key_below"], plan["slots"], plan["rows"]
        es = ep[keyed_perm(n, 0x1B873593, device)[:n_samp]].contiguous()
        if rows_per_launch:
            chunk = min(chunk, int(rows_per_launch))
        samp_rows = max(1, 2 ** 28 // n_samp)             # sample similarities, 1 GiB at a time
        by_status = {1: 0, 2: 0, 3: 0, 4: 0}
        for lo in range(p_lo, p_hi, chunk):
            hi = min(p_hi, lo + chunk)
            n_seg = 1
            while n_seg < 8 and ((hi - lo + 127) // 128) * n_seg < 6144 and n // (2 * n_seg) >= 4096:
                n_seg *= 2
            tau_lo = torch.full((hi - lo,), float("-inf"), dtype=torch.float32, device=device)
            tau_hi = torch.empty(hi - lo, dtype=torch.float32, device=device)
            for a in range(lo, hi, samp_rows):
                b = min(hi, a + samp_rows)
                sim = _lib.sim_sample(ep, kpad, a, b, es)
                vals = torch.gather(sim, 1, _lib.topk_long(sim, top).long())      # the row's `top` largest, unordered
                del sim
                tau_hi[a - lo:b - lo] = _lib.topk_rows(vals, r_hi, want_idx=False, want_kth=True)[1]
                if r_lo <= n_samp:
                    tau_lo[a - lo:b - lo] = _lib.topk_rows(vals, top, want_idx=False, want_kth=True)[1]
            cand, cnt, sure = _lib.sim_select_keyed(ep, kpad, lo, hi, tau_lo, tau_hi, ids32, seed, key_below, n_seg, slots // n_seg)
            out, status = _lib.keyed_finish(cand, cnt, sure, tau_hi, ids32[lo:hi], ids32, k, width, seed, key_below)
            del cand
            st = status.cpu().numpy()                     # the one read-back of a launch, as on the thresholded path
            bad = np.nonzero(st)[0]
            if bad.size == 0:
                table[ids[lo:hi]] = out
            else:
                good = torch.as_tensor(np.nonzero(st == 0)[0], dtype=torch.int64, device=device)
                table[ids[lo:hi][good]] = out[good]
                rows = torch.as_tensor(bad + lo, dtype=torch.int64, device=device)
                for a in range(0, rows.numel(), block_rows):
                    put(rows[a:a + block_rows])           # whole-row top k, thinned: the same row in the same order
                for s_, c_ in zip(*np.unique(st[bad], return_counts=True)):
                    by_status[int(s_)] = by_status.get(int(s_), 0) + int(c_)
        valid[ids[p_lo:p_hi]] = 1
        if stats is not None:
            stats.update(rows=p_hi - p_lo, redone=sum(by_status.values()), redone_by_status=by_status)
        return (table, valid) if part is None else (table, valid, ids[p_lo:p_hi])
    if not short:
        ep = _padded(e)
        for lo in range(p_lo, p_hi, block_rows):
            hi = min(p_hi, lo + block_rows)
            put(slice(lo, hi))
        valid[ids[p_lo:p_hi]] = 1
        return (table, valid) if part is None else (table, valid, ids[p_lo:p_hi])

    # The working order and the column sample are keyed permutations computed on the device with INTEGER arithmetic only
    # (argsort of a splitmix64-style mix of i + seed — `>>` on int64 is an arithmetic shift here, so it is not the textbook
    # function, only a fixed one): a function of (n, seed) alone, identical on every rank, device architecture and torch
    # build.  Round 3 drew them from a device torch.Generator — fast (a CPU permutation of 100K ids is 9 ms the GPU waits for),
    # but in part mode the slices of the multi-GPU refresh are DEFINED in this order, and a generator stream that differed
    # between ranks would silently leave candidate rows unfilled.  (keyed_perm, below.)
    # Work in a fixed random order of the entities: a row's hits are then spread evenly over the column segments whatever
    # the order of the ids (in id order similar entities sit together — URIs of one namespace, one generator block — and
    # most rows overflowed one of their segments on the DBP-WD-like folder: 54-75 % of the rows went to the full-width path).
    perm = keyed_perm(n, 0x3C6EF372, device)
    e, ids = e[perm], ids[perm]
    ep = _padded(e)
    ids32 = ids.to(torch.int32)
    samp = keyed_perm(n, 0x1B873593, device)[:n_samp]
    es = ep[samp].contiguous()
    m = min(n_samp, int(math.ceil(1.4 * k * n_samp / n)) + 8)
    chunk = (1 << 29) // slots - 128                      # rows per launch: 2^29 candidate slots (8 bytes each) at most
    if rows_per_launch:
        chunk = min(chunk, int(rows_per_launch))
    for lo in range(p_lo, p_hi, chunk):
        hi = min(p_hi, lo + chunk)
        # enough (row block, column segment) work items to fill the chip several times over, segments of >= 4096 columns
        n_seg = 1
        while n_seg < 8 and ((hi - lo + 127) // 128) * n_seg < 6144 and n // (2 * n_seg) >= 4096:
            n_seg *= 2
        tau = torch.empty(hi - lo, dtype=torch.float32, device=device)
        for a in range(lo, hi, 16384):                    # sample similarities, [16384, 4096] at a time
            b = min(hi, a + 16384)
            _, kth, _ = _lib.topk_rows(_lib.sim_sample(ep, kpad, a, b, es), m, want_idx=False, want_kth=True)
            tau[a - lo:b - lo] = kth
        cand, cnt = _lib.sim_select(ep, kpad, lo, hi, tau, n_seg, slots // n_seg)
        out, status = _lib.topk_candidates(cand, cnt, k, id_map=ids32)
        put(slice(lo, hi), out)                           # rows with status != 0 hold no list yet: redone below
        bad = torch.nonzero(status).reshape(-1)
        if bad.numel():
            rows = bad + lo
            for a in range(0, rows.numel(), block_rows):
                put(rows[a:a + block_rows])
    valid[ids[p_lo:p_hi]] = 1
    return (table, valid) if part is None else (table, valid, ids[p_lo:p_hi])


def keyed_perm(n, seed, device):
    """The keyed permutation of 0 .. n-1 behind neighbour_table's working order and its column samples."""
    x = torch.arange(n, dtype=torch.int64, device=device) + seed
    x = (x ^ (x >> 30)) * -4658895280553007687        # 0xBF58476D1CE4E5B9 as int64 (wrap-around multiply)
    x = (x ^ (x >> 27)) * -7723592293110705685        # 0x94D049BB133111EB
    x = x ^ (x >> 31)
    return torch.argsort(x, stable=True)


def keyed_key_below(m: int, k: int) -> int:
    """The key threshold of the keyed path: floor(2^64 * (m + 4 sqrt(m) + 8) / k) — the sweep keeps a sure neighbour with
    probability (m + 4 sqrt(m) + 8) / k, so that the m smallest keys of a row are among the kept ones but for ~4 standard
    deviations of their number.  Where the margin reaches k every key is wanted: 2^64 - 1, the largest threshold there is
    (a key equal to it is the one value still dropped).  sqrt is the double's; the division is exact."""
    num = Fraction(m + 4.0 * math.sqrt(m) + 8.0)
    return (1 << 64) - 1 if num >= k else int((num * (1 << 64)) // k)


def keyed_rows_per_launch(slots: int) -> int:
    """The most rows `mke_sim_select_keyed` takes in one launch at `slots` candidate slots a row: the row range rounded up to
    whole 128-row blocks, times the slots, stays below 2^29 (32-bit byte offsets of 8-byte slots)."""
    return max(1, ((1 << 29) - 1) // slots - 128)


KEYED_TOP_MAX = 4096          # the longest list mke_topk_rows ranks: the sample similarities a row's thresholds are taken from
KEYED_AUTO_MIN_N = 262_144    # the automatic rule: measured to win at n = 300,000 and 1,000,000, to lose where the thresholded sweep applies
KEYED_AUTO_MAX_SLOTS = 65_536  # ... and not measured beyond 16,384 slots a row: wider lists stay on the whole-row path unless forced


def keyed_plan(n: int, k: int, cap, short: bool, keyed=None, keyed_params=None, round_floats=None):
    """The decision of `neighbour_table(keyed=)` on the host: None (the call keeps the path it had), or the keyed path's plan
    dict(n_samp, z, r_hi, r_lo, top, key_below, slots, rows) — sample size, threshold ranks, how many of the largest sample
    similarities are ranked, candidate slots a row, rows a launch.  `short`: the thresholded sweep applies.

    keyed=False, no cap below k: None.  keyed=None (automatic): None unless the thresholded sweep does not apply and
    n >= KEYED_AUTO_MIN_N; the automatic rule never raises and never asks for more than the library takes — where the lower
    rank of the default (or given) sample lies beyond the KEYED_TOP_MAX values `mke_topk_rows` ranks (large k / n: s = k n_samp / n
    above ~3,900) it takes the largest sample whose rank fits, and where the list would need more than KEYED_AUTO_MAX_SLOTS
    slots a row it returns None.  keyed=True raises MultiKEHipError for a sample that does not fit or a list beyond the
    library's MKE_KEYED_MAX_LIST instead.  rows: at most `keyed_rows_per_launch(slots)`, and a candidate buffer of at most
    round_floats floats (default 2^28 = 1 GiB, the size of a whole-row round; 8 bytes a slot), at least one 128-row block."""
    from .. import _abi_keyed, _lib
    if keyed is False or cap is None or not 1 <= int(cap) < k:
        if keyed:
            raise _lib.MultiKEHipError(f"neighbour_table: keyed=True needs a capped table, 1 <= cap < k (cap {cap}, k {k})")
        return None
    if keyed is None and (short or n < KEYED_AUTO_MIN_N):
        return None
    kp = dict(keyed_params or {})
    z = float(kp.pop("z", 3.0))
    n_samp = max(1, min(n, int(kp.pop("n_samp", min(65_536, n // 8)))))
    if kp:
        raise _lib.MultiKEHipError(f"neighbour_table: unknown keyed_params {sorted(kp)}")

    def top_of(ns):                                       # r_lo beyond the sample: no lower threshold, everything is band
        return min(keyed_sample_ranks(k, n, ns, z)[1], ns)
    if top_of(n_samp) > KEYED_TOP_MAX:
        if keyed:
            raise _lib.MultiKEHipError(f"neighbour_table: the keyed path ranks the top {top_of(n_samp)} of {n_samp} sample "
                                       f"similarities, more than the {KEYED_TOP_MAX} mke_topk_rows holds: lower keyed_params['n_samp']")
        lo, hi = 1, n_samp                                # top_of is monotone in the sample size and top_of(1) = 1
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if top_of(mid) <= KEYED_TOP_MAX else (lo, mid - 1)
        n_samp = lo
    r_hi, r_lo = keyed_sample_ranks(k, n, n_samp, z)
    key_below = keyed_key_below(int(cap), k)
    expected = (min(r_lo, n_samp + 1) - r_hi) * n / n_samp + k * key_below / 2.0 ** 64    # band + kept sure
    slots = _pow2_at_least(int(1.25 * expected) + 64)
    if slots > (_abi_keyed.KEYED_MAX_LIST if keyed else KEYED_AUTO_MAX_SLOTS):
        if keyed:
            raise _lib.MultiKEHipError(f"neighbour_table: the keyed path would need {slots} candidate slots a row, more than the "
                                       f"{_abi_keyed.KEYED_MAX_LIST} of libmultike_keyed.so: the band is too wide (raise n_samp or lower z)")
        return None
    floats = int(2 ** 28 if round_floats is None else round_floats)
    rows = min(keyed_rows_per_launch(slots), max(128, floats // (2 * slots)))
    return dict(n_samp=n_samp, z=z, r_hi=r_hi, r_lo=r_lo, top=min(r_lo, n_samp), key_below=key_below, slots=slots, rows=rows)


def keyed_sample_ranks(k: int, n: int, n_samp: int, z: float):
    """(r_hi, r_lo): the ranks, from the top, of a row's two thresholds among its n_samp sample similarities.  s = k n_samp / n
    of them are expected in the top k, with a standard deviation below sqrt(s): r_hi = floor(s - z sqrt(s)), at least 1, and
    r_lo = ceil(s + z sqrt(s)) + 1.  r_lo may lie beyond the sample (tiny s, tiny samples): then there is no lower threshold."""
    s = k * n_samp / n
    return max(1, int(math.floor(s - z * math.sqrt(s)))), int(math.ceil(s + z * math.sqrt(s))) + 1


def refresh_seed(seed, epoch: int, kg_index: int) -> int:
    """The 64-bit seed of a capped refresh (`neighbour_table(cap=, seed=)`): a pure function of the run's seed, the epoch of
    the refresh and the KG (0 / 1) — the same on every rank, another subset at every refresh."""
    return ((int(seed) & 0xFFFFFFFF) << 32) | ((int(epoch) & 0x7FFFFFFF) << 1) | (int(kg_index) & 1)


def _pow2_at_least(x: int) -> int:
    p = 1
    while p < x:
        p *= 2
    return p


def generate_neighbours(entity_embeds, entity_list, neighbors_num, threads_num):
    """code/base/batch.py:119-140 — dict {entity: [k neighbours]} (the reference's return type)."""
    n_total = int(max(entity_list)) + 1
    table, _ = neighbour_table(entity_embeds, entity_list, neighbors_num, n_total)
    rows = table[torch.as_tensor(np.asarray(entity_list), dtype=torch.int64, device=table.device)].cpu().numpy()
    return {int(e): rows[i].tolist() for i, e in enumerate(entity_list)}
