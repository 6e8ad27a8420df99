"""Shared pieces of the owner-bucketed-codes tests (tests/test_oc_owned_codes_gpu.py, tests/test_oc_owned_codes_cpu.py): the NumPy
enumeration of the buckets and the owned index by the header's definition (include/multike_hip.h, section 13b), the C-ABI calls by
hand, and copies of the epoch generator / direct enumeration / plan check of tests/test_oc_em_plan_gpu.py and of the trainer factory
of tests/test_distributed_oc_gpu.py (existing test modules stay as they are)."""
import numpy as np
import torch

from multike_amd import _lib

GV, PLUS = 0x80000000, 1 << 24
MASK = 0x3FFFFFFF
NEED = 0xC0000000


# ---- NumPy enumerations ---------------------------------------------------------------------------------------------------
def np_bucket(codes, n_mine, N, pos0, G):
    """(need flags [n_mine] as uint32, [records of destination d in (position, n) order] for d < G) of a share of codes."""
    codes = np.asarray(codes, dtype=np.int64) & 0xFFFFFFFF
    need = (codes.reshape(n_mine, N)[:, 0] & NEED) if N else np.full(n_mine, 0x40000000, dtype=np.int64)
    c = codes[:n_mine * N] & MASK
    dest = (c >> 1) % G
    out = []
    for d in range(G):
        e = np.nonzero(dest == d)[0]                   # ascending element index = (position, n) order
        out.append(np.stack([pos0 + e // max(N, 1), e % max(N, 1), c[e]], 1).astype(np.int32).reshape(-1, 3))
    return need.astype(np.uint32), out


def np_owned(codes, n_all, N, G, rank):
    """(records this rank owns in (position, n) order, own_off [n_all + 1]) straight from the epoch's codes by position."""
    codes = np.asarray(codes, dtype=np.int64) & MASK
    recs = [(p, n, int(codes[p * N + n])) for p in range(n_all) for n in range(N) if (int(codes[p * N + n]) >> 1) % G == rank]
    recs = np.asarray(recs, dtype=np.int32).reshape(-1, 3)
    off = np.searchsorted(recs[:, 0], np.arange(n_all + 1)).astype(np.int32)
    return recs, off


# ---- C-ABI by hand ----------------------------------------------------------------------------------------------------------
def dev32(a, n_min=1):
    """int32 device tensor of the low 32 bits of `a` (codes with their flag bits wrap into the sign), at least n_min long."""
    a = (np.asarray(a, dtype=np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    t = torch.zeros(max(n_min, a.size), dtype=torch.int32, device="cuda")
    t[:a.size] = torch.as_tensor(a, device="cuda")
    return t


def bucket(codes, n_mine, N, pos0, G, cap, sentinel=0):
    """mke_oc_bucket_codes -> (need [n_mine] uint32, send [G][cap][3], counts [G], the 64 ints behind the send buffer).  Every int of
    the send buffer and of the guard behind it starts as `sentinel`: what the launch did not write still holds it."""
    c = dev32(codes)
    need = torch.full((max(1, n_mine),), 0x55, dtype=torch.int32, device="cuda")
    send = torch.full((3 * G * cap + 64,), sentinel, dtype=torch.int32, device="cuda")
    counts = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(G * _lib.OC_BUCKET_WAVES, dtype=torch.int32, device="cuda")
    _lib.oc_bucket_codes(c, n_mine, N, pos0, G, cap, need, send, counts, scratch)
    torch.cuda.synchronize()
    s = send.cpu().numpy()
    return need.cpu().numpy()[:n_mine].view(np.uint32), s[:3 * G * cap].reshape(G, cap, 3), counts.cpu().numpy(), s[3 * G * cap:]


def owned_index(recv, counts, G, cap, n_all):
    """mke_oc_owned_index -> (own_rec device tensor, own_off device tensor [n_all + 1], n_owned)."""
    r = dev32(np.asarray(recv, dtype=np.int32).reshape(-1))
    cn = dev32(np.asarray(counts, dtype=np.int32))
    own_rec = torch.full((max(1, 3 * G * cap),), -1, dtype=torch.int32, device="cuda")
    own_off = torch.full((n_all + 1,), -1, dtype=torch.int32, device="cuda")
    _lib.oc_owned_index(r, cn, G, cap, n_all, own_rec, own_off)
    torch.cuda.synchronize()
    return own_rec, own_off, int(own_off[n_all])


def exchange(codes, n_all, N, G, rank, cap):
    """What rank `rank` of G receives for an epoch's codes by position: every home rank's share (contiguous ceil(n_all / G)
    positions) bucketed on the device, destination `rank`'s bucket of each -> (recv [G][cap][3], counts [G], need_all [n_all])."""
    n_per = -(-n_all // G) if n_all else 0
    recv = np.zeros((G, max(cap, 0), 3), dtype=np.int32)
    counts = np.zeros(G, dtype=np.int32)
    need_all = np.zeros(n_all, dtype=np.uint32)
    codes = np.asarray(codes, dtype=np.int64)
    for g in range(G):
        lo, hi = min(n_all, g * n_per), min(n_all, (g + 1) * n_per)
        need, send, cnt, _ = bucket(codes[lo * N:hi * N], hi - lo, N, lo, G, cap)
        recv[g], counts[g] = send[rank], cnt[rank]
        need_all[lo:hi] = need
    return recv, counts, need_all


PLAN_OUT = ("refs", "rows", "off", "row0", "item_row", "item_off", "item_part", "long_row", "long_part0", "steps3", "n_refs")


def em_plan(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, n_local, n_rel, capacity, chunks=1, own=None):
    """mke_oc_em_plan by hand (tests/test_oc_em_plan_gpu.py::_plan), `own` = (own_rec, own_off, own_cap) device tensors for the
    owned-list form (codes is then not passed at all)."""
    dev = "cuda"
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev) if len(a) else torch.zeros(1, dtype=torch.int32, device=dev)
    n_steps = len(step_lo) - 1
    n_all = len(ph)
    t = dict(ph=i32(ph), pr=i32(pr), pt=i32(pt), codes=dev32(codes), sh=i32(sh), st=i32(st),
             step_lo=torch.as_tensor(np.asarray(step_lo, dtype=np.int64), device=dev))
    z32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    z64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    b = dict(keys=z64(capacity + 1), keys_alt=z64(capacity + 1), flags=z32(capacity + 1), scan=z32(capacity + 1), vals_alt=z32(capacity + 1),
             scratch8=z64(capacity + 1), waves=z32(2 * (_lib.OC_EM_WAVES + 1)), refs=z32(2 * capacity), rows=z32(capacity), off=z32(capacity + 1),
             row0=z64(n_steps + 1), item_row=z32(capacity + 1), item_off=z32(capacity + 1), item_part=z32(capacity + 1),
             long_row=z32(capacity // 32 + 2), long_part0=z32(capacity // 32 + 2), steps3=z64(3 * (n_steps + 1)), n_refs=z64(1),
             temp=torch.zeros(_lib.oc_em_plan_temp_bytes(capacity), dtype=torch.uint8, device=dev))
    a = _lib.OcEmPlanArgs()
    p = lambda x: x.data_ptr()
    a.pos_h, a.pos_r, a.pos_t, a.neg_per_pos = p(t["ph"]), p(t["pr"]), p(t["pt"]), N
    a.codes = p(t["codes"]) if own is None else None
    a.slot_h, a.slot_t, a.step_lo, a.n_steps, a.chunks = p(t["sh"]), p(t["st"]), p(t["step_lo"]), n_steps, chunks
    a.n_all = n_all
    a.max_step = int(max([step_lo[k + 1] - step_lo[k] for k in range(n_steps)], default=0))
    a.n_ranks, a.rank, a.n_local, a.n_rel = G, rank, n_local, n_rel
    a.keys, a.keys_alt, a.capacity = p(b["keys"]), p(b["keys_alt"]), capacity
    a.vals_alt, a.scratch8, a.wave_scratch = p(b["vals_alt"]), p(b["scratch8"]), p(b["waves"])
    a.refs, a.rows, a.off, a.flags, a.scan = p(b["refs"]), p(b["rows"]), p(b["off"]), p(b["flags"]), p(b["scan"])
    a.step_row0, a.n_refs = p(b["row0"]), p(b["n_refs"])
    a.item_row, a.item_off, a.item_part = p(b["item_row"]), p(b["item_off"]), p(b["item_part"])
    a.long_row, a.long_part0 = p(b["long_row"]), p(b["long_part0"])
    s3 = b["steps3"]
    a.step_item0, a.step_long0, a.step_part0 = p(s3), p(s3) + 8 * (n_steps + 1), p(s3) + 16 * (n_steps + 1)
    a.temp, a.temp_bytes = p(b["temp"]), b["temp"].numel()
    if own is not None:
        a.own_rec, a.own_off, a.own_cap = p(own[0]), p(own[1]), int(own[2])
    _lib.oc_em_plan(a)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in b.items() if k in PLAN_OUT}
    out["steps3"] = out["steps3"].reshape(3, n_steps + 1)
    return out


def plan_valid(out):
    """The defined extent of every output of a plan (the tails behind them are scratch), as a dict of arrays."""
    n_refs = int(out["n_refs"][0])
    U = int(out["row0"][-1])
    items, longs = int(out["steps3"][0][-1]), int(out["steps3"][1][-1])
    return dict(n_refs=out["n_refs"], refs=out["refs"][:2 * n_refs], rows=out["rows"][:U], off=out["off"][:U + 1], row0=out["row0"],
                item_row=out["item_row"][:items], item_off=out["item_off"][:items + 1], item_part=out["item_part"][:items],
                long_row=out["long_row"][:longs], long_part0=out["long_part0"][:longs + 1], steps3=out["steps3"])


def expected(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, n_local):
    """{(step, row): [(locator, coefficient index), ...]} in element order, by the header's definition."""
    n_all = len(ph)
    step_of = np.searchsorted(np.asarray(step_lo), np.arange(n_all), side="right") - 1
    lists = {}

    def add(p, ent, row, loc, cidx):
        if ent < 0 or ent % G != rank:
            return
        lists.setdefault((int(step_of[p]), int(row)), []).append((loc & 0xFFFFFFFF, cidx))

    for p in range(n_all):                       # the negatives, in code order
        i = p - step_lo[step_of[p]]
        for n in range(N):
            c = int(codes[p * N + n])
            ent, rt = (c & 0x3FFFFFFF) >> 1, c & 1
            src = pt[p] if rt else ph[p]         # the vector that travels: RT from the tail's owner, HR from the head's
            slot = st[p] if rt else sh[p]
            add(p, ent, ent // G, ((src % G) << 24) | (rt << 23) | slot, i * (N + 1) + n)
    for p in range(n_all):                       # own term, head / tail gradient vectors, the relation row's two
        i = p - step_lo[step_of[p]]
        hr = sh[p] >= 0
        own = pt[p] if hr else ph[p]
        rt = 0 if hr else 1
        src = pt[p] if rt else ph[p]
        add(p, own, own // G, ((src % G) << 24) | (rt << 23) | (st[p] if rt else sh[p]), i * (N + 1) + N)
        if sh[p] >= 0:
            add(p, ph[p], ph[p] // G, GV | sh[p], 0)
        if st[p] >= 0:
            add(p, pt[p], pt[p] // G, GV | (1 << 23) | st[p], 0)
        if sh[p] >= 0:
            add(p, ph[p], n_local + pr[p], GV | PLUS | sh[p], 0)
        if st[p] >= 0:
            add(p, pt[p], n_local + pr[p], GV | PLUS | (1 << 23) | st[p], 0)
    return lists


def case(seed, G, rank, n_ent, n_rel, sizes, N, hub=False):
    """An epoch: positives, codes WITH the need flags in every group's first code (as mke_oc_pack_codes leaves them), slots."""
    rng = np.random.default_rng(seed)
    n_all = int(sum(sizes))
    step_lo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    draw = (lambda n: np.minimum(rng.zipf(1.3, n) - 1, n_ent - 1)) if hub else (lambda n: rng.integers(0, n_ent, n))
    ph, pt, pr = draw(n_all), draw(n_all), rng.integers(0, n_rel, n_all)
    side = rng.integers(0, 2, n_all)                                    # one coin per positive ...
    both = rng.random(n_all) < 0.1                                      # ... and a few that need both vectors
    codes = np.zeros(n_all * N, dtype=np.int64)
    for p in range(n_all):
        for n in range(N):
            s = side[p] if not both[p] else rng.integers(0, 2)
            codes[p * N + n] = (int(draw(1)[0]) << 1) | int(s)
    need_rt = np.array([any(codes[p * N:(p + 1) * N] & 1) for p in range(n_all)]) if N else np.zeros(n_all, bool)
    need_hr = ~need_rt | np.array([any((codes[p * N:(p + 1) * N] & 1) == 0) for p in range(n_all)]) if N else np.ones(n_all, bool)
    sh, st = np.full(n_all, -1), np.full(n_all, -1)
    for s in range(len(sizes)):                                         # slots: per step and owner, in position order
        cnt_h, cnt_t = np.zeros(G, int), np.zeros(G, int)
        for p in range(step_lo[s], step_lo[s + 1]):
            if need_hr[p]:
                sh[p] = cnt_h[ph[p] % G]; cnt_h[ph[p] % G] += 1
            if need_rt[p]:
                st[p] = cnt_t[pt[p] % G]; cnt_t[pt[p] % G] += 1
    if N:
        codes[::N] |= need_hr.astype(np.int64) * 0x40000000 + need_rt.astype(np.int64) * 0x80000000
    return ph, pr, pt, codes, sh, st, step_lo


def check_plan(out, want, n_steps):
    """Every output of the plan against the direct enumeration `want` (tests/test_oc_em_plan_gpu.py::_check_plan)."""
    n_refs = sum(len(v) for v in want.values())
    assert int(out["n_refs"][0]) == n_refs
    keys = sorted(want)
    steps = np.array([s for s, _ in keys], dtype=np.int64)
    np.testing.assert_array_equal(out["row0"], np.searchsorted(steps, np.arange(n_steps + 1)))
    np.testing.assert_array_equal(out["rows"][:len(keys)], [r for _, r in keys])
    refs = out["refs"].view(np.uint32).reshape(-1, 2)
    off = [0]
    for key in keys:
        off.append(off[-1] + len(want[key]))
    np.testing.assert_array_equal(out["off"][:len(keys) + 1], off)
    got = [(int(a), int(b)) for a, b in refs[:n_refs]]
    assert got == [ref for key in keys for ref in want[key]]
    item_row, item_off, item_part, long_row, long_part0 = [], [], [], [], []
    step_firsts = np.zeros((3, n_steps + 1), dtype=np.int64)
    part = 0
    for u, (s, row) in enumerate(keys):
        lo, hi = off[u], off[u + 1]
        nseg = -(-(hi - lo) // 32)
        if nseg > 1:
            long_row.append(row)
            long_part0.append(part)
        for k in range(nseg):
            gv = nseg > 1 or bool((refs[lo + 32 * k:min(hi, lo + 32 * k + 32), 0] & GV).any())
            item_row.append(row | (0x80000000 if nseg > 1 else 0) | (0x40000000 if gv else 0))
            item_off.append(lo + 32 * k)
            item_part.append(part + k if nseg > 1 else -1)
        part += nseg if nseg > 1 else 0
        step_firsts[:, s + 1:] = np.array([len(item_row), len(long_row), part])[:, None]
    long_part0.append(part)
    item_off.append(n_refs)
    n_items = len(item_row)
    np.testing.assert_array_equal(out["item_row"][:n_items].view(np.uint32), item_row)
    np.testing.assert_array_equal(out["item_off"][:n_items + 1], item_off)
    np.testing.assert_array_equal(out["item_part"][:n_items], item_part)
    np.testing.assert_array_equal(out["long_row"][:len(long_row)], long_row)
    np.testing.assert_array_equal(out["long_part0"][:len(long_part0)], long_part0)
    np.testing.assert_array_equal(out["steps3"], step_firsts)


def fake_step(peers=2, em=True, **over):
    """A step descriptor that passes every argument check, all addresses fake (tests/test_oc_peer_em_abi.py::_step): 2 ranks,
    stride 80, 8 positives.  A call that launched on it would not return an argument code."""
    FAKE = 0x10000
    s = _lib.OcStepStruct()
    for f in ("ent", "ent_acc", "ent_grad", "ent_touched", "rel", "rel_acc", "rel_grad", "rel_touched", "pos_h", "pos_r", "pos_t",
              "slot_h", "slot_t", "own_h", "own_t", "codes"):
        setattr(s, f, FAKE)
    s.n_local, s.n_rel, s.rel_grad_copies = 100, 5, 1
    s.stride, s.dim, s.rank, s.n_ranks = 80, 75, 0, 2
    s.n_pos, s.per, s.n_own_h, s.n_own_t, s.neg_per_pos, s.capacity = 8, 4, 3, 2, 4, 16
    s.optimizer, s.lr, s.scale, s.tag = _lib.OPT_ADAGRAD, 0.01, 1.0, 1
    s.n_peers = peers
    for g in range(peers):
        s.peer_v[g], s.peer_g[g] = FAKE, FAKE
    if em:
        s.em_coef, s.em_chunks, s.em_block_floats = FAKE, 1, 2 * 16 * 80
        s.em_refs = s.em_rows = s.em_off = FAKE
        s.em_v[0] = s.em_gv[0] = FAKE
    for k, v in over.items():
        setattr(s, k, v)
    return s


# ---- trainers -------------------------------------------------------------------------------------------------------------
N_REL, SEED = 20, 11


class SkewKGs:
    """Two KGs whose entity populations fall on different owners at two ranks: KG 1 holds the EVEN ids and nine tenths of the
    triples, KG 2 the odd ids — nine tenths of an epoch's corrupt entities belong to rank 0 of 2."""

    def __init__(self, n_ent=400, n_triples=3000, seed=SEED):
        rng = np.random.default_rng(seed)
        self._ents = [np.arange(0, n_ent, 2, dtype=np.int32), np.arange(1, n_ent, 2, dtype=np.int32)]
        self.triples = []
        for k, n in enumerate((n_triples * 9 // 10, n_triples - n_triples * 9 // 10)):
            e = self._ents[k]
            t = np.stack([rng.choice(e, n), rng.integers(k * (N_REL // 2), (k + 1) * (N_REL // 2), n), rng.choice(e, n)], 1)
            self.triples.append(np.unique(t, axis=0).astype(np.int32))

    def entities(self, k):
        return self._ents[k]


def make_trainer(rank, world, comm=None, chunks=1, n_ent=600, dim=75, neg=8, b=100, zipf=0.0, kgs=None, **kw):
    """The trainer of tests/test_distributed_oc_gpu.py::_make (same tables from the same seed), with the keyword arguments of the
    form under test passed through (`codes=`, `entity_major=`, `peer_direct=`, `tuning=`)."""
    from oracle import multike_oracle as mo
    from multike_amd.distributed_oc import OwnerComputesTrainer
    from multike_amd.synthetic import SyntheticKGs
    if kgs is None:
        kgs = SyntheticKGs(n_ent=n_ent, n_rel=N_REL, seed=SEED, zipf=zipf)
    rng = np.random.default_rng(SEED)
    ent0 = mo.xavier_truncated_normal((n_ent, dim), rng)
    rel0 = mo.xavier_truncated_normal((N_REL, dim), rng)
    return OwnerComputesTrainer(kgs, ent0, rel0, b, neg, rank, world, seed=SEED, lr=0.02, comm=comm, chunks=chunks, **kw)
