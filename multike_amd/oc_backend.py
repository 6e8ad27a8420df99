"""Compute side of the owner-computes step (multike_amd/distributed_oc.py): `OcStep`, what a backend sees of one part of a
global step, and `OcHipBackend`, the product backend — every phase is a HIP kernel of libmultike_hip.so (mke_oc.hip,
mke_oc_em.hip, mke_update.hip), launched through mke_oc_run (the phases of `phases`, an OC_* bit mask, of one part) or
mke_oc_steps (whole runs of steps, collectives included, enqueued from C++).

The backend protocol: `device_type`, `make_known`, `sample_at`, `block_elems`, `pack_codes` and `run` are required;
`plan`, `em_plan` (+ `em_temp_bytes`), `bucket_codes`, `owned_index`, `prepare_epoch` and `run_steps` are the HIP backend's own —
the trainer probes for them, and a backend without them (the tests' NumPy oracle) gets the torch plan (and the torch bucketing of
owner-bucketed codes), the atomics form and the Python loop.
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .sampling import KnownTripleSet, side_array

BASES, COUNT, SCORE, APPLY, UPDATE, PASS2 = _lib.OC_BASES, _lib.OC_COUNT, _lib.OC_SCORE, _lib.OC_APPLY, _lib.OC_UPDATE, _lib.OC_PASS2
GVSUM = _lib.OC_GVSUM


@dataclass
class OcStep:
    """One part of a global step as the backends see it (tensors on the trainer's device)."""
    pos_h: torch.Tensor
    pos_r: torch.Tensor
    pos_t: torch.Tensor
    per: int
    slot_h: torch.Tensor
    slot_t: torch.Tensor
    own_h: torch.Tensor
    own_t: torch.Tensor
    tag: int
    codes: torch.Tensor = None      # the epoch's negative codes of every rank, [world][codes_per_rank]
    code_off: tuple = ()            # per home rank: offset of its codes of this part inside `codes`
    pos_w: torch.Tensor = None      # per-positive weights of the part (weighted cross-KG loops), or None
    own_rec: torch.Tensor = None    # owner-bucketed codes: this rank's owned negatives of the epoch as (position, n, code) records ...
    own_off: torch.Tensor = None    # ... and the part's [n_pos + 1] offsets into them (None: the code scan)


class OcHipBackend:
    """Product backend: every compute step is a HIP kernel of libmultike_hip.so (mke_oc.hip, mke_oc_em.hip, mke_update.hip)."""

    device_type = "cuda"

    def __init__(self):
        # all filled by `prepare_epoch` (once per epoch, from the trainer's current plan)
        self._cache = {}            # buffer-set key -> (ctypes array of mke_oc_step, list of views of its elements)
        self._parts_arr = None      # the current epoch's array: mke_oc_steps walks it
        self._steps = []            # ... and the views `run` re-tags and launches
        self._ring, self._ring_stride = 0, 0
        self._step_part0 = None     # first part of every global step (ctypes array the loop descriptor points into)
        self._loop = None           # mke_oc_loop of the epoch

    def make_known(self, h, r, t):
        return KnownTripleSet(h, r, t)

    def sample_at(self, pos, pos_index, pos_kg, side1, side2, neg_per_pos, seed, stream_id, out):
        _lib.neg_sample_at(pos, pos_index, pos_kg, side_array(side1, side2), neg_per_pos, 10, seed, stream_id, out)

    def block_elems(self, capacity, stride):
        return _lib.oc_block_floats(capacity, stride)

    def pack_codes(self, pos_h, neg_h, neg_t, neg_per_pos, codes):
        _lib.oc_pack_codes(pos_h, neg_h, neg_t, neg_per_pos, codes)

    def plan(self, pos_h, pos_t, codes, neg_per_pos, part_lo, n_parts, n_ranks, rank, slot_h, slot_t, own_h, own_t, counts):
        """slots, owned lists and per-(part, owner) counts of the whole epoch in ONE launch (mke_oc_plan)."""
        _lib.oc_plan(pos_h, pos_t, codes, neg_per_pos, part_lo, n_parts, n_ranks, rank, slot_h, slot_t, own_h, own_t, counts)

    def bucket_codes(self, codes, n_mine, neg_per_pos, pos0, n_ranks, cap, need, send, counts, scratch):
        """mke_oc_bucket_codes: this rank's share of the codes bucketed by owner, (position, n) order per destination, true counts."""
        _lib.oc_bucket_codes(codes, n_mine, neg_per_pos, pos0, n_ranks, cap, need, send, counts, scratch)

    def owned_index(self, recv, counts, n_ranks, cap, n_all, own_rec, own_off):
        """mke_oc_owned_index: the received buckets packed into this rank's owned list, with its offsets per epoch position."""
        _lib.oc_owned_index(recv, counts, n_ranks, cap, n_all, own_rec, own_off)

    def em_plan(self, tr, ph, pr, pt, codes, slot, em, own=None):
        """mke_oc_em_plan: the epoch's references to this rank's rows sorted by (step, row, positive, kind), the touched rows of
        every global step and their CSR offsets (entity-major second pass) — one native call, nothing synchronises."""
        i32, i64 = torch.int32, torch.int64
        a = _lib.OcEmPlanArgs()
        a.pos_h, a.pos_r, a.pos_t = _lib.ptr(ph, i32, "pos"), _lib.ptr(pr, i32, "pos"), _lib.ptr(pt, i32, "pos")
        a.codes, a.neg_per_pos = _lib.ptr(codes, i32, "codes"), tr.N
        a.slot_h, a.slot_t = _lib.ptr(slot[0], i32, "slot"), _lib.ptr(slot[1], i32, "slot")
        a.step_lo, a.n_steps, a.chunks = _lib.ptr(tr._step_lo, i64, "step_lo"), tr.steps, tr.chunks
        a.n_all, a.max_step = tr._n_all, tr._max_step
        a.n_ranks, a.rank, a.n_local, a.n_rel = tr.world, tr.rank, max(1, tr.n_local), tr.rel.shape[0]
        a.keys, a.keys_alt, a.capacity = _lib.ptr(em.keys, i64, "keys"), _lib.ptr(em.keys_alt, i64, "keys"), em.capacity
        a.vals_alt, a.wave_scratch = _lib.ptr(em.vals_alt, i32, "vals_alt"), _lib.ptr(em.waves, i32, "waves")
        a.scratch8 = _lib.ptr(em.scratch8, i64, "scratch8")
        a.refs, a.rows, a.off = _lib.ptr(em.refs, i32, "refs"), _lib.ptr(em.rows, i32, "rows"), _lib.ptr(em.off, i32, "off")
        a.flags, a.scan = _lib.ptr(em.flags, i32, "flags"), _lib.ptr(em.scan, i32, "scan")
        a.step_row0, a.n_refs = _lib.ptr(em.step_row0, i64, "row0"), _lib.ptr(em.n_refs_dev, i64, "n_refs")
        a.item_row, a.item_off = _lib.ptr(em.item_row, i32, "item_row"), _lib.ptr(em.item_off, i32, "item_off")
        a.item_part = _lib.ptr(em.item_part, i32, "item_part")
        a.long_row, a.long_part0 = _lib.ptr(em.long_row, i32, "long_row"), _lib.ptr(em.long_part0, i32, "long_part0")
        a.step_item0, a.step_long0, a.step_part0 = (_lib.ptr(em.steps3[k], i64, "steps3") for k in range(3))
        a.temp, a.temp_bytes = _lib.ptr(em.temp, torch.uint8, "temp"), em.temp.numel()
        if own is not None:     # the negatives from this rank's owned list (own_rec, own_off, records own_rec has room for)
            a.own_rec, a.own_off, a.own_cap = _lib.ptr(own[0], i32, "own_rec"), _lib.ptr(own[1], i32, "own_off"), int(own[2])
        _lib.oc_em_plan(a)

    def em_temp_bytes(self, capacity):
        return _lib.oc_em_plan_temp_bytes(capacity)

    def _struct(self, tr: "OwnerComputesTrainer", st: OcStep):
        f32, i32 = torch.float32, torch.int32
        s = _lib.OcStepStruct()
        s.ent, s.ent_acc = _lib.ptr(tr.ent, f32, "ent"), _lib.ptr(tr.ent_acc, f32, "acc")
        s.ent_grad = _lib.ptr(tr.ent_grad, f32, "grad") if tr.ent_grad is not None else None      # entity-major: no entity scratch
        s.ent_touched = _lib.ptr(tr.ent_touched, i32, "touched") if tr.ent_touched is not None else None
        s.ref_count = _lib.ptr(tr.ref_count, i32, "ref_count") if tr.ref_count is not None else None
        s.n_local = max(1, tr.n_local)     # as in the plan (em_plan): pass 2 finds relation row r at n_local + r
        s.rel, s.rel_grad = _lib.ptr(tr.rel, f32, "rel"), _lib.ptr(tr.rel_grad, f32, "rel_grad")
        s.rel_grad_copies = 1 if tr.rel_grad.dim() == 2 else tr.rel_grad.shape[0]     # privatised relation gradient (all-reduced whole)
        s.rel_acc = _lib.ptr(tr.rel_acc, f32, "rel_acc")
        s.rel_touched, s.n_rel = _lib.ptr(tr.rel_touched, i32, "rel_touched"), tr.rel.shape[0]
        s.stride, s.dim, s.rank, s.n_ranks = tr.stride, tr.dim, tr.rank, tr.world
        s.pos_h, s.pos_r, s.pos_t = (_lib.ptr(x, i32, "pos") for x in (st.pos_h, st.pos_r, st.pos_t))
        s.n_pos, s.per = st.pos_h.numel(), st.per
        s.slot_h, s.slot_t = _lib.ptr(st.slot_h, i32, "slot"), _lib.ptr(st.slot_t, i32, "slot")
        s.own_h, s.n_own_h = _lib.ptr(st.own_h, i32, "own"), st.own_h.numel()
        s.own_t, s.n_own_t = _lib.ptr(st.own_t, i32, "own"), st.own_t.numel()
        s.neg_per_pos, s.capacity = tr.N, tr.C
        s.codes = _lib.ptr(st.codes, i32, "codes")
        for g, o in enumerate(st.code_off):
            s.code_off[g] = int(o)
        s.optimizer, s.lr, s.scale, s.tag = tr.OPTIMIZER, tr.lr, tr.scale, st.tag
        s.pos_w = _lib.ptr(st.pos_w, f32, "pos_w") if st.pos_w is not None else None
        if tr.hot_slot is not None:           # hub rows of the shard: private gradient copies behind the shard's own rows
            s.hot.slot, s.hot.n_hot = _lib.ptr(tr.hot_slot, i32, "hot_slot"), tr.n_hot
            s.hot.copies, s.hot.row0 = tr.HOT_COPIES, tr.ent_grad_rows
        s.tuning = _lib.tuning_ptr(tr.tuning)
        if st.own_off is not None:            # owner-bucketed codes: the part's offsets into this rank's owned list
            s.own_rec, s.own_off = _lib.ptr(st.own_rec, i32, "own_rec"), _lib.ptr(st.own_off, i32, "own_off")
        s.n_peers = 0
        # peer-mapped blocks (chunk 0: peer-direct runs unchunked); with the entity-major form `prepare_epoch` points em_v[0] /
        # em_gv[0] at the LOCAL mirror and summed block (`_addr`), never at a peer's memory
        if tr.peer_direct and tr.world > 1:
            gb = 2 * tr.C * tr.stride * 4
            s.n_peers = tr.world
            for g in range(tr.world):
                s.peer_v[g] = tr._peer_send[g].data_ptr()
                s.peer_g[g] = tr._peer_inbox[g].data_ptr() + tr.rank * gb
        return s

    def prepare_epoch(self, tr):
        """One mke_oc_step per part of the epoch, from raw device addresses (the epoch buffers are persistent: positives,
        slots, owned lists keep their addresses; only the owned-list offsets change from epoch to epoch) — no tensor
        slicing and no struct building on the step path."""
        i32 = torch.int32
        b = tr.bat
        if not tr._parts:
            self._steps = []
            return
        oh, ot = _lib.ptr(tr._own[0], i32, "own"), _lib.ptr(tr._own[1], i32, "own")
        em = tr._em if tr.em else None
        key = (tr.C, b.pos_h.data_ptr(), tr._slot[0].data_ptr(), tr._slot[1].data_ptr(), oh, ot, tr._codes.data_ptr(), len(tr._parts),
               tuple(t.data_ptr() for t in (*tr._peer_send, *tr._peer_inbox)) if tr.peer_direct and tr.world > 1 else 0,
               (em.refs.data_ptr(), em.item_row.data_ptr(), em.item_off.data_ptr(), tr._em_coef.data_ptr(),
                tr._em_partials.data_ptr(), tr._addr[0][1], tr._addr[0][3]) if em else 0,
               (tr._own_rec.data_ptr(), tr._own_off.data_ptr()) if tr._own_off is not None else 0)
        if key not in self._cache:                        # first use of this buffer set, or a buffer was re-allocated
            base = self._struct(tr, tr._build_part_step(0, 0))
            ph, pr, pt = (_lib.ptr(x, i32, "pos") for x in (b.pos_h, b.pos_r, b.pos_t))
            sh, stt = _lib.ptr(tr._slot[0], i32, "slot"), _lib.ptr(tr._slot[1], i32, "slot")
            pw = getattr(b, "pos_w", None)
            pw = _lib.ptr(pw, torch.float32, "pos_w") if pw is not None else None
            oo = _lib.ptr(tr._own_off, i32, "own_off") if tr._own_off is not None else None
            arr = (_lib.OcStepStruct * len(tr._parts))()     # contiguous: mke_oc_steps walks it (the list below holds views)
            out = []
            for k, (_, lo, hi) in enumerate(tr._parts):
                s = arr[k]
                C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
                s.pos_h, s.pos_r, s.pos_t = ph + 4 * lo, pr + 4 * lo, pt + 4 * lo
                s.slot_h, s.slot_t = sh + 4 * lo, stt + 4 * lo
                s.pos_w = (pw + 4 * lo) if pw is not None else None
                if oo is not None:                      # (own_rec came with `base`: the list's base for every part)
                    s.own_off = oo + 4 * lo
                s.n_pos = hi - lo
                s.per = max(1, -(-(hi - lo) // tr.world))
                for g in range(tr.world):
                    s.code_off[g] = (lo + g * int(s.per)) * tr.N      # codes are laid out by epoch position
                if em:      # entity-major: the step's coefficient buffer, this part's first positive in it, the chunks' vector blocks
                    step = tr._parts[k][0]
                    s.em_coef, s.em_pos0 = tr._em_coef.data_ptr(), lo - int(b.off[step])
                    s.em_refs = em.refs.data_ptr()
                    s.em_chunks, s.em_block_floats = len(tr._parts_of[step]), tr.block
                    for c in range(int(s.em_chunks)):
                        s.em_v[c], s.em_gv[c] = tr._addr[c][1], tr._addr[c][3]
                out.append(s)
            if len(self._cache) > 4:                      # buffers that grew leave dead keys behind: start over
                self._cache.clear()
            self._cache[key] = (arr, out)
        self._parts_arr, self._steps = self._cache[key]   # the two epoch buffer sets alternate: one table each
        self._ring, self._ring_stride = tr.loss_ring.data_ptr(), tr.loss_ring.shape[1] * 8
        cnth, cntt = (x.tolist() for x in tr._own_cnt)
        for k, (s, (_, lo, _hi)) in enumerate(zip(self._steps, tr._parts)):     # a part's owned list starts at the part's own offset
            s.own_h, s.n_own_h = oh + 4 * lo, cnth[k]
            s.own_t, s.n_own_t = ot + 4 * lo, cntt[k]
        if em:              # the work items / long rows of each global step: positions change from epoch to epoch
            i0, l0, p0 = em.item0.tolist(), em.long0.tolist(), em.part0.tolist()
            rp, op, pp = em.item_row.data_ptr(), em.item_off.data_ptr(), em.item_part.data_ptr()
            lr, lp = em.long_row.data_ptr(), em.long_part0.data_ptr()
            for s, (step, _, _) in zip(self._steps, tr._parts):
                s.em_rows, s.em_off, s.em_n_rows = rp + 4 * i0[step], op + 4 * i0[step], i0[step + 1] - i0[step]
                s.em_part = pp + 4 * i0[step]
                s.em_long_rows, s.em_long_part0, s.em_n_long = lr + 4 * l0[step], lp + 4 * l0[step], l0[step + 1] - l0[step]
                s.em_part0, s.em_partials = p0[step], tr._em_partials.data_ptr()
        # the whole epoch's schedule for mke_oc_steps (one native call per run of steps)
        lp = _lib.OcLoopStruct()
        lp.parts, lp.n_steps, lp.chunks = C.addressof(self._parts_arr), tr.steps, tr.chunks
        first = (C.c_int32 * (tr.steps + 1))()
        k = 0
        for st in range(tr.steps):
            first[st] = k
            k += len(tr._parts_of.get(st, ()))
        first[tr.steps] = k
        self._step_part0 = first
        lp.step_part0 = C.addressof(first)
        for c in range(tr.chunks):
            lp.send[c], lp.v_all[c], lp.g_all[c], lp.gv[c] = tr._addr[c]
        lp.block_floats = tr.block
        lp.loss_ring, lp.loss_stride = self._ring, tr.loss_ring.shape[1]
        self._loop = lp

    def run_steps(self, tr, s0, s1, tag_base, comm_struct, comm_stream, overlap_rs=False):
        """Global steps [s0, s1) of the current epoch in ONE native call (mke_oc_steps): kernels, collectives and — with several
        parts per step — the two-stream pipeline are enqueued from C++."""
        lp = self._loop
        lp.tag_base = tag_base
        lp.comm = C.addressof(comm_struct) if comm_struct is not None else None
        lp.comm_stream = comm_stream
        lp.overlap_rs = int(bool(overlap_rs))
        _lib.oc_steps(lp, s0, s1)

    def run(self, tr, k, tag, phases, c, loss_slot):
        """The phases of `phases` (OC_* bit mask) of part k (chunk buffers c) in ONE native call; buffers by raw address
        (validated when they were allocated)."""
        a = tr._addr[c]
        s = self._steps[k]
        s.tag = tag
        _lib.oc_run(s, phases, a[0], a[1], tr.block, a[2], a[3], self._ring + loss_slot * self._ring_stride)
