"""Entity-row sharded relation-view training, "owner computes" form (RCCL over xGMI on MI355X).

The reference has no multi-device code; this is new design.  One process per GPU.
  * entity table + its Adagrad slot are row-sharded by  id % world  (local row = id // world);
  * the relation table is replicated;
  * a global step is `world` x batch_size positives in the reference's epoch order; rank g is HOME of the g-th
    contiguous slice and samples its negatives (Philox stream indexed by the GLOBAL epoch position: the negatives of a
    positive do not depend on the world size);
  * rows never leave their owner.  A negative differs from its positive (h, r, t) in one entity c and its score needs only
    c's row and one of two vectors of the positive — HR_p = h^ + r^ (corrupted tail: d = HR_p - c^) or RT_p = r^ - t^
    (corrupted head: d = c^ + RT_p) — so the NEGATIVES go to the rows.  And the reference's sampler tosses ONE coin per round
    (code/base/batch.py:97-105): a positive's negatives almost always corrupt the same side, so only ONE of the two vectors
    travels for it (both for the few positives whose re-draw rounds fell on the other side); the positive's own term
    d = HR_p - t^ (or h^ + RT_p) is scored like a negative by the owner of t (of h).
Once per epoch (`EpochPlan`; prefetched on a side stream): every rank draws 1 / world of the epoch's negatives as (entity, side)
codes with the group's need flags, one all-gather of the codes, then every travelling vector's slot and — entity-major form — the
reference lists of this rank's rows (`EmPlan`).  Capacity is known exactly before the epoch starts: nothing overflows mid-epoch.
`codes="owner"` (MKE_OC_CODES=owner; entity-major form only, opt-in): the home rank buckets its codes by the OWNER of the corrupt
entity and the buckets are exchanged all-to-all instead — a rank receives only the negatives it owns, in (position, n) order
(`_bucket` / `_plan_gather` / `_owned_lists`), the reference lists are built from that list and the score launch walks it per positive
instead of scanning every code.  Same lists, same sums, bit for bit.
Per global step, ENTITY-MAJOR form (the default of the HIP backend):
    owner of h_p builds HR_p, owner of t_p builds RT_p — the needed ones                                          [BASES]
    ALL-GATHER of the blocks (~1 vector per positive)
    every rank scores, for ALL world x batch positives, the negatives (and positives' own terms) whose entity it owns: one
    coefficient per (positive, owned negative) stored, partial dL/dHR_p, dL/dRT_p written into the vector's slot  [SCORE]
    REDUCE-SCATTER of the gradient vectors (same layout): the owner of h_p / t_p receives the sum
    every touched owned row finished in place from its reference list, in list order (no scratch, no atomics: the step is
    bit-reproducible run to run); this rank's partial relation gradient stored                                    [PASS2]
    ALL-REDUCE of the relation gradient;  update of the relation table                                            [UPDATE]
The ATOMICS form (`entity_major=False` / MKE_OC_EM=0; what peer-direct takes unless asked otherwise, and the tests' NumPy backend): the bases launch also
counts the references of the own rows [COUNT], SCORE adds the corrupt rows' gradients to a scratch (in place when a row is referenced
once), the head / tail / relation rows' gradients follow the reduce-scatter [APPLY], UPDATE updates every touched shard and relation
row.  Either way a row is updated once per step from the sum of all its contributions (dense-Adagrad-equivalent).
Bytes per rank and step over the links: (G-1)/G * 2 * ~1 * P stride 4 against (G-1)/G * 2 * P (N + 2) stride 4 of a
row exchange — 27x less at N = 25 / dim 75, 66x less at N = 64 / dim 256 (DESIGN.md §5 has the latency model).

`chunks` > 1 splits the global step's positives into that many parts whose all-gather / reduce-scatter run on the
communicator's own stream while the previous / next part is scored (split-batch pipelining; the single second pass / update
at the end sees every part's gradients, so the result is the same function).

The compute steps go through a backend (multike_amd/oc_backend.py: `OcHipBackend`, the product; tests inject a CPU backend built
on the oracle to exercise this logic under `gloo`), the collectives through a communicator (multike_amd/oc_comm.py).  A run of
steps inside an epoch is ONE native call (`run` -> mke_oc_steps) when both allow it; `step` is the same schedule from Python.
"""
import math
import os
from dataclasses import dataclass
from enum import Enum

import numpy as np
import torch

from . import _lib
from .oc_backend import APPLY, BASES, COUNT, GVSUM, PASS2, SCORE, UPDATE, OcHipBackend, OcStep     # noqa: F401 — this module is the import surface
from .oc_comm import OcComm, OcGlooComm, OcHostStagedComm, OcRcclComm, default_comm         # noqa: F401
from .sampling import KGSide, RelationBatcher
from .tables import ADAGRAD_INIT_ACC, PLACEMENT_LOG, placed_rows


class TripleListBatcher:
    """Epoch source of the owner-computes trainer for the cross-KG inference loops (code/MultiKE_model.py:349-369, 393-414):
    `steps = ceil(len / B)` steps per epoch, each `random.sample(triples, B)` (B = len when there is one step) — distinct
    inside a step, steps independent.  Positives only (no negative sampler: `neg_per_pos` must be 0).  The draws are a
    function of (seed, epoch) alone, so every rank lays out the same epoch without exchanging a byte: on the GPU through
    `mke_sample_distinct` (the sampler of the single-GPU loops, multike_amd/MultiKE_model.py `_positives_epoch`), on the CPU
    (gloo tests) through NumPy's generator."""

    def __init__(self, triples, batch_size: int, device="cuda", seed: int = 0):
        arr = np.ascontiguousarray(np.asarray([t[:3] for t in triples], dtype=np.int32).reshape(-1, 3))
        self.device, self.seed, self.n = torch.device(device), int(seed), int(arr.shape[0])
        self.cols = tuple(torch.as_tensor(np.ascontiguousarray(arr[:, k]), device=self.device) for k in range(3))
        # 4-tuples (h, r, t, w): the weighted loops (code/MultiKE_model.py:393-414); drawn with their triples
        self.w_all = (torch.as_tensor(np.asarray([t[3] for t in triples], dtype=np.float32), device=self.device)
                      if self.n and len(triples[0]) > 3 else None)
        self.steps = int(math.ceil(self.n / batch_size)) if self.n else 0
        self.bs = int(batch_size) if self.steps > 1 else self.n
        self.off = np.arange(self.steps + 1, dtype=np.int64) * self.bs
        self.epoch, self._alt = 0, None
        self.pos_kg = self.side1 = self.side2 = None           # no negatives: nothing the sampler would need
        (self.pos_h, self.pos_r, self.pos_t), self.pos_w = self._draw(0)

    def _draw(self, epoch: int):
        """((h, r, t), w or None) of every step of `epoch`, in step order."""
        total = self.steps * self.bs
        if total == 0:
            z = torch.zeros(1, dtype=torch.int32, device=self.device)
            return (z, z.clone(), z.clone()), None
        if self.device.type == "cuda":
            idx = _lib.sample_distinct(self.n, self.bs, self.steps, (self.seed & 0xFFFFFFFF, 0x434B47), epoch + 1,
                                       device=self.device).reshape(-1).long()
        else:
            rng = np.random.default_rng([self.seed, epoch])
            idx = torch.as_tensor(np.concatenate([rng.choice(self.n, self.bs, replace=False) for _ in range(self.steps)]))
        return tuple(c[idx].contiguous() for c in self.cols), (self.w_all[idx].contiguous() if self.w_all is not None else None)

    def shuffle(self):
        """The next epoch's draws, into the SAME buffers (native step descriptors point into them)."""
        self.epoch += 1
        cols, w = self._draw(self.epoch)
        for dst, src in zip((self.pos_h, self.pos_r, self.pos_t), cols):
            dst.copy_(src)
        if w is not None:
            self.pos_w.copy_(w)

    def stage_next_epoch(self):
        new, self._w_next = self._draw(self.epoch + 1)
        if self._alt is None:
            self._alt = new
        else:
            for dst, src in zip(self._alt, new):
                dst.copy_(src)
        return self._alt

    def commit_staged(self):
        cur = (self.pos_h, self.pos_r, self.pos_t)
        self.pos_h, self.pos_r, self.pos_t = self._alt
        self._alt = cur
        if self.pos_w is not None:
            self.pos_w.copy_(self._w_next)   # one weight buffer: the staged epoch's weights arrive with the swap
        self.epoch += 1

    @property
    def rng_seed(self):
        return (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)

    @property
    def rng_stream(self):
        return (self.epoch * 2) & 0xFFFFFFFF


def hub_rows_of_shard(triples, n_ent: int, global_batch: int, rank: int, world: int, hot_min: float = 20.0, hot_max: int = 1024):
    """LOCAL rows (id // world) of this rank's entities that are head or tail of >= hot_min positives of an average global
    step, from the two KGs' relation triples (static degrees: an epoch is the same triples in a new order) — what a holder
    of an EmbeddingTable shard passes to `set_hot_rows` before it builds the trainers on it."""
    ids = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1, 3)[:, [0, 2]].reshape(-1) for t in triples])
    n = sum(len(t) for t in triples)
    steps = max(1, -(-n // max(1, int(global_batch))))
    deg = np.bincount(ids, minlength=n_ent) / steps
    hot = np.nonzero((deg >= hot_min) & (np.arange(n_ent) % world == rank))[0]
    if len(hot) > hot_max:
        hot = hot[np.argsort(-deg[hot])[:hot_max]]
    return np.sort(hot // world)



class PlanStage(Enum):
    SAMPLED = 1         # this rank's share of the codes is drawn; the all-gather has not been issued
    GATHERED = 2        # every rank's codes are (being) gathered; slots and lists not yet computed
    DONE = 3            # everything enqueued: `ready` marks the end


@dataclass(slots=True)           # an undeclared attribute cannot be added
class EmPlan:
    """Entity-major reference lists of one epoch (mke_oc_em_plan's buffers; all allocated by the trainer's `_persist`).  Sort
    scratch is shared by the two buffer sets, outputs are per set.  The host readbacks are set by `_finish_plan`."""
    capacity: int                   # references the lists have room for
    keys: torch.Tensor              # -- scratch
    keys_alt: torch.Tensor
    flags: torch.Tensor
    scan: torch.Tensor
    vals_alt: torch.Tensor
    scratch8: torch.Tensor
    waves: torch.Tensor
    temp: torch.Tensor
    refs: torch.Tensor              # -- outputs: (locator, coefficient index) per reference, in list order
    rows: torch.Tensor              # touched rows of every step, and their CSR offsets into `refs`
    off: torch.Tensor
    step_row0: torch.Tensor         # [steps + 1] first touched row of every step
    item_row: torch.Tensor          # work items of the second pass (rows, or 32-reference segments of long rows)
    item_off: torch.Tensor
    item_part: torch.Tensor
    long_row: torch.Tensor          # long rows and their first partial slot
    long_part0: torch.Tensor
    steps3: torch.Tensor            # [3][steps + 1] first work item / long row / partial slot of every step
    n_refs_dev: torch.Tensor        # [1] references this rank owns (may exceed `capacity`: the plan is then redone)
    host: torch.Tensor = None       # pinned copy of step_row0 | steps3 | n_refs_dev (asynchronous; read by `_finish_plan`)
    row0: torch.Tensor = None       # -- host readbacks, [steps + 1] each
    item0: torch.Tensor = None
    long0: torch.Tensor = None
    part0: torch.Tensor = None
    n_refs: int = None


@dataclass(slots=True)           # an undeclared attribute cannot be added
class EpochPlan:
    """The plan of one epoch order in buffer set `bs`, filled stage by stage (`_plan_sample` -> `_plan_gather` -> `_plan_rest`)."""
    bs: int
    pos: tuple                      # (h, r, t) of the epoch, in epoch order
    codes: torch.Tensor             # the epoch's negative codes in position order
    stage: PlanStage = PlanStage.SAMPLED
    codes_all: torch.Tensor = None  # G > 1: the all-gather's output (a view of `codes`) ...
    mine: torch.Tensor = None       # ... and this rank's share, its input
    slot: list = None               # [2] slot of every positive's HR / RT vector in its owner's block (-1: stays home)
    own: list = None                # [2] this rank's owned positives per part, in slot order
    cnt_host: torch.Tensor = None   # pinned [2][parts][G] vectors per (part, owner)
    em: EmPlan = None
    # -- owner-bucketed codes (`codes="owner"`): this rank's share of the codes, the buckets and what comes back
    mine_codes: torch.Tensor = None     # this rank's share [n_per][N] as packed (kept: an overflowing bucket is filled again)
    own_cap: int = 0                    # records per (source, destination) pair of the exchange
    need_mine: torch.Tensor = None      # [n_per] need flags of this rank's positions ...
    need_all: torch.Tensor = None       # ... and of every position after the all-gather ([G n_per]: mke_oc_plan reads it with N = 1)
    cnt_mine: torch.Tensor = None       # [G] records this rank addresses to every owner (true counts: may exceed own_cap) ...
    cnt_all: torch.Tensor = None        # ... and the whole [G][G] table (source, destination)
    send: torch.Tensor = None           # [G][own_cap] records
    recv: torch.Tensor = None
    own_rec: torch.Tensor = None        # this rank's owned negatives, packed, in (position, n) order
    own_off: torch.Tensor = None        # [n_all + 1] their offsets per epoch position
    own_cnt_host: torch.Tensor = None   # pinned copy of cnt_all (asynchronous; read by `_finish_plan`)
    sampled: object = None          # events (HIP device only): share drawn / codes gathered / all of it enqueued
    gathered: object = None
    ready: object = None


class OwnerComputesTrainer:
    # hub rows of the shard (mke_oc_step.hot): entities that are head or tail of >= HOT_MIN positives of an average GLOBAL step get
    # HOT_COPIES private copies of their gradient row for mke_oc_apply and the positives' own terms (the fused runner's rule,
    # multike_amd/runner.py; measured as rank 0 of 8 on Zipf(1.0) triples: EXPERIMENTS R5.12)
    HOT_MIN, HOT_MAX, HOT_COPIES = 20.0, 1024, 8
    REL_COPIES = 4
    SAMPLE_RUN = 1 << 26          # ids per column of the epoch sampler's scratch (the plan samples its share in runs of SAMPLE_RUN / N positions)

    def __init__(self, kgs, ent0: np.ndarray, rel0: np.ndarray, batch_size: int, neg_per_pos: int, rank: int, world: int,
                 seed: int = 0, lr: float = 0.001, backend=None, device=None, dtype=torch.float32, comm=None,
                 exclusive_rows: bool = True, chunks: int = 1, peer_direct: bool = False, prefetch: bool = True,
                 batcher=None, scale: float = 1.0, tables_of: "OwnerComputesTrainer" = None, ent_table=None, rel_table=None,
                 opt_name: str = "relation", n_ent: int = None, tag_base: int = None, global_batch: int = None,
                 entity_major: bool = None, tuning: dict = None, codes: str = None):
        """batcher: an epoch source other than the two KGs' shuffled triples (`TripleListBatcher`: the cross-KG inference
        loops — positives only, `neg_per_pos` 0, `kgs` unused and `batch_size` the GLOBAL step size the batcher was built
        with); scale: the loss factor (2 for code/MultiKE_model.py:349-369); tables_of: another trainer of the same
        (rank, world, device, dtype) whose entity shard and relation table this one trains too — the graphs of one view
        share their variables and have one optimizer each (code/MultiKE_model.py:17-31): shared tables and (zero-invariant)
        gradient / flag scratch, own Adagrad accumulators, own tag range; `ent0` / `rel0` are then unused.
        codes: "gather" (every rank receives every code of the epoch) or "owner" (bucketed by owner and exchanged all-to-all: a rank
        receives the negatives it owns — entity-major form only); None reads MKE_OC_CODES, default "gather"."""
        self.scale = float(scale)
        self.tuning = _lib.tuning(**tuning) if tuning else None     # this trainer's knobs (mke_oc_step.tuning), e.g. {"oc_score_quarter": 1}
        # ent_table / rel_table (multike_amd.tables.EmbeddingTable: this rank's shard of `n_ent` global rows, and the
        # replicated relation table): train THOSE — the trainer then shares them with whatever else holds them (other
        # trainers, the common-space step of multike_amd.distributed_views) and takes its Adagrad slot by `opt_name`.
        if ent_table is not None:
            if rel_table is None or n_ent is None:
                raise _lib.MultiKEHipError("ent_table needs rel_table and n_ent (the global row count)")
            ent0 = np.empty((int(n_ent), ent_table.dim), dtype=np.float32)          # shapes only
            rel0 = np.empty((rel_table.n_rows, rel_table.dim), dtype=np.float32)
        if tables_of is not None:
            ent0 = np.empty((tables_of.n_ent, tables_of.dim), dtype=np.float32)    # shapes only
            rel0 = np.empty((tables_of.rel.shape[0], tables_of.dim), dtype=np.float32)
        self.backend = backend or OcHipBackend()
        self.device = torch.device(device or ("cuda" if self.backend.device_type == "cuda" else "cpu"))
        # MKE_OC_FORCE_COLLECTIVES=1: a one-rank group takes the G > 1 step path — its three collectives issued for real on the
        # one-rank communicator — so that the host cost of that path can be measured on one GPU (bench.py --force-sharded
        # reports `host_us_per_step`)
        self.force_collectives = os.environ.get("MKE_OC_FORCE_COLLECTIVES", "0") == "1"
        if comm is None:
            comm = default_comm(self.device, world, self.force_collectives)
        self.comm = comm            # the steps' three collectives AND the epoch plan's one (`_plan_gather`)
        self.rank, self.world, self.lr = rank, world, float(lr)
        self.dim = ent0.shape[1]
        self.stride = _lib.stride_for(self.dim)
        self.N = int(neg_per_pos)
        if not 0 <= self.N <= 64:   # 0: positives only (the shape of the cross-KG inference loops, code/MultiKE_model.py:349-369)
            raise _lib.MultiKEHipError("the sharded relation view takes 0..64 negatives per positive")
        self.n_ent = ent0.shape[0]
        if self.n_ent >= 1 << 29:   # a code is (entity << 1) | side with the group's two need flags above it
            raise _lib.MultiKEHipError("the sharded relation view packs entity ids into 29 bits")
        self.batch_size = int(batch_size)
        self.chunks = max(1, int(chunks))
        self.prefetch = bool(prefetch)
        self.peer_direct = bool(peer_direct) and world > 1       # opt-in (`_step_peer_direct`); runs unchunked
        if self.peer_direct:
            self.chunks = 1
        # entity-major form (module docstring): the default of a backend that has the plan for it, float32 tables;
        # MKE_OC_EM=0 / entity_major=False select the atomics form.  Peer-direct keeps the atomics form unless the entity-major one
        # is asked for by name: entity_major=True, or MKE_SHARD_PEER_EM=1 where the caller left the choice open (`_step_peer_em`)
        em = entity_major
        if em is None:
            em = os.environ.get("MKE_OC_EM", "1") != "0"
            if self.peer_direct:
                em = em and os.environ.get("MKE_SHARD_PEER_EM", "0") == "1"
        self.em = bool(em) and hasattr(self.backend, "em_plan") and self.chunks <= _lib.OC_EM_MAX_CHUNKS and dtype == torch.float32
        if self.em:
            exclusive_rows = False
        form = codes if codes is not None else os.environ.get("MKE_OC_CODES", "gather")
        if form not in ("gather", "owner"):
            raise _lib.MultiKEHipError(f'codes / MKE_OC_CODES: "gather" or "owner", got {form!r}')
        if form == "owner" and not self.em:
            raise _lib.MultiKEHipError('codes="owner" (MKE_OC_CODES=owner) is built for the entity-major form only: entity_major=False / '
                                       'MKE_OC_EM=0 (the atomics form, and a backend without the entity-major plan) counts its references '
                                       'over the all-gathered codes — use codes="gather" with it')
        self.codes_form = form
        dev, st = self.device, self.stride
        i32 = dict(dtype=torch.int32, device=dev)
        # --- row-sharded entity state ---------------------------------------------------------------
        mine = np.arange(rank, self.n_ent, world)
        self.n_local = len(mine)
        if ent_table is not None:
            if ent_table.n_rows != max(1, self.n_local) or ent_table.stride != st or rel_table.stride != st:
                raise _lib.MultiKEHipError("ent_table: the shard must hold ceil-share rows of n_ent with the trainer's stride")
            self.ent, self.ent_grad, self.ent_touched = ent_table.data, ent_table.grad, ent_table.touched
            self.rel, self.rel_grad, self.rel_touched = rel_table.data, rel_table.grad, rel_table.touched
            self.ref_count = ent_table.refcount if exclusive_rows else None
        elif tables_of is not None:
            o = tables_of
            if (o.rank, o.world, o.device, o.ent.dtype) != (rank, world, dev, dtype):
                raise _lib.MultiKEHipError("tables_of: the two trainers must agree on rank / world / device / dtype")
            self.ent, self.ent_grad, self.ent_touched = o.ent, o.ent_grad, o.ent_touched
            self.rel, self.rel_grad, self.rel_touched = o.rel, o.rel_grad, o.rel_touched
            if exclusive_rows and o.ref_count is None:
                o.ref_count = torch.zeros(max(1, self.n_local), **i32)
            self.ref_count = o.ref_count if exclusive_rows else None
        else:
            place = dtype == torch.float32          # big float32 shards: on the fastest of a few candidate allocations (tables.placed_rows)
            mk = (lambda fill, with_=(): placed_rows(max(1, self.n_local), st, dev, fill, PLACEMENT_LOG, with_)) if place else \
                (lambda fill, with_=(): torch.full((max(1, self.n_local), st), fill, dtype=dtype, device=dev))
            self.ent = mk(0.0)
            self.ent[:self.n_local, :self.dim] = torch.as_tensor(ent0[mine], dtype=dtype, device=dev)
            self.ent_grad = None                    # allocated by _declare_hot_rows (with the hub rows' copies behind the shard's rows)
            self._mk_rows = mk
            self.ent_touched = None if self.em else torch.zeros(max(1, self.n_local), **i32)
            self.ref_count = torch.zeros(max(1, self.n_local), **i32) if exclusive_rows else None
            # --- replicated relation state ----------------------------------------------------------
            self.rel = torch.zeros(rel0.shape[0], st, dtype=dtype, device=dev)
            self.rel[:, :self.dim] = torch.as_tensor(rel0, dtype=dtype, device=dev)
            # relation gradient: mke_oc_apply adds one vector per owned slot to the relation's row, and relation frequencies are
            # heavy-tailed (relation ids ~ Zipf(1.0): apply 7.7 -> 23.2 us as rank 0 of 8, Zipf(1.5): 68 us).  Privatised REL_COPIES
            # ways (slot k adds to copy k % copies; the all-reduce carries the copies, the update sums them) while that stays
            # under 1 MB on the wire — beyond (2K relations x 256 floats) one copy: the all-reduce would cost more than it saves
            copies = 1
            if self.backend.device_type == "cuda" and dtype == torch.float32 and not self.em:    # entity-major: one writer per relation row
                copies = max(1, min(self.REL_COPIES, (1 << 20) // max(1, self.rel.numel() * 4)))
            self.rel_grad = torch.zeros_like(self.rel) if copies == 1 else torch.zeros((copies,) + tuple(self.rel.shape), dtype=dtype, device=dev)
            self.rel_touched = torch.zeros(rel0.shape[0], **i32)
        if ent_table is not None:
            self.ent_acc, self.rel_acc = ent_table.slot(opt_name), rel_table.slot(opt_name)
        else:
            self.ent_acc = placed_rows(self.ent.shape[0], st, dev, ADAGRAD_INIT_ACC, PLACEMENT_LOG, [self.ent]) if self.ent.dtype == torch.float32 \
                else torch.full_like(self.ent, ADAGRAD_INIT_ACC)           # per-optimizer slots (code/MultiKE_model.py:17)
            self.rel_acc = torch.full_like(self.rel, ADAGRAD_INIT_ACC)
        # --- global epoch order (identical on every rank: same seed) ----------------------------------
        if batcher is not None:
            if self.N != 0:
                raise _lib.MultiKEHipError("an explicit epoch source carries positives only: neg_per_pos must be 0")
            self.bat = batcher
        else:
            sides = []
            for k in (0, 1):
                # the sampler's membership filter: `kgs.known[k]` when the caller has one (the reference filters against
                # local_relation_triples_set, which also holds the swapped training-link triples: SURVEY 3.1), else the KG's own
                kt = getattr(kgs, "known", None)
                t = torch.as_tensor(np.asarray(kt[k] if kt is not None else kgs.triples[k], dtype=np.int32).reshape(-1, 3), device=dev)
                known = self.backend.make_known(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous())
                sides.append(KGSide(kgs.entities(k), known, device=dev))
            # a global step = `global_batch` positives when given (the reference's batch_size whatever the world size: every
            # rank is home of ceil(global / world) of them, the last of fewer), else batch_size per rank (weak scaling)
            self.bat = RelationBatcher(kgs.triples[0], kgs.triples[1], sides[0], sides[1],
                                       int(global_batch) if global_batch else batch_size * world, neg_per_pos,
                                       device=dev, seed=seed)
        self.steps = self.bat.steps
        self.ent_grad_full = None     # the gradient scratch with the hub rows' copies behind it, when this trainer allocated one
        self._declare_hot_rows(ent_table, tables_of)
        # trainers sharing the touched-flag arrays keep apart in tag space (a flag is `touched[row] == tag`)
        self._n_sharing = 0
        if tables_of is not None:
            tables_of._n_sharing += 1
        self.tag = 0 if tables_of is None else (tables_of._n_sharing << 26)
        if tag_base is not None:
            self.tag = int(tag_base)
        self.loss_ring = torch.zeros(max(1, self.steps) * self.chunks, _lib.LOSS_PARTIALS, dtype=torch.float64, device=dev)
        self.score_events = None  # set to a list to collect (start, end, triples) HIP events of the score kernel
        self._dtype = dtype
        self._persistent = {}         # epoch buffers by (name, buffer set): `_persist`
        self._layout()
        # -- the current epoch's plan (`_finish_plan`) --
        self.C, self.block = 0, 0     # capacity of an exchange block in vectors per owner / its size in elements
        self._send = self._v_all = self._g_all = self._gv = self._addr = None     # exchange buffers per chunk, and their addresses
        self._inbox = self._peer_send = self._peer_inbox = self._bar = None       # peer-direct (`_map_peers`)
        self._codes = self._slot = self._own = self._own_cnt = None
        self._own_rec = self._own_off = None     # owned code lists of the current epoch (`codes="owner"`), else None
        self._own_cap = 0             # records per (source, destination) pair of the code exchange (0: not sized yet)
        self.owner_replans = 0        # epochs whose buckets overflowed the capacity and were exchanged again
        self._code_bytes = 0          # code bytes this rank received for the current epoch's plan
        self.vectors_planned = 0
        self._plan_bs = 0             # which of the two epoch buffer sets the current plan lives in
        self._st_cache = {}           # OcStep per part, for backends that take tensors (`_part_step`)
        self._em = None               # EmPlan of the current epoch (entity-major form)
        self._em_capacity = {}        # buffer set -> capacity of its reference lists
        self._em_partials = self._em_coef = None
        # -- the next epoch's plan and the streams --
        self._next_plan = None        # EpochPlan being prefetched
        self._side = None             # the plans' side stream
        self._comm_stream = None      # the native loop's communication stream
        self._comm_native, self._comm_native_key = None, None     # mke_oc_comm of `comm`, per exchange-buffer generation
        self._plan_epoch()

    def _declare_hot_rows(self, ent_table, tables_of):
        """hot_slot (int32 [n_local]: index among this rank's hub rows or -1), n_hot, and the gradient scratch with the copies
        behind the shard's own rows.  Performance only: any row may or may not be declared (the arithmetic is the same sum)."""
        self.hot_slot, self.n_hot, self.ent_grad_rows = None, 0, max(1, self.n_local)
        if self.em:                                         # entity-major: no entity scratch at all, nothing to privatise
            if ent_table is None and tables_of is None:
                self.ent_grad_full = self.ent_grad = None
            return
        if tables_of is not None:                           # shared scratch: the declaration comes with it
            self.hot_slot, self.n_hot, self.HOT_COPIES = tables_of.hot_slot, tables_of.n_hot, tables_of.HOT_COPIES
            return
        if ent_table is not None:                           # an EmbeddingTable shard: whatever its holder declared
            if ent_table.n_hot:
                self.hot_slot, self.n_hot, self.HOT_COPIES = ent_table.hot_slot, ent_table.n_hot, ent_table.hot_copies
                self.ent_grad = ent_table.grad
            return
        b, G = self.bat, self.world
        n_all = int(b.off[-1]) if self.steps else 0
        if self.device.type == "cuda" and isinstance(self.backend, OcHipBackend) and n_all and self.ent.dtype == torch.float32:
            ids = torch.cat([b.pos_h[:n_all], b.pos_t[:n_all]]).long()
            deg = torch.bincount(ids, minlength=self.n_ent).float() / max(1, self.steps)      # references per global step
            hot = torch.nonzero(deg >= self.HOT_MIN).reshape(-1)
            hot = hot[hot % G == self.rank]
            if hot.numel() > self.HOT_MAX:
                hot = hot[torch.topk(deg[hot], self.HOT_MAX).indices]
            if hot.numel():
                slot = torch.full((max(1, self.n_local),), -1, dtype=torch.int32, device=self.device)
                slot[(hot // G)] = torch.arange(hot.numel(), dtype=torch.int32, device=self.device)
                self.hot_slot, self.n_hot = slot, int(hot.numel())
        rows = self.ent_grad_rows + self.HOT_COPIES * self.n_hot
        full = self._mk_rows(0.0, [self.ent, self.ent_acc]) if rows == self.ent.shape[0] else torch.zeros(rows, self.stride, dtype=self.ent.dtype, device=self.device)
        self.ent_grad_full, self.ent_grad = full, full[:self.ent.shape[0]]

    # ------------------------------------------------------------------------------------------------
    def parts_of_step(self, s: int):
        """[(lo, hi)] epoch-position ranges of the `chunks` parts of global step s (contiguous, ceil split; empty parts
        are dropped)."""
        lo, hi = int(self.bat.off[s]), int(self.bat.off[s + 1])
        if hi <= lo:
            return []
        size = int(math.ceil((hi - lo) / self.chunks))
        return [(a, min(hi, a + size)) for a in range(lo, hi, size)]

    def my_slice(self, lo: int, hi: int):
        """(per, a, e): positives per home rank in [lo, hi) and this rank's contiguous share [a, e)."""
        per = max(1, int(math.ceil((hi - lo) / self.world)))
        a = min(hi, lo + self.rank * per)
        return per, a, min(hi, a + per)

    def _layout(self):
        """What depends only on the sizes of the epoch (fixed across epochs: a shuffle permutes contents, not the step /
        part / slice boundaries): parts, every rank's slice of every part, this rank's epoch positions, part ids.  Once, at construction."""
        b, G, dev = self.bat, self.world, self.device
        parts = [(s, lo, hi) for s in range(self.steps) for (lo, hi) in self.parts_of_step(s)]
        self._parts = parts
        self._n_all = int(b.off[-1]) if self.steps else 0
        lo = np.array([p[1] for p in parts], dtype=np.int64)
        hi = np.array([p[2] for p in parts], dtype=np.int64)
        per = np.maximum(1, -(-(hi - lo) // G))
        self._all_idx = torch.arange(self._n_all, dtype=torch.int32, device=dev)
        self._part_id = torch.repeat_interleave(torch.arange(len(parts), device=dev), torch.as_tensor(hi - lo, device=dev)) \
            if len(parts) else torch.zeros(0, dtype=torch.int64, device=dev)
        self._lo_of = torch.as_tensor(lo, device=dev)
        self._part_lo = torch.as_tensor(np.concatenate([lo, [self._n_all]]).astype(np.int64), device=dev)   # [parts + 1]
        self._parts_of = {}
        for k, (ps, _, _) in enumerate(parts):
            self._parts_of.setdefault(ps, []).append(k)
        off = np.asarray(b.off[:self.steps + 1], dtype=np.int64) if self.steps else np.zeros(1, dtype=np.int64)
        self._step_lo = torch.as_tensor(off, device=dev)                       # [steps + 1] epoch positions of the global steps
        self._max_step = int((off[1:] - off[:-1]).max()) if self.steps else 0

    # ---- per-epoch plan: table-independent, so the NEXT epoch's is computed on a side stream while this epoch trains -----
    def _compute_plan(self, pos, rng_stream, bs):
        """The whole plan of an epoch order in line on the current stream: this rank's share of the negatives as codes, the
        all-gather of the codes ON THE STEP COMMUNICATOR, the slots and reference lists."""
        plan = self._plan_sample(pos, rng_stream, bs)
        self._plan_gather(plan)
        return self._plan_rest(plan)

    def _plan_gather(self, plan):
        """The ONE collective of an epoch plan: every rank's 1 / G of the epoch's negative codes, all-gathered on the step
        communicator, on the stream the steps run on, at a fixed point of the step sequence (`_gather_at`) — so the ranks issue
        every collective of the job in one order."""
        if plan.send is not None:
            # owner-bucketed codes: three collectives at the same point — the positions' need flags (all-gather), every rank's counts
            # per destination (all-gather: every rank holds the whole table and takes the same overflow decision), the buckets
            # (equal-split all-to-all).  One rank without forced collectives: its one bucket is what it would receive.
            if self.world > 1 or self.force_collectives:
                if plan.sampled is not None:
                    torch.cuda.current_stream().wait_event(plan.sampled)
                self.comm.all_gather(plan.need_all, plan.need_mine)
                self.comm.all_gather(plan.cnt_all, plan.cnt_mine)
                self.comm.all_to_all(plan.recv, plan.send)
                if self.device.type == "cuda":
                    plan.gathered = torch.cuda.Event()
                    plan.gathered.record()
        elif plan.mine is not None and (self.world > 1 or self.force_collectives):
            if plan.sampled is not None:
                torch.cuda.current_stream().wait_event(plan.sampled)
            self.comm.all_gather(plan.codes_all, plan.mine)
            if self.device.type == "cuda":
                plan.gathered = torch.cuda.Event()
                plan.gathered.record()
        plan.stage = PlanStage.GATHERED

    def _bucket(self, plan):
        """Owner form, after the share is packed (device work only): this rank's codes as records bucketed by owner, `own_cap` per
        destination, with the true counts; the need flags of its positions on their own."""
        G, dev, N = self.world, self.device, self.N
        i32 = dict(dtype=torch.int32, device=dev)
        z = torch.zeros(0, **i32)
        n_all = self._n_all
        n_per = -(-n_all // G)
        lo_r, hi_r = min(n_all, self.rank * n_per), min(n_all, (self.rank + 1) * n_per)
        cap = self._own_cap
        if not cap:
            # a rank's share spread over G owners + 6 % + 4,096 (the rule of the reference lists' capacity): the all-to-all moves
            # the CAPACITY, so slack is bytes on the wire every epoch; a pair that holds more is exchanged again at the exact maximum
            cap = self._own_cap = n_per * N if G == 1 else int(1.06 * n_per * N / G) + 4096
        R = _lib.OC_REC_INTS
        plan.own_cap = cap
        plan.need_mine = self._persist(("own_need_mine", plan.bs), z, n_per)[:n_per]
        plan.cnt_mine = self._persist(("own_cnt_mine", plan.bs), z, G)[:G]
        plan.send = self._persist(("own_send",), z, R * G * cap)[:R * G * cap]
        split = G > 1 or self.force_collectives
        plan.need_all = self._persist(("own_need", plan.bs), z, G * n_per)[:G * n_per] if split else plan.need_mine
        plan.cnt_all = self._persist(("own_cnt", plan.bs), z, G * G)[:G * G] if split else plan.cnt_mine
        plan.recv = self._persist(("own_recv",), z, R * G * cap)[:R * G * cap] if split else plan.send
        if hasattr(self.backend, "bucket_codes"):
            self.backend.bucket_codes(plan.mine_codes, hi_r - lo_r, N, lo_r, G, cap, plan.need_mine, plan.send, plan.cnt_mine,
                                      self._persist(("own_scratch",), z, G * _lib.OC_BUCKET_WAVES))
        else:       # the tests' CPU backend: the same stable partition in torch
            c = plan.mine_codes[:(hi_r - lo_r) * N]
            code = c & _lib.OC_CODE_MASK
            dest = (code >> 1) % G
            order = torch.argsort(dest, stable=True)
            cnt = torch.bincount(dest, minlength=G)
            start = torch.cumsum(cnt, 0) - cnt
            k = torch.arange(order.numel(), device=dev) - start[dest[order]]
            keep = k < cap
            o, d, k = order[keep], dest[order][keep].long(), k[keep]
            send = plan.send.view(G, cap, R)
            send[d, k, 0] = (lo_r + o // N).to(torch.int32)
            send[d, k, 1] = (o % N).to(torch.int32)
            send[d, k, 2] = code[o]
            plan.cnt_mine.copy_(cnt.to(torch.int32))
            if hi_r > lo_r:
                plan.need_mine[:hi_r - lo_r].copy_(c.view(hi_r - lo_r, N)[:, 0] & -0x40000000)

    def _owned_lists(self, plan):
        """Owner form, after the exchange (device work only): the received buckets packed into this rank's owned list with its
        offsets per epoch position; the counts table on its way to pinned memory."""
        G, dev = self.world, self.device
        i32 = dict(dtype=torch.int32, device=dev)
        z = torch.zeros(0, **i32)
        R, cap, n_all = _lib.OC_REC_INTS, plan.own_cap, self._n_all
        plan.own_rec = self._persist(("own_rec", plan.bs), z, R * G * cap)
        plan.own_off = self._persist(("own_off", plan.bs), z, n_all + 1)
        col = plan.cnt_all.view(-1, G)[:, self.rank].contiguous()         # what every source addressed to this rank
        if hasattr(self.backend, "owned_index"):
            self.backend.owned_index(plan.recv, col, G, cap, n_all, plan.own_rec, plan.own_off)
        else:
            got = col.clamp(max=cap).tolist()
            recs = torch.cat([plan.recv.view(G, cap, R)[s, :got[s]] for s in range(G)]) if cap else plan.recv.view(0, R)
            plan.own_rec[:recs.numel()].copy_(recs.reshape(-1))
            plan.own_off[:n_all + 1].copy_(torch.searchsorted(recs[:, 0].contiguous(), torch.arange(n_all + 1, **i32)).to(torch.int32))
        host = self._persistent.get(("own_cnt_host", plan.bs))
        if host is None or host.numel() != plan.cnt_all.numel():
            host = self._persistent[("own_cnt_host", plan.bs)] = torch.empty(plan.cnt_all.numel(), dtype=torch.int32, pin_memory=dev.type == "cuda")
        host.copy_(plan.cnt_all, non_blocking=True)
        plan.own_cnt_host = host

    def _plan_sample(self, pos, rng_stream, bs):
        """First stage of a plan, into buffer set `bs` (device work only, no host synchronisation): this rank draws the negatives
        of ITS contiguous 1 / G of the epoch positions (the Philox stream is a function of the epoch position, so who draws a
        positive's negatives does not matter) and packs them as codes; `_plan_gather` then gives every rank the whole epoch's
        codes in position order.  (Rounds 2-4: every rank drew all of them — 63 us per step of rank compute at the C5 shape
        with 8 ranks.)"""
        b, G, dev, N = self.bat, self.world, self.device, self.N
        i32 = dict(dtype=torch.int32, device=dev)
        ph, pr, pt = pos
        n_all = self._n_all
        n_per = -(-n_all // G) if n_all else 0            # positions per rank (the last rank's share may be shorter)
        owner = self.codes_form == "owner" and n_all > 0 and N > 0
        # (owner form on several ranks: nobody holds the whole epoch's codes)
        codes = self._persist(("codes", bs), torch.zeros(0, **i32), 1 if owner and G > 1 else max(1, G * n_per * N))
        plan = EpochPlan(bs, pos, codes)
        if n_all and N:
            lo_r, hi_r = min(n_all, self.rank * n_per), min(n_all, (self.rank + 1) * n_per)
            mine = codes[self.rank * n_per * N:(self.rank + 1) * n_per * N] if G == 1 else \
                self._persist(("codes_mine", bs), torch.zeros(0, **i32), n_per * N)[:n_per * N]
            if hi_r > lo_r:
                # scratch of the sampler's (h, r, t) output: kept across epochs (a fresh allocation per epoch was tens of ms of
                # hipMalloc inside the plan) and BOUNDED — the share is sampled in runs of at most 2^26 / N positions (256 MB per
                # column; the whole share at once was 2.4 GB per column at the C5 shape on one rank: round-4 advice); one plan at a
                # time writes it (plans are computed in epoch order on one stream)
                run = max(1, self.SAMPLE_RUN // N)
                neg = tuple(self._persist(("neg", k_), torch.zeros(0, **i32), min(n_per, run) * N) for k_ in range(3))
                for a in range(lo_r, hi_r, run):
                    e = min(hi_r, a + run)
                    out = tuple(x[:(e - a) * N] for x in neg)
                    self.backend.sample_at((ph[a:e], pr[a:e], pt[a:e]), self._all_idx[a:e], b.pos_kg[a:e],
                                           b.side1, b.side2, N, b.rng_seed, rng_stream, out)
                    self.backend.pack_codes(ph[a:e], out[0], out[2], N, mine[(a - lo_r) * N:(e - lo_r) * N])
            if owner:
                plan.mine_codes = mine
                self._bucket(plan)
            elif G > 1 or self.force_collectives:      # (forced at one rank: an in-place all-gather of the whole array)
                plan.codes_all, plan.mine = codes[:G * n_per * N], mine[:n_per * N]
        if dev.type == "cuda":
            plan.sampled = torch.cuda.Event()
            plan.sampled.record()
        return plan

    def _plan_rest(self, plan):
        """What follows the codes' all-gather (device work only): slots, owned lists, counts, the entity-major reference lists."""
        b, G, dev, N = self.bat, self.world, self.device, self.N
        i32 = dict(dtype=torch.int32, device=dev)
        ph, pr, pt = plan.pos
        bs, codes = plan.bs, plan.codes
        n_all, parts, part_id = self._n_all, self._parts, self._part_id
        if plan.gathered is not None:
            torch.cuda.current_stream().wait_event(plan.gathered)
        # slot of every positive's HR / RT vector in its owner's block (rank among the positives of its part that NEED that
        # vector — the group flags in the first code of every positive — and have the same owner, epoch order; -1 when not
        # needed), this rank's owned positives per part in slot order (part k's list starts at own[lo_k]), and the
        # per-(part, owner) counts.  HIP backend: one launch (mke_oc_plan); other backends (the CPU tests): torch.
        slot = [self._persist(("slot", x, bs), torch.zeros(0, **i32), max(1, n_all)) for x in range(2)]
        own = [self._persist(("own", x, bs), torch.zeros(0, **i32), max(1, n_all)) for x in range(2)]
        plan.slot, plan.own = slot, own
        owner = plan.send is not None
        if owner:
            self._owned_lists(plan)
        if n_all:
            cnt = self._persist(("cnt", bs), torch.zeros(0, **i32), 2 * len(parts) * G)
            if hasattr(self.backend, "plan"):
                # (owner form: the all-gathered need flags are the layout the launch reads with one code per position)
                self.backend.plan(ph, pt, plan.need_all if owner else codes, 1 if owner else N, self._part_lo, len(parts), G, self.rank,
                                  slot[0], slot[1], own[0], own[1], cnt)
            else:
                if N:
                    first = (plan.need_all[:n_all] if owner else codes[:n_all * N].view(n_all, N)[:, 0]).long() & 0xFFFFFFFF
                    needs = ((first & _lib.OC_NEED_HR) != 0, (first & _lib.OC_NEED_RT) != 0)
                else:
                    needs = (torch.ones(n_all, dtype=torch.bool, device=dev), torch.zeros(n_all, dtype=torch.bool, device=dev))
                for x, ids in enumerate((ph, pt)):
                    owner = torch.where(needs[x], ids[:n_all].long() % G, G)        # bucket G: the vector does not travel
                    key = part_id * (G + 1) + owner
                    order = torch.argsort(key, stable=True)
                    ks = key[order]
                    counts = torch.bincount(ks, minlength=len(parts) * (G + 1))
                    start = torch.cumsum(counts, 0) - counts
                    sl = torch.empty(n_all, dtype=torch.int64, device=dev)
                    sl[order] = torch.arange(n_all, device=dev) - start[ks]
                    slot[x][:n_all].copy_(torch.where(needs[x], sl, -1).to(torch.int32))
                    mine = torch.nonzero(owner == self.rank).reshape(-1)
                    lo_m = self._lo_of[part_id[mine]]
                    own[x][(lo_m + sl[mine])] = (mine - lo_m).to(torch.int32)
                    cnt[x * len(parts) * G:(x + 1) * len(parts) * G].copy_(counts.view(len(parts), G + 1)[:, :G].reshape(-1).to(torch.int32))
            c = cnt[:2 * len(parts) * G].view(2, len(parts), G)
            host = self._persistent.get(("cnt_host", bs))
            if host is None or host.shape != c.shape:
                host = torch.empty(c.shape, dtype=torch.int32, pin_memory=dev.type == "cuda")
                self._persistent[("cnt_host", bs)] = host
            host.copy_(c, non_blocking=True)
            plan.cnt_host = host
        if self.em:
            plan.em = self._compute_em_plan(ph, pr, pt, codes, slot, bs, own=self._own_of(plan))
        if dev.type == "cuda":
            plan.ready = torch.cuda.Event()
            plan.ready.record()
        plan.stage = PlanStage.DONE
        return plan

    def _em_buffers(self, bs, capacity):
        """Scratch (shared by the two buffer sets: plans are computed one at a time on one stream) and outputs (per buffer set)
        of the entity-major plan at `capacity` references."""
        dev = self.device
        z32, z64 = (torch.zeros(0, dtype=t, device=dev) for t in (torch.int32, torch.int64))
        p = self._persist
        S1 = self.steps + 1
        return EmPlan(
            capacity=capacity,
            keys=p(("em_keys",), z64, capacity + 1), keys_alt=p(("em_keys_alt",), z64, capacity + 1),
            flags=p(("em_flags",), z32, capacity + 1), scan=p(("em_scan",), z32, capacity + 1),
            vals_alt=p(("em_vals_alt",), z32, capacity + 1), scratch8=p(("em_scratch8",), z64, capacity + 1),
            waves=p(("em_waves",), z32, 2 * (_lib.OC_EM_WAVES + 1)),
            temp=p(("em_temp",), torch.zeros(0, dtype=torch.uint8, device=dev), self.backend.em_temp_bytes(capacity)),
            refs=p(("em_refs", bs), z32, 2 * capacity), rows=p(("em_rows", bs), z32, capacity), off=p(("em_off", bs), z32, capacity + 1),
            step_row0=p(("em_row0", bs), z64, S1),
            item_row=p(("em_item_row", bs), z32, capacity + 1), item_off=p(("em_item_off", bs), z32, capacity + 1),
            item_part=p(("em_item_part", bs), z32, capacity + 1),
            long_row=p(("em_long_row", bs), z32, capacity // 32 + 2), long_part0=p(("em_long_part0", bs), z32, capacity // 32 + 2),
            steps3=p(("em_steps3", bs), z64, 3 * S1).view(-1)[:3 * S1].view(3, S1),
            n_refs_dev=p(("em_n_refs", bs), z64, 1))

    @staticmethod
    def _own_of(plan):
        """(own_rec, own_off, records own_rec has room for) of a plan with owner-bucketed codes, else None."""
        return (plan.own_rec, plan.own_off, plan.own_rec.numel() // _lib.OC_REC_INTS) if plan.own_off is not None else None

    def _compute_em_plan(self, ph, pr, pt, codes, slot, bs, capacity=None, own=None):
        """The entity-major reference lists of the epoch in buffer set `bs` (device work only; the touched-row offsets of the
        steps and the reference count go to pinned host memory asynchronously, read by `_finish_plan`).  own: the negatives from
        this rank's owned list (`_own_of`) instead of the all-gathered codes."""
        G, N = self.world, self.N
        upper = max(1, self._n_all * (N + 5))                          # every element of every positive
        if capacity is None:
            capacity = self._em_capacity.get(bs, 0)
            if not capacity:
                # 1 / G of the epoch's references + 6 % + 4,096: the sort, the gather and the row walks run over the CAPACITY (the unused
                # tail is sentinels), so slack is paid every epoch — uniform corruptions put a rank within 0.1 % of its share, hub
                # entities move only the five non-negative elements of a position; a rank that owns more re-plans once at the exact size
                capacity = upper if G == 1 else min(upper, int(1.06 * self._n_all * (N + 3) / G) + 4096)
        self._em_capacity[bs] = capacity
        em = self._em_buffers(bs, capacity)
        if own is None:
            self.backend.em_plan(self, ph, pr, pt, codes, slot, em)
        else:
            self.backend.em_plan(self, ph, pr, pt, codes, slot, em, own=own)
        S1 = self.steps + 1
        host = self._persistent.get(("em_host", bs))
        if host is None or host.numel() != 4 * S1 + 1:
            host = self._persistent[("em_host", bs)] = torch.empty(4 * S1 + 1, dtype=torch.int64, pin_memory=self.device.type == "cuda")
        host[:S1].copy_(em.step_row0[:S1], non_blocking=True)
        host[S1:4 * S1].copy_(em.steps3.reshape(-1), non_blocking=True)
        host[4 * S1:].copy_(em.n_refs_dev[:1], non_blocking=True)
        em.host = host
        return em

    def _finish_plan(self, plan):
        """Make a computed plan the current one: wait for its counts (the only host synchronisation of an epoch), size the
        exchange blocks exactly, rebuild the native step descriptors."""
        G, dev = self.world, self.device
        if plan.ready is not None:
            plan.ready.synchronize()
        if plan.send is not None:
            # owner-bucketed codes: every rank holds the same [G][G] table of true counts.  A pair beyond the capacity: every rank
            # buckets, exchanges and plans again, in line, with room for the largest (the rule of the reference lists' regrow below)
            most = int(plan.own_cnt_host.max())
            if most > plan.own_cap:
                self._own_cap = most
                self.owner_replans += 1
                plan.sampled = plan.gathered = None          # everything below is on the current stream
                self._bucket(plan)
                self._plan_gather(plan)
                self._plan_rest(plan)
                if plan.ready is not None:
                    plan.ready.synchronize()
            self._own_rec, self._own_off = plan.own_rec, plan.own_off
            G, n_per = self.world, -(-self._n_all // self.world)
            split = G > 1 or self.force_collectives
            self._code_bytes = (4 * _lib.OC_REC_INTS * G * plan.own_cap + 4 * G * n_per + 4 * G * G) if split else 0
        else:
            self._own_rec = self._own_off = None
            n_per = -(-self._n_all // self.world) if self._n_all else 0
            self._code_bytes = 4 * self.world * n_per * self.N if plan.mine is not None else 0
        parts = self._parts
        self._codes, self._slot, self._own = plan.codes, plan.slot, plan.own
        self._own_cnt = []                      # per part: how many HR / RT vectors of it this rank owns
        worst = 0
        self.vectors_planned = 0                # HR + RT vectors that travel in this epoch (all owners): ~1 per positive
        for x in range(2):
            mine = np.zeros(len(parts), dtype=np.int64)
            if self._n_all:
                cnt = plan.cnt_host[x].numpy().reshape(len(parts), G)
                worst = max(worst, int(cnt.max()))
                self.vectors_planned += int(cnt.sum())
                mine = cnt[:, self.rank].astype(np.int64)
            self._own_cnt.append(mine)
        # -- capacity: exact for this epoch, buffers only ever grow ----------------------------------------
        need = max(worst, 1)
        if need > self.C:
            self.C = int(need * 1.05) + 16
            self.block = int(self.backend.block_elems(self.C, self.stride))
            gb = 2 * self.C * self.stride
            mk = lambda n: torch.zeros(n, dtype=self._dtype, device=dev)
            self._send = [mk(self.block) for _ in range(self.chunks)]
            self._v_all = [self._send[c] if G == 1 else mk(G * self.block) for c in range(self.chunks)]
            self._g_all = [mk(G * gb) for _ in range(self.chunks)]
            self._gv = [self._g_all[c] if G == 1 else mk(gb) for c in range(self.chunks)]
            if self.peer_direct:
                self._map_peers(gb)
            self._addr = [tuple(t.data_ptr() for t in (self._send[c], self._v_all[c], self._g_all[c], self._gv[c]))
                          for c in range(self.chunks)]
        if self.em:
            em = plan.em
            S1 = self.steps + 1
            n_refs = int(em.host[4 * S1])
            if n_refs > em.capacity:        # more references than the 1 / G estimate allowed for (skewed ownership): re-plan in line, exactly
                em = plan.em = self._compute_em_plan(*plan.pos, plan.codes, plan.slot, plan.bs, capacity=int(n_refs * 1.1) + 4096,
                                                     own=self._own_of(plan))
                if dev.type == "cuda":
                    torch.cuda.current_stream().synchronize()
                n_refs = int(em.host[4 * S1])
            em.row0, em.item0, em.long0, em.part0 = (em.host[k * S1:(k + 1) * S1].clone() for k in range(4))
            em.n_refs = n_refs
            # the long rows' partial sums of ONE step (stride + 16 floats per slot: the gradient vector and the coefficient sum)
            need_parts = int((em.part0[1:] - em.part0[:-1]).max()) if self.steps else 0
            need_parts = max(1, need_parts) * (self.stride + 16)
            if self._em_partials is None or self._em_partials.numel() < need_parts:
                self._em_partials = torch.zeros(need_parts, dtype=torch.float32, device=dev)
            self._em = em
            need_coef = max(1, self._max_step * (self.N + 1))
            if self._em_coef is None or self._em_coef.numel() < need_coef:
                self._em_coef = torch.zeros(need_coef, dtype=torch.float32, device=dev)
        self._plan_bs = plan.bs
        self._st_cache = {}
        if hasattr(self.backend, "prepare_epoch"):
            self.backend.prepare_epoch(self)

    def _plan_epoch(self):
        """Plan of the CURRENT epoch order, in line (construction, or an epoch boundary without a prefetched plan)."""
        b = self.bat
        self._finish_plan(self._compute_plan((b.pos_h, b.pos_r, b.pos_t), b.rng_stream, 0))
        self._next_plan = None

    def _prefetch_next_epoch(self):
        """Draw the next epoch's permutation into the batcher's alternate buffers and compute its plan on a side stream (the
        sampler, two sorts): by the time the epoch ends it is waiting in the other buffer set."""
        b = self.bat
        nxt = ((b.epoch + 1) * 2) & 0xFFFFFFFF
        bs = 1 - self._plan_bs
        split = self.world > 1 or self.force_collectives
        first = self._plan_sample if split else self._compute_plan               # G > 1: the collective waits for `_gather_at`
        if self.device.type != "cuda":
            self._next_plan = first(b.stage_next_epoch(), nxt, bs)
            return
        # the permutation too goes to the side stream (two device sorts: ~190 us per epoch at the C2 shape — 8 us per global step
        # of an 8-rank epoch when it sat on the steps' stream)
        self._on_side(lambda: setattr(self, "_next_plan", first(b.stage_next_epoch(), nxt, bs)))

    def _on_side(self, fn):
        """Run fn with the plan's side stream current (and pinned for the native calls), ordered after the current stream."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            old = _lib.pin_stream(self._side.cuda_stream)
            try:
                fn()
            finally:
                _lib.pin_stream(old)

    @property
    def _gather_at(self):
        """The step of an epoch before which the NEXT epoch's codes are all-gathered: an eighth into the epoch — the sampling of a
        rank's share is short (0.2 ms at the C2 shape with 8 ranks, 1.5 ms at C5) and the lists that follow the gather (1 - 12 ms)
        want the rest of the epoch, or the host waits for them at the boundary with the GPU idle (measured at C2 with 8 ranks and
        the gather mid-epoch: 117 us per global step for 65 us of kernels)."""
        return min(self.steps - 1, max(1, self.steps // 8)) if self.steps > 1 else 0

    def _plan_midpoint(self):
        """At step `_gather_at` of every epoch, on every rank: the prefetched plan's collective (main stream, step communicator),
        then the rest of the plan back on the side stream."""
        plan = self._next_plan
        if plan is None or plan.stage is not PlanStage.SAMPLED:
            return
        self._plan_gather(plan)
        if self.device.type != "cuda":
            self._plan_rest(plan)
        else:
            self._on_side(lambda: self._plan_rest(plan))

    def _advance_epoch(self):
        """Epoch boundary: random.shuffle of both positive lists (code/MultiKE_model.py:314-315) + the new epoch's plan."""
        if self._next_plan is not None:
            self._plan_midpoint()                            # (an epoch of one step: its midpoint is the boundary itself)
            plan, self._next_plan = self._next_plan, None
            if plan.ready is not None:
                torch.cuda.current_stream().wait_event(plan.ready)
            self.bat.commit_staged()
            self._finish_plan(plan)
        else:
            self.bat.shuffle()
            self._plan_epoch()

    def set_neighbours(self, tables):
        """Truncated negative sampling (code/MultiKE_CSL.py:89-102): install ((cand_table, cand_valid), (...)) for the two KGs
        (None = back to uniform) — identical on every rank.  Takes effect with the NEXT epoch, as in the reference (the refresh
        sits at the end of an epoch): a plan of that epoch prefetched with the old candidates is dropped."""
        for side, nb in ((self.bat.side1, tables[0]), (self.bat.side2, tables[1])):
            side.set_neighbours(*(nb if nb is not None else (None, None)))
        if self._next_plan is not None:
            if self._side is not None:
                torch.cuda.current_stream().wait_stream(self._side)    # the dropped plan may still be writing its buffer set
            self._next_plan = None

    def _map_peers(self, gb):
        """Exchange IPC handles of this rank's send block and gradient inbox ([world][2 C][stride]: one slice per writer) and
        map every peer's (torch's CUDA-IPC tensor reductions: hipIpcGetMemHandle / hipIpcOpenMemHandle underneath).
        Entity-major form: `_v_all[0]` stays the LOCAL [world][block] buffer — the mirror the score launch fills with every vector
        it reads — and `_gv[0]` the LOCAL [2 C][stride] block the inbox is summed into (GVSUM); the second pass reads those two
        (`_addr` -> em_v[0] / em_gv[0] in `prepare_epoch`), only the send block and the inbox are shared."""
        from torch.multiprocessing.reductions import reduce_tensor
        G = self.world
        if self._peer_send is not None and self.device.type == "cuda":
            # re-mapping (the capacity grew): the exchange below is a host rendezvous, so once every rank's device is idle here no
            # kernel anywhere still reads or writes the blocks that are about to be released
            torch.cuda.synchronize()
        self._inbox = torch.zeros(G * gb, dtype=self._dtype, device=self.device)
        if not self.em:
            self._gv = [self._inbox]
            self._v_all = [self._send[0]]                  # unused in peer mode (kept non-null for the address table)
        self._g_all = [self._inbox]
        mine = (reduce_tensor(self._send[0]), reduce_tensor(self._inbox))
        every = self.comm.all_gather_object(mine)
        self._peer_send, self._peer_inbox = [], []
        for g, ((f1, a1), (f2, a2)) in enumerate(every):
            self._peer_send.append(self._send[0] if g == self.rank else f1(*a1))
            self._peer_inbox.append(self._inbox if g == self.rank else f2(*a2))
        self._bar = torch.zeros(1, dtype=torch.float32, device=self.device)

    def _persist(self, key, value, capacity):
        """Epoch buffers keep their device addresses across epochs (the native step descriptors point into them)."""
        buf = self._persistent.get(key)
        if buf is None or buf.numel() < max(capacity, value.numel(), 1):
            buf = self._persistent[key] = torch.zeros(max(capacity, value.numel(), 1), dtype=value.dtype, device=value.device)
        buf[:value.numel()].copy_(value)
        return buf

    def global_scored(self, i: int) -> int:
        s = i % self.steps
        return int(self.bat.off[s + 1] - self.bat.off[s]) * (1 + self.N)

    def _part_step(self, k: int, tag: int) -> OcStep:
        st = self._st_cache.get(k)
        if st is None:
            st = self._st_cache[k] = self._build_part_step(k, tag)
        st.tag = tag
        return st

    def _build_part_step(self, k: int, tag: int) -> OcStep:
        _, lo, hi = self._parts[k]
        b = self.bat
        per, _, _ = self.my_slice(lo, hi)
        nh, nt = int(self._own_cnt[0][k]), int(self._own_cnt[1][k])
        code_off = tuple((lo + g * per) * self.N for g in range(self.world))   # codes are laid out by epoch position
        pw = getattr(b, "pos_w", None)
        return OcStep(b.pos_h[lo:hi], b.pos_r[lo:hi], b.pos_t[lo:hi], per, self._slot[0][lo:hi], self._slot[1][lo:hi],
                      self._own[0][lo:lo + nh], self._own[1][lo:lo + nt], tag, self._codes, code_off,
                      pos_w=(pw[lo:hi] if pw is not None else None),
                      own_rec=self._own_rec, own_off=(self._own_off[lo:hi + 1] if self._own_off is not None else None))

    def _exchange_tensors(self):
        return [*self._send, *self._v_all, *self._g_all, *self._gv, self.rel_grad]

    def _native_loop(self):
        """(usable, mke_oc_comm or None): the step loop can go through mke_oc_steps — HIP backend, a communicator with a native
        form (RCCL through ctypes, the tests' host-staged ranks, the tools' loop-back) or a single rank, no peer-direct, no
        per-launch event collection.  MKE_OC_NATIVE=0 keeps the Python loop."""
        if not hasattr(self.backend, "run_steps") or self.peer_direct or self.score_events is not None or self.chunks > _lib.OC_EM_MAX_CHUNKS \
                or os.environ.get("MKE_OC_NATIVE", "1") == "0":
            return False, None
        if self.world == 1 and not self.force_collectives:
            return True, None
        if not hasattr(self.comm, "native"):
            return False, None
        key = (self.C, self._send[0].data_ptr())
        if self._comm_native_key != key:                     # callbacks look the exchange buffers up by address
            self._comm_native, self._comm_native_key = self.comm.native(self), key
        return True, self._comm_native

    OVERLAP_RS_MIN_BYTES = 16 << 20
    # the update rule of the step descriptors: the reference's relation view trains with Adagrad (code/MultiKE_model.py:17-31) and the
    # multi-GPU drivers accept nothing else (distributed_run.py); plain SGD (code/MultiKE_model.py:24) is the kernels' other rule,
    # reachable through the C-ABI — a subclass sets it for the tests
    OPTIMIZER = _lib.OPT_ADAGRAD

    def _overlap_rs(self) -> bool:
        """Entity-major, one part per step: put the reduce-scatter on the communication stream and run, under it, the second pass's
        work items that do not need its result (at 8 ranks ~95 % of the rows: the corrupt entities) — two stream hops per step
        (~26 us), so only when the reduce-scatter is long: >= 16 MB received per rank (the C5 shape at 8 ranks: 40 MB = 122 us in the
        link model; C2: 12 MB = 48 us, not worth the hops).  MKE_OC_OVERLAP_RS=0 / 1 forces it."""
        if not self.em or self.peer_direct or self.chunks != 1 or self.world < 2 and not self.force_collectives:
            return False                                     # (peer-direct has no reduce-scatter to hide)
        env = os.environ.get("MKE_OC_OVERLAP_RS")
        if env is not None:
            return env == "1"
        return (self.world - 1) * 2 * self.C * self.stride * 4 >= self.OVERLAP_RS_MIN_BYTES

    def run(self, i0: int, n: int):
        """Global steps i0 .. i0 + n - 1 (in order): one native call per run of steps inside an epoch (mke_oc_steps) when the
        communicator has a native form, else the Python step loop."""
        i, end = i0, i0 + n
        while i < end:
            s = i % self.steps
            m = min(end - i, self.steps - s)
            ok, cs = self._native_loop()
            if not ok:
                for k in range(m):
                    self.step(i + k)
                i += m
                continue
            # the epoch prologue of `_begin_step`, except that a run which would pass the gather point is cut there
            if s == 0 and i > 0:
                self._advance_epoch()
            if s == 0 and self.prefetch:
                self._prefetch_next_epoch()
            k = self._gather_at
            if s == k:
                self._plan_midpoint()
            elif s < k < s + m and self._next_plan is not None and self._next_plan.stage is PlanStage.SAMPLED:
                m = k - s                                    # stop at the epoch's gather point: the collective goes between two steps
            ok, cs = self._native_loop()                     # the exchange buffers may have grown with the new epoch's plan
            comm_stream = None
            overlap = self._overlap_rs() if cs is not None else False
            if cs is not None and (self.chunks > 1 or overlap) and self.device.type == "cuda":
                if self._comm_stream is None:
                    self._comm_stream = torch.cuda.Stream(device=self.device)
                comm_stream = self._comm_stream.cuda_stream
            self.backend.run_steps(self, s, s + m, self.tag, cs, comm_stream, overlap)
            self.tag += m
            i += m

    def _begin_step(self, s: int, i: int):
        """What precedes step s of an epoch (global step i), on every rank at the same point of the step sequence."""
        if s == 0 and i > 0:
            self._advance_epoch()
        if s == 0 and self.prefetch:
            self._prefetch_next_epoch()                      # the next epoch's plan overlaps this epoch's steps
        if s == self._gather_at:
            self._plan_midpoint()                            # ... and its one collective goes between two steps

    def _score(self, k: int, tag: int, c: int, loss_slot: int, share: int):
        """SCORE of part k, between two HIP events when `score_events` collects them (`share`: ranks the part's triples are spread over)."""
        ev = self.score_events
        if ev is None:
            self.backend.run(self, k, tag, SCORE, c, loss_slot)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.backend.run(self, k, tag, SCORE, c, loss_slot)
        e1.record()
        ev.append((e0, e1, (self._parts[k][2] - self._parts[k][1]) * (1 + self.N) // share))

    def _exchange(self, ks, tag, slot0, first_phases, share):
        """bases -> ALL-GATHER -> score -> REDUCE-SCATTER of every part; with several parts the collectives are asynchronous and
        part c is scored while part c + 1's all-gather / part c - 1's reduce-scatter are on the wire.  Returns the reduce-scatters'
        handles (None: already in stream order) for the caller to wait on where its tail needs them."""
        be, cm = self.backend, self.comm
        pipelined = len(ks) > 1 and self.device.type == "cuda"
        ag, rs = [], []
        for c, k in enumerate(ks):
            be.run(self, k, tag, first_phases, c, slot0 + c)
            ag.append(cm.all_gather(self._v_all[c], self._send[c], async_op=pipelined))
        for c, k in enumerate(ks):
            if ag[c] is not None:
                ag[c].wait()
            self._score(k, tag, c, slot0 + c, share)
            rs.append(cm.reduce_scatter(self._gv[c], self._g_all[c], async_op=pipelined))
        return rs

    def _step_local(self, ks, tag, slot0):
        """A one-rank step: every row is local, no collective between the phases — one native call when there is one part."""
        be, last = self.backend, len(ks) - 1
        if last == 0 and self.score_events is None:
            be.run(self, ks[0], tag, BASES | SCORE | PASS2 | UPDATE if self.em else BASES | COUNT | SCORE | APPLY | UPDATE, 0, slot0)
        elif self.em:
            for c, k in enumerate(ks):
                be.run(self, k, tag, BASES, c, slot0 + c)
                self._score(k, tag, c, slot0 + c, 1)
            be.run(self, ks[-1], tag, PASS2 | UPDATE, 0, slot0)
        else:
            for c, k in enumerate(ks):
                be.run(self, k, tag, BASES | COUNT, c, slot0 + c)       # counts of ALL parts before any is scored
            for c, k in enumerate(ks):
                self._score(k, tag, c, slot0 + c, 1)
            for c, k in enumerate(ks):
                be.run(self, k, tag, APPLY | (UPDATE if c == last else 0), c, slot0 + c)

    def _step_peer_direct(self, ks, tag, slot0):
        """Atomics form without all-gather / reduce-scatter: every rank maps the other ranks' send blocks and gradient inboxes (IPC
        handles exchanged once, `_map_peers`) and the score launch reads / writes them straight over xGMI; two stream-ordered
        barriers per part.  Correct by construction and tested with two ranks on one GPU; not measured on several."""
        be, cm = self.backend, self.comm
        for k in ks:
            be.run(self, k, tag, BASES | COUNT, 0, slot0)
            cm.barrier(self._bar)                            # every rank's vectors are in its send block
            be.run(self, k, tag, SCORE, 0, slot0)            # reads peers' blocks, writes its slice of peers' inboxes
            cm.barrier(self._bar)                            # every writer's slice of every inbox is complete
            be.run(self, k, tag, APPLY, 0, slot0)
        cm.all_reduce(self.rel_grad)
        if ks:
            be.run(self, ks[-1], tag, UPDATE, 0, slot0)

    def _step_peer_em(self, ks, tag, slot0):
        """Entity-major form without all-gather / reduce-scatter (unchunked: one part).  The score launch reads the vectors from
        the owners' send blocks, MIRRORS them into this rank's local [world][block] buffer and writes its partial gradient
        vectors into its slice of the owners' inboxes; after the second barrier every rank sums its own inbox in rank order into
        a local block and runs the second pass on the two local buffers — the collective form's second pass, unchanged.
        The buffers may be reused by the next step without a further barrier: a peer reads this rank's send block and writes
        this rank's inbox only inside its SCORE, i.e. between the step's two barriers; this rank rewrites its send block (next
        BASES) and rereads its inbox (next GVSUM) only after the all-reduce of the relation gradient below, the step's third
        rendezvous, which no rank passes before every rank has left SCORE; and the next step's writes into this rank's inbox wait
        at that step's first barrier, which this rank enters after its GVSUM | PASS2.  Mirror, summed block and coefficients are
        local.  Correct by construction and tested with two and three ranks on one GPU; never run on several."""
        be, cm = self.backend, self.comm
        k = ks[-1]                                           # (peer-direct runs unchunked: the step's only part)
        be.run(self, k, tag, BASES, 0, slot0)
        cm.barrier(self._bar)                                # every rank's vectors are in its send block
        be.run(self, k, tag, SCORE, 0, slot0)                # reads peers' blocks (and mirrors them), writes its slice of peers' inboxes
        cm.barrier(self._bar)                                # every writer's slice of every inbox is complete
        be.run(self, k, tag, GVSUM | PASS2, 0, slot0)
        cm.all_reduce(self.rel_grad)                         # this rank's partial relation gradient, stored by the second pass
        be.run(self, k, tag, UPDATE, 0, slot0)

    def step(self, i: int):
        """Global step i (steps must be issued in order): the schedule of the module docstring, enqueued from Python."""
        s = i % self.steps
        self._begin_step(s, i)
        be, cm = self.backend, self.comm
        ks = self._parts_of.get(s, [])
        self.tag += 1
        tag, slot0 = self.tag, s * self.chunks
        if self.em and not ks:
            return
        if self.world == 1 and not self.force_collectives:
            self._step_local(ks, tag, slot0)
        elif self.peer_direct and self.em:
            self._step_peer_em(ks, tag, slot0)
        elif self.peer_direct:
            self._step_peer_direct(ks, tag, slot0)
        elif self.em:
            # every part's vectors and gradient vectors in place, then ONE second pass over the touched owned rows of the whole step
            for w in self._exchange(ks, tag, slot0, BASES, self.world):
                if w is not None:
                    w.wait()
            be.run(self, ks[-1], tag, PASS2, 0, slot0)
            cm.all_reduce(self.rel_grad)                     # this rank's partial relation gradient, stored by the second pass
            be.run(self, ks[-1], tag, UPDATE, 0, slot0)
        else:
            # the reference counts over the WHOLE global step (all parts) are complete before any part is scored: they need only the
            # epoch's codes and ride on blocks of the bases launch
            rs = self._exchange(ks, tag, slot0, BASES | (COUNT if self.ref_count is not None else 0), self.world)
            for c, k in enumerate(ks):
                if rs[c] is not None:
                    rs[c].wait()
                be.run(self, k, tag, APPLY, c, slot0 + c)
            cm.all_reduce(self.rel_grad)                     # replicated relation table: the (small) dense gradient; one update of everything
            if ks:
                be.run(self, ks[-1], tag, UPDATE, 0, slot0)

    # ------------------------------------------------------------------------------------------------
    def check(self) -> dict:
        """Capacity is fixed per epoch from the data before the epoch runs (`_plan_epoch`): nothing to flag."""
        out = {"capacity_vectors_per_owner": self.C, "block_bytes": self.block * 4, "chunks": self.chunks,
               "vectors_per_positive": self.vectors_planned / max(1, self._n_all),
               "entity_major": bool(self.em), "peer_direct": bool(self.peer_direct), "native_step_loop": bool(self._native_loop()[0]),
               "reduce_scatter_under_second_pass": bool(self._overlap_rs()), "communicator": type(self.comm).__name__,
               "codes": self.codes_form, "code_bytes_received_per_epoch": int(self._code_bytes)}
        if self.codes_form == "owner":
            out["owner_code_capacity_per_pair"] = int(self._own_cap)
            out["owner_replans"] = int(self.owner_replans)
        if self.em:
            out["references_per_global_step"] = self._em.n_refs / max(1, self.steps)
            out["long_rows_per_global_step"] = int(self._em.long0[-1]) / max(1, self.steps)
        return out

    def scratch_clean(self) -> bool:
        """The zero invariants between steps: gradient scratch all zero, reference counts all zero (the entity-major form has
        no entity scratch and no counts: only the relation gradient)."""
        ok = float(self.rel_grad.abs().max()) == 0.0
        g = self.ent_grad_full if self.ent_grad_full is not None else self.ent_grad
        if g is not None:
            ok = ok and float(g.abs().max()) == 0.0
        if self.ref_count is not None:
            ok = ok and int(self.ref_count.abs().sum()) == 0
        return ok

    def gather_entity_table(self) -> torch.Tensor:
        """Reassemble the full [n_ent, dim] raw table on every rank (tests / checkpoint)."""
        pad = int(math.ceil(self.n_ent / self.world))
        mine = torch.zeros(pad, self.stride, dtype=self.ent.dtype, device=self.device)
        mine[:self.n_local] = self.ent[:self.n_local]
        if self.world == 1:
            return mine[:self.n_local, :self.dim].clone()
        parts = [torch.empty_like(mine) for _ in range(self.world)]
        self.comm.all_gather_list(parts, mine)
        full = torch.zeros(self.n_ent, self.dim, dtype=self.ent.dtype, device=self.device)
        for r in range(self.world):
            n = len(range(r, self.n_ent, self.world))
            full[r::self.world] = parts[r][:n, :self.dim]
        return full

    def epoch_loss(self) -> float:
        t = self.loss_ring.sum()
        if self.world > 1:
            self.comm.all_reduce(t)
        self.loss_ring.zero_()
        return float(t)
