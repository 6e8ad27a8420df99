"""ctypes binding of libmultike_hip.so (the C-ABI declared in include/multike_hip.h).

This is the only place the product touches native code.  There is NO fallback: if the library is
missing or a tensor is not on the GPU the call raises.  PyTorch is used for device memory and streams
only — every pointer handed to the library is `tensor.data_ptr()` of a CUDA(HIP) tensor and the stream
is torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libmultike_hip.so")

# The structs, the prototypes and the MKE_* constants (MKE_X as X) come from _abi.py, which tools/gen_abi.py writes from the
# header: nothing of the header is typed a second time here.  The names below are the ones the rest of the tree uses.
from . import _abi
from ._abi import *  # noqa: F401,F403  (LOSS_PARTIALS, MAX_STRIDE, OPT_*, OC_*, MAP_*, ATTR_*, AE_*, CODE_*, METRIC_*, ...)

SYMBOLS = tuple(_abi.FUNCTIONS)     # every symbol include/multike_hip.h declares (tests/test_abi.py: the .so exports each of them)
AttrStepArgs = _abi.mke_attr_step_args
AlignTableStruct, AlignTermStruct, AlignPlanStruct = _abi.mke_align_table, _abi.mke_align_term, _abi.mke_align_plan
MappingViewStruct, MappingStepArgs = _abi.mke_mapping_view, _abi.mke_mapping_step_args
HotRowsStruct, ScoreArgs, UpdateTableStruct = _abi.mke_hot_rows, _abi.mke_score_args, _abi.mke_update_table
KGSideStruct, RelationPlanStruct = _abi.mke_kg_side, _abi.mke_relation_plan
OcStepStruct, OcEmPlanArgs, OcCommStruct, OcLoopStruct = _abi.mke_oc_step, _abi.mke_oc_em_plan_args, _abi.mke_oc_comm, _abi.mke_oc_loop
AEPlanStruct, OptimizerStruct = _abi.mke_ae_plan, _abi.mke_optimizer          # mke_optimizer: TF1 defaults in optimizer_struct
TopkMeanArgs, AlignArgs, LseArgs, MutualArgs = _abi.mke_topk_mean_args, _abi.mke_align_args, _abi.mke_lse_args, _abi.mke_mutual_args
StableListsArgs, StableMatchArgs = _abi.mke_stable_lists_args, _abi.mke_stable_match_args
AssignArgs, SwapArgs = _abi.mke_assign_args, _abi.mke_swap_args
TuningStruct = _abi.mke_tuning      # the performance knobs of ONE plan / call (a field at TUNE_DEFAULT follows mke_set_option's default)
TUNING_FIELDS = tuple(f for f, _ in TuningStruct._fields_ if f != "reserved")

# what the header gives only in prose
DENSE_OPTS = {"Adam": OPT_ADAM, "Adadelta": OPT_ADADELTA}   # TF1 rules that move zero-gradient weights: whole-variable kernels
_SUPPORTED_FPL = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 20)
ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2
OC_CB_MOVE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)     # all_gather / reduce_scatter callbacks
OC_CB_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)              # all_reduce callback


def tuning(**knobs) -> TuningStruct:
    """A mke_tuning with the given knobs set and every other field at the process default.  The caller keeps it alive for as long
    as a plan points at it."""
    t = TuningStruct()
    _check(lib().mke_tuning_init(C.byref(t)), "mke_tuning_init")
    for k, v in knobs.items():
        if k not in TUNING_FIELDS:
            raise MultiKEHipError(f"unknown tuning knob {k!r}")
        setattr(t, k, int(v))
    return t


def tuning_ptr(t) -> int | None:
    return C.addressof(t) if t is not None else None


def optimizer_struct(name: str, lr: float, step: int = 1) -> OptimizerStruct:
    return OptimizerStruct(DENSE_OPTS[name], float(lr), 0.9, 0.999, 1e-8, 0.95, int(step))


_lib = None


class MultiKEHipError(RuntimeError):
    pass


def lib():
    """Load the library (once).  Raises if it has not been built — there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise MultiKEHipError(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C multike_amd/csrc`.  multike_amd has no CPU fallback.")
        L = C.CDLL(SO_PATH)
        for name, (restype, argtypes) in _abi.FUNCTIONS.items():      # a wrongly typed argument raises ctypes.ArgumentError
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
        # MKE_OPTIONS="name=value,name=value": mke_set_option calls applied at load (performance knobs for experiments)
        for kv in filter(None, os.environ.get("MKE_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            if L.mke_set_option(k.strip().encode(), int(v), None):
                raise MultiKEHipError(f"MKE_OPTIONS: {L.mke_last_error().decode()}")
    return _lib


def stride_for(dim: int) -> int:
    """Smallest supported row stride (floats) >= dim: a multiple of 16 whose /16 the kernels instantiate."""
    need = (dim + 15) // 16
    for f in _SUPPORTED_FPL:
        if f >= need:
            return f * 16
    raise MultiKEHipError(f"dim {dim} exceeds the largest supported stride {MAX_STRIDE}")


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().mke_last_error().decode("utf-8", "replace")
        raise MultiKEHipError(f"{what} failed (code {rc}): {msg}")


def ptr(t: torch.Tensor | None, dtype, name: str) -> int | None:
    """Raw device address of a contiguous CUDA tensor of the given dtype (None -> None = NULL), for an argument or a struct member."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MultiKEHipError(f"{name}: expected a CUDA/HIP tensor, got device {t.device} (no CPU path exists)")
    if t.dtype != dtype:
        raise MultiKEHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MultiKEHipError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


_dev = ptr      # for stable_match_args, whose own argument is called ptr


_pinned_stream = None  # raw hipStream_t handle pinned by a hot loop (saves a torch.cuda.current_stream() per launch)


def pin_stream(handle: int | None):
    """Pin the stream every launch goes to (a raw `stream.cuda_stream` handle), or None to follow torch's current
    stream again.  Returns the previous pin."""
    global _pinned_stream
    old, _pinned_stream = _pinned_stream, handle
    return old


def _stream():
    if _pinned_stream is not None:
        return _pinned_stream
    return torch.cuda.current_stream().cuda_stream


def version() -> int:
    return lib().mke_version()


def set_option(name: str, value: int) -> int:
    old = C.c_int(0)
    _check(lib().mke_set_option(name.encode(), value, C.byref(old)), "mke_set_option")
    return old.value


def stage_reduce(stage_rows, sorted_keys, order, grad_ent, grad_rel, touched_ent, touched_rel, tag):
    rc = lib().mke_stage_reduce(ptr(stage_rows, torch.float32, "stage_rows"), ptr(sorted_keys, torch.int64, "keys"),
                                ptr(order, torch.int64, "order"), sorted_keys.numel(), stage_rows.shape[1],
                                ptr(grad_ent, torch.float32, "grad_ent"), ptr(grad_rel, torch.float32, "grad_rel"),
                                ptr(touched_ent, torch.int32, "touched"), ptr(touched_rel, torch.int32, "touched"), tag,
                                _stream())
    _check(rc, "mke_stage_reduce")


def get_option(name: str) -> int:
    old = set_option(name, 0)
    set_option(name, old)
    return old


def count_entity_refs(pos_h, pos_t, neg_h, neg_t, neg_per_pos, ref_count):
    rc = lib().mke_count_entity_refs(ptr(pos_h, torch.int32, "pos_h"), ptr(pos_t, torch.int32, "pos_t"),
                                     pos_h.numel(), ptr(neg_h, torch.int32, "neg_h"),
                                     ptr(neg_t, torch.int32, "neg_t"), 0 if neg_h is None else neg_h.numel(),
                                     neg_per_pos, ptr(ref_count, torch.int32, "ref_count"), _stream())
    _check(rc, "mke_count_entity_refs")


def _score_step(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent, grad_rel,
                touched_ent, touched_rel, tag, loss_partials, **more):
    """mke_triple_score_step: one ScoreArgs filled from tensors (pos / neg = (h, r, t) int32 CUDA tensors, neg may be None;
    grad_rel [K, n_rel, stride] = K privatised copies, or [n_rel, stride]).  `more`: the remaining fields, as values ready
    for the struct."""
    i32, f32 = torch.int32, torch.float32
    a = ScoreArgs(**more)
    a.ent_table, a.n_ent, a.ent_normalize = ptr(ent, f32, "ent_table"), ent.shape[0], int(ent_normalize)
    a.rel_table, a.n_rel, a.rel_normalize = ptr(rel, f32, "rel_table"), rel.shape[0], int(rel_normalize)
    a.stride, a.dim = ent.shape[1], dim
    ph, pr, pt = pos
    nh, nr, nt = neg if neg is not None else (None, None, None)
    a.pos_h, a.pos_r, a.pos_t = ptr(ph, i32, "pos_h"), ptr(pr, i32, "pos_r"), ptr(pt, i32, "pos_t")
    a.pos_w, a.n_pos = ptr(pos_w, f32, "pos_w"), ph.numel()
    a.neg_h, a.neg_r, a.neg_t = ptr(nh, i32, "neg_h"), ptr(nr, i32, "neg_r"), ptr(nt, i32, "neg_t")
    a.neg_w, a.n_neg = ptr(neg_w, f32, "neg_w"), 0 if nh is None else nh.numel()
    a.neg_per_pos, a.scale = neg_per_pos, scale
    a.grad_ent, a.grad_rel = ptr(grad_ent, f32, "grad_ent"), ptr(grad_rel, f32, "grad_rel")
    a.grad_rel_copies = 1 if grad_rel is None or grad_rel.dim() == 2 else grad_rel.shape[0]
    a.touched_ent, a.touched_rel, a.tag = ptr(touched_ent, i32, "touched_ent"), ptr(touched_rel, i32, "touched_rel"), tag
    a.loss_partials = ptr(loss_partials, torch.float64, "loss_partials")
    _check(lib().mke_triple_score_step(C.byref(a), _stream()), "mke_triple_score_step")


def triple_score_fwd_bwd(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale,
                         grad_ent, grad_rel, touched_ent, touched_rel, tag, loss_partials):
    """The fused relation-view step, forward (grad_ent None) or forward / backward (header section (1))."""
    _score_step(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent, grad_rel,
                touched_ent, touched_rel, tag, loss_partials)


def triple_score_fwd_bwd_x(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent,
                           grad_rel, touched_ent, touched_rel, tag, ref_count, ent_acc, optimizer, lr, loss_partials, hot=None,
                           tuning=None):
    """The fused step with the exclusive-row fast path (ref_count filled by count_entity_refs for the same batch).  hot
    (HotRowsStruct of the entity table, `EmbeddingTable.hot_struct()`): the hub rows' flushes go to their private copies
    (mke_score_args.hot); the update must then get the same struct.  tuning: this call's knobs (TuningStruct)."""
    more = {"hot": hot} if hot is not None and hot.n_hot > 0 else {}
    _score_step(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent, grad_rel,
                touched_ent, touched_rel, tag, loss_partials, ref_count=ptr(ref_count, torch.int32, "ref_count"),
                ent_acc=ptr(ent_acc, torch.float32, "ent_acc"), optimizer=optimizer, lr=lr, tuning=tuning_ptr(tuning), **more)


def triple_score_fwd_bwd_det(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent,
                             grad_rel, touched_ent, touched_rel, tag, ref_count, ent_acc, optimizer, lr, stage_rows, stage_keys,
                             loss_partials):
    """The same step in deterministic mode: contributions stored into stage_rows / stage_keys (then stage_reduce)."""
    _score_step(ent, ent_normalize, rel, rel_normalize, dim, pos, pos_w, neg, neg_w, neg_per_pos, scale, grad_ent, grad_rel,
                touched_ent, touched_rel, tag, loss_partials, ref_count=ptr(ref_count, torch.int32, "ref_count"),
                ent_acc=ptr(ent_acc, torch.float32, "ent_acc"), optimizer=optimizer, lr=lr,
                stage_rows=ptr(stage_rows, torch.float32, "stage_rows"), stage_keys=ptr(stage_keys, torch.int64, "stage_keys"),
                stage_slots=stage_keys.numel())


def rows_update(table, acc, grad, touched, tag, dim, normalize, optimizer, lr):
    copies = 1 if grad.dim() == 2 else grad.shape[0]
    rc = lib().mke_rows_update(
        ptr(table, torch.float32, "table"), ptr(acc, torch.float32, "acc"), ptr(grad, torch.float32, "grad"),
        copies, ptr(touched, torch.int32, "touched"), tag, table.shape[0], table.shape[1],
        dim, int(normalize), optimizer, lr, _stream())
    _check(rc, "mke_rows_update")


def rows_update_multi(tables, tag, stride, dim, optimizer, lr, tuning=None):
    """tables: list of (data, acc, grad, touched, normalize[, ref_count[, hot]]) (hot: the table's HotRowsStruct); or, for the owner side of the sharded
    step, a dict(table=, acc=, normalize=, src_rows=, slot_of=, n_ranks=, capacity=) (mke_update_table.slot_of)."""
    arr = (UpdateTableStruct * len(tables))()
    for k, tpl in enumerate(tables):
        if isinstance(tpl, dict):
            arr[k].table = ptr(tpl["table"], torch.float32, "table")
            arr[k].acc = ptr(tpl["acc"], torch.float32, "acc")
            arr[k].n_rows = tpl["table"].shape[0]
            arr[k].normalize = int(tpl["normalize"])
            arr[k].grad_copies = 1
            arr[k].src_rows = ptr(tpl["src_rows"], torch.float32, "src_rows")
            arr[k].slot_of = ptr(tpl["slot_of"], torch.int32, "slot_of")
            arr[k].n_ranks = int(tpl["n_ranks"])
            arr[k].capacity = int(tpl["capacity"])
            if tpl["slot_of"].numel() < arr[k].n_rows * arr[k].n_ranks or tpl["src_rows"].shape[0] < arr[k].n_ranks * arr[k].capacity:
                raise ValueError("slot_of / src_rows are smaller than n_rows * n_ranks / n_ranks * capacity")
            continue
        data, acc, grad, touched, normalize = tpl[:5]
        arr[k].ref_count = ptr(tpl[5], torch.int32, "ref_count") if len(tpl) > 5 and tpl[5] is not None else None
        if len(tpl) > 6 and tpl[6] is not None:
            arr[k].hot = tpl[6]
        arr[k].table = ptr(data, torch.float32, "table")
        arr[k].acc = ptr(acc, torch.float32, "acc")
        arr[k].grad = ptr(grad, torch.float32, "grad")
        arr[k].touched = ptr(touched, torch.int32, "touched") if touched is not None else None
        arr[k].n_rows = data.shape[0]
        arr[k].normalize = int(normalize)
        arr[k].grad_copies = 1 if grad.dim() == 2 else grad.shape[0]
    if tuning is not None:       # this call's knobs (TuningStruct)
        rc = lib().mke_rows_update_multi_t(arr, len(tables), tag, stride, dim,
                                           optimizer, lr, None, C.byref(tuning), _stream())
        _check(rc, "mke_rows_update_multi_t")
        return
    rc = lib().mke_rows_update_multi(arr, len(tables), tag, stride, dim,
                                     optimizer, lr, _stream())
    _check(rc, "mke_rows_update_multi")


def neg_sample(pos, pos_offset, pos_kg, sides, neg_per_pos, max_try, seed, stream_id, neg_out):
    """sides: (KGSideStruct * 2) host array; pos_kg: uint8 CUDA tensor or None (all KG 0)."""
    ph, pr, pt = pos
    nh, nr, nt = neg_out
    rc = lib().mke_neg_sample(
        ptr(ph, torch.int32, "pos_h"), ptr(pr, torch.int32, "pos_r"), ptr(pt, torch.int32, "pos_t"),
        ph.numel(), pos_offset, ptr(pos_kg, torch.uint8, "pos_kg"), sides,
        neg_per_pos, max_try, seed[0] & 0xFFFFFFFF, seed[1] & 0xFFFFFFFF,
        stream_id & 0xFFFFFFFF, ptr(nh, torch.int32, "neg_h"), ptr(nr, torch.int32, "neg_r"),
        ptr(nt, torch.int32, "neg_t"), _stream())
    _check(rc, "mke_neg_sample")


def neg_sample_at(pos, pos_index, pos_kg, sides, neg_per_pos, max_try, seed, stream_id, neg_out):
    """mke_neg_sample_at: like neg_sample, with an explicit int32 epoch position per positive."""
    ph, pr, pt = pos
    nh, nr, nt = neg_out
    rc = lib().mke_neg_sample_at(
        ptr(ph, torch.int32, "pos_h"), ptr(pr, torch.int32, "pos_r"), ptr(pt, torch.int32, "pos_t"),
        ph.numel(), ptr(pos_index, torch.int32, "pos_index"), ptr(pos_kg, torch.uint8, "pos_kg"), sides,
        neg_per_pos, max_try, seed[0] & 0xFFFFFFFF, seed[1] & 0xFFFFFFFF,
        stream_id & 0xFFFFFFFF, ptr(nh, torch.int32, "neg_h"), ptr(nr, torch.int32, "neg_r"),
        ptr(nt, torch.int32, "neg_t"), _stream())
    _check(rc, "mke_neg_sample_at")


SIM_SELECT_KPADS = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)   # instantiations of k_sim_select / k_sim_sample / k_align_rank: up to MAX_STRIDE


def _candidates(cand: torch.Tensor):
    """The (column, similarity bits) int32 pairs of sim_select as the mke_candidate* the prototypes declare."""
    return C.cast(ptr(cand, torch.int32, "cand"), C.POINTER(_abi.mke_candidate))


def sim_select(emb: torch.Tensor, kpad: int, row_lo: int, row_hi: int, tau: torch.Tensor, n_seg: int, seg_cap: int):
    """mke_sim_select -> (cand int32 [rows, n_seg, seg_cap, 2] = (column, similarity bits) pairs, seg_count int32 [rows, n_seg])."""
    if emb.dim() != 2 or emb.stride(1) != 1 or emb.dtype != torch.float32:
        raise MultiKEHipError("sim_select: emb must be a row-major float32 matrix")
    rows = row_hi - row_lo
    if tau.numel() != rows:
        raise MultiKEHipError("sim_select: one threshold per row")
    cand = torch.empty(rows, n_seg, seg_cap, 2, dtype=torch.int32, device=emb.device)
    cnt = torch.empty(rows, n_seg, dtype=torch.int32, device=emb.device)
    rc = lib().mke_sim_select(emb.data_ptr(), emb.stride(0), kpad, emb.shape[0],
                              row_lo, row_hi, ptr(tau, torch.float32, "tau"), n_seg,
                              seg_cap, _candidates(cand), ptr(cnt, torch.int32, "seg_count"), _stream())
    _check(rc, "mke_sim_select")
    return cand, cnt


def sim_sample(emb: torch.Tensor, kpad: int, row_lo: int, row_hi: int, samp: torch.Tensor):
    """mke_sim_sample -> float32 [row_hi - row_lo, n_samp] similarities of the rows to the sample rows."""
    out = torch.empty(row_hi - row_lo, samp.shape[0], dtype=torch.float32, device=emb.device)
    rc = lib().mke_sim_sample(ptr(emb, torch.float32, "emb"), emb.stride(0), kpad, emb.shape[0],
                              row_lo, row_hi, ptr(samp, torch.float32, "samp"), samp.stride(0),
                              samp.shape[0], ptr(out, torch.float32, "out"), _stream())
    _check(rc, "mke_sim_sample")
    return out


def topk_candidates(cand: torch.Tensor, seg_count: torch.Tensor, k: int, id_map=None):
    """mke_topk_candidates over sim_select's pairs -> (out_idx int32 [rows, k], status int32 [rows])."""
    rows, n_seg, seg_cap, _ = cand.shape
    out = torch.empty(rows, k, dtype=torch.int32, device=cand.device)
    status = torch.empty(rows, dtype=torch.int32, device=cand.device)
    rc = lib().mke_topk_candidates(_candidates(cand), ptr(seg_count, torch.int32, "seg_count"), rows,
                                   n_seg, seg_cap, k, ptr(id_map, torch.int32, "id_map"),
                                   ptr(out, torch.int32, "out_idx"), None, ptr(status, torch.int32, "status"), _stream())
    _check(rc, "mke_topk_candidates")
    return out, status


def topk_rows(vals: torch.Tensor, k: int, idx=None, seg_count=None, id_map=None, want_idx=True, want_kth=False):
    """mke_topk_rows over vals [rows, n_seg, seg_cap] (or [rows, seg_cap]) -> (out_idx int32 [rows, k] | None,
    kth float32 [rows] | None, status int32 [rows])."""
    if vals.dim() == 2:
        vals = vals.unsqueeze(1)
    if not vals.is_contiguous():
        raise MultiKEHipError("topk_rows: vals must be contiguous")
    rows, n_seg, seg_cap = vals.shape
    out = torch.empty(rows, k, dtype=torch.int32, device=vals.device) if want_idx else None
    kth = torch.empty(rows, dtype=torch.float32, device=vals.device) if want_kth else None
    status = torch.empty(rows, dtype=torch.int32, device=vals.device)
    rc = lib().mke_topk_rows(ptr(vals, torch.float32, "vals"), ptr(idx, torch.int32, "idx"),
                             ptr(seg_count, torch.int32, "seg_count"), rows, n_seg, seg_cap,
                             k, ptr(id_map, torch.int32, "id_map"), ptr(out, torch.int32, "out_idx"),
                             ptr(kth, torch.float32, "out_kth"), ptr(status, torch.int32, "status"), _stream())
    _check(rc, "mke_topk_rows")
    return out, kth, status


def topk_long(vals: torch.Tensor, k: int, id_map=None) -> torch.Tensor:
    """mke_topk_long over whole rows vals [rows, n] (any n) -> int32 [rows, k], column order."""
    if vals.dim() != 2 or vals.stride(1) != 1:
        raise MultiKEHipError("topk_long: vals must be [rows, n] with unit column stride")
    rows, n = vals.shape
    out = torch.empty(rows, k, dtype=torch.int32, device=vals.device)
    rc = lib().mke_topk_long(vals.data_ptr() if vals.is_cuda and vals.dtype == torch.float32 else ptr(vals, torch.float32, "vals"),
                             rows, n, vals.stride(0) if rows > 1 else n, k,
                             ptr(id_map, torch.int32, "id_map"), ptr(out, torch.int32, "out_idx"), _stream())
    _check(rc, "mke_topk_long")
    return out


THIN_SO_PATH = os.path.join(_HERE, "libmultike_thin.so")     # include/multike_thin.h: a library and a generated module of its own
_thin = None


def thin_lib():
    """Load libmultike_thin.so (once), typed from _abi_thin.py as lib() is from _abi.py.  Raises if it has not been built."""
    global _thin
    if _thin is None:
        from . import _abi_thin
        if not os.path.exists(THIN_SO_PATH):
            raise MultiKEHipError(f"{THIN_SO_PATH} not found: build it with `make -C multike_amd/csrc`.  multike_amd has no CPU fallback.")
        L = C.CDLL(THIN_SO_PATH)
        for name, (restype, argtypes) in _abi_thin.FUNCTIONS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _thin = L
    return _thin


def idlist_thin(ids: torch.Tensor, m: int, seed: int, row_ids=None) -> torch.Tensor:
    """mke_idlist_thin over the id lists ids int32 [rows, k] (unit column stride) -> int32 [rows, m]: the keyed m-subset of
    every row, in list order.  row_ids int32 [rows]: the entity id that keys each row (None: the row number)."""
    if ids.dim() != 2 or ids.stride(1) != 1:
        raise MultiKEHipError("idlist_thin: ids must be [rows, k] with unit column stride")
    rows, k = ids.shape
    if row_ids is not None and row_ids.numel() != rows:
        raise MultiKEHipError("idlist_thin: one row id per row")
    out = torch.empty(rows, max(0, int(m)), dtype=torch.int32, device=ids.device)
    L = thin_lib()
    rc = L.mke_idlist_thin(ids.data_ptr() if ids.is_cuda and ids.dtype == torch.int32 else ptr(ids, torch.int32, "ids"),
                           rows, k, ids.stride(0) if rows > 1 else k, ptr(row_ids, torch.int32, "row_ids"), int(m),
                           int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out, torch.int32, "out"), _stream())
    if rc != 0:
        raise MultiKEHipError(f"mke_idlist_thin failed (code {rc}): {L.mke_thin_last_error().decode('utf-8', 'replace')}")
    return out


KEYED_SO_PATH = os.path.join(_HERE, "libmultike_keyed.so")   # include/multike_keyed.h: a library and a generated module of its own
# instantiations of k_sim_select_keyed.  224 is there for the kernel tests alone (the first width with 32-column tiles, next to
# 208, the last with 64): k_sim_sample has no 224, so neighbour_table takes its kpad from SIM_SELECT_KPADS on every path and rows
# of 209 .. 224 floats run at 256 as they always have
KEYED_KPADS = tuple(sorted(SIM_SELECT_KPADS + (224,)))
_keyed = None


def keyed_lib():
    """Load libmultike_keyed.so (once), typed from _abi_keyed.py as lib() is from _abi.py.  Raises if it has not been built."""
    global _keyed
    if _keyed is None:
        from . import _abi_keyed
        if not os.path.exists(KEYED_SO_PATH):
            raise MultiKEHipError(f"{KEYED_SO_PATH} not found: build it with `make -C multike_amd/csrc`.  multike_amd has no CPU fallback.")
        L = C.CDLL(KEYED_SO_PATH)
        for name, (restype, argtypes) in _abi_keyed.FUNCTIONS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _keyed = L
    return _keyed


def _keyed_check(rc: int, what: str):
    if rc != 0:
        raise MultiKEHipError(f"{what} failed (code {rc}): {keyed_lib().mke_keyed_last_error().decode('utf-8', 'replace')}")


def _keyed_candidates(cand: torch.Tensor):
    from . import _abi_keyed
    return C.cast(ptr(cand, torch.int32, "cand"), C.POINTER(_abi_keyed.mke_keyed_candidate))


def sim_select_keyed(emb: torch.Tensor, kpad: int, row_lo: int, row_hi: int, tau_lo: torch.Tensor, tau_hi: torch.Tensor,
                     col_ids: torch.Tensor, seed: int, key_below: int, n_seg: int, seg_cap: int):
    """mke_sim_select_keyed -> (cand int32 [rows, n_seg, seg_cap, 2] = (column, similarity bits) pairs, seg_count int32
    [rows, n_seg], seg_sure int32 [rows, n_seg]).  col_ids int32 [n]: the entity id of every working row / column."""
    if emb.dim() != 2 or emb.stride(1) != 1 or emb.dtype != torch.float32:
        raise MultiKEHipError("sim_select_keyed: emb must be a row-major float32 matrix")
    rows = row_hi - row_lo
    if tau_lo.numel() != rows or tau_hi.numel() != rows:
        raise MultiKEHipError("sim_select_keyed: one pair of thresholds per row")
    if col_ids.numel() != emb.shape[0]:
        raise MultiKEHipError("sim_select_keyed: one id per row of emb")
    cand = torch.empty(rows, n_seg, seg_cap, 2, dtype=torch.int32, device=emb.device)
    cnt = torch.empty(rows, n_seg, dtype=torch.int32, device=emb.device)
    sure = torch.empty(rows, n_seg, dtype=torch.int32, device=emb.device)
    rc = keyed_lib().mke_sim_select_keyed(emb.data_ptr(), emb.stride(0), kpad, emb.shape[0], row_lo, row_hi,
                                          ptr(tau_lo, torch.float32, "tau_lo"), ptr(tau_hi, torch.float32, "tau_hi"),
                                          ptr(col_ids, torch.int32, "col_ids"), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          int(key_below) & 0xFFFFFFFFFFFFFFFF, n_seg, seg_cap, _keyed_candidates(cand),
                                          ptr(cnt, torch.int32, "seg_count"), ptr(sure, torch.int32, "seg_sure"), _stream())
    _keyed_check(rc, "mke_sim_select_keyed")
    return cand, cnt, sure


def keyed_finish(cand: torch.Tensor, seg_count: torch.Tensor, seg_sure: torch.Tensor, tau_hi: torch.Tensor, row_ids: torch.Tensor,
                 col_ids: torch.Tensor, k: int, m: int, seed: int, key_below: int, out=None):
    """mke_keyed_finish over sim_select_keyed's lists -> (out int32 [rows, m], status int32 [rows]); rows whose status is not 0
    are not written (`out`: a tensor to write into, e.g. to see that)."""
    rows, n_seg, seg_cap, _ = cand.shape
    if tau_hi.numel() != rows or row_ids.numel() != rows:
        raise MultiKEHipError("keyed_finish: one threshold and one row id per row")
    if out is None:
        out = torch.empty(rows, max(0, int(m)), dtype=torch.int32, device=cand.device)
    status = torch.empty(rows, dtype=torch.int32, device=cand.device)
    rc = keyed_lib().mke_keyed_finish(_keyed_candidates(cand), ptr(seg_count, torch.int32, "seg_count"),
                                      ptr(seg_sure, torch.int32, "seg_sure"), rows, n_seg, seg_cap,
                                      ptr(tau_hi, torch.float32, "tau_hi"), ptr(row_ids, torch.int32, "row_ids"),
                                      ptr(col_ids, torch.int32, "col_ids"), int(k), int(m), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                      int(key_below) & 0xFFFFFFFFFFFFFFFF, ptr(out, torch.int32, "out"),
                                      ptr(status, torch.int32, "status"), _stream())
    _keyed_check(rc, "mke_keyed_finish")
    return out, status


LINKS_SO_PATH = os.path.join(_HERE, "libmultike_links.so")   # include/multike_links.h: a library and a generated module of its own
_links = None


def links_lib():
    """Load libmultike_links.so (once), typed from _abi_links.py as lib() is from _abi.py.  Raises if it has not been built."""
    global _links
    if _links is None:
        from . import _abi_links
        if not os.path.exists(LINKS_SO_PATH):
            raise MultiKEHipError(f"{LINKS_SO_PATH} not found: build it with `make -C multike_amd/csrc`.  multike_amd has no CPU fallback.")
        L = C.CDLL(LINKS_SO_PATH)
        for name, (restype, argtypes) in _abi_links.FUNCTIONS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _links = L
    return _links


def links_edit(held, match, a, b, kpad, metric=METRIC_INNER, sq_a=None, sq_b=None, csls_row=None, csls_col=None,
               retain=float("-inf"), new_score=None, want_score=True, out=None):
    """mke_links_edit over the link set held int32 [n_a], this refresh's match int32 [n_a] and the decode's operands (row-major
    padded a [n_a, lda] / b [n_b, ldb], as align_mutual takes them) -> (out int32 [n_a], score float32 [n_a] or None, counts
    int32 [7]).  `out` = (out, score or None, inv int32 [n_b], counts) to write into instead of fresh tensors.  Nothing is read
    back here."""
    from . import _abi_links
    n_a, n_b = a.shape[0], b.shape[0]
    if held.numel() != n_a or match.numel() != n_a:
        raise MultiKEHipError(f"links_edit: held has {held.numel()} rows, match {match.numel()}, a {n_a}")
    dev = a.device
    if out is None:
        out = (torch.empty(n_a, dtype=torch.int32, device=dev), torch.empty(n_a, dtype=torch.float32, device=dev) if want_score else None,
               torch.empty(n_b, dtype=torch.int32, device=dev), torch.empty(_abi_links.LINKS_COUNTS, dtype=torch.int32, device=dev))
    o, score, inv, counts = out
    if o.numel() < n_a or inv.numel() < n_b or (score is not None and score.numel() < n_a) or counts.numel() < _abi_links.LINKS_COUNTS:
        raise MultiKEHipError("links_edit: out is shorter than the link set")
    if n_a > 0 and n_b == 0:                # the call zeroes the counters and nothing else: no column, no link
        o[:n_a] = -1
        if score is not None:
            score[:n_a] = 0.0
    args = _abi_links.mke_links_args(ptr(held, torch.int32, "held"), ptr(match, torch.int32, "match"), n_a, n_b,
                                     ptr(a, torch.float32, "a"), a.stride(0), ptr(b, torch.float32, "b"), b.stride(0), kpad, metric,
                                     ptr(sq_a, torch.float32, "sq_a"), ptr(sq_b, torch.float32, "sq_b"),
                                     ptr(csls_row, torch.float32, "csls_row"), ptr(csls_col, torch.float32, "csls_col"),
                                     float(retain), ptr(new_score, torch.float32, "new_score"), ptr(inv, torch.int32, "inv"),
                                     ptr(o, torch.int32, "out"), ptr(score, torch.float32, "score"), ptr(counts, torch.int32, "counts"))
    L = links_lib()
    rc = L.mke_links_edit(C.byref(args), _stream())
    if rc != 0:
        raise MultiKEHipError(f"mke_links_edit failed (code {rc}): {L.mke_links_last_error().decode('utf-8', 'replace')}")
    return o, score, counts


SPARSE_SO_PATH = os.path.join(_HERE, "libmultike_sparse.so")   # include/multike_sparse.h: a library and a generated module of its own
_sparse = None


def sparse_lib():
    """Load libmultike_sparse.so (once), typed from _abi_sparse.py as lib() is from _abi.py.  Raises if it has not been built."""
    global _sparse
    if _sparse is None:
        from . import _abi_sparse
        if not os.path.exists(SPARSE_SO_PATH):
            raise MultiKEHipError(f"{SPARSE_SO_PATH} not found: build it with `make -C multike_amd/csrc`.  multike_amd has no CPU fallback.")
        L = C.CDLL(SPARSE_SO_PATH)
        for name, (restype, argtypes) in _abi_sparse.FUNCTIONS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _sparse = L
    return _sparse


def _sparse_check(rc, what):
    if rc != 0:
        raise MultiKEHipError(f"{what} failed (code {rc}): {sparse_lib().mke_sparse_last_error().decode('utf-8', 'replace')}")


class SparseSupport:
    """The device arrays mke_sparse_support writes (include/multike_sparse.h) and the sizes they were built for.  `count` is a
    device word: nothing is read back to build or to iterate."""
    __slots__ = ("n_a", "n_b", "capacity", "row_off", "row_seg", "ent_col", "ent_val", "col_off", "col_seg", "ent_row", "ent_idx",
                 "count", "lse_temp")

    def entries(self):
        """The entry count, read back (reports and tests only)."""
        return int(self.count.item())


def sparse_support(val_r, col_r, val_c, row_c, out=None):
    """mke_sparse_support over the row lists val_r / col_r [n_a, cut_r] and the column lists val_c / row_c [n_b, cut_c] -> a
    SparseSupport.  `out` = a SparseSupport whose arrays are written in place of fresh ones (tests: poisoned buffers)."""
    from . import _abi_sparse
    (n_a, cut_r), (n_b, cut_c) = col_r.shape, row_c.shape
    if val_r.shape != col_r.shape or val_c.shape != row_c.shape:
        raise MultiKEHipError("sparse_support: a list's values and indices differ in shape")
    dev = col_r.device
    L = sparse_lib()
    need = L.mke_sparse_support_temp_bytes(n_a, n_b, cut_r, cut_c)
    if need < 0:
        _sparse_check(int(need), "mke_sparse_support_temp_bytes")
    s = out
    if s is None:
        s = SparseSupport()
        s.n_a, s.n_b, s.capacity = n_a, n_b, n_a * cut_r + n_b * cut_c
        s.row_off = torch.empty(n_a + 1, dtype=torch.int64, device=dev)
        s.col_off = torch.empty(n_b + 1, dtype=torch.int64, device=dev)
        s.row_seg = torch.empty(n_a + 1, dtype=torch.int32, device=dev)
        s.col_seg = torch.empty(n_b + 1, dtype=torch.int32, device=dev)
        s.ent_col, s.ent_row, s.ent_idx = (torch.empty(s.capacity, dtype=torch.int32, device=dev) for _ in range(3))
        s.ent_val = torch.empty(s.capacity, dtype=torch.float32, device=dev)
        s.count = torch.empty(1, dtype=torch.int64, device=dev)
        s.lse_temp = torch.empty(max(int(L.mke_sparse_lse_temp_bytes(s.capacity)), 8) // 4, dtype=torch.int32, device=dev)
    temp = torch.empty(max(int(need), 4) // 4, dtype=torch.int32, device=dev)
    args = _abi_sparse.mke_sparse_support_args(
        ptr(val_r, torch.float32, "val_r"), ptr(col_r, torch.int32, "col_r"), ptr(val_c, torch.float32, "val_c"),
        ptr(row_c, torch.int32, "row_c"), n_a, n_b, cut_r, cut_c, s.capacity,
        ptr(s.row_off, torch.int64, "row_off"), ptr(s.row_seg, torch.int32, "row_seg"), ptr(s.ent_col, torch.int32, "ent_col"),
        ptr(s.ent_val, torch.float32, "ent_val"), ptr(s.col_off, torch.int64, "col_off"), ptr(s.col_seg, torch.int32, "col_seg"),
        ptr(s.ent_row, torch.int32, "ent_row"), ptr(s.ent_idx, torch.int32, "ent_idx"), ptr(s.count, torch.int64, "count"),
        ptr(temp, torch.int32, "temp"), temp.numel() * 4)
    _sparse_check(L.mke_sparse_support(C.byref(args), _stream()), "mke_sparse_support")
    return s


def sparse_lse(s, columns, tau, sub=None, out=None):
    """One mke_sparse_lse call over the rows (columns = False) or the columns (True) of a SparseSupport: out float32 [n],
    out[i] = tau log sum over the list's entries of exp((value - sub[the entry's other index]) / tau); sub None = zeros."""
    from . import _abi_sparse
    n = s.n_b if columns else s.n_a
    if sub is not None and sub.numel() != (s.n_a if columns else s.n_b):
        raise MultiKEHipError(f"sparse_lse: sub has {sub.numel()} elements, the other side {s.n_a if columns else s.n_b}")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=s.row_off.device)
    off, seg, other, idx = (s.col_off, s.col_seg, s.ent_row, s.ent_idx) if columns else (s.row_off, s.row_seg, s.ent_col, None)
    args = _abi_sparse.mke_sparse_lse_args(n, ptr(off, torch.int64, "off"), ptr(seg, torch.int32, "seg"), ptr(other, torch.int32, "other"),
                                           ptr(s.ent_val, torch.float32, "val"), ptr(idx, torch.int32, "idx"),
                                           ptr(sub, torch.float32, "sub"), float(tau), ptr(out, torch.float32, "out"), s.capacity,
                                           ptr(s.lse_temp, torch.int32, "temp"), s.lse_temp.numel() * 4)
    _sparse_check(sparse_lib().mke_sparse_lse(C.byref(args), _stream()), "mke_sparse_lse")
    return out


def mapping_scratch_floats(n: int, dim: int) -> int:
    return int(lib().mke_mapping_scratch_floats(n, dim))


def mapping_step_phases(args: MappingStepArgs, loss_partials: torch.Tensor, phases: int):
    rc = lib().mke_mapping_step_phases(C.byref(args), ptr(loss_partials, torch.float64, "loss_partials"), phases, _stream())
    _check(rc, "mke_mapping_step_phases")


def mapping_step(args: MappingStepArgs, loss_partials: torch.Tensor):
    rc = lib().mke_mapping_step(C.byref(args), ptr(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_mapping_step")


def mapping_steps(args: MappingStepArgs, step_off: np.ndarray, loss_ring: torch.Tensor):
    """loss_ring: float64 [ring, 4, LOSS_PARTIALS]."""
    off = np.ascontiguousarray(step_off, dtype=np.int64)
    rc = lib().mke_mapping_steps(C.byref(args), off.ctypes.data, len(off) - 1,
                                 ptr(loss_ring, torch.float64, "loss_ring"), loss_ring.shape[0], _stream())
    _check(rc, "mke_mapping_steps")


def align_steps(plan: AlignPlanStruct):
    rc = lib().mke_align_steps(C.byref(plan), _stream())
    _check(rc, "mke_align_steps")


def relation_steps(plan: RelationPlanStruct, step_begin: int, step_end: int):
    rc = lib().mke_relation_steps(C.byref(plan), step_begin, step_end, _stream())
    _check(rc, "mke_relation_steps")


def neg_code_row_words(n_ent: int) -> int:
    """Words of one step's row of the code-word bake's bitmap (2 bits per entity)."""
    return int(lib().mke_neg_code_row_words(n_ent))


def neg_codes(pos, step_off_dev, step_begin, step_end, pos_begin, pos_end, neg, neg_per_pos, n_ent, bits, neg_code):
    """mke_neg_codes: one code word per negative of steps [step_begin, step_end).  pos: the epoch's (h, r, t); neg: the chunk's."""
    rc = lib().mke_neg_codes(*(ptr(x, torch.int32, "pos") for x in pos), ptr(step_off_dev, torch.int64, "step_off"),
                             step_begin, step_end, pos_begin, pos_end,
                             *(ptr(x, torch.int32, "neg") for x in neg), neg_per_pos, n_ent,
                             ptr(bits, torch.int32, "bits"), bits.numel(), ptr(neg_code, torch.int32, "neg_code"), _stream())
    _check(rc, "mke_neg_codes")


def neg_sample_codes(pos, pos_offset, pos_index, pos_kg, sides, neg_per_pos, max_try, seed, stream_id, code_out):
    """The sampler's code-word form (header section (1c)): mke_neg_sample (pos_index None) or mke_neg_sample_at with neg_r and neg_t
    left out, one word per negative into `code_out`."""
    ph, pr, pt = pos
    head = (ptr(ph, torch.int32, "pos_h"), ptr(pr, torch.int32, "pos_r"), ptr(pt, torch.int32, "pos_t"), ph.numel())
    tail = (ptr(pos_kg, torch.uint8, "pos_kg"), sides, neg_per_pos, max_try, seed[0] & 0xFFFFFFFF, seed[1] & 0xFFFFFFFF,
            stream_id & 0xFFFFFFFF, ptr(code_out, torch.int32, "neg_code"), None, None, _stream())
    if pos_index is None:
        _check(lib().mke_neg_sample(*head, pos_offset, *tail), "mke_neg_sample")
    else:
        _check(lib().mke_neg_sample_at(*head, ptr(pos_index, torch.int32, "pos_index"), *tail), "mke_neg_sample_at")


def neg_codes_inplace(pos, step_off_dev, step_begin, step_end, pos_begin, pos_end, neg_per_pos, n_ent, bits, neg_code):
    """mke_neg_codes without id arrays: `neg_code` holds the words neg_sample_codes wrote and is baked in place; pos: the epoch's."""
    rc = lib().mke_neg_codes(*(ptr(x, torch.int32, "pos") for x in pos), ptr(step_off_dev, torch.int64, "step_off"),
                             step_begin, step_end, pos_begin, pos_end, None, None, None, neg_per_pos, n_ent,
                             ptr(bits, torch.int32, "bits"), bits.numel(), ptr(neg_code, torch.int32, "neg_code"), _stream())
    _check(rc, "mke_neg_codes")


def tripleset_build(h, r, t, keys):
    rc = lib().mke_tripleset_build(ptr(h, torch.int32, "h"), ptr(r, torch.int32, "r"), ptr(t, torch.int32, "t"),
                                   h.numel(), ptr(keys, torch.int64, "keys"), keys.numel(),
                                   _stream())
    _check(rc, "mke_tripleset_build")


def tripleset_forget(keys):
    """Drop the library's prefilter of the table at `keys` (a tensor or a raw address); no-op when it has none."""
    addr = keys if isinstance(keys, int) else keys.data_ptr()
    _check(lib().mke_tripleset_forget(addr), "mke_tripleset_forget")


def tripleset_filter_bytes(keys) -> int:
    """Size of the prefilter the sampler uses for this table; 0 when it has none (the table is probed directly)."""
    return int(lib().mke_tripleset_filter_bytes(ptr(keys, torch.int64, "keys"), keys.numel()))


def epoch_positives(list1, list2, perm1, perm2, b1, b2, n_steps, list1_out, list2_out, pos):
    """mke_epoch_positives: lists [n, 3] int32, perms int64 or None, pos = (pos_h, pos_r, pos_t) int32."""
    i32, i64 = torch.int32, torch.int64
    n1, n2 = list1.shape[0], list2.shape[0]
    need = min(n_steps * b1, n1) + min(n_steps * b2, n2)
    for x in pos:
        if x.numel() < need:
            raise MultiKEHipError(f"epoch buffers hold {x.numel()} positives, the layout needs {need}")
    for pm, n in ((perm1, n1), (perm2, n2)):
        if pm is not None and pm.numel() != n:
            raise MultiKEHipError("a permutation must be as long as its list")
    for o, l in ((list1_out, list1), (list2_out, list2)):
        if o is not None and o.shape != l.shape:
            raise MultiKEHipError("a shuffled list must have its list's shape")
    rc = lib().mke_epoch_positives(ptr(list1, i32, "list1"), ptr(list2, i32, "list2"), n1, n2,
                                   ptr(perm1, i64, "perm1"), ptr(perm2, i64, "perm2"), b1, b2,
                                   n_steps, ptr(list1_out, i32, "list1_out"), ptr(list2_out, i32, "list2_out"),
                                   ptr(pos[0], i32, "pos_h"), ptr(pos[1], i32, "pos_r"), ptr(pos[2], i32, "pos_t"), _stream())
    _check(rc, "mke_epoch_positives")


def tripleset_query(h, r, t, keys, out):
    rc = lib().mke_tripleset_query(ptr(h, torch.int32, "h"), ptr(r, torch.int32, "r"), ptr(t, torch.int32, "t"),
                                   h.numel(), ptr(keys, torch.int64, "keys"), keys.numel(),
                                   ptr(out, torch.uint8, "out"), _stream())
    _check(rc, "mke_tripleset_query")


def gathered_logistic_fwd_bwd(hs, rs, ts, ws, sign, gh, gr, gt, loss_partials):
    n, dim = hs.shape
    rc = lib().mke_gathered_logistic_fwd_bwd(
        ptr(hs, torch.float32, "hs"), ptr(rs, torch.float32, "rs"), ptr(ts, torch.float32, "ts"),
        ptr(ws, torch.float32, "ws"), n, dim, dim, sign,
        ptr(gh, torch.float32, "gh"), ptr(gr, torch.float32, "gr"), ptr(gt, torch.float32, "gt"),
        ptr(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_gathered_logistic_fwd_bwd")


def gathered_alignment_fwd_bwd(a, b, ga, gb, loss_partials):
    n, dim = a.shape
    rc = lib().mke_gathered_alignment_fwd_bwd(
        ptr(a, torch.float32, "a"), ptr(b, torch.float32, "b"), n, dim, dim,
        ptr(ga, torch.float32, "ga"), ptr(gb, torch.float32, "gb"),
        ptr(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_gathered_alignment_fwd_bwd")


def align_fwd_bwd(table_a, a_normalize, table_b, b_normalize, dim, ia, ib, weight, grad_a, touched_a, grad_b, touched_b,
                  tag, loss_partials):
    rc = lib().mke_align_fwd_bwd(
        ptr(table_a, torch.float32, "table_a"), int(a_normalize), ptr(table_b, torch.float32, "table_b"),
        int(b_normalize), table_a.shape[1], dim, ptr(ia, torch.int32, "ia"),
        ptr(ib, torch.int32, "ib"), ia.numel(), weight, ptr(grad_a, torch.float32, "grad_a"),
        ptr(touched_a, torch.int32, "touched_a"), ptr(grad_b, torch.float32, "grad_b"),
        ptr(touched_b, torch.int32, "touched_b"), tag, ptr(loss_partials, torch.float64, "loss_partials"),
        _stream())
    _check(rc, "mke_align_fwd_bwd")


def gather_rows(table, normalize, dim, idx, out):
    n = out.shape[0]
    rc = lib().mke_gather_rows(ptr(table, torch.float32, "table"), int(normalize), table.shape[1],
                               dim, ptr(idx, torch.int32, "idx"), n,
                               ptr(out, torch.float32, "out"), _stream())
    _check(rc, "mke_gather_rows")


def probe_rows(a, b, c, idx, out):
    """mke_probe_rows: rows idx of a (and b, c when given) read together; out [len(idx)] float32."""
    rc = lib().mke_probe_rows(ptr(a, torch.float32, "a"), ptr(b, torch.float32, "b"), ptr(c, torch.float32, "c"),
                              a.shape[1], ptr(idx, torch.int32, "idx"), idx.numel(),
                              ptr(out, torch.float32, "out"), _stream())
    _check(rc, "mke_probe_rows")


def rowset_build(streams, flags, counts, req, id_map, overflow, n_ranks, capacity):
    """streams: up to four int32 id tensors."""
    args = []
    for k in range(4):
        t = streams[k] if k < len(streams) else None
        args += [ptr(t, torch.int32, f"ids{k}"), 0 if t is None else t.numel()]
    rc = lib().mke_rowset_build(*args, ptr(flags, torch.int32, "flags"), ptr(counts, torch.int32, "counts"),
                                ptr(req, torch.int32, "req"), ptr(id_map, torch.int32, "id_map"),
                                ptr(overflow, torch.int32, "overflow"), n_ranks, capacity, _stream())
    _check(rc, "mke_rowset_build")


def rowset_remap(streams, outs, id_map, flags, reset_req=None, reset_counts=None, want=None, slot_of=None, n_ranks=0,
                 capacity=0):
    args = []
    for k in range(4):
        t = streams[k] if k < len(streams) else None
        o = outs[k] if k < len(outs) else None
        args += [ptr(t, torch.int32, f"ids{k}"), ptr(o, torch.int32, f"out{k}"), 0 if t is None else t.numel()]
    rc = lib().mke_rowset_remap(*args, ptr(id_map, torch.int32, "id_map"), ptr(flags, torch.int32, "flags"),
                                ptr(reset_req, torch.int32, "reset_req"), 0 if reset_req is None else reset_req.numel(),
                                ptr(reset_counts, torch.int32, "reset_counts"),
                                0 if reset_counts is None else reset_counts.numel(),
                                ptr(want, torch.int32, "want"), ptr(slot_of, torch.int32, "slot_of"), n_ranks,
                                capacity, _stream())
    _check(rc, "mke_rowset_remap")


def rows_gather_padded(table, idx, out, zero_rows=None):
    rc = lib().mke_rows_gather_padded(ptr(table, torch.float32, "table"), table.shape[1],
                                      ptr(idx, torch.int32, "idx"), idx.numel(),
                                      ptr(out, torch.float32, "out"), ptr(zero_rows, torch.float32, "zero_rows"), _stream())
    _check(rc, "mke_rows_gather_padded")


def rows_scatter_add(idx, rows, dim, grad, touched, tag, reset_req=None, reset_counts=None):
    rc = lib().mke_rows_scatter_add(ptr(idx, torch.int32, "idx"), ptr(rows, torch.float32, "rows"),
                                    idx.numel(), grad.shape[1], dim,
                                    ptr(grad, torch.float32, "grad"), ptr(touched, torch.int32, "touched"), tag,
                                    ptr(reset_req, torch.int32, "reset_req"), ptr(reset_counts, torch.int32, "reset_counts"),
                                    0 if reset_counts is None else reset_counts.numel(), _stream())
    _check(rc, "mke_rows_scatter_add")


def cnn_conv_params(dim: int) -> int:
    return 2 * dim + 52


def cnn_params(dim: int) -> int:
    return cnn_conv_params(dim) + 4 * dim * dim + dim


def attr_conv_fwd(attr, attr_normalize, lit, dim, ia, iv, params, flat):
    rc = lib().mke_attr_conv_fwd(ptr(attr, torch.float32, "attr_table"), attr.shape[1], int(attr_normalize),
                                 ptr(lit, torch.float32, "lit_table"), lit.shape[1], dim,
                                 ptr(ia, torch.int32, "ia"), ptr(iv, torch.int32, "iv"), ia.numel(),
                                 ptr(params, torch.float32, "params"), ptr(flat, torch.float32, "flat"),
                                 flat.shape[1], _stream())
    _check(rc, "mke_attr_conv_fwd")


def cnn_workspace_floats(dim: int) -> int:
    """MKE_CNN_WORKSPACE_FLOATS(dim)"""
    return 32 * (2 * dim + 64)


def attr_conv_bwd(attr, attr_normalize, lit, dim, ia, iv, params, dflat, grad_params, grad_attr, touched_attr, tag,
                  workspace=None):
    rc = lib().mke_attr_conv_bwd(ptr(attr, torch.float32, "attr_table"), attr.shape[1], int(attr_normalize),
                                 ptr(lit, torch.float32, "lit_table"), lit.shape[1], dim,
                                 ptr(ia, torch.int32, "ia"), ptr(iv, torch.int32, "iv"), ia.numel(),
                                 ptr(params, torch.float32, "params"), ptr(dflat, torch.float32, "dflat"),
                                 ptr(grad_params, torch.float32, "grad_params"), ptr(grad_attr, torch.float32, "grad_attr"),
                                 ptr(touched_attr, torch.int32, "touched_attr"), tag,
                                 ptr(workspace, torch.float32, "workspace"), _stream())
    _check(rc, "mke_attr_conv_bwd")


def attr_tail_z(z, bias, sumsq_partials):
    n, dim = z.shape
    rc = lib().mke_attr_tail_z(ptr(z, torch.float32, "z"), ptr(bias, torch.float32, "bias"), n, dim,
                               ptr(sumsq_partials, torch.float64, "sumsq_partials"), _stream())
    _check(rc, "mke_attr_tail_z")


def attr_tail_loss(z, sumsq_partials, ent, ent_normalize, ih, weights, scale, gout, dot_partials, grad_ent, touched_ent, tag,
                   loss_partials):
    n, dim = z.shape
    rc = lib().mke_attr_tail_loss(ptr(z, torch.float32, "z"), ptr(sumsq_partials, torch.float64, "sumsq"),
                                  ptr(ent, torch.float32, "ent_table"), ent.shape[1], int(ent_normalize),
                                  ptr(ih, torch.int32, "ih"), ptr(weights, torch.float32, "weights"), scale,
                                  n, dim, ptr(gout, torch.float32, "gout"),
                                  ptr(dot_partials, torch.float64, "dot_partials"), ptr(grad_ent, torch.float32, "grad_ent"),
                                  ptr(touched_ent, torch.int32, "touched_ent"), tag,
                                  ptr(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_attr_tail_loss")


def attr_tail_bwd(z, gout, sumsq_partials, dot_partials, grad_bias=None):
    n, dim = z.shape
    rc = lib().mke_attr_tail_bwd(ptr(z, torch.float32, "z"), ptr(gout, torch.float32, "gout"),
                                 ptr(sumsq_partials, torch.float64, "sumsq"), ptr(dot_partials, torch.float64, "dot"),
                                 n, dim, ptr(grad_bias, torch.float32, "grad_bias"), _stream())
    _check(rc, "mke_attr_tail_bwd")


def dense_update(param, acc, grad, optimizer, lr):
    rc = lib().mke_dense_update(ptr(param, torch.float32, "param"), ptr(acc, torch.float32, "acc"),
                                ptr(grad, torch.float32, "grad"), param.numel(), optimizer, lr,
                                _stream())
    _check(rc, "mke_dense_update")


def oc_block_floats(capacity: int, stride: int) -> int:
    return int(lib().mke_oc_block_floats(capacity, stride))


def oc_pack_codes(pos_h, neg_h, neg_t, neg_per_pos: int, codes):
    rc = lib().mke_oc_pack_codes(ptr(pos_h, torch.int32, "pos_h"), ptr(neg_h, torch.int32, "neg_h"),
                                 ptr(neg_t, torch.int32, "neg_t"), pos_h.numel(), neg_per_pos,
                                 ptr(codes, torch.int32, "codes"), _stream())
    _check(rc, "mke_oc_pack_codes")


OC_CODE_MASK = 0x3FFFFFFF       # a code without its OC_NEED_* group flags


def oc_plan(pos_h, pos_t, codes, neg_per_pos: int, part_lo, n_parts: int, n_ranks: int, rank: int, slot_h, slot_t, own_h, own_t, counts):
    """The epoch's slots / owned lists / per-(part, owner) counts in one launch (mke_oc_plan); `codes`: the whole epoch's codes
    by epoch position (their group flags say which vector a positive needs), None when neg_per_pos == 0."""
    i32 = torch.int32
    rc = lib().mke_oc_plan(ptr(pos_h, i32, "pos_h"), ptr(pos_t, i32, "pos_t"),
                           ptr(codes, i32, "codes") if neg_per_pos else None, neg_per_pos, ptr(part_lo, torch.int64, "part_lo"),
                           n_parts, n_ranks, rank, ptr(slot_h, i32, "slot_h"), ptr(slot_t, i32, "slot_t"),
                           ptr(own_h, i32, "own_h"), ptr(own_t, i32, "own_t"), ptr(counts, i32, "counts"), _stream())
    _check(rc, "mke_oc_plan")


OC_REC_INTS = 3     # an owned-code record: (epoch position, n, code without flags), int32 each


def oc_bucket_codes(codes, n_mine: int, neg_per_pos: int, pos0: int, n_ranks: int, cap: int, need, send, counts, scratch):
    """mke_oc_bucket_codes: this rank's share of the epoch's codes bucketed by the owner of the corrupt entity ((position, n) order
    inside each destination, true counts), and the positions' need flags alone."""
    i32 = torch.int32
    if scratch.numel() < n_ranks * OC_BUCKET_WAVES or counts.numel() < n_ranks or need.numel() < n_mine or send.numel() < OC_REC_INTS * n_ranks * cap:
        raise MultiKEHipError("mke_oc_bucket_codes: need / send / counts / scratch too small")
    rc = lib().mke_oc_bucket_codes(ptr(codes, i32, "codes"), n_mine, neg_per_pos, pos0, n_ranks,
                                   cap, ptr(need, i32, "need"), ptr(send, i32, "send"), ptr(counts, i32, "counts"),
                                   ptr(scratch, i32, "scratch"), _stream())
    _check(rc, "mke_oc_bucket_codes")


def oc_owned_index(recv, counts, n_ranks: int, cap: int, n_all: int, own_rec, own_off):
    """mke_oc_owned_index: the records addressed to this rank packed in (position, n) order, and their offsets per epoch position."""
    i32 = torch.int32
    if own_rec.numel() < OC_REC_INTS * n_ranks * cap or own_off.numel() < n_all + 1 or recv.numel() < OC_REC_INTS * n_ranks * cap or counts.numel() < n_ranks:
        raise MultiKEHipError("mke_oc_owned_index: recv / counts / own_rec / own_off too small")
    rc = lib().mke_oc_owned_index(ptr(recv, i32, "recv"), ptr(counts, i32, "counts"), n_ranks, cap, n_all,
                                  ptr(own_rec, i32, "own_rec"), ptr(own_off, i32, "own_off"), _stream())
    _check(rc, "mke_oc_owned_index")


def oc_em_plan_temp_bytes(capacity: int) -> int:
    n = lib().mke_oc_em_plan_temp_bytes(capacity)
    if n < 0:
        raise MultiKEHipError("mke_oc_em_plan_temp_bytes: capacity out of range")
    return int(n)


def oc_em_plan(args: OcEmPlanArgs):
    """mke_oc_em_plan: the epoch's references to this rank's rows, sorted by (step, row) — struct of raw device addresses."""
    _check(lib().mke_oc_em_plan(C.byref(args), _stream()), "mke_oc_em_plan")


def oc_steps(loop: OcLoopStruct, step_begin: int, step_end: int):
    """mke_oc_steps: global steps [step_begin, step_end) of the current epoch enqueued by one native call."""
    _check(lib().mke_oc_steps(C.byref(loop), step_begin, step_end, _stream()), "mke_oc_steps")


def oc_pass2(step: OcStepStruct):
    _check(lib().mke_oc_pass2(C.byref(step), _stream()), "mke_oc_pass2")


def oc_gv_sum(step: OcStepStruct, inbox, gv):
    """mke_oc_gv_sum: the writers' slices of this rank's gradient inbox summed, in rank order, into the local block `gv`
    (peer-direct entity-major steps only)."""
    rc = lib().mke_oc_gv_sum(C.byref(step), ptr(inbox, torch.float32, "inbox"), ptr(gv, torch.float32, "gv"), _stream())
    _check(rc, "mke_oc_gv_sum")


def oc_run(step: OcStepStruct, phases: int, send, v_all, block_floats: int, g_all, gv, loss_partials):
    """mke_oc_run with RAW device addresses (ints / None) — the caller validated the tensors once per epoch."""
    rc = lib().mke_oc_run(C.byref(step), phases, send, v_all, block_floats,
                          g_all, gv, loss_partials, _stream())
    _check(rc, "mke_oc_run")


def ae_scratch_floats(plan: AEPlanStruct, rows: int) -> int:
    n = lib().mke_ae_scratch_floats(C.byref(plan), rows)
    if n < 0:
        raise MultiKEHipError("mke_ae_scratch_floats: bad plan")
    return int(n)


def ae_train_steps(plan: AEPlanStruct, x: torch.Tensor, batch_rows: int, loss_out: torch.Tensor):
    """mke_ae_train_steps over the rows of x (float32 [n, ldx] CUDA, row-major); loss_out: float64 [n_batches]."""
    rc = lib().mke_ae_train_steps(C.byref(plan), ptr(x, torch.float32, "x"), x.shape[0], x.stride(0),
                                  batch_rows, ptr(loss_out, torch.float64, "loss_out"), _stream())
    _check(rc, "mke_ae_train_steps")


def ae_step_phases(plan: AEPlanStruct, x, rows: int, ldx: int, global_rows: int, phases: int, loss_out: torch.Tensor):
    """mke_ae_step_phases: one batch of the auto-encoder cut at its batch-wide sums (x: float32 [rows, ldx] CUDA or None)."""
    rc = lib().mke_ae_step_phases(C.byref(plan), (ptr(x, torch.float32, "x") if rows else None), rows, ldx,
                                  global_rows, phases, ptr(loss_out, torch.float64, "loss_out"), _stream())
    _check(rc, "mke_ae_step_phases")


def ae_encode(plan: AEPlanStruct, x: torch.Tensor, out: torch.Tensor):
    rc = lib().mke_ae_encode(C.byref(plan), ptr(x, torch.float32, "x"), x.shape[0], x.stride(0),
                             ptr(out, torch.float32, "out"), out.stride(0), _stream())
    _check(rc, "mke_ae_encode")


def dense_layer_fwd(x: torch.Tensor, w: torch.Tensor, b, act: int, out: torch.Tensor):
    """out = act(x @ w + b) on the hand-written MFMA GEMM (bias / activation in its epilogue)."""
    M, K = x.shape
    K2, N = w.shape
    if K != K2 or tuple(out.shape) != (M, N) or x.stride(1) != 1 or w.stride(1) != 1 or out.stride(1) != 1:
        raise MultiKEHipError(f"dense_layer_fwd: shapes {tuple(x.shape)} x {tuple(w.shape)} -> {tuple(out.shape)} (row-major)")
    for t, nm in ((x, "x"), (w, "w"), (out, "out")):       # row-major with any row stride (padded rows are not "contiguous")
        if not t.is_cuda or t.dtype != torch.float32:
            raise MultiKEHipError(f"dense_layer_fwd: {nm} must be a float32 CUDA tensor")
    rc = lib().mke_dense_layer_fwd(x.data_ptr(), x.stride(0), w.data_ptr(),
                                   w.stride(0), ptr(b, torch.float32, "b"), act,
                                   out.data_ptr(), out.stride(0), M, N, K,
                                   _stream())
    _check(rc, "mke_dense_layer_fwd")


def align_rank(emb1, emb2, kpad, n1, n2, rank, best, ties=None):
    """mke_align_rank over row-major padded emb1 [n1, ld1] / emb2 [n2, ld2]."""
    rc = lib().mke_align_rank(ptr(emb1, torch.float32, "emb1"), emb1.shape[1], ptr(emb2, torch.float32, "emb2"),
                              emb2.shape[1], kpad, n1, n2,
                              ptr(rank, torch.int32, "rank"), ptr(ties, torch.int32, "ties"), ptr(best, torch.int64, "best"),
                              _stream())
    _check(rc, "mke_align_rank")


def align_topk_mean_temp_bytes(n_a: int, n_b: int, kpad: int, k: int) -> int:
    """mke_align_topk_mean_temp_bytes; raises on the arguments mke_align_topk_mean would reject."""
    r = int(lib().mke_align_topk_mean_temp_bytes(n_a, n_b, kpad, k))
    _check(r if r < 0 else 0, "mke_align_topk_mean_temp_bytes")
    return r


def align_topk_mean(a, b, kpad, k, metric=METRIC_INNER, sq_a=None, sq_b=None):
    """mke_align_topk_mean over row-major padded a [n_a, lda] / b [n_b, ldb] -> float32 [n_a]: the mean of each a row's k
    largest similarities to the b rows."""
    n_a, n_b = a.shape[0], b.shape[0]
    need = align_topk_mean_temp_bytes(n_a, n_b, kpad, k)
    out = torch.empty(n_a, dtype=torch.float32, device=a.device)
    temp = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=a.device)
    args = TopkMeanArgs(ptr(a, torch.float32, "a"), a.shape[1], ptr(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                        ptr(sq_a, torch.float32, "sq_a"), ptr(sq_b, torch.float32, "sq_b"), k, ptr(out, torch.float32, "out"),
                        ptr(temp, torch.float32, "temp"), temp.numel() * 4)
    _check(lib().mke_align_topk_mean(C.byref(args), _stream()), "mke_align_topk_mean")
    return out


def align_rank_ex(emb1, emb2, kpad, rank, ties, best, metric=METRIC_INNER, sq1=None, sq2=None, csls_row=None, csls_col=None):
    """mke_align_rank_ex over row-major padded emb1 [n1, ld1] / emb2 [n2, ld2] (rank / ties / best zeroed by the caller)."""
    args = AlignArgs(ptr(emb1, torch.float32, "emb1"), emb1.shape[1], ptr(emb2, torch.float32, "emb2"), emb2.shape[1], kpad,
                     emb1.shape[0], emb2.shape[0], metric, ptr(sq1, torch.float32, "sq1"), ptr(sq2, torch.float32, "sq2"),
                     ptr(csls_row, torch.float32, "csls_row"), ptr(csls_col, torch.float32, "csls_col"),
                     ptr(rank, torch.int32, "rank"), ptr(ties, torch.int32, "ties"), ptr(best, torch.int64, "best"))
    _check(lib().mke_align_rank_ex(C.byref(args), _stream()), "mke_align_rank_ex")


def align_lse_temp_bytes(n_a: int, n_b: int, kpad: int) -> int:
    """mke_align_lse_temp_bytes; raises on the arguments mke_align_lse would reject."""
    r = int(lib().mke_align_lse_temp_bytes(n_a, n_b, kpad))
    _check(r if r < 0 else 0, "mke_align_lse_temp_bytes")
    return r


def align_lse(a, b, kpad, tau, metric=METRIC_INNER, sq_a=None, sq_b=None, sub_b=None, out=None):
    """mke_align_lse over row-major padded a [n_a, lda] / b [n_b, ldb] -> float32 [n_a]: tau log sum_j exp((sim(i, j) -
    sub_b[j]) / tau), sub_b None = zeros.  `out` (float32, at least n_a long) is written in its first n_a entries."""
    n_a, n_b = a.shape[0], b.shape[0]
    need = align_lse_temp_bytes(n_a, n_b, kpad)
    if out is None:
        out = torch.empty(n_a, dtype=torch.float32, device=a.device)
    elif out.numel() < n_a:
        raise MultiKEHipError(f"align_lse: out holds {out.numel()} floats, {n_a} rows")
    temp = torch.empty(max(need, 8) // 4, dtype=torch.float32, device=a.device)
    args = LseArgs(ptr(a, torch.float32, "a"), a.shape[1], ptr(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                   ptr(sq_a, torch.float32, "sq_a"), ptr(sq_b, torch.float32, "sq_b"), ptr(sub_b, torch.float32, "sub_b"),
                   float(tau), ptr(out, torch.float32, "out"), ptr(temp, torch.float32, "temp"), temp.numel() * 4)
    _check(lib().mke_align_lse(C.byref(args), _stream()), "mke_align_lse")
    return out


def stable_lists_temp_bytes(n_a: int, n_b: int, kpad: int, cut: int, whole_rows: bool = False) -> int:
    """mke_stable_lists_temp_bytes; raises on the arguments mke_stable_lists would reject."""
    r = int(lib().mke_stable_lists_temp_bytes(n_a, n_b, kpad, cut, int(whole_rows)))
    _check(r if r < 0 else 0, "mke_stable_lists_temp_bytes")
    return r


def stable_lists(a, b, kpad, cut, metric=METRIC_INNER, sq_a=None, sq_b=None, csls_row=None, csls_col=None, sim_mat=None,
                 whole_rows=False, sample_cols=0):
    """mke_stable_lists -> (val float32 [n_a, cut], col int32 [n_a, cut], flags int32 [n_a]): per row of a its `cut` best
    columns of b (value descending, column ascending; short lists padded with column -1).  Rows with flags == 1 are NOT
    valid: the caller redoes them with whole_rows = True (base.alignment.candidate_lists does).  With `sim_mat` (float32
    [n_a, >= n_b] on the device) the operands are ignored and the caller's similarities are used."""
    if sim_mat is not None:
        n_a, n_b, dev = sim_mat.shape[0], sim_mat.shape[1], sim_mat.device
        if sim_mat.stride(1) != 1 and sim_mat.numel() > 0:
            raise MultiKEHipError("stable_lists: sim_mat must be row-major")
        whole_rows = True
    else:
        n_a, n_b, dev = a.shape[0], b.shape[0], a.device
    need = stable_lists_temp_bytes(n_a, n_b, kpad if sim_mat is None else 16, cut, whole_rows)
    val = torch.empty(n_a, cut, dtype=torch.float32, device=dev)
    col = torch.empty(n_a, cut, dtype=torch.int32, device=dev)
    flags = torch.zeros(n_a, dtype=torch.int32, device=dev)
    temp = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=dev)
    args = StableListsArgs()
    if sim_mat is None:
        args.a, args.lda, args.b, args.ldb = ptr(a, torch.float32, "a"), a.shape[1], ptr(b, torch.float32, "b"), b.shape[1]
        args.kpad, args.metric = kpad, metric
        args.sq_a, args.sq_b = ptr(sq_a, torch.float32, "sq_a"), ptr(sq_b, torch.float32, "sq_b")
        args.csls_row, args.csls_col = ptr(csls_row, torch.float32, "csls_row"), ptr(csls_col, torch.float32, "csls_col")
    else:
        if not sim_mat.is_cuda or sim_mat.dtype != torch.float32:
            raise MultiKEHipError("stable_lists: sim_mat must be a float32 CUDA/HIP tensor (no CPU path exists)")
        args.sim_mat, args.ld_sim = sim_mat.data_ptr(), sim_mat.stride(0) if n_a > 1 else max(n_b, 1)
    args.n_a, args.n_b, args.cut, args.whole_rows, args.sample_cols = n_a, n_b, cut, int(bool(whole_rows)), sample_cols
    args.out_val, args.out_col = ptr(val, torch.float32, "out_val"), ptr(col, torch.int32, "out_col")
    args.flags, args.temp, args.temp_bytes = ptr(flags, torch.int32, "flags"), ptr(temp, torch.int64, "temp"), temp.numel() * 8
    _check(lib().mke_stable_lists(C.byref(args), _stream()), "mke_stable_lists")
    return val, col, flags


def stable_match_args(val, col, n_b, ptr, holder, proposals, match=None, counts=None) -> StableMatchArgs:
    """mke_stable_match_args over the lists val / col [n_a, cut] and the state ptr [n_a] int32, holder [n_b] int64,
    proposals [n] int32 (all zeroed before round 0); match [n_a] int32 and counts [2] int32 for stable_finish."""
    n_a, cut = col.shape
    return StableMatchArgs(n_a, n_b, cut, _dev(val, torch.float32, "val"), _dev(col, torch.int32, "col"),
                           _dev(ptr, torch.int32, "ptr"), _dev(holder, torch.int64, "holder"),
                           _dev(proposals, torch.int32, "proposals"), proposals.numel() if proposals is not None else 0,
                           _dev(match, torch.int32, "match"), _dev(counts, torch.int32, "counts"))


def stable_rounds(args: StableMatchArgs, first_round: int, n_rounds: int):
    """mke_stable_rounds: enqueue rounds first_round .. first_round + n_rounds - 1 (no synchronisation)."""
    _check(lib().mke_stable_rounds(C.byref(args), first_round, n_rounds, _stream()), "mke_stable_rounds")


def stable_finish(args: StableMatchArgs):
    """mke_stable_finish: match[i] = the column holding suitor i or -1; counts = (matched, matched to its own index)."""
    _check(lib().mke_stable_finish(C.byref(args), _stream()), "mke_stable_finish")


def align_mutual(a, b, kpad, metric=METRIC_INNER, sq_a=None, sq_b=None, csls_row=None, csls_col=None, flags=0, out=None):
    """mke_align_mutual over row-major padded a [n_a, lda] / b [n_b, ldb] -> (row_best int64 [n_a], col_best int64 [n_b]):
    per row the packed (re-scored similarity, best column), per column the packed (same similarity, best row), from one
    sweep.  `out` = (row_best, col_best) zeroed by the caller, in place of fresh tensors."""
    n_a, n_b = a.shape[0], b.shape[0]
    row_best, col_best = out if out is not None else (torch.zeros(n_a, dtype=torch.int64, device=a.device),
                                                      torch.zeros(n_b, dtype=torch.int64, device=a.device))
    if row_best.numel() < n_a or col_best.numel() < n_b:
        raise MultiKEHipError(f"align_mutual: out holds ({row_best.numel()}, {col_best.numel()}) words, ({n_a}, {n_b}) rows and columns")
    args = MutualArgs(ptr(a, torch.float32, "a"), a.shape[1], ptr(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                      ptr(sq_a, torch.float32, "sq_a"), ptr(sq_b, torch.float32, "sq_b"),
                      ptr(csls_row, torch.float32, "csls_row"), ptr(csls_col, torch.float32, "csls_col"),
                      ptr(row_best, torch.int64, "row_best"), ptr(col_best, torch.int64, "col_best"), flags)
    _check(lib().mke_align_mutual(C.byref(args), _stream()), "mke_align_mutual")
    return row_best, col_best


def mutual_pairs(row_best, col_best, threshold=float("-inf")):
    """mke_mutual_pairs over the words of align_mutual -> (match int32 [n_a], counts int32 [2]): match[i] = the column whose best
    row is i and that is i's best column, at a value >= threshold, else -1; counts = (matched, matched to its own index)."""
    n_a, n_b = row_best.numel(), col_best.numel()
    match = torch.empty(n_a, dtype=torch.int32, device=row_best.device)
    counts = torch.empty(2, dtype=torch.int32, device=row_best.device)     # zeroed by the call
    rc = lib().mke_mutual_pairs(ptr(row_best, torch.int64, "row_best"), ptr(col_best, torch.int64, "col_best"), n_a,
                                n_b, threshold, ptr(match, torch.int32, "match"),
                                ptr(counts, torch.int32, "counts"), _stream())
    _check(rc, "mke_mutual_pairs")
    return match, counts


ASSIGN_TAIL_MAX = 4096                     # tail_cap values above this act as it (ASSIGN_TAIL_CAP: the default hand-over point)
ASSIGN_MIN_EPS = 2.0 ** -14


def assign_temp_bytes(n_a: int, n_b: int, tail_cap: int = 0) -> int:
    """mke_assign_temp_bytes; raises on the arguments mke_assign_rounds would reject."""
    r = int(lib().mke_assign_temp_bytes(n_a, n_b, tail_cap))
    _check(r if r < 0 else 0, "mke_assign_temp_bytes")
    return r


def assign_args(val, col, n_b, eps, floor, state, price, owner, bid, progress, temp, tail_cap=0, flags=0, match=None,
                counts=None) -> AssignArgs:
    """mke_assign_args over the lists val / col [n_a, cut] and the state of a run: state [n_a] int32, price [n_b] float32,
    owner [n_b] int32, bid [n_b] int64, progress [4] int64 (all zeroed before the first round), temp (int32, at least
    assign_temp_bytes); match [n_a] int32 and counts [3] int32 for assign_finish."""
    n_a, cut = col.shape
    return AssignArgs(n_a, n_b, cut, ptr(val, torch.float32, "val"), ptr(col, torch.int32, "col"), float(eps), float(floor),
                      ptr(state, torch.int32, "state"), ptr(price, torch.float32, "price"), ptr(owner, torch.int32, "owner"),
                      ptr(bid, torch.int64, "bid"), ptr(progress, torch.int64, "progress"), tail_cap, flags,
                      ptr(temp, torch.int32, "temp"), temp.numel() * 4 if temp is not None else 0,
                      ptr(match, torch.int32, "match"), ptr(counts, torch.int32, "counts"))


def assign_rounds(args: AssignArgs, n_rounds: int):
    """mke_assign_rounds: enqueue at most n_rounds more rounds of the auction (no synchronisation)."""
    _check(lib().mke_assign_rounds(C.byref(args), n_rounds, _stream()), "mke_assign_rounds")


def assign_finish(args: AssignArgs):
    """mke_assign_finish: match[i] = the column row i holds or -1; counts = (matched, matched to its own index, settled unmatched)."""
    _check(lib().mke_assign_finish(C.byref(args), _stream()), "mke_assign_finish")


def boot_partner(match, ids_a, ids_b, n_entities: int, out=None):
    """mke_boot_partner -> partner int32 [n_entities]: -1 everywhere, then partner[ids_a[i]] = ids_b[match[i]] and back for every
    matched row i of the one-to-one `match` int32 [n_a] (-1 = unmatched).  `out` = a table to overwrite instead of a fresh one."""
    partner = out if out is not None else torch.empty(n_entities, dtype=torch.int32, device=match.device)
    if partner.numel() != n_entities:
        raise MultiKEHipError(f"boot_partner: out holds {partner.numel()} words, the table has {n_entities}")
    if match.numel() != ids_a.numel():
        raise MultiKEHipError(f"boot_partner: match has {match.numel()} rows, ids_a {ids_a.numel()}")
    rc = lib().mke_boot_partner(ptr(match, torch.int32, "match"), ptr(ids_a, torch.int32, "ids_a"), ids_a.numel(),
                                ptr(ids_b, torch.int32, "ids_b"), ids_b.numel(), ptr(partner, torch.int32, "partner"),
                                n_entities, _stream())
    _check(rc, "mke_boot_partner")
    return partner


def swap_temp_bytes(n: int) -> int:
    """mke_swap_temp_bytes; raises on an n mke_swap_triples would reject."""
    r = int(lib().mke_swap_temp_bytes(n))
    _check(r if r < 0 else 0, "mke_swap_temp_bytes")
    return r


def swap_triples(h, p, t, partner, heads_only=False, weight=None, capacity=None, out=None):
    """mke_swap_triples over the int32 columns h, p, t [n] and the link table `partner` int32 [n_entities] -> ((out_h, out_p,
    out_t), out_w or None, count int64 [1] on the device): the 'swapping' supervision entries in the order of the walk over the
    list.  capacity: None = the worst case (2 n, or n with heads_only); entries past it are counted, not stored.  `out` =
    (out_h, out_p, out_t, out_w or None) of at least `capacity` words instead of fresh tensors.  Nothing is read back here."""
    n = h.numel()
    if p.numel() != n or t.numel() != n:
        raise MultiKEHipError(f"swap_triples: columns of {n}, {p.numel()}, {t.numel()} triples")
    cap = (n if heads_only else 2 * n) if capacity is None else int(capacity)
    dev = h.device
    if out is None:
        out = tuple(torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)) + (
            None if weight is None else torch.empty(cap, dtype=torch.float32, device=dev),)
    out_h, out_p, out_t, out_w = out
    if min(x.numel() for x in out if x is not None) < cap:
        raise MultiKEHipError(f"swap_triples: out is shorter than the capacity {cap}")
    if weight is not None and weight.numel() != partner.numel():
        raise MultiKEHipError(f"swap_triples: weight has {weight.numel()} entries, partner {partner.numel()}")
    count = torch.empty(1, dtype=torch.int64, device=dev)
    temp = torch.empty((swap_temp_bytes(n) + 7) // 8, dtype=torch.int64, device=dev)
    args = SwapArgs(ptr(h, torch.int32, "h"), ptr(p, torch.int32, "p"), ptr(t, torch.int32, "t"), n,
                    ptr(partner, torch.int32, "partner"), partner.numel(), ptr(weight, torch.float32, "weight"),
                    1 if heads_only else 0, ptr(out_h, torch.int32, "out_h"), ptr(out_p, torch.int32, "out_p"),
                    ptr(out_t, torch.int32, "out_t"), ptr(out_w, torch.float32, "out_w"), cap, ptr(count, torch.int64, "count"),
                    ptr(temp, torch.int64, "temp"), temp.numel() * 8, 0)
    _check(lib().mke_swap_triples(C.byref(args), _stream()), "mke_swap_triples")
    return (out_h, out_p, out_t), out_w, count


def gemm_f32(lhs, rhs, out, transpose_a=False, transpose_b=False, splits=1, accumulate=False):
    """out (=|+=) op(lhs) @ op(rhs) for 2-D float32 CUDA tensors of any strides; `out` row-major."""
    a = lhs.t() if transpose_a else lhs
    b = rhs.t() if transpose_b else rhs
    M, K = a.shape
    K2, N = b.shape
    if K != K2 or tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise MultiKEHipError(f"gemm_f32: shapes {tuple(a.shape)} x {tuple(b.shape)} -> {tuple(out.shape)}")
    for t, nm in ((lhs, "lhs"), (rhs, "rhs"), (out, "out")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise MultiKEHipError(f"gemm_f32: {nm} must be a float32 CUDA tensor")
    rc = lib().mke_gemm_f32(a.data_ptr(), a.stride(0), a.stride(1),
                            b.data_ptr(), b.stride(0), b.stride(1),
                            out.data_ptr(), out.stride(0), M, N, K,
                            splits, int(accumulate), _stream())
    _check(rc, "mke_gemm_f32")


def rows_update_dense(table, slot1, slot2, grad, dim, normalize, opt: OptimizerStruct):
    """mke_rows_update_dense: Adam / Adadelta over EVERY row of the table (grad consumed)."""
    rc = lib().mke_rows_update_dense(ptr(table, torch.float32, "table"), ptr(slot1, torch.float32, "slot1"),
                                     ptr(slot2, torch.float32, "slot2"), ptr(grad, torch.float32, "grad"),
                                     table.shape[0], table.shape[1], dim, int(normalize),
                                     C.byref(opt), _stream())
    _check(rc, "mke_rows_update_dense")


def dense_update_opt(param, slot1, slot2, grad, opt: OptimizerStruct):
    """mke_dense_update_opt: Adam / Adadelta over a flat parameter buffer (grad consumed)."""
    rc = lib().mke_dense_update_opt(ptr(param, torch.float32, "param"), ptr(slot1, torch.float32, "slot1"),
                                    ptr(slot2, torch.float32, "slot2"), ptr(grad, torch.float32, "grad"),
                                    param.numel(), C.byref(opt), _stream())
    _check(rc, "mke_dense_update_opt")


def attr_scratch_floats(n: int, dim: int) -> int:
    return int(lib().mke_attr_scratch_floats(n, dim))


def attr_steps(args: AttrStepArgs, step_off: np.ndarray, loss_ring: torch.Tensor):
    """mke_attr_steps: `step_off` host int64 [n_steps + 1]; loss_ring float64 [ring, LOSS_PARTIALS] on the device."""
    off = np.ascontiguousarray(step_off, dtype=np.int64)
    rc = lib().mke_attr_steps(C.byref(args), off.ctypes.data, len(off) - 1,
                              ptr(loss_ring, torch.float64, "loss_ring"), loss_ring.shape[0], _stream())
    _check(rc, "mke_attr_steps")


def sample_distinct(n: int, batch: int, n_steps: int, seed=(0, 0), stream_id: int = 0, device="cuda") -> torch.Tensor:
    """mke_sample_distinct -> int32 [n_steps, batch]: `batch` distinct positions of range(n) per step."""
    out = torch.empty(n_steps, batch, dtype=torch.int32, device=device)
    rc = lib().mke_sample_distinct(n, batch, n_steps, seed[0] & 0xFFFFFFFF,
                                   seed[1] & 0xFFFFFFFF, stream_id & 0xFFFFFFFF,
                                   ptr(out, torch.int32, "out"), _stream())
    _check(rc, "mke_sample_distinct")
    return out


def attr_step_phases(args: AttrStepArgs, phases: int):
    rc = lib().mke_attr_step_phases(C.byref(args), phases, _stream())
    _check(rc, "mke_attr_step_phases")


def attr_step(args: AttrStepArgs):
    rc = lib().mke_attr_step(C.byref(args), _stream())
    _check(rc, "mke_attr_step")
