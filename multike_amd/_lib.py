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

LOSS_PARTIALS = 2048  # MKE_LOSS_PARTIALS
MAX_STRIDE = 320  # MKE_MAX_STRIDE
OPT_ADAGRAD, OPT_SGD, OPT_ADAM, OPT_ADADELTA = 0, 1, 2, 3
DENSE_OPTS = {"Adam": OPT_ADAM, "Adadelta": OPT_ADADELTA}   # TF1 rules that move zero-gradient weights: whole-variable kernels
_SUPPORTED_FPL = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 20)

# every symbol include/multike_hip.h declares (tests/test_abi.py checks the .so exports each of them)
SYMBOLS = (
    "mke_version", "mke_last_error", "mke_set_option", "mke_triple_score_fwd_bwd", "mke_triple_score_step",
    "mke_count_entity_refs", "mke_stage_reduce", "mke_rows_update", "mke_rows_update_multi", "mke_rows_update_multi_count",
    "mke_neg_sample", "mke_tripleset_build", "mke_tripleset_query", "mke_gathered_logistic_fwd_bwd",
    "mke_gathered_alignment_fwd_bwd", "mke_align_fwd_bwd", "mke_gather_rows", "mke_relation_steps",
    "mke_rowset_build", "mke_rowset_remap", "mke_rows_gather_padded", "mke_rows_scatter_add",
    "mke_attr_conv_fwd", "mke_attr_conv_bwd", "mke_attr_tail_z", "mke_attr_tail_loss", "mke_attr_tail_bwd",
    "mke_dense_update", "mke_align_rank", "mke_gemm_f32", "mke_attr_scratch_floats", "mke_attr_step", "mke_attr_steps", "mke_attr_step_phases",
    "mke_sample_distinct", "mke_neg_sample_at", "mke_rows_update_dense", "mke_dense_update_opt", "mke_align_steps", "mke_sim_select", "mke_sim_sample", "mke_topk_rows", "mke_topk_candidates", "mke_mapping_scratch_floats", "mke_mapping_step", "mke_mapping_step_phases", "mke_mapping_steps",
    "mke_ae_scratch_floats", "mke_ae_train_steps", "mke_ae_step_phases", "mke_ae_encode", "mke_dense_layer_fwd",
    "mke_topk_long", "mke_probe_rows", "mke_oc_block_floats", "mke_oc_pack_codes", "mke_oc_plan", "mke_oc_bases", "mke_oc_count", "mke_oc_score", "mke_oc_apply", "mke_oc_run",
    "mke_oc_em_plan_temp_bytes", "mke_oc_em_plan", "mke_oc_pass2", "mke_oc_steps", "mke_oc_gv_sum",
    "mke_oc_bucket_codes", "mke_oc_owned_index",
    "mke_tuning_init", "mke_rows_update_multi_t",
    "mke_align_topk_mean_temp_bytes", "mke_align_topk_mean", "mke_align_rank_ex",
    "mke_stable_lists_temp_bytes", "mke_stable_lists", "mke_stable_rounds", "mke_stable_finish",
    "mke_tripleset_forget", "mke_tripleset_filter_bytes", "mke_epoch_positives",
    "mke_align_lse_temp_bytes", "mke_align_lse",
    "mke_align_mutual", "mke_mutual_pairs",
    "mke_assign_temp_bytes", "mke_assign_rounds", "mke_assign_finish",
    "mke_boot_partner", "mke_swap_temp_bytes", "mke_swap_triples",
    "mke_neg_code_row_words", "mke_neg_codes",
)
ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2
AE_MAX_LAYERS = 4


class AttrStepArgs(C.Structure):
    """mke_attr_step_args"""
    _fields_ = [
        ("ent_table", C.c_void_p), ("n_ent", C.c_int64), ("ent_stride", C.c_int), ("ent_normalize", C.c_int),
        ("ent_acc", C.c_void_p), ("ent_grad", C.c_void_p), ("ent_touched", C.c_void_p),
        ("attr_table", C.c_void_p), ("n_attr", C.c_int64), ("attr_stride", C.c_int), ("attr_normalize", C.c_int),
        ("attr_acc", C.c_void_p), ("attr_grad", C.c_void_p), ("attr_touched", C.c_void_p),
        ("lit_table", C.c_void_p), ("lit_stride", C.c_int), ("dim", C.c_int),
        ("ih", C.c_void_p), ("ia", C.c_void_p), ("iv", C.c_void_p), ("weights", C.c_void_p), ("n", C.c_int64),
        ("scale", C.c_float), ("params", C.c_void_p), ("param_grads", C.c_void_p), ("param_acc", C.c_void_p),
        ("scratch", C.c_void_p), ("partials", C.c_void_p), ("optimizer", C.c_int), ("lr", C.c_float), ("tag", C.c_int32),
        ("update", C.c_int), ("workspace", C.c_void_p), ("attr_grad_copies", C.c_int), ("tuning", C.c_void_p),
    ]


class AlignTableStruct(C.Structure):
    """mke_align_table"""
    _fields_ = [("table", C.c_void_p), ("acc", C.c_void_p), ("grad", C.c_void_p), ("touched", C.c_void_p), ("n_rows", C.c_int64),
                ("normalize", C.c_int)]


class AlignTermStruct(C.Structure):
    """mke_align_term"""
    _fields_ = [("a", C.c_int), ("b", C.c_int), ("weight", C.c_float)]


class AlignPlanStruct(C.Structure):
    """mke_align_plan"""
    _fields_ = [("tables", AlignTableStruct * 4), ("n_tables", C.c_int), ("terms", AlignTermStruct * 4), ("n_terms", C.c_int),
                ("stride", C.c_int), ("dim", C.c_int), ("ia", C.c_void_p), ("ib", C.c_void_p),
                ("step_off", C.POINTER(C.c_int64)), ("n_steps", C.c_int), ("optimizer", C.c_int), ("lr", C.c_float),
                ("tag_base", C.c_int32), ("loss_partials", C.c_void_p)]


class MappingViewStruct(C.Structure):
    """mke_mapping_view"""
    _fields_ = [("table", C.c_void_p), ("normalize", C.c_int)]


class MappingStepArgs(C.Structure):
    """mke_mapping_step_args"""
    _fields_ = [("ent_table", C.c_void_p), ("n_ent", C.c_int64), ("ent_normalize", C.c_int), ("ent_acc", C.c_void_p),
                ("ent_grad", C.c_void_p), ("ent_touched", C.c_void_p), ("views", MappingViewStruct * 3), ("n_views", C.c_int),
                ("stride", C.c_int), ("dim", C.c_int), ("idx", C.c_void_p), ("n", C.c_int64), ("M", C.c_void_p), ("gM", C.c_void_p),
                ("accM", C.c_void_p), ("orthogonal_weight", C.c_float), ("norm_w", C.c_float), ("scratch", C.c_void_p),
                ("partials", C.c_void_p), ("optimizer", C.c_int), ("lr", C.c_float), ("tag", C.c_int32), ("update", C.c_int)]


class HotRowsStruct(C.Structure):
    """mke_hot_rows"""
    _fields_ = [("slot", C.c_void_p), ("n_hot", C.c_int32), ("copies", C.c_int32), ("row0", C.c_int64)]


class ScoreArgs(C.Structure):
    """mke_score_args"""
    _fields_ = [("ent_table", C.c_void_p), ("n_ent", C.c_int64), ("ent_normalize", C.c_int),
                ("rel_table", C.c_void_p), ("n_rel", C.c_int64), ("rel_normalize", C.c_int), ("stride", C.c_int), ("dim", C.c_int),
                ("pos_h", C.c_void_p), ("pos_r", C.c_void_p), ("pos_t", C.c_void_p), ("pos_w", C.c_void_p), ("n_pos", C.c_int64),
                ("neg_h", C.c_void_p), ("neg_r", C.c_void_p), ("neg_t", C.c_void_p), ("neg_w", C.c_void_p), ("n_neg", C.c_int64),
                ("neg_per_pos", C.c_int), ("scale", C.c_float),
                ("grad_ent", C.c_void_p), ("grad_rel", C.c_void_p), ("grad_rel_copies", C.c_int),
                ("touched_ent", C.c_void_p), ("touched_rel", C.c_void_p), ("tag", C.c_int32),
                ("ref_count", C.c_void_p), ("ent_acc", C.c_void_p), ("optimizer", C.c_int), ("lr", C.c_float),
                ("next_count", C.c_void_p), ("hot", HotRowsStruct),
                ("stage_rows", C.c_void_p), ("stage_keys", C.c_void_p), ("stage_slots", C.c_int64),
                ("loss_partials", C.c_void_p), ("tuning", C.c_void_p), ("neg_code", C.c_void_p)]


class OcStepStruct(C.Structure):
    """mke_oc_step"""
    _fields_ = [("ent", C.c_void_p), ("ent_acc", C.c_void_p), ("ent_grad", C.c_void_p), ("ent_touched", C.c_void_p),
                ("ref_count", C.c_void_p), ("n_local", C.c_int64),
                ("rel", C.c_void_p), ("rel_acc", C.c_void_p), ("rel_grad", C.c_void_p), ("rel_grad_copies", C.c_int), ("rel_touched", C.c_void_p),
                ("n_rel", C.c_int64), ("stride", C.c_int), ("dim", C.c_int), ("rank", C.c_int), ("n_ranks", C.c_int),
                ("pos_h", C.c_void_p), ("pos_r", C.c_void_p), ("pos_t", C.c_void_p), ("n_pos", C.c_int64), ("per", C.c_int64),
                ("slot_h", C.c_void_p), ("slot_t", C.c_void_p), ("own_h", C.c_void_p), ("n_own_h", C.c_int64),
                ("own_t", C.c_void_p), ("n_own_t", C.c_int64), ("neg_per_pos", C.c_int), ("capacity", C.c_int64),
                ("codes", C.c_void_p), ("code_off", C.c_int64 * 16),
                ("optimizer", C.c_int), ("lr", C.c_float), ("scale", C.c_float), ("tag", C.c_int32),
                ("n_peers", C.c_int), ("peer_v", C.c_void_p * 16), ("peer_g", C.c_void_p * 16), ("pos_w", C.c_void_p),
                ("hot", HotRowsStruct),
                # version 105: entity-major second pass
                ("em_coef", C.c_void_p), ("em_pos0", C.c_int64), ("em_refs", C.c_void_p), ("em_rows", C.c_void_p), ("em_off", C.c_void_p),
                ("em_n_rows", C.c_int64), ("em_chunks", C.c_int), ("em_block_floats", C.c_int64), ("em_v", C.c_void_p * 4),
                ("em_gv", C.c_void_p * 4),
                ("em_part", C.c_void_p), ("em_long_rows", C.c_void_p), ("em_long_part0", C.c_void_p), ("em_n_long", C.c_int64),
                ("em_part0", C.c_int64), ("em_partials", C.c_void_p), ("em_mode", C.c_int), ("tuning", C.c_void_p),
                # owned code lists (mke_oc_owned_index) in place of the code scan; own_off advanced to the part's first positive
                ("own_rec", C.c_void_p), ("own_off", C.c_void_p)]


TUNE_DEFAULT = -2
TUNING_FIELDS = ("score_splits", "score_half_groups", "score_offsets32", "score_lane_ids", "count_in_score", "update_chunk",
                 "oc_score_quarter", "attr_fused_bwd", "sampler_fast", "neg_codes")


class TuningStruct(C.Structure):
    """mke_tuning: the performance knobs of ONE plan / call (a field at TUNE_DEFAULT follows mke_set_option's process default)."""
    _fields_ = [(f, C.c_int) for f in TUNING_FIELDS] + [("reserved", C.c_int * 6)]


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


OC_EM_MAX_CHUNKS = 4
OC_EM_WAVES = 32768


class OcEmPlanArgs(C.Structure):
    """mke_oc_em_plan_args"""
    _fields_ = [("pos_h", C.c_void_p), ("pos_r", C.c_void_p), ("pos_t", C.c_void_p), ("codes", C.c_void_p), ("neg_per_pos", C.c_int),
                ("slot_h", C.c_void_p), ("slot_t", C.c_void_p), ("step_lo", C.c_void_p), ("n_steps", C.c_int), ("chunks", C.c_int),
                ("n_all", C.c_int64), ("max_step", C.c_int64), ("n_ranks", C.c_int), ("rank", C.c_int), ("n_local", C.c_int64), ("n_rel", C.c_int64),
                ("keys", C.c_void_p), ("keys_alt", C.c_void_p), ("capacity", C.c_int64), ("vals_alt", C.c_void_p), ("scratch8", C.c_void_p), ("wave_scratch", C.c_void_p),
                ("refs", C.c_void_p), ("rows", C.c_void_p), ("off", C.c_void_p), ("flags", C.c_void_p), ("scan", C.c_void_p),
                ("step_row0", C.c_void_p), ("n_refs", C.c_void_p),
                ("item_row", C.c_void_p), ("item_off", C.c_void_p), ("item_part", C.c_void_p), ("long_row", C.c_void_p), ("long_part0", C.c_void_p),
                ("step_item0", C.c_void_p), ("step_long0", C.c_void_p), ("step_part0", C.c_void_p),
                ("temp", C.c_void_p), ("temp_bytes", C.c_int64),
                ("own_rec", C.c_void_p), ("own_off", C.c_void_p), ("own_cap", C.c_int64)]


OC_COMM_NCCL, OC_COMM_CALLBACK, OC_COMM_LOOPBACK = 0, 1, 2
OC_CB_MOVE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)     # all_gather / reduce_scatter callbacks
OC_CB_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)              # all_reduce callback


class OcCommStruct(C.Structure):
    """mke_oc_comm"""
    _fields_ = [("kind", C.c_int), ("ctx", C.c_void_p), ("all_gather", C.c_void_p), ("reduce_scatter", C.c_void_p), ("all_reduce", C.c_void_p),
                ("world", C.c_int), ("rank", C.c_int), ("wire_gbps", C.c_float), ("latency_us", C.c_float)]


class OcLoopStruct(C.Structure):
    """mke_oc_loop"""
    _fields_ = [("parts", C.c_void_p), ("step_part0", C.c_void_p), ("n_steps", C.c_int), ("chunks", C.c_int),
                ("send", C.c_void_p * 4), ("v_all", C.c_void_p * 4), ("g_all", C.c_void_p * 4), ("gv", C.c_void_p * 4), ("block_floats", C.c_int64),
                ("loss_ring", C.c_void_p), ("loss_stride", C.c_int64), ("tag_base", C.c_int32), ("comm", C.c_void_p), ("comm_stream", C.c_void_p),
                ("overlap_rs", C.c_int)]


class AEPlanStruct(C.Structure):
    """mke_ae_plan"""
    _fields_ = [("n_layers", C.c_int), ("dims", C.c_int * 5), ("act", C.c_int), ("normalize", C.c_int),
                ("params", C.c_void_p), ("grads", C.c_void_p), ("acc", C.c_void_p), ("n_params", C.c_int64),
                ("w_off", C.c_int64 * 8), ("b_off", C.c_int64 * 8), ("optimizer", C.c_int), ("lr", C.c_float),
                ("update", C.c_int), ("scratch", C.c_void_p), ("scratch_floats", C.c_int64), ("partials", C.c_void_p),
                ("scalars", C.c_void_p)]


class OptimizerStruct(C.Structure):
    """mke_optimizer (TF1 defaults)"""
    _fields_ = [("kind", C.c_int), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float),
                ("rho", C.c_float), ("step", C.c_int64)]


def optimizer_struct(name: str, lr: float, step: int = 1) -> OptimizerStruct:
    return OptimizerStruct(DENSE_OPTS[name], float(lr), 0.9, 0.999, 1e-8, 0.95, int(step))


class KGSideStruct(C.Structure):
    """mke_kg_side"""
    _fields_ = [("ent_list", C.c_void_p), ("ent_lo", C.c_int32), ("n_ent", C.c_int32), ("cand_table", C.c_void_p),
                ("cand_valid", C.c_void_p), ("cand_k", C.c_int32), ("known_keys", C.c_void_p),
                ("known_capacity", C.c_uint64)]


class UpdateTableStruct(C.Structure):
    """mke_update_table"""
    _fields_ = [("table", C.c_void_p), ("acc", C.c_void_p), ("grad", C.c_void_p), ("touched", C.c_void_p),
                ("n_rows", C.c_int64), ("normalize", C.c_int), ("grad_copies", C.c_int), ("ref_count", C.c_void_p),
                ("src_rows", C.c_void_p), ("slot_of", C.c_void_p), ("n_ranks", C.c_int), ("capacity", C.c_int64),
                ("hot", HotRowsStruct)]


class RelationPlanStruct(C.Structure):
    """mke_relation_plan"""
    _fields_ = [
        ("ent_table", C.c_void_p), ("n_ent", C.c_int64), ("ent_normalize", C.c_int),
        ("rel_table", C.c_void_p), ("n_rel", C.c_int64), ("rel_normalize", C.c_int),
        ("ent_acc", C.c_void_p), ("rel_acc", C.c_void_p), ("ent_grad", C.c_void_p), ("rel_grad", C.c_void_p),
        ("rel_grad_copies", C.c_int),
        ("ent_touched", C.c_void_p), ("rel_touched", C.c_void_p), ("ent_ref_count", C.c_void_p), ("overlap", C.c_int),
        ("neg_chunk_capacity", C.c_int64), ("stride", C.c_int), ("dim", C.c_int),
        ("pos_h", C.c_void_p), ("pos_r", C.c_void_p), ("pos_t", C.c_void_p), ("pos_kg", C.c_void_p),
        ("step_off", C.POINTER(C.c_int64)), ("n_steps", C.c_int), ("sides", KGSideStruct * 2),
        ("neg_per_pos", C.c_int), ("max_try", C.c_int), ("sample_chunk", C.c_int), ("negatives_ready", C.c_int),
        ("neg_h", C.c_void_p), ("neg_r", C.c_void_p), ("neg_t", C.c_void_p),
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("stream_id", C.c_uint32),
        ("optimizer", C.c_int), ("lr", C.c_float), ("scale", C.c_float),
        ("loss_partials", C.c_void_p), ("loss_ring", C.c_int), ("tag_base", C.c_int32), ("pos_w", C.c_void_p),
        ("hot", HotRowsStruct), ("tuning", C.c_void_p),
        ("step_off_dev", C.c_void_p), ("neg_code", C.c_void_p), ("code_bits", C.c_void_p), ("code_bits_words", C.c_int64),
    ]

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
        L.mke_version.restype = C.c_int
        L.mke_last_error.restype = C.c_char_p
        for name in SYMBOLS[2:]:
            getattr(L, name).restype = C.c_int
        L.mke_attr_scratch_floats.restype = C.c_int64
        L.mke_mapping_scratch_floats.restype = C.c_int64
        L.mke_ae_scratch_floats.restype = C.c_int64
        L.mke_oc_block_floats.restype = C.c_int64
        L.mke_oc_em_plan_temp_bytes.restype = C.c_int64
        L.mke_align_topk_mean_temp_bytes.restype = C.c_int64
        L.mke_stable_lists_temp_bytes.restype = C.c_int64
        L.mke_align_lse_temp_bytes.restype = C.c_int64
        L.mke_tripleset_filter_bytes.restype = C.c_int64
        L.mke_assign_temp_bytes.restype = C.c_int64
        L.mke_swap_temp_bytes.restype = C.c_int64
        L.mke_neg_code_row_words.restype = C.c_int64
        _lib = L
        # MKE_OPTIONS="name=value,name=value": mke_set_option calls applied at load (performance knobs for experiments)
        for kv in filter(None, os.environ.get("MKE_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            if L.mke_set_option(k.strip().encode(), C.c_int(int(v)), None):
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


def _dev(t: torch.Tensor | None, dtype, name: str):
    """data_ptr of a contiguous CUDA tensor of the given dtype (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise MultiKEHipError(f"{name}: expected a CUDA/HIP tensor, got device {t.device} (no CPU path exists)")
    if t.dtype != dtype:
        raise MultiKEHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MultiKEHipError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


_pinned_stream = None  # raw hipStream_t handle pinned by a hot loop (saves a torch.cuda.current_stream() per launch)


def pin_stream(handle: int | None):
    """Pin the stream every launch goes to (a raw `stream.cuda_stream` handle), or None to follow torch's current
    stream again.  Returns the previous pin."""
    global _pinned_stream
    old, _pinned_stream = _pinned_stream, handle
    return old


def _stream():
    if _pinned_stream is not None:
        return C.c_void_p(_pinned_stream)
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def version() -> int:
    return lib().mke_version()


def set_option(name: str, value: int) -> int:
    old = C.c_int(0)
    _check(lib().mke_set_option(name.encode(), C.c_int(value), C.byref(old)), "mke_set_option")
    return old.value


def stage_reduce(stage_rows, sorted_keys, order, grad_ent, grad_rel, touched_ent, touched_rel, tag):
    rc = lib().mke_stage_reduce(_dev(stage_rows, torch.float32, "stage_rows"), _dev(sorted_keys, torch.int64, "keys"),
                                _dev(order, torch.int64, "order"), C.c_int64(sorted_keys.numel()), C.c_int(stage_rows.shape[1]),
                                _dev(grad_ent, torch.float32, "grad_ent"), _dev(grad_rel, torch.float32, "grad_rel"),
                                _dev(touched_ent, torch.int32, "touched"), _dev(touched_rel, torch.int32, "touched"), C.c_int32(tag),
                                _stream())
    _check(rc, "mke_stage_reduce")


def get_option(name: str) -> int:
    old = set_option(name, 0)
    set_option(name, old)
    return old


def count_entity_refs(pos_h, pos_t, neg_h, neg_t, neg_per_pos, ref_count):
    rc = lib().mke_count_entity_refs(_dev(pos_h, torch.int32, "pos_h"), _dev(pos_t, torch.int32, "pos_t"),
                                     C.c_int64(pos_h.numel()), _dev(neg_h, torch.int32, "neg_h"),
                                     _dev(neg_t, torch.int32, "neg_t"), C.c_int64(0 if neg_h is None else neg_h.numel()),
                                     C.c_int(neg_per_pos), _dev(ref_count, torch.int32, "ref_count"), _stream())
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
        _dev(table, torch.float32, "table"), _dev(acc, torch.float32, "acc"), _dev(grad, torch.float32, "grad"),
        C.c_int(copies), _dev(touched, torch.int32, "touched"), C.c_int32(tag), C.c_int64(table.shape[0]), C.c_int(table.shape[1]),
        C.c_int(dim), C.c_int(int(normalize)), C.c_int(optimizer), C.c_float(lr), _stream())
    _check(rc, "mke_rows_update")


def ptr(t: torch.Tensor | None, dtype, name: str) -> int | None:
    """Raw device address (for the plan / side structs)."""
    return _dev(t, dtype, name).value


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
        rc = lib().mke_rows_update_multi_t(arr, C.c_int(len(tables)), C.c_int32(tag), C.c_int(stride), C.c_int(dim),
                                           C.c_int(optimizer), C.c_float(lr), None, C.byref(tuning), _stream())
        _check(rc, "mke_rows_update_multi_t")
        return
    rc = lib().mke_rows_update_multi(arr, C.c_int(len(tables)), C.c_int32(tag), C.c_int(stride), C.c_int(dim),
                                     C.c_int(optimizer), C.c_float(lr), _stream())
    _check(rc, "mke_rows_update_multi")


def neg_sample(pos, pos_offset, pos_kg, sides, neg_per_pos, max_try, seed, stream_id, neg_out):
    """sides: (KGSideStruct * 2) host array; pos_kg: uint8 CUDA tensor or None (all KG 0)."""
    ph, pr, pt = pos
    nh, nr, nt = neg_out
    rc = lib().mke_neg_sample(
        _dev(ph, torch.int32, "pos_h"), _dev(pr, torch.int32, "pos_r"), _dev(pt, torch.int32, "pos_t"),
        C.c_int64(ph.numel()), C.c_int64(pos_offset), _dev(pos_kg, torch.uint8, "pos_kg"), sides,
        C.c_int(neg_per_pos), C.c_int(max_try), C.c_uint32(seed[0] & 0xFFFFFFFF), C.c_uint32(seed[1] & 0xFFFFFFFF),
        C.c_uint32(stream_id & 0xFFFFFFFF), _dev(nh, torch.int32, "neg_h"), _dev(nr, torch.int32, "neg_r"),
        _dev(nt, torch.int32, "neg_t"), _stream())
    _check(rc, "mke_neg_sample")


def neg_sample_at(pos, pos_index, pos_kg, sides, neg_per_pos, max_try, seed, stream_id, neg_out):
    """mke_neg_sample_at: like neg_sample, with an explicit int32 epoch position per positive."""
    ph, pr, pt = pos
    nh, nr, nt = neg_out
    rc = lib().mke_neg_sample_at(
        _dev(ph, torch.int32, "pos_h"), _dev(pr, torch.int32, "pos_r"), _dev(pt, torch.int32, "pos_t"),
        C.c_int64(ph.numel()), _dev(pos_index, torch.int32, "pos_index"), _dev(pos_kg, torch.uint8, "pos_kg"), sides,
        C.c_int(neg_per_pos), C.c_int(max_try), C.c_uint32(seed[0] & 0xFFFFFFFF), C.c_uint32(seed[1] & 0xFFFFFFFF),
        C.c_uint32(stream_id & 0xFFFFFFFF), _dev(nh, torch.int32, "neg_h"), _dev(nr, torch.int32, "neg_r"),
        _dev(nt, torch.int32, "neg_t"), _stream())
    _check(rc, "mke_neg_sample_at")


SIM_SELECT_KPADS = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 208, 256, 320)   # instantiations of k_sim_select / k_sim_sample / k_align_rank: up to MAX_STRIDE


def sim_select(emb: torch.Tensor, kpad: int, row_lo: int, row_hi: int, tau: torch.Tensor, n_seg: int, seg_cap: int):
    """mke_sim_select -> (cand int32 [rows, n_seg, seg_cap, 2] = (column, similarity bits) pairs, seg_count int32 [rows, n_seg])."""
    if emb.dim() != 2 or emb.stride(1) != 1 or emb.dtype != torch.float32:
        raise MultiKEHipError("sim_select: emb must be a row-major float32 matrix")
    rows = row_hi - row_lo
    if tau.numel() != rows:
        raise MultiKEHipError("sim_select: one threshold per row")
    cand = torch.empty(rows, n_seg, seg_cap, 2, dtype=torch.int32, device=emb.device)
    cnt = torch.empty(rows, n_seg, dtype=torch.int32, device=emb.device)
    rc = lib().mke_sim_select(C.c_void_p(emb.data_ptr()), C.c_int(emb.stride(0)), C.c_int(kpad), C.c_int64(emb.shape[0]),
                              C.c_int64(row_lo), C.c_int64(row_hi), _dev(tau, torch.float32, "tau"), C.c_int(n_seg),
                              C.c_int(seg_cap), _dev(cand, torch.int32, "cand"), _dev(cnt, torch.int32, "seg_count"), _stream())
    _check(rc, "mke_sim_select")
    return cand, cnt


def sim_sample(emb: torch.Tensor, kpad: int, row_lo: int, row_hi: int, samp: torch.Tensor):
    """mke_sim_sample -> float32 [row_hi - row_lo, n_samp] similarities of the rows to the sample rows."""
    out = torch.empty(row_hi - row_lo, samp.shape[0], dtype=torch.float32, device=emb.device)
    rc = lib().mke_sim_sample(_dev(emb, torch.float32, "emb"), C.c_int(emb.stride(0)), C.c_int(kpad), C.c_int64(emb.shape[0]),
                              C.c_int64(row_lo), C.c_int64(row_hi), _dev(samp, torch.float32, "samp"), C.c_int(samp.stride(0)),
                              C.c_int(samp.shape[0]), _dev(out, torch.float32, "out"), _stream())
    _check(rc, "mke_sim_sample")
    return out


def topk_candidates(cand: torch.Tensor, seg_count: torch.Tensor, k: int, id_map=None):
    """mke_topk_candidates over sim_select's pairs -> (out_idx int32 [rows, k], status int32 [rows])."""
    rows, n_seg, seg_cap, _ = cand.shape
    out = torch.empty(rows, k, dtype=torch.int32, device=cand.device)
    status = torch.empty(rows, dtype=torch.int32, device=cand.device)
    rc = lib().mke_topk_candidates(_dev(cand, torch.int32, "cand"), _dev(seg_count, torch.int32, "seg_count"), C.c_int64(rows),
                                   C.c_int(n_seg), C.c_int(seg_cap), C.c_int(k), _dev(id_map, torch.int32, "id_map"),
                                   _dev(out, torch.int32, "out_idx"), C.c_void_p(0), _dev(status, torch.int32, "status"), _stream())
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
    rc = lib().mke_topk_rows(_dev(vals, torch.float32, "vals"), _dev(idx, torch.int32, "idx"),
                             _dev(seg_count, torch.int32, "seg_count"), C.c_int64(rows), C.c_int(n_seg), C.c_int(seg_cap),
                             C.c_int(k), _dev(id_map, torch.int32, "id_map"), _dev(out, torch.int32, "out_idx"),
                             _dev(kth, torch.float32, "out_kth"), _dev(status, torch.int32, "status"), _stream())
    _check(rc, "mke_topk_rows")
    return out, kth, status


def topk_long(vals: torch.Tensor, k: int, id_map=None) -> torch.Tensor:
    """mke_topk_long over whole rows vals [rows, n] (any n) -> int32 [rows, k], column order."""
    if vals.dim() != 2 or vals.stride(1) != 1:
        raise MultiKEHipError("topk_long: vals must be [rows, n] with unit column stride")
    rows, n = vals.shape
    out = torch.empty(rows, k, dtype=torch.int32, device=vals.device)
    rc = lib().mke_topk_long(C.c_void_p(vals.data_ptr()) if vals.is_cuda and vals.dtype == torch.float32 else _dev(vals, torch.float32, "vals"),
                             C.c_int64(rows), C.c_int64(n), C.c_int64(vals.stride(0) if rows > 1 else n), C.c_int(k),
                             _dev(id_map, torch.int32, "id_map"), _dev(out, torch.int32, "out_idx"), _stream())
    _check(rc, "mke_topk_long")
    return out


def mapping_scratch_floats(n: int, dim: int) -> int:
    return int(lib().mke_mapping_scratch_floats(C.c_int64(n), C.c_int(dim)))


MAP_FWD, MAP_TAIL, MAP_BWD, MAP_UPD, MAP_ALL = 1, 2, 4, 8, 15
MAPPING_MAX_VIEWS = 3


def mapping_step_phases(args: MappingStepArgs, loss_partials: torch.Tensor, phases: int):
    rc = lib().mke_mapping_step_phases(C.byref(args), _dev(loss_partials, torch.float64, "loss_partials"), C.c_int(phases), _stream())
    _check(rc, "mke_mapping_step_phases")


def mapping_step(args: MappingStepArgs, loss_partials: torch.Tensor):
    rc = lib().mke_mapping_step(C.byref(args), _dev(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_mapping_step")


def mapping_steps(args: MappingStepArgs, step_off: np.ndarray, loss_ring: torch.Tensor):
    """loss_ring: float64 [ring, 4, LOSS_PARTIALS]."""
    off = np.ascontiguousarray(step_off, dtype=np.int64)
    rc = lib().mke_mapping_steps(C.byref(args), off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(len(off) - 1),
                                 _dev(loss_ring, torch.float64, "loss_ring"), C.c_int(loss_ring.shape[0]), _stream())
    _check(rc, "mke_mapping_steps")


def align_steps(plan: AlignPlanStruct):
    rc = lib().mke_align_steps(C.byref(plan), _stream())
    _check(rc, "mke_align_steps")


def relation_steps(plan: RelationPlanStruct, step_begin: int, step_end: int):
    rc = lib().mke_relation_steps(C.byref(plan), C.c_int(step_begin), C.c_int(step_end), _stream())
    _check(rc, "mke_relation_steps")


CODE_ENT_BITS, CODE_HEAD, CODE_FAST, CODE_EXCL = 26, 1 << 26, 1 << 27, 1 << 28   # MKE_CODE_*


def neg_code_row_words(n_ent: int) -> int:
    """Words of one step's row of the code-word bake's bitmap (2 bits per entity)."""
    return int(lib().mke_neg_code_row_words(C.c_int64(n_ent)))


def neg_codes(pos, step_off_dev, step_begin, step_end, pos_begin, pos_end, neg, neg_per_pos, n_ent, bits, neg_code):
    """mke_neg_codes: one code word per negative of steps [step_begin, step_end).  pos: the epoch's (h, r, t); neg: the chunk's."""
    rc = lib().mke_neg_codes(*(_dev(x, torch.int32, "pos") for x in pos), _dev(step_off_dev, torch.int64, "step_off"),
                             C.c_int(step_begin), C.c_int(step_end), C.c_int64(pos_begin), C.c_int64(pos_end),
                             *(_dev(x, torch.int32, "neg") for x in neg), C.c_int(neg_per_pos), C.c_int64(n_ent),
                             _dev(bits, torch.int32, "bits"), C.c_int64(bits.numel()), _dev(neg_code, torch.int32, "neg_code"), _stream())
    _check(rc, "mke_neg_codes")


def tripleset_build(h, r, t, keys):
    rc = lib().mke_tripleset_build(_dev(h, torch.int32, "h"), _dev(r, torch.int32, "r"), _dev(t, torch.int32, "t"),
                                   C.c_int64(h.numel()), _dev(keys, torch.int64, "keys"), C.c_uint64(keys.numel()),
                                   _stream())
    _check(rc, "mke_tripleset_build")


def tripleset_forget(keys):
    """Drop the library's prefilter of the table at `keys` (a tensor or a raw address); no-op when it has none."""
    addr = keys if isinstance(keys, int) else keys.data_ptr()
    _check(lib().mke_tripleset_forget(C.c_void_p(addr)), "mke_tripleset_forget")


def tripleset_filter_bytes(keys) -> int:
    """Size of the prefilter the sampler uses for this table; 0 when it has none (the table is probed directly)."""
    return int(lib().mke_tripleset_filter_bytes(_dev(keys, torch.int64, "keys"), C.c_uint64(keys.numel())))


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
    rc = lib().mke_epoch_positives(_dev(list1, i32, "list1"), _dev(list2, i32, "list2"), C.c_int64(n1), C.c_int64(n2),
                                   _dev(perm1, i64, "perm1"), _dev(perm2, i64, "perm2"), C.c_int64(b1), C.c_int64(b2),
                                   C.c_int64(n_steps), _dev(list1_out, i32, "list1_out"), _dev(list2_out, i32, "list2_out"),
                                   _dev(pos[0], i32, "pos_h"), _dev(pos[1], i32, "pos_r"), _dev(pos[2], i32, "pos_t"), _stream())
    _check(rc, "mke_epoch_positives")


def tripleset_query(h, r, t, keys, out):
    rc = lib().mke_tripleset_query(_dev(h, torch.int32, "h"), _dev(r, torch.int32, "r"), _dev(t, torch.int32, "t"),
                                   C.c_int64(h.numel()), _dev(keys, torch.int64, "keys"), C.c_uint64(keys.numel()),
                                   _dev(out, torch.uint8, "out"), _stream())
    _check(rc, "mke_tripleset_query")


def gathered_logistic_fwd_bwd(hs, rs, ts, ws, sign, gh, gr, gt, loss_partials):
    n, dim = hs.shape
    rc = lib().mke_gathered_logistic_fwd_bwd(
        _dev(hs, torch.float32, "hs"), _dev(rs, torch.float32, "rs"), _dev(ts, torch.float32, "ts"),
        _dev(ws, torch.float32, "ws"), C.c_int64(n), C.c_int(dim), C.c_int(dim), C.c_int(sign),
        _dev(gh, torch.float32, "gh"), _dev(gr, torch.float32, "gr"), _dev(gt, torch.float32, "gt"),
        _dev(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_gathered_logistic_fwd_bwd")


def gathered_alignment_fwd_bwd(a, b, ga, gb, loss_partials):
    n, dim = a.shape
    rc = lib().mke_gathered_alignment_fwd_bwd(
        _dev(a, torch.float32, "a"), _dev(b, torch.float32, "b"), C.c_int64(n), C.c_int(dim), C.c_int(dim),
        _dev(ga, torch.float32, "ga"), _dev(gb, torch.float32, "gb"),
        _dev(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_gathered_alignment_fwd_bwd")


def align_fwd_bwd(table_a, a_normalize, table_b, b_normalize, dim, ia, ib, weight, grad_a, touched_a, grad_b, touched_b,
                  tag, loss_partials):
    rc = lib().mke_align_fwd_bwd(
        _dev(table_a, torch.float32, "table_a"), C.c_int(int(a_normalize)), _dev(table_b, torch.float32, "table_b"),
        C.c_int(int(b_normalize)), C.c_int(table_a.shape[1]), C.c_int(dim), _dev(ia, torch.int32, "ia"),
        _dev(ib, torch.int32, "ib"), C.c_int64(ia.numel()), C.c_float(weight), _dev(grad_a, torch.float32, "grad_a"),
        _dev(touched_a, torch.int32, "touched_a"), _dev(grad_b, torch.float32, "grad_b"),
        _dev(touched_b, torch.int32, "touched_b"), C.c_int32(tag), _dev(loss_partials, torch.float64, "loss_partials"),
        _stream())
    _check(rc, "mke_align_fwd_bwd")


def gather_rows(table, normalize, dim, idx, out):
    n = out.shape[0]
    rc = lib().mke_gather_rows(_dev(table, torch.float32, "table"), C.c_int(int(normalize)), C.c_int(table.shape[1]),
                               C.c_int(dim), _dev(idx, torch.int32, "idx"), C.c_int64(n),
                               _dev(out, torch.float32, "out"), _stream())
    _check(rc, "mke_gather_rows")


def probe_rows(a, b, c, idx, out):
    """mke_probe_rows: rows idx of a (and b, c when given) read together; out [len(idx)] float32."""
    rc = lib().mke_probe_rows(_dev(a, torch.float32, "a"), _dev(b, torch.float32, "b"), _dev(c, torch.float32, "c"),
                              C.c_int(a.shape[1]), _dev(idx, torch.int32, "idx"), C.c_int64(idx.numel()),
                              _dev(out, torch.float32, "out"), _stream())
    _check(rc, "mke_probe_rows")


def rowset_build(streams, flags, counts, req, id_map, overflow, n_ranks, capacity):
    """streams: up to four int32 id tensors."""
    args = []
    for k in range(4):
        t = streams[k] if k < len(streams) else None
        args += [_dev(t, torch.int32, f"ids{k}"), C.c_int64(0 if t is None else t.numel())]
    rc = lib().mke_rowset_build(*args, _dev(flags, torch.int32, "flags"), _dev(counts, torch.int32, "counts"),
                                _dev(req, torch.int32, "req"), _dev(id_map, torch.int32, "id_map"),
                                _dev(overflow, torch.int32, "overflow"), C.c_int(n_ranks), C.c_int(capacity), _stream())
    _check(rc, "mke_rowset_build")


def rowset_remap(streams, outs, id_map, flags, reset_req=None, reset_counts=None, want=None, slot_of=None, n_ranks=0,
                 capacity=0):
    args = []
    for k in range(4):
        t = streams[k] if k < len(streams) else None
        o = outs[k] if k < len(outs) else None
        args += [_dev(t, torch.int32, f"ids{k}"), _dev(o, torch.int32, f"out{k}"), C.c_int64(0 if t is None else t.numel())]
    rc = lib().mke_rowset_remap(*args, _dev(id_map, torch.int32, "id_map"), _dev(flags, torch.int32, "flags"),
                                _dev(reset_req, torch.int32, "reset_req"), C.c_int64(0 if reset_req is None else reset_req.numel()),
                                _dev(reset_counts, torch.int32, "reset_counts"),
                                C.c_int(0 if reset_counts is None else reset_counts.numel()),
                                _dev(want, torch.int32, "want"), _dev(slot_of, torch.int32, "slot_of"), C.c_int(n_ranks),
                                C.c_int(capacity), _stream())
    _check(rc, "mke_rowset_remap")


def rows_gather_padded(table, idx, out, zero_rows=None):
    rc = lib().mke_rows_gather_padded(_dev(table, torch.float32, "table"), C.c_int(table.shape[1]),
                                      _dev(idx, torch.int32, "idx"), C.c_int64(idx.numel()),
                                      _dev(out, torch.float32, "out"), _dev(zero_rows, torch.float32, "zero_rows"), _stream())
    _check(rc, "mke_rows_gather_padded")


def rows_scatter_add(idx, rows, dim, grad, touched, tag, reset_req=None, reset_counts=None):
    rc = lib().mke_rows_scatter_add(_dev(idx, torch.int32, "idx"), _dev(rows, torch.float32, "rows"),
                                    C.c_int64(idx.numel()), C.c_int(grad.shape[1]), C.c_int(dim),
                                    _dev(grad, torch.float32, "grad"), _dev(touched, torch.int32, "touched"), C.c_int32(tag),
                                    _dev(reset_req, torch.int32, "reset_req"), _dev(reset_counts, torch.int32, "reset_counts"),
                                    C.c_int(0 if reset_counts is None else reset_counts.numel()), _stream())
    _check(rc, "mke_rows_scatter_add")


def cnn_conv_params(dim: int) -> int:
    return 2 * dim + 52


def cnn_params(dim: int) -> int:
    return cnn_conv_params(dim) + 4 * dim * dim + dim


def attr_conv_fwd(attr, attr_normalize, lit, dim, ia, iv, params, flat):
    rc = lib().mke_attr_conv_fwd(_dev(attr, torch.float32, "attr_table"), C.c_int(attr.shape[1]), C.c_int(int(attr_normalize)),
                                 _dev(lit, torch.float32, "lit_table"), C.c_int(lit.shape[1]), C.c_int(dim),
                                 _dev(ia, torch.int32, "ia"), _dev(iv, torch.int32, "iv"), C.c_int64(ia.numel()),
                                 _dev(params, torch.float32, "params"), _dev(flat, torch.float32, "flat"),
                                 C.c_int(flat.shape[1]), _stream())
    _check(rc, "mke_attr_conv_fwd")


def cnn_workspace_floats(dim: int) -> int:
    """MKE_CNN_WORKSPACE_FLOATS(dim)"""
    return 32 * (2 * dim + 64)


def attr_conv_bwd(attr, attr_normalize, lit, dim, ia, iv, params, dflat, grad_params, grad_attr, touched_attr, tag,
                  workspace=None):
    rc = lib().mke_attr_conv_bwd(_dev(attr, torch.float32, "attr_table"), C.c_int(attr.shape[1]), C.c_int(int(attr_normalize)),
                                 _dev(lit, torch.float32, "lit_table"), C.c_int(lit.shape[1]), C.c_int(dim),
                                 _dev(ia, torch.int32, "ia"), _dev(iv, torch.int32, "iv"), C.c_int64(ia.numel()),
                                 _dev(params, torch.float32, "params"), _dev(dflat, torch.float32, "dflat"),
                                 _dev(grad_params, torch.float32, "grad_params"), _dev(grad_attr, torch.float32, "grad_attr"),
                                 _dev(touched_attr, torch.int32, "touched_attr"), C.c_int32(tag),
                                 _dev(workspace, torch.float32, "workspace"), _stream())
    _check(rc, "mke_attr_conv_bwd")


def attr_tail_z(z, bias, sumsq_partials):
    n, dim = z.shape
    rc = lib().mke_attr_tail_z(_dev(z, torch.float32, "z"), _dev(bias, torch.float32, "bias"), C.c_int64(n), C.c_int(dim),
                               _dev(sumsq_partials, torch.float64, "sumsq_partials"), _stream())
    _check(rc, "mke_attr_tail_z")


def attr_tail_loss(z, sumsq_partials, ent, ent_normalize, ih, weights, scale, gout, dot_partials, grad_ent, touched_ent, tag,
                   loss_partials):
    n, dim = z.shape
    rc = lib().mke_attr_tail_loss(_dev(z, torch.float32, "z"), _dev(sumsq_partials, torch.float64, "sumsq"),
                                  _dev(ent, torch.float32, "ent_table"), C.c_int(ent.shape[1]), C.c_int(int(ent_normalize)),
                                  _dev(ih, torch.int32, "ih"), _dev(weights, torch.float32, "weights"), C.c_float(scale),
                                  C.c_int64(n), C.c_int(dim), _dev(gout, torch.float32, "gout"),
                                  _dev(dot_partials, torch.float64, "dot_partials"), _dev(grad_ent, torch.float32, "grad_ent"),
                                  _dev(touched_ent, torch.int32, "touched_ent"), C.c_int32(tag),
                                  _dev(loss_partials, torch.float64, "loss_partials"), _stream())
    _check(rc, "mke_attr_tail_loss")


def attr_tail_bwd(z, gout, sumsq_partials, dot_partials, grad_bias=None):
    n, dim = z.shape
    rc = lib().mke_attr_tail_bwd(_dev(z, torch.float32, "z"), _dev(gout, torch.float32, "gout"),
                                 _dev(sumsq_partials, torch.float64, "sumsq"), _dev(dot_partials, torch.float64, "dot"),
                                 C.c_int64(n), C.c_int(dim), _dev(grad_bias, torch.float32, "grad_bias"), _stream())
    _check(rc, "mke_attr_tail_bwd")


def dense_update(param, acc, grad, optimizer, lr):
    rc = lib().mke_dense_update(_dev(param, torch.float32, "param"), _dev(acc, torch.float32, "acc"),
                                _dev(grad, torch.float32, "grad"), C.c_int64(param.numel()), C.c_int(optimizer), C.c_float(lr),
                                _stream())
    _check(rc, "mke_dense_update")


def oc_block_floats(capacity: int, stride: int) -> int:
    return int(lib().mke_oc_block_floats(C.c_int64(capacity), C.c_int(stride)))


def oc_pack_codes(pos_h, neg_h, neg_t, neg_per_pos: int, codes):
    rc = lib().mke_oc_pack_codes(_dev(pos_h, torch.int32, "pos_h"), _dev(neg_h, torch.int32, "neg_h"),
                                 _dev(neg_t, torch.int32, "neg_t"), C.c_int64(pos_h.numel()), C.c_int(neg_per_pos),
                                 _dev(codes, torch.int32, "codes"), _stream())
    _check(rc, "mke_oc_pack_codes")


OC_NEED_HR, OC_NEED_RT, OC_CODE_MASK = 0x40000000, 0x80000000, 0x3FFFFFFF


def oc_plan(pos_h, pos_t, codes, neg_per_pos: int, part_lo, n_parts: int, n_ranks: int, rank: int, slot_h, slot_t, own_h, own_t, counts):
    """The epoch's slots / owned lists / per-(part, owner) counts in one launch (mke_oc_plan); `codes`: the whole epoch's codes
    by epoch position (their group flags say which vector a positive needs), None when neg_per_pos == 0."""
    i32 = torch.int32
    rc = lib().mke_oc_plan(_dev(pos_h, i32, "pos_h"), _dev(pos_t, i32, "pos_t"),
                           _dev(codes, i32, "codes") if neg_per_pos else None, C.c_int(neg_per_pos), _dev(part_lo, torch.int64, "part_lo"),
                           C.c_int(n_parts), C.c_int(n_ranks), C.c_int(rank), _dev(slot_h, i32, "slot_h"), _dev(slot_t, i32, "slot_t"),
                           _dev(own_h, i32, "own_h"), _dev(own_t, i32, "own_t"), _dev(counts, i32, "counts"), _stream())
    _check(rc, "mke_oc_plan")


OC_BASES, OC_COUNT, OC_SCORE, OC_APPLY, OC_UPDATE, OC_PASS2 = 1, 2, 4, 8, 16, 32
OC_GVSUM = 64       # peer-direct entity-major: the inbox (mke_oc_run's g_all) summed into the local block (gv), before OC_PASS2


OC_BUCKET_WAVES = 8192
OC_REC_INTS = 3     # an owned-code record: (epoch position, n, code without flags), int32 each


def oc_bucket_codes(codes, n_mine: int, neg_per_pos: int, pos0: int, n_ranks: int, cap: int, need, send, counts, scratch):
    """mke_oc_bucket_codes: this rank's share of the epoch's codes bucketed by the owner of the corrupt entity ((position, n) order
    inside each destination, true counts), and the positions' need flags alone."""
    i32 = torch.int32
    if scratch.numel() < n_ranks * OC_BUCKET_WAVES or counts.numel() < n_ranks or need.numel() < n_mine or send.numel() < OC_REC_INTS * n_ranks * cap:
        raise MultiKEHipError("mke_oc_bucket_codes: need / send / counts / scratch too small")
    rc = lib().mke_oc_bucket_codes(_dev(codes, i32, "codes"), C.c_int64(n_mine), C.c_int(neg_per_pos), C.c_int64(pos0), C.c_int(n_ranks),
                                   C.c_int64(cap), _dev(need, i32, "need"), _dev(send, i32, "send"), _dev(counts, i32, "counts"),
                                   _dev(scratch, i32, "scratch"), _stream())
    _check(rc, "mke_oc_bucket_codes")


def oc_owned_index(recv, counts, n_ranks: int, cap: int, n_all: int, own_rec, own_off):
    """mke_oc_owned_index: the records addressed to this rank packed in (position, n) order, and their offsets per epoch position."""
    i32 = torch.int32
    if own_rec.numel() < OC_REC_INTS * n_ranks * cap or own_off.numel() < n_all + 1 or recv.numel() < OC_REC_INTS * n_ranks * cap or counts.numel() < n_ranks:
        raise MultiKEHipError("mke_oc_owned_index: recv / counts / own_rec / own_off too small")
    rc = lib().mke_oc_owned_index(_dev(recv, i32, "recv"), _dev(counts, i32, "counts"), C.c_int(n_ranks), C.c_int64(cap), C.c_int64(n_all),
                                  _dev(own_rec, i32, "own_rec"), _dev(own_off, i32, "own_off"), _stream())
    _check(rc, "mke_oc_owned_index")


def oc_em_plan_temp_bytes(capacity: int) -> int:
    n = lib().mke_oc_em_plan_temp_bytes(C.c_int64(capacity))
    if n < 0:
        raise MultiKEHipError("mke_oc_em_plan_temp_bytes: capacity out of range")
    return int(n)


def oc_em_plan(args: OcEmPlanArgs):
    """mke_oc_em_plan: the epoch's references to this rank's rows, sorted by (step, row) — struct of raw device addresses."""
    _check(lib().mke_oc_em_plan(C.byref(args), _stream()), "mke_oc_em_plan")


def oc_steps(loop: OcLoopStruct, step_begin: int, step_end: int):
    """mke_oc_steps: global steps [step_begin, step_end) of the current epoch enqueued by one native call."""
    _check(lib().mke_oc_steps(C.byref(loop), C.c_int(step_begin), C.c_int(step_end), _stream()), "mke_oc_steps")


def oc_pass2(step: OcStepStruct):
    _check(lib().mke_oc_pass2(C.byref(step), _stream()), "mke_oc_pass2")


def oc_gv_sum(step: OcStepStruct, inbox, gv):
    """mke_oc_gv_sum: the writers' slices of this rank's gradient inbox summed, in rank order, into the local block `gv`
    (peer-direct entity-major steps only)."""
    rc = lib().mke_oc_gv_sum(C.byref(step), _dev(inbox, torch.float32, "inbox"), _dev(gv, torch.float32, "gv"), _stream())
    _check(rc, "mke_oc_gv_sum")


def oc_run(step: OcStepStruct, phases: int, send, v_all, block_floats: int, g_all, gv, loss_partials):
    """mke_oc_run with RAW device addresses (ints / None) — the caller validated the tensors once per epoch."""
    rc = lib().mke_oc_run(C.byref(step), C.c_int(phases), C.c_void_p(send), C.c_void_p(v_all), C.c_int64(block_floats),
                          C.c_void_p(g_all), C.c_void_p(gv), C.c_void_p(loss_partials), _stream())
    _check(rc, "mke_oc_run")


def ae_scratch_floats(plan: AEPlanStruct, rows: int) -> int:
    n = lib().mke_ae_scratch_floats(C.byref(plan), C.c_int64(rows))
    if n < 0:
        raise MultiKEHipError("mke_ae_scratch_floats: bad plan")
    return int(n)


def ae_train_steps(plan: AEPlanStruct, x: torch.Tensor, batch_rows: int, loss_out: torch.Tensor):
    """mke_ae_train_steps over the rows of x (float32 [n, ldx] CUDA, row-major); loss_out: float64 [n_batches]."""
    rc = lib().mke_ae_train_steps(C.byref(plan), _dev(x, torch.float32, "x"), C.c_int64(x.shape[0]), C.c_int64(x.stride(0)),
                                  C.c_int64(batch_rows), _dev(loss_out, torch.float64, "loss_out"), _stream())
    _check(rc, "mke_ae_train_steps")


AE_ENC, AE_DEC, AE_BWD, AE_UPD, AE_ALL = 1, 2, 4, 8, 15


def ae_step_phases(plan: AEPlanStruct, x, rows: int, ldx: int, global_rows: int, phases: int, loss_out: torch.Tensor):
    """mke_ae_step_phases: one batch of the auto-encoder cut at its batch-wide sums (x: float32 [rows, ldx] CUDA or None)."""
    rc = lib().mke_ae_step_phases(C.byref(plan), (_dev(x, torch.float32, "x") if rows else None), C.c_int64(rows), C.c_int64(ldx),
                                  C.c_int64(global_rows), C.c_int(phases), _dev(loss_out, torch.float64, "loss_out"), _stream())
    _check(rc, "mke_ae_step_phases")


def ae_encode(plan: AEPlanStruct, x: torch.Tensor, out: torch.Tensor):
    rc = lib().mke_ae_encode(C.byref(plan), _dev(x, torch.float32, "x"), C.c_int64(x.shape[0]), C.c_int64(x.stride(0)),
                             _dev(out, torch.float32, "out"), C.c_int64(out.stride(0)), _stream())
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
    rc = lib().mke_dense_layer_fwd(C.c_void_p(x.data_ptr()), C.c_int64(x.stride(0)), C.c_void_p(w.data_ptr()),
                                   C.c_int64(w.stride(0)), _dev(b, torch.float32, "b"), C.c_int(act),
                                   C.c_void_p(out.data_ptr()), C.c_int64(out.stride(0)), C.c_int(M), C.c_int(N), C.c_int(K),
                                   _stream())
    _check(rc, "mke_dense_layer_fwd")


def align_rank(emb1, emb2, kpad, n1, n2, rank, best, ties=None):
    """mke_align_rank over row-major padded emb1 [n1, ld1] / emb2 [n2, ld2]."""
    rc = lib().mke_align_rank(_dev(emb1, torch.float32, "emb1"), C.c_int(emb1.shape[1]), _dev(emb2, torch.float32, "emb2"),
                              C.c_int(emb2.shape[1]), C.c_int(kpad), C.c_int64(n1), C.c_int64(n2),
                              _dev(rank, torch.int32, "rank"), _dev(ties, torch.int32, "ties"), _dev(best, torch.int64, "best"),
                              _stream())
    _check(rc, "mke_align_rank")


METRIC_INNER, METRIC_EUCLIDEAN = 0, 1   # MKE_METRIC_*


class TopkMeanArgs(C.Structure):
    """mke_topk_mean_args"""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int), ("b", C.c_void_p), ("ldb", C.c_int), ("kpad", C.c_int),
                ("n_a", C.c_int64), ("n_b", C.c_int64), ("metric", C.c_int), ("sq_a", C.c_void_p), ("sq_b", C.c_void_p),
                ("k", C.c_int), ("out", C.c_void_p), ("temp", C.c_void_p), ("temp_bytes", C.c_int64)]


class AlignArgs(C.Structure):
    """mke_align_args"""
    _fields_ = [("emb1", C.c_void_p), ("ld1", C.c_int), ("emb2", C.c_void_p), ("ld2", C.c_int), ("kpad", C.c_int),
                ("n1", C.c_int64), ("n2", C.c_int64), ("metric", C.c_int), ("sq1", C.c_void_p), ("sq2", C.c_void_p),
                ("csls_row", C.c_void_p), ("csls_col", C.c_void_p), ("rank", C.c_void_p), ("ties", C.c_void_p),
                ("best", C.c_void_p)]


def align_topk_mean_temp_bytes(n_a: int, n_b: int, kpad: int, k: int) -> int:
    """mke_align_topk_mean_temp_bytes; raises on the arguments mke_align_topk_mean would reject."""
    r = int(lib().mke_align_topk_mean_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(kpad), C.c_int(k)))
    _check(r if r < 0 else 0, "mke_align_topk_mean_temp_bytes")
    return r


def align_topk_mean(a, b, kpad, k, metric=METRIC_INNER, sq_a=None, sq_b=None):
    """mke_align_topk_mean over row-major padded a [n_a, lda] / b [n_b, ldb] -> float32 [n_a]: the mean of each a row's k
    largest similarities to the b rows."""
    n_a, n_b = a.shape[0], b.shape[0]
    need = align_topk_mean_temp_bytes(n_a, n_b, kpad, k)
    out = torch.empty(n_a, dtype=torch.float32, device=a.device)
    temp = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=a.device)
    args = TopkMeanArgs(_dev(a, torch.float32, "a"), a.shape[1], _dev(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                        _dev(sq_a, torch.float32, "sq_a"), _dev(sq_b, torch.float32, "sq_b"), k, _dev(out, torch.float32, "out"),
                        _dev(temp, torch.float32, "temp"), temp.numel() * 4)
    _check(lib().mke_align_topk_mean(C.byref(args), _stream()), "mke_align_topk_mean")
    return out


def align_rank_ex(emb1, emb2, kpad, rank, ties, best, metric=METRIC_INNER, sq1=None, sq2=None, csls_row=None, csls_col=None):
    """mke_align_rank_ex over row-major padded emb1 [n1, ld1] / emb2 [n2, ld2] (rank / ties / best zeroed by the caller)."""
    args = AlignArgs(_dev(emb1, torch.float32, "emb1"), emb1.shape[1], _dev(emb2, torch.float32, "emb2"), emb2.shape[1], kpad,
                     emb1.shape[0], emb2.shape[0], metric, _dev(sq1, torch.float32, "sq1"), _dev(sq2, torch.float32, "sq2"),
                     _dev(csls_row, torch.float32, "csls_row"), _dev(csls_col, torch.float32, "csls_col"),
                     _dev(rank, torch.int32, "rank"), _dev(ties, torch.int32, "ties"), _dev(best, torch.int64, "best"))
    _check(lib().mke_align_rank_ex(C.byref(args), _stream()), "mke_align_rank_ex")


class LseArgs(C.Structure):
    """mke_lse_args"""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int), ("b", C.c_void_p), ("ldb", C.c_int), ("kpad", C.c_int),
                ("n_a", C.c_int64), ("n_b", C.c_int64), ("metric", C.c_int), ("sq_a", C.c_void_p), ("sq_b", C.c_void_p),
                ("sub_b", C.c_void_p), ("tau", C.c_float), ("out", C.c_void_p), ("temp", C.c_void_p), ("temp_bytes", C.c_int64)]


def align_lse_temp_bytes(n_a: int, n_b: int, kpad: int) -> int:
    """mke_align_lse_temp_bytes; raises on the arguments mke_align_lse would reject."""
    r = int(lib().mke_align_lse_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(kpad)))
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
    args = LseArgs(_dev(a, torch.float32, "a"), a.shape[1], _dev(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                   _dev(sq_a, torch.float32, "sq_a"), _dev(sq_b, torch.float32, "sq_b"), _dev(sub_b, torch.float32, "sub_b"),
                   float(tau), _dev(out, torch.float32, "out"), _dev(temp, torch.float32, "temp"), temp.numel() * 4)
    _check(lib().mke_align_lse(C.byref(args), _stream()), "mke_align_lse")
    return out


class StableListsArgs(C.Structure):
    """mke_stable_lists_args"""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int), ("b", C.c_void_p), ("ldb", C.c_int), ("kpad", C.c_int),
                ("n_a", C.c_int64), ("n_b", C.c_int64), ("metric", C.c_int), ("sq_a", C.c_void_p), ("sq_b", C.c_void_p),
                ("csls_row", C.c_void_p), ("csls_col", C.c_void_p), ("sim_mat", C.c_void_p), ("ld_sim", C.c_int64),
                ("cut", C.c_int), ("whole_rows", C.c_int), ("sample_cols", C.c_int), ("out_val", C.c_void_p),
                ("out_col", C.c_void_p), ("flags", C.c_void_p), ("temp", C.c_void_p), ("temp_bytes", C.c_int64)]


class StableMatchArgs(C.Structure):
    """mke_stable_match_args"""
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("cut", C.c_int), ("val", C.c_void_p), ("col", C.c_void_p),
                ("ptr", C.c_void_p), ("holder", C.c_void_p), ("proposals", C.c_void_p), ("n_proposals", C.c_int64),
                ("match", C.c_void_p), ("counts", C.c_void_p)]


def stable_lists_temp_bytes(n_a: int, n_b: int, kpad: int, cut: int, whole_rows: bool = False) -> int:
    """mke_stable_lists_temp_bytes; raises on the arguments mke_stable_lists would reject."""
    r = int(lib().mke_stable_lists_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(kpad), C.c_int(cut), C.c_int(int(whole_rows))))
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
        args.a, args.lda, args.b, args.ldb = _dev(a, torch.float32, "a"), a.shape[1], _dev(b, torch.float32, "b"), b.shape[1]
        args.kpad, args.metric = kpad, metric
        args.sq_a, args.sq_b = _dev(sq_a, torch.float32, "sq_a"), _dev(sq_b, torch.float32, "sq_b")
        args.csls_row, args.csls_col = _dev(csls_row, torch.float32, "csls_row"), _dev(csls_col, torch.float32, "csls_col")
    else:
        if not sim_mat.is_cuda or sim_mat.dtype != torch.float32:
            raise MultiKEHipError("stable_lists: sim_mat must be a float32 CUDA/HIP tensor (no CPU path exists)")
        args.sim_mat, args.ld_sim = C.c_void_p(sim_mat.data_ptr()), sim_mat.stride(0) if n_a > 1 else max(n_b, 1)
    args.n_a, args.n_b, args.cut, args.whole_rows, args.sample_cols = n_a, n_b, cut, int(bool(whole_rows)), sample_cols
    args.out_val, args.out_col = _dev(val, torch.float32, "out_val"), _dev(col, torch.int32, "out_col")
    args.flags, args.temp, args.temp_bytes = _dev(flags, torch.int32, "flags"), _dev(temp, torch.int64, "temp"), temp.numel() * 8
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
    _check(lib().mke_stable_rounds(C.byref(args), C.c_int64(first_round), C.c_int(n_rounds), _stream()), "mke_stable_rounds")


def stable_finish(args: StableMatchArgs):
    """mke_stable_finish: match[i] = the column holding suitor i or -1; counts = (matched, matched to its own index)."""
    _check(lib().mke_stable_finish(C.byref(args), _stream()), "mke_stable_finish")


MUTUAL_NO_LDS_FOLD, MUTUAL_FILTER = 1, 2   # MKE_MUTUAL_*: the other forms of the column fold, for measurements


class MutualArgs(C.Structure):
    """mke_mutual_args"""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int), ("b", C.c_void_p), ("ldb", C.c_int), ("kpad", C.c_int),
                ("n_a", C.c_int64), ("n_b", C.c_int64), ("metric", C.c_int), ("sq_a", C.c_void_p), ("sq_b", C.c_void_p),
                ("csls_row", C.c_void_p), ("csls_col", C.c_void_p), ("row_best", C.c_void_p), ("col_best", C.c_void_p),
                ("flags", C.c_int)]


def align_mutual(a, b, kpad, metric=METRIC_INNER, sq_a=None, sq_b=None, csls_row=None, csls_col=None, flags=0, out=None):
    """mke_align_mutual over row-major padded a [n_a, lda] / b [n_b, ldb] -> (row_best int64 [n_a], col_best int64 [n_b]):
    per row the packed (re-scored similarity, best column), per column the packed (same similarity, best row), from one
    sweep.  `out` = (row_best, col_best) zeroed by the caller, in place of fresh tensors."""
    n_a, n_b = a.shape[0], b.shape[0]
    row_best, col_best = out if out is not None else (torch.zeros(n_a, dtype=torch.int64, device=a.device),
                                                      torch.zeros(n_b, dtype=torch.int64, device=a.device))
    if row_best.numel() < n_a or col_best.numel() < n_b:
        raise MultiKEHipError(f"align_mutual: out holds ({row_best.numel()}, {col_best.numel()}) words, ({n_a}, {n_b}) rows and columns")
    args = MutualArgs(_dev(a, torch.float32, "a"), a.shape[1], _dev(b, torch.float32, "b"), b.shape[1], kpad, n_a, n_b, metric,
                      _dev(sq_a, torch.float32, "sq_a"), _dev(sq_b, torch.float32, "sq_b"),
                      _dev(csls_row, torch.float32, "csls_row"), _dev(csls_col, torch.float32, "csls_col"),
                      _dev(row_best, torch.int64, "row_best"), _dev(col_best, torch.int64, "col_best"), flags)
    _check(lib().mke_align_mutual(C.byref(args), _stream()), "mke_align_mutual")
    return row_best, col_best


def mutual_pairs(row_best, col_best, threshold=float("-inf")):
    """mke_mutual_pairs over the words of align_mutual -> (match int32 [n_a], counts int32 [2]): match[i] = the column whose best
    row is i and that is i's best column, at a value >= threshold, else -1; counts = (matched, matched to its own index)."""
    n_a, n_b = row_best.numel(), col_best.numel()
    match = torch.empty(n_a, dtype=torch.int32, device=row_best.device)
    counts = torch.empty(2, dtype=torch.int32, device=row_best.device)     # zeroed by the call
    rc = lib().mke_mutual_pairs(_dev(row_best, torch.int64, "row_best"), _dev(col_best, torch.int64, "col_best"), C.c_int64(n_a),
                                C.c_int64(n_b), C.c_float(threshold), _dev(match, torch.int32, "match"),
                                _dev(counts, torch.int32, "counts"), _stream())
    _check(rc, "mke_mutual_pairs")
    return match, counts


ASSIGN_TAIL_CAP = 16                       # MKE_ASSIGN_TAIL_CAP: the default hand-over point of the auction's tail kernel
ASSIGN_TAIL_MAX = 4096                     # larger tail_cap values act as this one
ASSIGN_NO_TAIL, ASSIGN_TAIL_ONLY = 1, 2    # MKE_ASSIGN_*
ASSIGN_MIN_EPS = 2.0 ** -14


class AssignArgs(C.Structure):
    """mke_assign_args"""
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("cut", C.c_int), ("val", C.c_void_p), ("col", C.c_void_p),
                ("eps", C.c_float), ("floor", C.c_float), ("state", C.c_void_p), ("price", C.c_void_p), ("owner", C.c_void_p),
                ("bid", C.c_void_p), ("progress", C.c_void_p), ("tail_cap", C.c_int), ("flags", C.c_int), ("temp", C.c_void_p),
                ("temp_bytes", C.c_int64), ("match", C.c_void_p), ("counts", C.c_void_p)]


def assign_temp_bytes(n_a: int, n_b: int, tail_cap: int = 0) -> int:
    """mke_assign_temp_bytes; raises on the arguments mke_assign_rounds would reject."""
    r = int(lib().mke_assign_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), C.c_int(tail_cap)))
    _check(r if r < 0 else 0, "mke_assign_temp_bytes")
    return r


def assign_args(val, col, n_b, eps, floor, state, price, owner, bid, progress, temp, tail_cap=0, flags=0, match=None,
                counts=None) -> AssignArgs:
    """mke_assign_args over the lists val / col [n_a, cut] and the state of a run: state [n_a] int32, price [n_b] float32,
    owner [n_b] int32, bid [n_b] int64, progress [4] int64 (all zeroed before the first round), temp (int32, at least
    assign_temp_bytes); match [n_a] int32 and counts [3] int32 for assign_finish."""
    n_a, cut = col.shape
    return AssignArgs(n_a, n_b, cut, _dev(val, torch.float32, "val"), _dev(col, torch.int32, "col"), float(eps), float(floor),
                      _dev(state, torch.int32, "state"), _dev(price, torch.float32, "price"), _dev(owner, torch.int32, "owner"),
                      _dev(bid, torch.int64, "bid"), _dev(progress, torch.int64, "progress"), tail_cap, flags,
                      _dev(temp, torch.int32, "temp"), temp.numel() * 4 if temp is not None else 0,
                      _dev(match, torch.int32, "match"), _dev(counts, torch.int32, "counts"))


def assign_rounds(args: AssignArgs, n_rounds: int):
    """mke_assign_rounds: enqueue at most n_rounds more rounds of the auction (no synchronisation)."""
    _check(lib().mke_assign_rounds(C.byref(args), C.c_int(n_rounds), _stream()), "mke_assign_rounds")


def assign_finish(args: AssignArgs):
    """mke_assign_finish: match[i] = the column row i holds or -1; counts = (matched, matched to its own index, settled unmatched)."""
    _check(lib().mke_assign_finish(C.byref(args), _stream()), "mke_assign_finish")


SWAP_TILE = 64                             # MKE_SWAP_TILE: triples per tile of the ordered compaction (one wavefront)


class SwapArgs(C.Structure):
    """mke_swap_args"""
    _fields_ = [("h", C.c_void_p), ("p", C.c_void_p), ("t", C.c_void_p), ("n", C.c_int64), ("partner", C.c_void_p),
                ("n_entities", C.c_int64), ("weight", C.c_void_p), ("heads_only", C.c_int), ("out_h", C.c_void_p),
                ("out_p", C.c_void_p), ("out_t", C.c_void_p), ("out_w", C.c_void_p), ("capacity", C.c_int64), ("count", C.c_void_p),
                ("temp", C.c_void_p), ("temp_bytes", C.c_int64), ("flags", C.c_int)]


def boot_partner(match, ids_a, ids_b, n_entities: int, out=None):
    """mke_boot_partner -> partner int32 [n_entities]: -1 everywhere, then partner[ids_a[i]] = ids_b[match[i]] and back for every
    matched row i of the one-to-one `match` int32 [n_a] (-1 = unmatched).  `out` = a table to overwrite instead of a fresh one."""
    partner = out if out is not None else torch.empty(n_entities, dtype=torch.int32, device=match.device)
    if partner.numel() != n_entities:
        raise MultiKEHipError(f"boot_partner: out holds {partner.numel()} words, the table has {n_entities}")
    if match.numel() != ids_a.numel():
        raise MultiKEHipError(f"boot_partner: match has {match.numel()} rows, ids_a {ids_a.numel()}")
    rc = lib().mke_boot_partner(_dev(match, torch.int32, "match"), _dev(ids_a, torch.int32, "ids_a"), C.c_int64(ids_a.numel()),
                                _dev(ids_b, torch.int32, "ids_b"), C.c_int64(ids_b.numel()), _dev(partner, torch.int32, "partner"),
                                C.c_int64(n_entities), _stream())
    _check(rc, "mke_boot_partner")
    return partner


def swap_temp_bytes(n: int) -> int:
    """mke_swap_temp_bytes; raises on an n mke_swap_triples would reject."""
    r = int(lib().mke_swap_temp_bytes(C.c_int64(n)))
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
    args = SwapArgs(_dev(h, torch.int32, "h"), _dev(p, torch.int32, "p"), _dev(t, torch.int32, "t"), n,
                    _dev(partner, torch.int32, "partner"), partner.numel(), _dev(weight, torch.float32, "weight"),
                    1 if heads_only else 0, _dev(out_h, torch.int32, "out_h"), _dev(out_p, torch.int32, "out_p"),
                    _dev(out_t, torch.int32, "out_t"), _dev(out_w, torch.float32, "out_w"), cap, _dev(count, torch.int64, "count"),
                    _dev(temp, torch.int64, "temp"), temp.numel() * 8, 0)
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
    rc = lib().mke_gemm_f32(C.c_void_p(a.data_ptr()), C.c_int64(a.stride(0)), C.c_int64(a.stride(1)),
                            C.c_void_p(b.data_ptr()), C.c_int64(b.stride(0)), C.c_int64(b.stride(1)),
                            C.c_void_p(out.data_ptr()), C.c_int64(out.stride(0)), C.c_int(M), C.c_int(N), C.c_int(K),
                            C.c_int(splits), C.c_int(int(accumulate)), _stream())
    _check(rc, "mke_gemm_f32")


def rows_update_dense(table, slot1, slot2, grad, dim, normalize, opt: OptimizerStruct):
    """mke_rows_update_dense: Adam / Adadelta over EVERY row of the table (grad consumed)."""
    rc = lib().mke_rows_update_dense(_dev(table, torch.float32, "table"), _dev(slot1, torch.float32, "slot1"),
                                     _dev(slot2, torch.float32, "slot2"), _dev(grad, torch.float32, "grad"),
                                     C.c_int64(table.shape[0]), C.c_int(table.shape[1]), C.c_int(dim), C.c_int(int(normalize)),
                                     C.byref(opt), _stream())
    _check(rc, "mke_rows_update_dense")


def dense_update_opt(param, slot1, slot2, grad, opt: OptimizerStruct):
    """mke_dense_update_opt: Adam / Adadelta over a flat parameter buffer (grad consumed)."""
    rc = lib().mke_dense_update_opt(_dev(param, torch.float32, "param"), _dev(slot1, torch.float32, "slot1"),
                                    _dev(slot2, torch.float32, "slot2"), _dev(grad, torch.float32, "grad"),
                                    C.c_int64(param.numel()), C.byref(opt), _stream())
    _check(rc, "mke_dense_update_opt")


def attr_scratch_floats(n: int, dim: int) -> int:
    return int(lib().mke_attr_scratch_floats(C.c_int64(n), C.c_int(dim)))


def attr_steps(args: AttrStepArgs, step_off: np.ndarray, loss_ring: torch.Tensor):
    """mke_attr_steps: `step_off` host int64 [n_steps + 1]; loss_ring float64 [ring, LOSS_PARTIALS] on the device."""
    off = np.ascontiguousarray(step_off, dtype=np.int64)
    rc = lib().mke_attr_steps(C.byref(args), off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(len(off) - 1),
                              _dev(loss_ring, torch.float64, "loss_ring"), C.c_int(loss_ring.shape[0]), _stream())
    _check(rc, "mke_attr_steps")


def sample_distinct(n: int, batch: int, n_steps: int, seed=(0, 0), stream_id: int = 0, device="cuda") -> torch.Tensor:
    """mke_sample_distinct -> int32 [n_steps, batch]: `batch` distinct positions of range(n) per step."""
    out = torch.empty(n_steps, batch, dtype=torch.int32, device=device)
    rc = lib().mke_sample_distinct(C.c_int64(n), C.c_int(batch), C.c_int(n_steps), C.c_uint32(seed[0] & 0xFFFFFFFF),
                                   C.c_uint32(seed[1] & 0xFFFFFFFF), C.c_uint32(stream_id & 0xFFFFFFFF),
                                   _dev(out, torch.int32, "out"), _stream())
    _check(rc, "mke_sample_distinct")
    return out


ATTR_FWD, ATTR_TAIL, ATTR_BWD, ATTR_UPD = 1, 2, 4, 8


def attr_step_phases(args: AttrStepArgs, phases: int):
    rc = lib().mke_attr_step_phases(C.byref(args), C.c_int(phases), _stream())
    _check(rc, "mke_attr_step_phases")


def attr_step(args: AttrStepArgs):
    rc = lib().mke_attr_step(C.byref(args), _stream())
    _check(rc, "mke_attr_step")
