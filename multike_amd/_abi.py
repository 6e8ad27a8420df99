"""generated from include/multike_hip.h by tools/gen_abi.py — do not edit

The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,
and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).
"""
import ctypes as C

VERSION = 107
OK = 0
E_NULL = -1
E_SHAPE = -2
E_UNSUPPORTED = -3
E_RANGE = -4
LOSS_PARTIALS = 2048
MAX_STRIDE = 320
OPT_ADAGRAD = 0
OPT_SGD = 1
OPT_ADAM = 2
OPT_ADADELTA = 3
TUNE_DEFAULT = -2
CODE_ENT_BITS = 26
CODE_HEAD = 0x4000000
CODE_FAST = 0x8000000
CODE_EXCL = 0x10000000
MAX_UPDATE_TABLES = 4
ALIGN_MAX_TABLES = 4
ALIGN_MAX_TERMS = 4
ATTR_FWD = 1
ATTR_TAIL = 2
ATTR_BWD = 4
ATTR_UPD = 8
ATTR_ALL = 15
MAPPING_MAX_VIEWS = 3
MAP_FWD = 1
MAP_TAIL = 2
MAP_BWD = 4
MAP_UPD = 8
MAP_ALL = 15
METRIC_INNER = 0
METRIC_EUCLIDEAN = 1
MUTUAL_NO_LDS_FOLD = 1
MUTUAL_FILTER = 2
ASSIGN_TAIL_CAP = 16
ASSIGN_NO_TAIL = 1
ASSIGN_TAIL_ONLY = 2
SWAP_TILE = 64
AE_MAX_LAYERS = 4
AE_ENC = 1
AE_DEC = 2
AE_BWD = 4
AE_UPD = 8
AE_ALL = 15
OC_MAX_RANKS = 16
OC_NEED_HR = 0x40000000
OC_NEED_RT = 0x80000000
OC_EM_MAX_CHUNKS = 4
OC_EM_WAVES = 32768
OC_BASES = 1
OC_COUNT = 2
OC_SCORE = 4
OC_APPLY = 8
OC_UPDATE = 16
OC_PASS2 = 32
OC_GVSUM = 64
OC_BUCKET_WAVES = 8192
OC_COMM_NCCL = 0
OC_COMM_CALLBACK = 1
OC_COMM_LOOPBACK = 2


class mke_tuning(C.Structure):
    _fields_ = [
        ("score_splits", C.c_int),
        ("score_half_groups", C.c_int),
        ("score_offsets32", C.c_int),
        ("score_lane_ids", C.c_int),
        ("count_in_score", C.c_int),
        ("update_chunk", C.c_int),
        ("oc_score_quarter", C.c_int),
        ("attr_fused_bwd", C.c_int),
        ("retired_sampler_fast", C.c_int),
        ("neg_codes", C.c_int),
        ("sampler_codes", C.c_int),
        ("retired_sampler_lean", C.c_int),
        ("reserved", C.c_int * 4),
    ]


class mke_count_job(C.Structure):
    _fields_ = [
        ("pos_h", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("n_pos", C.c_int64),
        ("neg_h", C.c_void_p),
        ("neg_t", C.c_void_p),
        ("n_neg", C.c_int64),
        ("neg_per_pos", C.c_int),
        ("ref_count", C.c_void_p),
    ]


class mke_hot_rows(C.Structure):
    _fields_ = [
        ("slot", C.c_void_p),
        ("n_hot", C.c_int32),
        ("copies", C.c_int32),
        ("row0", C.c_int64),
    ]


class mke_score_args(C.Structure):
    _fields_ = [
        ("ent_table", C.c_void_p),
        ("n_ent", C.c_int64),
        ("ent_normalize", C.c_int),
        ("rel_table", C.c_void_p),
        ("n_rel", C.c_int64),
        ("rel_normalize", C.c_int),
        ("stride", C.c_int),
        ("dim", C.c_int),
        ("pos_h", C.c_void_p),
        ("pos_r", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("pos_w", C.c_void_p),
        ("n_pos", C.c_int64),
        ("neg_h", C.c_void_p),
        ("neg_r", C.c_void_p),
        ("neg_t", C.c_void_p),
        ("neg_w", C.c_void_p),
        ("n_neg", C.c_int64),
        ("neg_per_pos", C.c_int),
        ("scale", C.c_float),
        ("grad_ent", C.c_void_p),
        ("grad_rel", C.c_void_p),
        ("grad_rel_copies", C.c_int),
        ("touched_ent", C.c_void_p),
        ("touched_rel", C.c_void_p),
        ("tag", C.c_int32),
        ("ref_count", C.c_void_p),
        ("ent_acc", C.c_void_p),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("next_count", C.c_void_p),
        ("hot", mke_hot_rows),
        ("stage_rows", C.c_void_p),
        ("stage_keys", C.c_void_p),
        ("stage_slots", C.c_int64),
        ("loss_partials", C.c_void_p),
        ("tuning", C.c_void_p),
        ("neg_code", C.c_void_p),
    ]


class mke_update_table(C.Structure):
    _fields_ = [
        ("table", C.c_void_p),
        ("acc", C.c_void_p),
        ("grad", C.c_void_p),
        ("touched", C.c_void_p),
        ("n_rows", C.c_int64),
        ("normalize", C.c_int),
        ("grad_copies", C.c_int),
        ("ref_count", C.c_void_p),
        ("src_rows", C.c_void_p),
        ("slot_of", C.c_void_p),
        ("n_ranks", C.c_int),
        ("capacity", C.c_int64),
        ("hot", mke_hot_rows),
        ("bits", C.c_void_p),
        ("pos_h", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("n_pos", C.c_int64),
    ]


class mke_kg_side(C.Structure):
    _fields_ = [
        ("ent_list", C.c_void_p),
        ("ent_lo", C.c_int32),
        ("n_ent", C.c_int32),
        ("cand_table", C.c_void_p),
        ("cand_valid", C.c_void_p),
        ("cand_k", C.c_int32),
        ("known_keys", C.c_void_p),
        ("known_capacity", C.c_uint64),
    ]


class mke_align_table(C.Structure):
    _fields_ = [
        ("table", C.c_void_p),
        ("acc", C.c_void_p),
        ("grad", C.c_void_p),
        ("touched", C.c_void_p),
        ("n_rows", C.c_int64),
        ("normalize", C.c_int),
    ]


class mke_align_term(C.Structure):
    _fields_ = [
        ("a", C.c_int),
        ("b", C.c_int),
        ("weight", C.c_float),
    ]


class mke_align_plan(C.Structure):
    _fields_ = [
        ("tables", mke_align_table * 4),
        ("n_tables", C.c_int),
        ("terms", mke_align_term * 4),
        ("n_terms", C.c_int),
        ("stride", C.c_int),
        ("dim", C.c_int),
        ("ia", C.c_void_p),
        ("ib", C.c_void_p),
        ("step_off", C.c_void_p),
        ("n_steps", C.c_int),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("tag_base", C.c_int32),
        ("loss_partials", C.c_void_p),
    ]


class mke_relation_plan(C.Structure):
    _fields_ = [
        ("ent_table", C.c_void_p),
        ("n_ent", C.c_int64),
        ("ent_normalize", C.c_int),
        ("rel_table", C.c_void_p),
        ("n_rel", C.c_int64),
        ("rel_normalize", C.c_int),
        ("ent_acc", C.c_void_p),
        ("rel_acc", C.c_void_p),
        ("ent_grad", C.c_void_p),
        ("rel_grad", C.c_void_p),
        ("rel_grad_copies", C.c_int),
        ("ent_touched", C.c_void_p),
        ("rel_touched", C.c_void_p),
        ("ent_ref_count", C.c_void_p),
        ("overlap", C.c_int),
        ("neg_chunk_capacity", C.c_int64),
        ("stride", C.c_int),
        ("dim", C.c_int),
        ("pos_h", C.c_void_p),
        ("pos_r", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("pos_kg", C.c_void_p),
        ("step_off", C.c_void_p),
        ("n_steps", C.c_int),
        ("sides", mke_kg_side * 2),
        ("neg_per_pos", C.c_int),
        ("max_try", C.c_int),
        ("sample_chunk", C.c_int),
        ("negatives_ready", C.c_int),
        ("neg_h", C.c_void_p),
        ("neg_r", C.c_void_p),
        ("neg_t", C.c_void_p),
        ("seed_lo", C.c_uint32),
        ("seed_hi", C.c_uint32),
        ("stream_id", C.c_uint32),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("scale", C.c_float),
        ("loss_partials", C.c_void_p),
        ("loss_ring", C.c_int),
        ("tag_base", C.c_int32),
        ("pos_w", C.c_void_p),
        ("hot", mke_hot_rows),
        ("tuning", C.c_void_p),
        ("step_off_dev", C.c_void_p),
        ("neg_code", C.c_void_p),
        ("code_bits", C.c_void_p),
        ("code_bits_words", C.c_int64),
        ("ids_stale", C.c_void_p),
    ]


class mke_candidate(C.Structure):
    _fields_ = [
        ("idx", C.c_int32),
        ("sim", C.c_float),
    ]


class mke_attr_step_args(C.Structure):
    _fields_ = [
        ("ent_table", C.c_void_p),
        ("n_ent", C.c_int64),
        ("ent_stride", C.c_int),
        ("ent_normalize", C.c_int),
        ("ent_acc", C.c_void_p),
        ("ent_grad", C.c_void_p),
        ("ent_touched", C.c_void_p),
        ("attr_table", C.c_void_p),
        ("n_attr", C.c_int64),
        ("attr_stride", C.c_int),
        ("attr_normalize", C.c_int),
        ("attr_acc", C.c_void_p),
        ("attr_grad", C.c_void_p),
        ("attr_touched", C.c_void_p),
        ("lit_table", C.c_void_p),
        ("lit_stride", C.c_int),
        ("dim", C.c_int),
        ("ih", C.c_void_p),
        ("ia", C.c_void_p),
        ("iv", C.c_void_p),
        ("weights", C.c_void_p),
        ("n", C.c_int64),
        ("scale", C.c_float),
        ("params", C.c_void_p),
        ("param_grads", C.c_void_p),
        ("param_acc", C.c_void_p),
        ("scratch", C.c_void_p),
        ("partials", C.c_void_p),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("tag", C.c_int32),
        ("update", C.c_int),
        ("workspace", C.c_void_p),
        ("attr_grad_copies", C.c_int),
        ("tuning", C.c_void_p),
    ]


class mke_optimizer(C.Structure):
    _fields_ = [
        ("kind", C.c_int),
        ("lr", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("epsilon", C.c_float),
        ("rho", C.c_float),
        ("step", C.c_int64),
    ]


class mke_mapping_view(C.Structure):
    _fields_ = [
        ("table", C.c_void_p),
        ("normalize", C.c_int),
    ]


class mke_mapping_step_args(C.Structure):
    _fields_ = [
        ("ent_table", C.c_void_p),
        ("n_ent", C.c_int64),
        ("ent_normalize", C.c_int),
        ("ent_acc", C.c_void_p),
        ("ent_grad", C.c_void_p),
        ("ent_touched", C.c_void_p),
        ("views", mke_mapping_view * 3),
        ("n_views", C.c_int),
        ("stride", C.c_int),
        ("dim", C.c_int),
        ("idx", C.c_void_p),
        ("n", C.c_int64),
        ("M", C.c_void_p),
        ("gM", C.c_void_p),
        ("accM", C.c_void_p),
        ("orthogonal_weight", C.c_float),
        ("norm_w", C.c_float),
        ("scratch", C.c_void_p),
        ("partials", C.c_void_p),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("tag", C.c_int32),
        ("update", C.c_int),
    ]


class mke_topk_mean_args(C.Structure):
    _fields_ = [
        ("a", C.c_void_p),
        ("lda", C.c_int),
        ("b", C.c_void_p),
        ("ldb", C.c_int),
        ("kpad", C.c_int),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("metric", C.c_int),
        ("sq_a", C.c_void_p),
        ("sq_b", C.c_void_p),
        ("k", C.c_int),
        ("out", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
    ]


class mke_align_args(C.Structure):
    _fields_ = [
        ("emb1", C.c_void_p),
        ("ld1", C.c_int),
        ("emb2", C.c_void_p),
        ("ld2", C.c_int),
        ("kpad", C.c_int),
        ("n1", C.c_int64),
        ("n2", C.c_int64),
        ("metric", C.c_int),
        ("sq1", C.c_void_p),
        ("sq2", C.c_void_p),
        ("csls_row", C.c_void_p),
        ("csls_col", C.c_void_p),
        ("rank", C.c_void_p),
        ("ties", C.c_void_p),
        ("best", C.c_void_p),
    ]


class mke_stable_lists_args(C.Structure):
    _fields_ = [
        ("a", C.c_void_p),
        ("lda", C.c_int),
        ("b", C.c_void_p),
        ("ldb", C.c_int),
        ("kpad", C.c_int),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("metric", C.c_int),
        ("sq_a", C.c_void_p),
        ("sq_b", C.c_void_p),
        ("csls_row", C.c_void_p),
        ("csls_col", C.c_void_p),
        ("sim_mat", C.c_void_p),
        ("ld_sim", C.c_int64),
        ("cut", C.c_int),
        ("whole_rows", C.c_int),
        ("sample_cols", C.c_int),
        ("out_val", C.c_void_p),
        ("out_col", C.c_void_p),
        ("flags", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
    ]


class mke_stable_match_args(C.Structure):
    _fields_ = [
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("cut", C.c_int),
        ("val", C.c_void_p),
        ("col", C.c_void_p),
        ("ptr", C.c_void_p),
        ("holder", C.c_void_p),
        ("proposals", C.c_void_p),
        ("n_proposals", C.c_int64),
        ("match", C.c_void_p),
        ("counts", C.c_void_p),
    ]


class mke_lse_args(C.Structure):
    _fields_ = [
        ("a", C.c_void_p),
        ("lda", C.c_int),
        ("b", C.c_void_p),
        ("ldb", C.c_int),
        ("kpad", C.c_int),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("metric", C.c_int),
        ("sq_a", C.c_void_p),
        ("sq_b", C.c_void_p),
        ("sub_b", C.c_void_p),
        ("tau", C.c_float),
        ("out", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
    ]


class mke_mutual_args(C.Structure):
    _fields_ = [
        ("a", C.c_void_p),
        ("lda", C.c_int),
        ("b", C.c_void_p),
        ("ldb", C.c_int),
        ("kpad", C.c_int),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("metric", C.c_int),
        ("sq_a", C.c_void_p),
        ("sq_b", C.c_void_p),
        ("csls_row", C.c_void_p),
        ("csls_col", C.c_void_p),
        ("row_best", C.c_void_p),
        ("col_best", C.c_void_p),
        ("flags", C.c_int),
    ]


class mke_assign_args(C.Structure):
    _fields_ = [
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("cut", C.c_int),
        ("val", C.c_void_p),
        ("col", C.c_void_p),
        ("eps", C.c_float),
        ("floor", C.c_float),
        ("state", C.c_void_p),
        ("price", C.c_void_p),
        ("owner", C.c_void_p),
        ("bid", C.c_void_p),
        ("progress", C.c_void_p),
        ("tail_cap", C.c_int),
        ("flags", C.c_int),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
        ("match", C.c_void_p),
        ("counts", C.c_void_p),
    ]


class mke_swap_args(C.Structure):
    _fields_ = [
        ("h", C.c_void_p),
        ("p", C.c_void_p),
        ("t", C.c_void_p),
        ("n", C.c_int64),
        ("partner", C.c_void_p),
        ("n_entities", C.c_int64),
        ("weight", C.c_void_p),
        ("heads_only", C.c_int),
        ("out_h", C.c_void_p),
        ("out_p", C.c_void_p),
        ("out_t", C.c_void_p),
        ("out_w", C.c_void_p),
        ("capacity", C.c_int64),
        ("count", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
        ("flags", C.c_int),
    ]


class mke_ae_plan(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int),
        ("dims", C.c_int * 5),
        ("act", C.c_int),
        ("normalize", C.c_int),
        ("params", C.c_void_p),
        ("grads", C.c_void_p),
        ("acc", C.c_void_p),
        ("n_params", C.c_int64),
        ("w_off", C.c_int64 * 8),
        ("b_off", C.c_int64 * 8),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("update", C.c_int),
        ("scratch", C.c_void_p),
        ("scratch_floats", C.c_int64),
        ("partials", C.c_void_p),
        ("scalars", C.c_void_p),
    ]


class mke_oc_step(C.Structure):
    _fields_ = [
        ("ent", C.c_void_p),
        ("ent_acc", C.c_void_p),
        ("ent_grad", C.c_void_p),
        ("ent_touched", C.c_void_p),
        ("ref_count", C.c_void_p),
        ("n_local", C.c_int64),
        ("rel", C.c_void_p),
        ("rel_acc", C.c_void_p),
        ("rel_grad", C.c_void_p),
        ("rel_grad_copies", C.c_int),
        ("rel_touched", C.c_void_p),
        ("n_rel", C.c_int64),
        ("stride", C.c_int),
        ("dim", C.c_int),
        ("rank", C.c_int),
        ("n_ranks", C.c_int),
        ("pos_h", C.c_void_p),
        ("pos_r", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("n_pos", C.c_int64),
        ("per", C.c_int64),
        ("slot_h", C.c_void_p),
        ("slot_t", C.c_void_p),
        ("own_h", C.c_void_p),
        ("n_own_h", C.c_int64),
        ("own_t", C.c_void_p),
        ("n_own_t", C.c_int64),
        ("neg_per_pos", C.c_int),
        ("capacity", C.c_int64),
        ("codes", C.c_void_p),
        ("code_off", C.c_int64 * 16),
        ("optimizer", C.c_int),
        ("lr", C.c_float),
        ("scale", C.c_float),
        ("tag", C.c_int32),
        ("n_peers", C.c_int),
        ("peer_v", C.c_void_p * 16),
        ("peer_g", C.c_void_p * 16),
        ("pos_w", C.c_void_p),
        ("hot", mke_hot_rows),
        ("em_coef", C.c_void_p),
        ("em_pos0", C.c_int64),
        ("em_refs", C.c_void_p),
        ("em_rows", C.c_void_p),
        ("em_off", C.c_void_p),
        ("em_n_rows", C.c_int64),
        ("em_chunks", C.c_int),
        ("em_block_floats", C.c_int64),
        ("em_v", C.c_void_p * 4),
        ("em_gv", C.c_void_p * 4),
        ("em_part", C.c_void_p),
        ("em_long_rows", C.c_void_p),
        ("em_long_part0", C.c_void_p),
        ("em_n_long", C.c_int64),
        ("em_part0", C.c_int64),
        ("em_partials", C.c_void_p),
        ("em_mode", C.c_int),
        ("tuning", C.c_void_p),
        ("own_rec", C.c_void_p),
        ("own_off", C.c_void_p),
    ]


class mke_oc_em_plan_args(C.Structure):
    _fields_ = [
        ("pos_h", C.c_void_p),
        ("pos_r", C.c_void_p),
        ("pos_t", C.c_void_p),
        ("codes", C.c_void_p),
        ("neg_per_pos", C.c_int),
        ("slot_h", C.c_void_p),
        ("slot_t", C.c_void_p),
        ("step_lo", C.c_void_p),
        ("n_steps", C.c_int),
        ("chunks", C.c_int),
        ("n_all", C.c_int64),
        ("max_step", C.c_int64),
        ("n_ranks", C.c_int),
        ("rank", C.c_int),
        ("n_local", C.c_int64),
        ("n_rel", C.c_int64),
        ("keys", C.c_void_p),
        ("keys_alt", C.c_void_p),
        ("capacity", C.c_int64),
        ("vals_alt", C.c_void_p),
        ("scratch8", C.c_void_p),
        ("wave_scratch", C.c_void_p),
        ("refs", C.c_void_p),
        ("rows", C.c_void_p),
        ("off", C.c_void_p),
        ("flags", C.c_void_p),
        ("scan", C.c_void_p),
        ("step_row0", C.c_void_p),
        ("n_refs", C.c_void_p),
        ("item_row", C.c_void_p),
        ("item_off", C.c_void_p),
        ("item_part", C.c_void_p),
        ("long_row", C.c_void_p),
        ("long_part0", C.c_void_p),
        ("step_item0", C.c_void_p),
        ("step_long0", C.c_void_p),
        ("step_part0", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
        ("own_rec", C.c_void_p),
        ("own_off", C.c_void_p),
        ("own_cap", C.c_int64),
    ]


class mke_oc_comm(C.Structure):
    _fields_ = [
        ("kind", C.c_int),
        ("ctx", C.c_void_p),
        ("all_gather", C.c_void_p),
        ("reduce_scatter", C.c_void_p),
        ("all_reduce", C.c_void_p),
        ("world", C.c_int),
        ("rank", C.c_int),
        ("wire_gbps", C.c_float),
        ("latency_us", C.c_float),
    ]


class mke_oc_loop(C.Structure):
    _fields_ = [
        ("parts", C.c_void_p),
        ("step_part0", C.c_void_p),
        ("n_steps", C.c_int),
        ("chunks", C.c_int),
        ("send", C.c_void_p * 4),
        ("v_all", C.c_void_p * 4),
        ("g_all", C.c_void_p * 4),
        ("gv", C.c_void_p * 4),
        ("block_floats", C.c_int64),
        ("loss_ring", C.c_void_p),
        ("loss_stride", C.c_int64),
        ("tag_base", C.c_int32),
        ("comm", C.c_void_p),
        ("comm_stream", C.c_void_p),
        ("overlap_rs", C.c_int),
    ]


STRUCTS = (mke_tuning, mke_count_job, mke_hot_rows, mke_score_args, mke_update_table, mke_kg_side, mke_align_table, mke_align_term, mke_align_plan, mke_relation_plan, mke_candidate, mke_attr_step_args, mke_optimizer, mke_mapping_view, mke_mapping_step_args, mke_topk_mean_args, mke_align_args, mke_stable_lists_args, mke_stable_match_args, mke_lse_args, mke_mutual_args, mke_assign_args, mke_swap_args, mke_ae_plan, mke_oc_step, mke_oc_em_plan_args, mke_oc_comm, mke_oc_loop)

FUNCTIONS = {
    "mke_version": (C.c_int, ()),
    "mke_last_error": (C.c_char_p, ()),
    "mke_tuning_init": (C.c_int, (C.POINTER(mke_tuning),)),
    "mke_set_option": (C.c_int, (C.c_char_p, C.c_int, C.c_void_p,)),
    "mke_triple_score_fwd_bwd": (C.c_int, (C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,)),
    "mke_triple_score_step": (C.c_int, (C.POINTER(mke_score_args), C.c_void_p,)),
    "mke_stage_reduce": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,)),
    "mke_count_entity_refs": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_neg_code_row_words": (C.c_int64, (C.c_int64,)),
    "mke_neg_codes": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,)),
    "mke_rows_update": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,)),
    "mke_rows_update_multi": (C.c_int, (C.POINTER(mke_update_table), C.c_int, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,)),
    "mke_rows_update_multi_count": (C.c_int, (C.POINTER(mke_update_table), C.c_int, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(mke_count_job), C.c_void_p,)),
    "mke_neg_sample": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(mke_kg_side), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_neg_sample_at": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(mke_kg_side), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_tripleset_build": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p,)),
    "mke_tripleset_forget": (C.c_int, (C.c_void_p,)),
    "mke_tripleset_filter_bytes": (C.c_int64, (C.c_void_p, C.c_uint64,)),
    "mke_tripleset_query": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,)),
    "mke_sample_distinct": (C.c_int, (C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,)),
    "mke_epoch_positives": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_gathered_logistic_fwd_bwd": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_gathered_alignment_fwd_bwd": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_align_fwd_bwd": (C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,)),
    "mke_align_steps": (C.c_int, (C.POINTER(mke_align_plan), C.c_void_p,)),
    "mke_gather_rows": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,)),
    "mke_probe_rows": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,)),
    "mke_relation_steps": (C.c_int, (C.POINTER(mke_relation_plan), C.c_int, C.c_int, C.c_void_p,)),
    "mke_sim_select": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(mke_candidate), C.c_void_p, C.c_void_p,)),
    "mke_sim_sample": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_topk_candidates": (C.c_int, (C.POINTER(mke_candidate), C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_topk_long": (C.c_int, (C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_topk_rows": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_rowset_build": (C.c_int, (C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,)),
    "mke_rowset_remap": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,)),
    "mke_rows_gather_padded": (C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_rows_scatter_add": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,)),
    "mke_attr_conv_fwd": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,)),
    "mke_attr_conv_bwd": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,)),
    "mke_attr_tail_z": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_attr_tail_loss": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,)),
    "mke_attr_tail_bwd": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_attr_scratch_floats": (C.c_int64, (C.c_int64, C.c_int,)),
    "mke_attr_step": (C.c_int, (C.POINTER(mke_attr_step_args), C.c_void_p,)),
    "mke_attr_step_phases": (C.c_int, (C.POINTER(mke_attr_step_args), C.c_int, C.c_void_p,)),
    "mke_attr_steps": (C.c_int, (C.POINTER(mke_attr_step_args), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,)),
    "mke_rows_update_dense": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(mke_optimizer), C.c_void_p,)),
    "mke_dense_update_opt": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(mke_optimizer), C.c_void_p,)),
    "mke_mapping_scratch_floats": (C.c_int64, (C.c_int64, C.c_int,)),
    "mke_mapping_step": (C.c_int, (C.POINTER(mke_mapping_step_args), C.c_void_p, C.c_void_p,)),
    "mke_mapping_step_phases": (C.c_int, (C.POINTER(mke_mapping_step_args), C.c_void_p, C.c_int, C.c_void_p,)),
    "mke_mapping_steps": (C.c_int, (C.POINTER(mke_mapping_step_args), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,)),
    "mke_dense_update": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p,)),
    "mke_align_rank": (C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_align_topk_mean_temp_bytes": (C.c_int64, (C.c_int64, C.c_int64, C.c_int, C.c_int,)),
    "mke_align_topk_mean": (C.c_int, (C.POINTER(mke_topk_mean_args), C.c_void_p,)),
    "mke_align_rank_ex": (C.c_int, (C.POINTER(mke_align_args), C.c_void_p,)),
    "mke_stable_lists_temp_bytes": (C.c_int64, (C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,)),
    "mke_stable_lists": (C.c_int, (C.POINTER(mke_stable_lists_args), C.c_void_p,)),
    "mke_stable_rounds": (C.c_int, (C.POINTER(mke_stable_match_args), C.c_int64, C.c_int, C.c_void_p,)),
    "mke_stable_finish": (C.c_int, (C.POINTER(mke_stable_match_args), C.c_void_p,)),
    "mke_align_lse_temp_bytes": (C.c_int64, (C.c_int64, C.c_int64, C.c_int,)),
    "mke_align_lse": (C.c_int, (C.POINTER(mke_lse_args), C.c_void_p,)),
    "mke_align_mutual": (C.c_int, (C.POINTER(mke_mutual_args), C.c_void_p,)),
    "mke_mutual_pairs": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_assign_temp_bytes": (C.c_int64, (C.c_int64, C.c_int64, C.c_int,)),
    "mke_assign_rounds": (C.c_int, (C.POINTER(mke_assign_args), C.c_int, C.c_void_p,)),
    "mke_assign_finish": (C.c_int, (C.POINTER(mke_assign_args), C.c_void_p,)),
    "mke_boot_partner": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,)),
    "mke_swap_temp_bytes": (C.c_int64, (C.c_int64,)),
    "mke_swap_triples": (C.c_int, (C.POINTER(mke_swap_args), C.c_void_p,)),
    "mke_gemm_f32": (C.c_int, (C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,)),
    "mke_ae_scratch_floats": (C.c_int64, (C.POINTER(mke_ae_plan), C.c_int64,)),
    "mke_ae_train_steps": (C.c_int, (C.POINTER(mke_ae_plan), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,)),
    "mke_ae_step_phases": (C.c_int, (C.POINTER(mke_ae_plan), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_ae_encode": (C.c_int, (C.POINTER(mke_ae_plan), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,)),
    "mke_dense_layer_fwd": (C.c_int, (C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,)),
    "mke_oc_block_floats": (C.c_int64, (C.c_int64, C.c_int,)),
    "mke_oc_pack_codes": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,)),
    "mke_oc_plan": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_bases": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p, C.c_void_p,)),
    "mke_oc_count": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p,)),
    "mke_oc_score": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_apply": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p, C.c_void_p,)),
    "mke_oc_gv_sum": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_run": (C.c_int, (C.POINTER(mke_oc_step), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_em_plan_temp_bytes": (C.c_int64, (C.c_int64,)),
    "mke_oc_em_plan": (C.c_int, (C.POINTER(mke_oc_em_plan_args), C.c_void_p,)),
    "mke_oc_pass2": (C.c_int, (C.POINTER(mke_oc_step), C.c_void_p,)),
    "mke_oc_bucket_codes": (C.c_int, (C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_owned_index": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_oc_steps": (C.c_int, (C.POINTER(mke_oc_loop), C.c_int, C.c_int, C.c_void_p,)),
    "mke_rows_update_multi_t": (C.c_int, (C.POINTER(mke_update_table), C.c_int, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(mke_count_job), C.POINTER(mke_tuning), C.c_void_p,)),
}
