"""CPU-side checks of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol
include/multike_hip.h declares, and argument validation returns error codes (no compute without a GPU).  That the ctypes
structs, prototypes and constants are the header's: test_abi_generated.py."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _header():
    with open(os.path.join(ROOT, "include", "multike_hip.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def test_header_symbols_are_exported_and_bound(lib):
    from multike_amd import _lib
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(mke_\w+)\s*\(", _header(), flags=re.M))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    raw = C.CDLL(_lib.SO_PATH)
    for sym in declared:
        assert getattr(raw, sym) is not None


def test_version_and_constants(lib):
    from multike_amd import _lib
    h = _header()
    assert lib.mke_version() == int(re.search(r"#define MKE_VERSION (\d+)", h).group(1))
    assert _lib.LOSS_PARTIALS == int(re.search(r"#define MKE_LOSS_PARTIALS (\d+)", h).group(1))
    assert _lib.MAX_STRIDE == int(re.search(r"#define MKE_MAX_STRIDE (\d+)", h).group(1))


def test_argument_validation_without_gpu(lib):
    """Bad arguments are rejected before any launch: error code < 0 and a message."""
    null = C.c_void_p(0)
    rc = lib.mke_rows_update(null, null, null, C.c_int(1), null, C.c_int32(1), C.c_int64(4), C.c_int(80), C.c_int(75), C.c_int(1),
                             C.c_int(0), C.c_float(0.1), null)
    assert rc == -1 and b"NULL" in lib.mke_last_error()
    one = C.c_void_p(16)
    rc = lib.mke_rows_update(one, one, one, C.c_int(1), one, C.c_int32(1), C.c_int64(4), C.c_int(75), C.c_int(75), C.c_int(1),
                             C.c_int(0), C.c_float(0.1), null)
    assert rc == -2 and b"stride" in lib.mke_last_error()
    rc = lib.mke_rows_update(one, one, one, C.c_int(1), one, C.c_int32(1), C.c_int64(4), C.c_int(80), C.c_int(75), C.c_int(1),
                             C.c_int(7), C.c_float(0.1), null)
    assert rc == -3
    rc = lib.mke_gathered_logistic_fwd_bwd(one, one, one, null, C.c_int64(3), C.c_int(75), C.c_int(75), C.c_int(2), null,
                                           null, null, one, null)
    assert rc == -2 and b"sign" in lib.mke_last_error()
    # empty work is a no-op success without touching the device
    assert lib.mke_rows_update(one, one, one, C.c_int(1), one, C.c_int32(1), C.c_int64(0), C.c_int(80), C.c_int(75), C.c_int(1),
                               C.c_int(0), C.c_float(0.1), null) == 0


def test_product_refuses_cpu_tensors():
    import torch
    from multike_amd import _lib
    from multike_amd import losses
    with pytest.raises(_lib.MultiKEHipError, match="no CPU path"):
        losses.alignment_loss(torch.zeros(2, 75), torch.zeros(2, 75))


def test_product_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under multike_amd/ may reference it."""
    pkg = os.path.join(ROOT, "multike_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h")):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn
                assert "libmke_oracle" not in src, fn


def test_stride_for():
    from multike_amd import _lib
    assert _lib.stride_for(75) == 80 and _lib.stride_for(256) == 256 and _lib.stride_for(4) == 16
    assert _lib.stride_for(100) == 112 and _lib.stride_for(129) == 160
    with pytest.raises(_lib.MultiKEHipError):
        _lib.stride_for(400)


def test_round6_entry_points_validate_without_gpu(lib):
    """ABI 105: the entity-major plan / second pass, the native step loop and the per-call tuning reject bad arguments before any
    launch (NULL structs, a step that is not entity-major, chunk counts, a communicator without entry points, a hub-row table
    mixed with a slot_of table in one update call)."""
    from multike_amd import _lib
    null = C.c_void_p(0)
    assert lib.mke_oc_em_plan(None, null) == -1 and b"NULL" in lib.mke_last_error()      # a struct pointer: None, byref or an array
    assert lib.mke_oc_pass2(None, null) == -1
    assert lib.mke_oc_steps(None, C.c_int(0), C.c_int(1), null) == -1
    assert lib.mke_tuning_init(None) == -1
    a = _lib.OcEmPlanArgs()
    a.n_ranks, a.rank, a.n_local, a.n_rel, a.chunks, a.capacity = 2, 0, 10, 3, 9, 100
    assert lib.mke_oc_em_plan(C.byref(a), null) == -2 and b"chunks" in lib.mke_last_error()
    a.chunks = 1
    assert lib.mke_oc_em_plan(C.byref(a), null) == -1 and b"NULL output" in lib.mke_last_error()
    st = _lib.OcStepStruct()
    assert lib.mke_oc_pass2(C.byref(st), null) == -3 and b"entity-major" in lib.mke_last_error()
    lp = _lib.OcLoopStruct()
    assert lib.mke_oc_steps(C.byref(lp), C.c_int(0), C.c_int(0), null) == -1 and b"NULL parts" in lib.mke_last_error()
    t = _lib.tuning(score_splits=2)
    assert [getattr(t, f) for f in _lib.TUNING_FIELDS] == [2] + [_lib.TUNE_DEFAULT] * (len(_lib.TUNING_FIELDS) - 1)
    # a hub-row table and a slot_of table in one update call: refused (the launch instantiates one form or the other)
    arr = (_lib.UpdateTableStruct * 2)()
    for k in (0, 1):
        arr[k].table, arr[k].acc, arr[k].grad, arr[k].n_rows, arr[k].normalize, arr[k].grad_copies = 16, 16, 16, 8, 1, 1
    arr[0].slot_of, arr[0].src_rows, arr[0].n_ranks, arr[0].capacity = 16, 16, 2, 4
    arr[1].hot.slot, arr[1].hot.n_hot, arr[1].hot.copies, arr[1].hot.row0 = 16, 2, 4, 8
    rc = lib.mke_rows_update_multi(arr, C.c_int(2), C.c_int32(1), C.c_int(80), C.c_int(75), C.c_int(0), C.c_float(0.1), null)
    assert rc == -3 and b"cannot share" in lib.mke_last_error()
    arr[0].slot_of = None
    arr[1].hot.row0 = 2                       # copies inside the table's own rows
    rc = lib.mke_rows_update_multi(arr, C.c_int(2), C.c_int32(1), C.c_int(80), C.c_int(75), C.c_int(0), C.c_float(0.1), null)
    assert rc == -2 and b"hub rows" in lib.mke_last_error()


def test_score_step_validates_without_gpu(lib):
    """mke_triple_score_step rejects bad arguments before any launch.  The codes are the ones the positional variants it
    replaced (ABI 106: _x, _xch, _det, plain) returned for the same arguments, recorded from a build of that version; the one
    difference: ref_count without grad_ent in deterministic mode was -2 from the staging check and is -1 from the common one."""
    from multike_amd import _abi, _lib
    one = 16

    def rc(**fields):
        a = _lib.ScoreArgs(ent_table=one, n_ent=10, ent_normalize=1, rel_table=one, n_rel=3, rel_normalize=1, stride=80, dim=75,
                           pos_h=one, pos_r=one, pos_t=one, n_pos=2, neg_h=one, neg_r=one, neg_t=one, n_neg=4, neg_per_pos=2,
                           scale=1.0, grad_ent=one, grad_rel=one, grad_rel_copies=1, touched_ent=one, touched_rel=one, tag=1,
                           ent_acc=one, optimizer=_lib.OPT_ADAGRAD, lr=0.1, loss_partials=one)
        for k, v in fields.items():
            setattr(a, k, v)
        return lib.mke_triple_score_step(C.byref(a), None)

    det = dict(stage_rows=one, stage_keys=one, stage_slots=1000)      # 2 groups of 1 + 2 triples, 3 rows each: 18 slots needed
    assert lib.mke_triple_score_step(None, None) == -1 and b"NULL args" in lib.mke_last_error()
    assert rc(ent_table=None) == -1 and b"NULL table/loss" in lib.mke_last_error()
    assert rc(rel_table=None) == -1
    assert rc(loss_partials=None) == -1
    assert rc(stride=75) == -2 and b"stride" in lib.mke_last_error()
    assert rc(n_neg=5) == -2 and b"grouped negatives" in lib.mke_last_error()
    assert rc(grad_rel=None) == -1 and b"both" in lib.mke_last_error()
    assert rc(grad_rel_copies=65) == -2 and b"grad_rel_copies" in lib.mke_last_error()
    assert rc(optimizer=7) == -3 and b"optimizer" in lib.mke_last_error()
    assert rc(ref_count=one, ent_acc=None) == -1 and b"ent_acc" in lib.mke_last_error()
    assert rc(ref_count=one, grad_ent=None, grad_rel=None) == -1 and b"gradient scratch" in lib.mke_last_error()
    assert rc(ref_count=one, grad_ent=None, grad_rel=None, **det) == -1       # was -2 (see above)
    assert rc(**dict(det, stage_rows=None)) == -1 and b"staging" in lib.mke_last_error()
    assert rc(**dict(det, stage_slots=17)) == -2 and b"18 staging slots needed, 17 given" in lib.mke_last_error()
    assert rc(hot=_lib.HotRowsStruct(one, 2, 4, 5)) == -2 and b"hub rows" in lib.mke_last_error()      # row0 5 < n_ent 10
    cj = _abi.mke_count_job(pos_h=one, pos_t=one, n_pos=2, neg_h=one, neg_t=one, n_neg=4, neg_per_pos=2, ref_count=None)
    assert rc(next_count=C.addressof(cj)) == -1 and b"count job" in lib.mke_last_error()
    # the positional wrapper that stays goes through the same checks
    p, null = C.c_void_p(one), C.c_void_p(0)
    assert lib.mke_triple_score_fwd_bwd(p, C.c_int64(10), C.c_int(1), p, C.c_int64(3), C.c_int(1), C.c_int(75), C.c_int(75), p, p, p, null,
                                        C.c_int64(2), p, p, p, null, C.c_int64(4), C.c_int(2), C.c_float(1.0), p, p, C.c_int(1), p, p,
                                        C.c_int32(1), p, null) == -2 and b"stride" in lib.mke_last_error()
