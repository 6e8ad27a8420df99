"""generated from include/multike_sparse.h by tools/gen_abi.py — do not edit

The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,
and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).
"""
import ctypes as C

SPARSE_VERSION = 1
SPARSE_OK = 0
SPARSE_E_NULL = -1
SPARSE_E_SHAPE = -2
SPARSE_E_UNSUPPORTED = -3
SPARSE_E_RANGE = -4
SPARSE_Q = 256
SPARSE_SEG = 1024
SPARSE_MAX_SLOTS = 0x7fffff00


class mke_sparse_support_args(C.Structure):
    _fields_ = [
        ("val_r", C.c_void_p),
        ("col_r", C.c_void_p),
        ("val_c", C.c_void_p),
        ("row_c", C.c_void_p),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("cut_r", C.c_int),
        ("cut_c", C.c_int),
        ("capacity", C.c_int64),
        ("row_off", C.c_void_p),
        ("row_seg", C.c_void_p),
        ("ent_col", C.c_void_p),
        ("ent_val", C.c_void_p),
        ("col_off", C.c_void_p),
        ("col_seg", C.c_void_p),
        ("ent_row", C.c_void_p),
        ("ent_idx", C.c_void_p),
        ("count", C.c_void_p),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
    ]


class mke_sparse_lse_args(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("off", C.c_void_p),
        ("seg", C.c_void_p),
        ("other", C.c_void_p),
        ("val", C.c_void_p),
        ("idx", C.c_void_p),
        ("sub", C.c_void_p),
        ("tau", C.c_float),
        ("out", C.c_void_p),
        ("capacity", C.c_int64),
        ("temp", C.c_void_p),
        ("temp_bytes", C.c_int64),
    ]


STRUCTS = (mke_sparse_support_args, mke_sparse_lse_args)

FUNCTIONS = {
    "mke_sparse_last_error": (C.c_char_p, ()),
    "mke_sparse_version": (C.c_int, ()),
    "mke_sparse_support_temp_bytes": (C.c_int64, (C.c_int64, C.c_int64, C.c_int, C.c_int,)),
    "mke_sparse_support": (C.c_int, (C.POINTER(mke_sparse_support_args), C.c_void_p,)),
    "mke_sparse_lse_temp_bytes": (C.c_int64, (C.c_int64,)),
    "mke_sparse_lse": (C.c_int, (C.POINTER(mke_sparse_lse_args), C.c_void_p,)),
}
