"""generated from include/multike_links.h by tools/gen_abi.py — do not edit

The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,
and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).
"""
import ctypes as C

LINKS_VERSION = 1
LINKS_OK = 0
LINKS_E_NULL = -1
LINKS_E_SHAPE = -2
LINKS_E_UNSUPPORTED = -3
LINKS_E_RANGE = -4
LINKS_METRIC_INNER = 0
LINKS_METRIC_EUCLIDEAN = 1
LINKS_COUNTS = 7


class mke_links_args(C.Structure):
    _fields_ = [
        ("held", C.c_void_p),
        ("match", C.c_void_p),
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("a", C.c_void_p),
        ("lda", C.c_int),
        ("b", C.c_void_p),
        ("ldb", C.c_int),
        ("kpad", C.c_int),
        ("metric", C.c_int),
        ("sq_a", C.c_void_p),
        ("sq_b", C.c_void_p),
        ("csls_row", C.c_void_p),
        ("csls_col", C.c_void_p),
        ("retain", C.c_float),
        ("new_score", C.c_void_p),
        ("inv", C.c_void_p),
        ("out", C.c_void_p),
        ("score", C.c_void_p),
        ("counts", C.c_void_p),
    ]


STRUCTS = (mke_links_args)

FUNCTIONS = {
    "mke_links_last_error": (C.c_char_p, ()),
    "mke_links_version": (C.c_int, ()),
    "mke_links_edit": (C.c_int, (C.POINTER(mke_links_args), C.c_void_p,)),
}
