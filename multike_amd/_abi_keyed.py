"""generated from include/multike_keyed.h by tools/gen_abi.py — do not edit

The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,
and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).
"""
import ctypes as C

KEYED_OK = 0
KEYED_E_NULL = -1
KEYED_E_SHAPE = -2
KEYED_E_UNSUPPORTED = -3
KEYED_E_RANGE = -4
KEYED_MAX_SEG = 64
KEYED_MAX_LIST = 0x100000


class mke_keyed_candidate(C.Structure):
    _fields_ = [
        ("idx", C.c_int32),
        ("sim", C.c_float),
    ]


STRUCTS = (mke_keyed_candidate)

FUNCTIONS = {
    "mke_keyed_last_error": (C.c_char_p, ()),
    "mke_sim_select_keyed": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(mke_keyed_candidate), C.c_void_p, C.c_void_p, C.c_void_p,)),
    "mke_keyed_finish": (C.c_int, (C.POINTER(mke_keyed_candidate), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,)),
}
