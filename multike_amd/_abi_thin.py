"""generated from include/multike_thin.h by tools/gen_abi.py — do not edit

The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,
and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).
"""
import ctypes as C



STRUCTS = ()

FUNCTIONS = {
    "mke_thin_last_error": (C.c_char_p, ()),
    "mke_idlist_thin": (C.c_int, (C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,)),
}
