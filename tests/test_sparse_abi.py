"""include/multike_sparse.h: multike_amd/_abi_sparse.py is what tools/gen_abi.py writes from it, a C compiler agrees with the
layout, libmultike_sparse.so exports exactly its prototypes, and every refusal comes with its status and a message naming the
argument before anything is enqueued.  No GPU: nothing here launches."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import abi_header as ah


@pytest.fixture(scope="module")
def L():
    from multike_amd import _lib
    if not os.path.exists(_lib.SPARSE_SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.sparse_lib()


def test_sparse_abi_module_layout_and_symbols(tmp_path, L):
    from multike_amd import _abi, _abi_keyed, _abi_links, _abi_sparse, _abi_thin, _lib
    header = os.path.join(os.path.dirname(ah.HEADER), "multike_sparse.h")
    out = tmp_path / "_abi_sparse.py"
    subprocess.check_call([sys.executable, ah.GENERATOR, header, str(out)])
    assert out.read_bytes() == open(os.path.join(os.path.dirname(ah.GENERATED), "_abi_sparse.py"), "rb").read(), \
        "run tools/gen_abi.py include/multike_sparse.h multike_amd/_abi_sparse.py and commit it"
    assert list(_abi_sparse.FUNCTIONS) == ["mke_sparse_last_error", "mke_sparse_version", "mke_sparse_support_temp_bytes",
                                           "mke_sparse_support", "mke_sparse_lse_temp_bytes", "mke_sparse_lse"]
    others = set(_abi.FUNCTIONS) | set(_abi_thin.FUNCTIONS) | set(_abi_keyed.FUNCTIONS) | set(_abi_links.FUNCTIONS)
    assert not set(_abi_sparse.FUNCTIONS) & others
    text = open(header).read()
    assert "#include" not in text.replace("#include <stdint.h>", "")                      # the header stands alone
    assert (_abi_sparse.SPARSE_E_NULL, _abi_sparse.SPARSE_E_SHAPE, _abi_sparse.SPARSE_E_UNSUPPORTED, _abi_sparse.SPARSE_E_RANGE) == \
        (_abi.E_NULL, _abi.E_SHAPE, _abi.E_UNSUPPORTED, _abi.E_RANGE)
    assert _abi_sparse.SPARSE_Q % 16 == 0 and _abi_sparse.SPARSE_SEG % 64 == 0 and _abi_sparse.SPARSE_Q <= _abi_sparse.SPARSE_SEG
    # a C compiler's sizeof / offsetof of the header (given to the shared helper under the name it includes)
    (tmp_path / "inc").mkdir()
    (tmp_path / "inc" / "multike_hip.h").write_text(text)
    structs = {st.__name__: [f for f, _ in st._fields_] for st in _abi_sparse.STRUCTS}
    consts = ah.header_constant_names(text)
    assert ah.header_struct_names(text) == list(structs) == ["mke_sparse_support_args", "mke_sparse_lse_args"] and len(consts) == 9
    sizes, fields, values = ah.c_layout(tmp_path, structs, consts, include_dir=str(tmp_path / "inc"))
    assert sizes == {st.__name__: C.sizeof(st) for st in _abi_sparse.STRUCTS}
    assert len(fields) == sum(len(m) for m in structs.values()) == 20 + 12
    for st in _abi_sparse.STRUCTS:
        assert all(fields[st.__name__, f] == (getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_)
    assert values == {"MKE_" + k: v for k, v in vars(_abi_sparse).items() if k.isupper() and isinstance(v, int)}
    assert ah.exported_symbols(_lib.SPARSE_SO_PATH) == set(_abi_sparse.FUNCTIONS)
    for name, (restype, argtypes) in _abi_sparse.FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert L.mke_sparse_version() == _abi_sparse.SPARSE_VERSION == 1
    assert _lib.SYMBOLS == tuple(_abi.FUNCTIONS)                               # the main library's list does not know the new one


P = 0x10000                                                                    # a non-NULL address nobody dereferences


def test_support_refusals(L):
    from multike_amd import _abi_sparse as ab

    def support(**over):
        kw = dict(val_r=P, col_r=P, val_c=P, row_c=P, n_a=100, n_b=90, cut_r=8, cut_c=8, capacity=100 * 8 + 90 * 8, row_off=P, row_seg=P,
                  ent_col=P, ent_val=P, col_off=P, col_seg=P, ent_row=P, ent_idx=P, count=P, temp=P, temp_bytes=0)
        kw.update(over)
        return L.mke_sparse_support(C.byref(ab.mke_sparse_support_args(**kw)), None), L.mke_sparse_last_error()

    assert L.mke_sparse_support(None, None) == ab.SPARSE_E_NULL and b"NULL args" in L.mke_sparse_last_error()
    for kw in (dict(n_a=-1), dict(n_b=-1), dict(n_a=0x7FFFFF01), dict(n_b=0x7FFFFF01)):
        rc, msg = support(**kw)
        assert rc == ab.SPARSE_E_SHAPE and b"n_a / n_b" in msg, (kw, rc, msg)
    for kw in (dict(cut_r=0), dict(cut_c=0), dict(cut_r=-3)):
        rc, msg = support(**kw)
        assert rc == ab.SPARSE_E_SHAPE and b"cut_r and cut_c must be >= 1" in msg, (kw, rc, msg)
    # a count the sort cannot hold is a stated range error, in the temp query too: never a wrap
    for kw in (dict(n_a=1 << 24, cut_r=128), dict(n_a=0x7FFFFF00, n_b=0x7FFFFF00, cut_r=0x7FFFFFFF, cut_c=0x7FFFFFFF),
               dict(n_a=0x7FFFFF00, n_b=1, cut_r=1, cut_c=1)):
        rc, msg = support(**kw)
        assert rc == ab.SPARSE_E_RANGE and b"list slots exceed" in msg, (kw, rc, msg)
        full = dict(n_a=100, n_b=90, cut_r=8, cut_c=8)
        full.update(kw)
        assert L.mke_sparse_support_temp_bytes(full["n_a"], full["n_b"], full["cut_r"], full["cut_c"]) == ab.SPARSE_E_RANGE
    assert support(n_a=0x7FFFFF00, n_b=0, cut_r=1)[0] != ab.SPARSE_E_RANGE      # the largest count the sort holds
    for name in ("row_off", "col_off", "row_seg", "col_seg", "count"):
        rc, msg = support(**{name: None})
        assert rc == ab.SPARSE_E_NULL and name.encode() in msg, name
    for name, word in (("val_r", b"list"), ("col_r", b"list"), ("val_c", b"list"), ("row_c", b"list"), ("ent_col", b"ent_col"),
                       ("ent_val", b"ent_val"), ("ent_row", b"ent_row"), ("ent_idx", b"ent_idx"), ("temp", b"temp")):
        rc, msg = support(**{name: None})
        assert rc == ab.SPARSE_E_NULL and word in msg, name
    rc, msg = support(capacity=100 * 8 + 90 * 8 - 1)
    assert rc == ab.SPARSE_E_SHAPE and b"capacity" in msg
    need = L.mke_sparse_support_temp_bytes(100, 90, 8, 8)
    assert need >= (100 * 8 + 90 * 8) * 36                                      # two key and value buffers, flags, positions, rows
    for short in (0, need - 1):
        rc, msg = support(temp_bytes=short)
        assert rc == ab.SPARSE_E_SHAPE and b"temp_bytes" in msg and str(need).encode() in msg
    assert L.mke_sparse_support_temp_bytes(0, 0, 1, 1) == 0


def test_lse_refusals(L):
    from multike_amd import _abi_sparse as ab

    def lse(**over):
        kw = dict(n=100, off=P, seg=P, other=P, val=P, idx=None, sub=None, tau=0.05, out=P, capacity=1520, temp=P, temp_bytes=0)
        kw.update(over)
        return L.mke_sparse_lse(C.byref(ab.mke_sparse_lse_args(**kw)), None), L.mke_sparse_last_error()

    assert L.mke_sparse_lse(None, None) == ab.SPARSE_E_NULL and b"NULL args" in L.mke_sparse_last_error()
    for kw in (dict(n=-1), dict(n=0x7FFFFF01)):
        rc, msg = lse(**kw)
        assert rc == ab.SPARSE_E_SHAPE and b"bad n" in msg
    rc, msg = lse(capacity=-1)
    assert rc == ab.SPARSE_E_SHAPE and b"capacity" in msg
    for tau in (0.0, -0.05, float("inf"), float("nan")):
        rc, msg = lse(tau=tau)
        assert rc == ab.SPARSE_E_RANGE and b"tau must be positive and finite" in msg, tau
    for name in ("off", "seg", "out", "other", "val", "temp"):
        rc, msg = lse(**{name: None})
        assert rc == ab.SPARSE_E_NULL and name.encode() in msg, name
    need = L.mke_sparse_lse_temp_bytes(1520)
    assert need == (1520 // ab.SPARSE_Q + 1) * 8
    rc, msg = lse(temp_bytes=need - 1)
    assert rc == ab.SPARSE_E_SHAPE and b"temp_bytes" in msg
    assert lse(n=0, tau=0.05, off=None)[0] == ab.SPARSE_OK                      # nothing to do, nothing enqueued
    assert lse(n=0, tau=0.0)[0] == ab.SPARSE_E_RANGE                            # a wrong argument is reported even then
    assert L.mke_sparse_lse_temp_bytes(-1) == ab.SPARSE_E_SHAPE
