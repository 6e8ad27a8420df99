"""multike_amd/_abi.py is what tools/gen_abi.py writes from include/multike_hip.h, and a C compiler agrees with it: sizes, offsets
and member sizes of every struct, the value of every constant, the prototypes the loader installs.  The last tests show that the
checks can fail and that a wrongly typed argument does not reach the library.  No GPU: nothing here launches."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import abi_header as ah


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def committed():
    with open(ah.GENERATED, encoding="utf-8") as f:
        return f.read()


def constants_of(abi):
    return {"MKE_" + k: v for k, v in vars(abi).items() if k.isupper() and isinstance(v, int)}


def test_generated_module_is_fresh(tmp_path):
    out = tmp_path / "_abi.py"
    subprocess.check_call([sys.executable, ah.GENERATOR, ah.HEADER, str(out)])
    assert out.read_bytes() == open(ah.GENERATED, "rb").read(), "run tools/gen_abi.py and commit multike_amd/_abi.py"
    text = committed()
    assert text.splitlines()[0].endswith("generated from include/multike_hip.h by tools/gen_abi.py — do not edit")
    imports = [ln for ln in text.splitlines() if ln.startswith(("import ", "from "))]
    assert imports == ["import ctypes as C"]


def layout_mismatches(abi, sizes, fields, values):
    """Everything in which the ctypes module `abi` differs from what the C compiler printed."""
    bad = []
    for st in abi.STRUCTS:
        if C.sizeof(st) != sizes[st.__name__]:
            bad.append((st.__name__, "sizeof", C.sizeof(st), sizes[st.__name__]))
        for name, _ in st._fields_:
            f = getattr(st, name)
            if (f.offset, f.size) != fields[st.__name__, name]:
                bad.append((st.__name__, name, (f.offset, f.size), fields[st.__name__, name]))
    bad += [(k, "value", v, values.get(k)) for k, v in constants_of(abi).items() if values.get(k) != v]
    return bad


def test_layout_and_constants_match_the_c_compiler(tmp_path):
    from multike_amd import _abi
    text = ah.header_text()
    names = ah.header_struct_names(text)
    assert names == [st.__name__ for st in _abi.STRUCTS] and len(names) == 28
    consts = ah.header_constant_names(text)
    assert set(consts) == set(constants_of(_abi)) and len(consts) == len(set(consts))
    sizes, fields, values = ah.c_layout(tmp_path, {st.__name__: [f for f, _ in st._fields_] for st in _abi.STRUCTS}, consts)
    assert layout_mismatches(_abi, sizes, fields, values) == []
    assert sum(len(st._fields_) for st in _abi.STRUCTS) == len(fields)


def test_loader_installs_the_generated_prototypes(lib):
    from multike_amd import _abi, _lib
    assert _lib.SYMBOLS == tuple(_abi.FUNCTIONS)
    for name, (restype, argtypes) in _abi.FUNCTIONS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert ah.exported_symbols(_lib.SO_PATH) == set(_abi.FUNCTIONS)
    assert len(_abi.FUNCTIONS) == 93        # the prototypes the header declares today
    assert _lib.TUNING_FIELDS == tuple(ah.members("mke_tuning")[:-1]) and ah.members("mke_tuning")[-1] == "reserved"


EDITS = {
    "swapped members": ("int64_t n_a, n_b; int cut;\n  const float* val; const int32_t* col;     /* [n_a][cut], mke_stable_lists' layout */",
                        "int64_t n_a; int cut; int64_t n_b;\n  const float* val; const int32_t* col;     /* [n_a][cut], mke_stable_lists' layout */"),
    "narrowed parameter": ("int step_begin, int step_end, int64_t pos_begin /* step_off[step_begin] */",
                           "int step_begin, int step_end, int pos_begin /* step_off[step_begin] */"),
    "changed constant": ("#define MKE_LOSS_PARTIALS 2048", "#define MKE_LOSS_PARTIALS 4096"),
}


@pytest.mark.parametrize("edit", sorted(EDITS))
def test_an_edited_header_is_noticed(edit, tmp_path):
    """One edit of a copy of the header: the generator's output is no longer the committed module."""
    old, new = EDITS[edit]
    text = ah.header_text()
    assert text.count(old) == 1
    edited = text.replace(old, new)
    fresh = ah.generator().generate(edited)
    assert fresh != committed()
    assert ah.generator().generate(text) == committed()
    if edit == "swapped members":       # and the compiler's layout of that header is no longer the committed module's
        from multike_amd import _abi
        (tmp_path / "multike_hip.h").write_text(edited)
        got = ah.c_layout(tmp_path, {"mke_assign_args": [f for f, _ in _abi.mke_assign_args._fields_]}, [], include_dir=str(tmp_path))
        sizes = {st.__name__: got[0].get(st.__name__, C.sizeof(st)) for st in _abi.STRUCTS}
        fields = {(st.__name__, f): got[1].get((st.__name__, f), (getattr(st, f).offset, getattr(st, f).size))
                  for st in _abi.STRUCTS for f, _ in st._fields_}
        bad = layout_mismatches(_abi, sizes, fields, constants_of(_abi))
        assert {b[:2] for b in bad} == {("mke_assign_args", "n_b"), ("mke_assign_args", "cut")}, bad


def test_a_wrongly_typed_argument_is_refused(lib):
    with pytest.raises(C.ArgumentError):
        lib.mke_assign_temp_bytes(C.c_int(100), C.c_int64(60), 0)        # n_a is an int64_t
    assert lib.mke_assign_temp_bytes(C.c_int64(100), C.c_int64(60), 0) == lib.mke_assign_temp_bytes(100, 60, 0) > 0
