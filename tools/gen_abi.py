#!/usr/bin/env python3
"""Generate multike_amd/_abi.py, the ctypes view of the C-ABI, from include/multike_hip.h.

    python tools/gen_abi.py [header [output]]
    python tools/gen_abi.py include/multike_thin.h multike_amd/_abi_thin.py      (libmultike_thin.so, a header of its own)
    python tools/gen_abi.py include/multike_keyed.h multike_amd/_abi_keyed.py    (libmultike_keyed.so, likewise)
    python tools/gen_abi.py include/multike_links.h multike_amd/_abi_links.py    (libmultike_links.so, likewise)

The header is the only place a struct, a prototype or a constant is typed; this script turns its small vocabulary (fixed-width
scalars, pointers, arrays sized by literals or MKE_* constants, structs by value, integer #defines) into ctypes and stops at
anything else.  Pure standard library, no compiler.  tests/test_abi_generated.py checks that the committed module is what
this script writes and that a C compiler agrees with its layout.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multike_hip.h")
OUTPUT = os.path.join(ROOT, "multike_amd", "_abi.py")

SCALARS = {"int": "C.c_int", "int32_t": "C.c_int32", "uint32_t": "C.c_uint32", "int64_t": "C.c_int64", "uint64_t": "C.c_uint64",
           "uint8_t": "C.c_uint8", "float": "C.c_float", "double": "C.c_double"}
_INT = r"-?\s*(?:0[xX][0-9a-fA-F]+|\d+)[uU]?"


class HeaderError(ValueError):
    pass


def _int(text, constants):
    """Value of an integer expression of the header: a literal (decimal, hex, `u` suffix, negative), `(1 << n)`, or sums and
    products of literals and MKE_* constants (array lengths)."""
    text = re.sub(r"MKE_\w+", lambda m: str(constants[m.group(0)[4:]]) if m.group(0)[4:] in constants else m.group(0), text)
    text = re.sub(r"(0[xX][0-9a-fA-F]+|\d+)[uU]\b", r"\1", text)
    if not re.fullmatch(r"[\s()+*\-<0-9a-fA-FxX]+", text) or "**" in text:
        raise HeaderError(f"not an integer expression: {text!r}")
    return int(eval(text, {"__builtins__": {}}))


def parse(header):
    """-> (constants {name without MKE_: int}, structs [(name, [(member, ctypes expression)])], functions [(name, restype, [argtypes])])."""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+MKE_(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):   # not MKE_X(args)
        constants[name] = _int(value, constants)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    structs, known = [], set()

    def pointer_free(base, what):
        if base in SCALARS:
            return SCALARS[base]
        if base in known:
            return base
        raise HeaderError(f"{what}: unknown type {base!r}")

    def struct(m):
        name, body = m.group(1), m.group(2)
        if m.group(3) != name:
            raise HeaderError(f"typedef struct {name} is named {m.group(3)}")
        members = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            dm = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)", decl, flags=re.S)
            if not dm:
                raise HeaderError(f"{name}: cannot read {decl!r}")
            base, star, rest = dm.groups()
            parts = [p.strip() for p in rest.split(",")]
            if star and len(parts) > 1:
                raise HeaderError(f"{name}: one pointer member per declaration, not {decl!r}")
            for part in parts:
                pm = re.fullmatch(r"(\w+)\s*(?:\[([^\]]+)\])?", part)
                if not pm:
                    raise HeaderError(f"{name}: cannot read member {part!r} of {decl!r}")
                if star and base != "void":
                    pointer_free(base, name)       # the pointee must be a type the header has declared
                kind = "C.c_void_p" if star else pointer_free(base, name)
                if pm.group(2):
                    kind += f" * {_int(pm.group(2), constants)}"
                members.append((pm.group(1), kind))
        structs.append((name, members))
        known.add(name)
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)

    functions = []
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        fm = re.fullmatch(r"(const\s+char\s*\*|int64_t|int)\s*(mke_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not fm:
            raise HeaderError(f"cannot read the declaration {decl!r}")
        ret, name, params = fm.groups()
        restype = "C.c_char_p" if ret.startswith("const") else SCALARS[ret]
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            am = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*\w+\s*", p)
            if not am:
                raise HeaderError(f"{name}: cannot read the parameter {p!r}")
            const, base, star = am.groups()
            if not star:
                argtypes.append(pointer_free(base, name))
            elif base in known:
                argtypes.append(f"C.POINTER({base})")
            elif base == "char" and const:
                argtypes.append("C.c_char_p")
            elif base == "void" or base in SCALARS:
                argtypes.append("C.c_void_p")
            else:
                raise HeaderError(f"{name}: unknown type {base!r}")
        functions.append((name, restype, argtypes))
    return constants, structs, functions


def generate(header, source="include/multike_hip.h"):
    """The text of multike_amd/_abi.py for the text of the header (`source`: the header's name in the module's first line)."""
    constants, structs, functions = parse(header)
    out = [f'"""generated from {source} by tools/gen_abi.py — do not edit',
           "",
           "The C-ABI as ctypes: every integer #define (MKE_X as X), every struct under its C name with its members in header order,",
           "and FUNCTIONS = {name: (restype, argtypes)} in header order.  Pointers inside structs are plain addresses (c_void_p).",
           '"""',
           "import ctypes as C",
           ""]
    out += [f"{name} = {value:#x}" if value >= 1 << 16 else f"{name} = {value}" for name, value in constants.items()]
    for name, members in structs:
        out += ["", "", f"class {name}(C.Structure):", "    _fields_ = ["]
        out += [f'        ("{member}", {kind}),' for member, kind in members]
        out += ["    ]"]
    out += ["", "", "STRUCTS = (" + ", ".join(name for name, _ in structs) + ")", "", "FUNCTIONS = {"]
    for name, restype, argtypes in functions:
        out.append(f'    "{name}": ({restype}, ({"".join(a + ", " for a in argtypes).rstrip()})),')
    out += ["}", ""]
    return "\n".join(out)


def main(argv):
    header = argv[0] if argv else HEADER
    output = argv[1] if len(argv) > 1 else OUTPUT
    with open(header, encoding="utf-8") as f:
        text = generate(f.read(), os.path.relpath(os.path.abspath(header), ROOT).replace(os.sep, "/"))
    with open(output, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
