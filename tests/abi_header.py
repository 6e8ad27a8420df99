"""What the ABI tests share: the header, the generator of multike_amd/_abi.py, and what a C compiler says about the header."""
import importlib.util
import os
import re
import shutil
import struct
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "multike_hip.h")
GENERATOR = os.path.join(ROOT, "tools", "gen_abi.py")
GENERATED = os.path.join(ROOT, "multike_amd", "_abi.py")


def header_text():
    with open(HEADER, encoding="utf-8") as f:
        return f.read()


def generator():
    """tools/gen_abi.py as a module (tools/ is not a package)."""
    spec = importlib.util.spec_from_file_location("gen_abi", GENERATOR)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def members(struct, text=None):
    """Member names of a struct of the header, in the header's order."""
    _, structs, _ = generator().parse(header_text() if text is None else text)
    return [m for m, _ in dict(structs)[struct]]


def c_compiler():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("gcc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cc, "no host C compiler (cc, gcc or ROCm's clang)"
    return cc


def c_layout(tmp_path, struct_members, constants, include_dir=None):
    """Compile a C program against the header and return what it prints: ({struct: size}, {(struct, member): (offset, size)},
    {MKE_X: value}).  struct_members: {struct: [member names]}; constants: MKE_* names."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "multike_hip.h"', "int main(void) {"]
    for s, ms in struct_members.items():
        lines.append(f'  printf("S {s} - %zu 0\\n", sizeof({s}));')
        lines += [f'  printf("M {s} {m} %zu %zu\\n", offsetof({s}, {m}), sizeof((({s}*)0)->{m}));' for m in ms]
    lines += [f'  printf("C {c} - %lld 0\\n", (long long)({c}));' for c in constants]
    lines += ["  return 0;", "}", ""]
    src, exe = tmp_path / "abi_layout.c", tmp_path / "abi_layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([c_compiler(), "-std=c99", "-I", include_dir or os.path.dirname(HEADER), str(src), "-o", str(exe)])
    sizes, fields, values = {}, {}, {}
    for kind, a, b, x, y in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()):
        if kind == "S":
            sizes[a] = int(x)
        elif kind == "M":
            fields[a, b] = (int(x), int(y))
        else:
            values[a] = int(x)
    return sizes, fields, values


def offsets_and_size(tmp_path, struct, fields):
    """[offsetof of every field ..., sizeof(struct)] as the C compiler sees the header."""
    sizes, members_, _ = c_layout(tmp_path, {struct: fields}, [])
    return [members_[struct, f][0] for f in fields] + [sizes[struct]]


def header_struct_names(text):
    return re.findall(r"typedef\s+struct\s+(\w+)\s*\{", text)


def header_constant_names(text):
    """Object-like MKE_* macros with a value (function-like ones, MKE_X(dim), are not constants)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MKE_\w+)[ \t]+\S", text, flags=re.M)


def exported_symbols(so_path):
    """mke_* functions the shared library exports: the defined global FUNC entries of its .dynsym (ELF64, little-endian)."""
    with open(so_path, "rb") as f:
        data = f.read()
    assert data[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    (shoff,), (shentsize, shnum) = struct.unpack_from("<Q", data, 0x28), struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = set()
    for _, kind, _, _, off, size, link, _, _, entsize in sections:
        if kind != 11:      # SHT_DYNSYM
            continue
        strings = sections[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, st_shndx, _, _ = struct.unpack_from("<IBBHQQ", data, off + k * entsize)
            name = data[strings + st_name:data.index(b"\0", strings + st_name)].decode()
            if st_shndx != 0 and st_info == (1 << 4 | 2) and name.startswith("mke_"):       # defined, GLOBAL FUNC
                out.add(name)
    return out
