"""What tests/test_abi_conformance.py reads out of a public header of include/: its text without comments, the functions
it declares, the structures it defines, its integer-literal macros -- and, from the compiler itself, the record layout of
every structure the public headers define (a host-only, syntax-only compile; nothing is built or run)."""
import ctypes as C
import functools
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

INCLUDE = Path(__file__).resolve().parents[1] / "include"
SCALARS = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "float": C.c_float, "double": C.c_double}


@functools.lru_cache(maxsize=None)
def text(header: str) -> str:
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", (INCLUDE / header).read_text(), flags=re.S)


def functions(header: str) -> dict:
    """name -> number of declared parameters, for every `<type> ce_*(...);` of the header."""
    out = {}
    for name, params in re.findall(r"\b(ce_\w+)\s*\(([^()]*)\)\s*;", text(header)):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def struct_names(header: str) -> list:
    """The structures the header itself defines (an opaque `typedef struct ce_x ce_x;` has no body and is none)."""
    return re.findall(r"typedef\s+struct\s+(ce_\w+)\s*\{", text(header))


def int_defines(header: str) -> dict:
    return {name: int(value, 0) for name, value in re.findall(r"^[ \t]*#define[ \t]+(CE_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[uU]?[ \t]*$", text(header), flags=re.M)}


@functools.lru_cache(maxsize=None)
def record_layouts(headers: tuple) -> dict:
    """struct name -> (sizeof, [(offset, C type, field name)]) as clang lays the structures of `headers` out, direct fields only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # the compiler _lib.build() uses
    names = [s for h in headers for s in struct_names(h)]
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "layouts.cpp"
        src.write_text("".join(f'#include "{h}"\n' for h in headers) + "".join(f"static_assert(sizeof({s}) > 0, \"\");\n" for s in names))
        dump = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", "-Xclang", "-fdump-record-layouts", f"-I{INCLUDE}", str(src)],
                              check=True, capture_output=True, text=True).stdout
    out = {}
    for block in dump.split("*** Dumping AST Record Layout")[1:]:
        head = re.search(r"^\s*0 \| struct (\w+)$", block, flags=re.M)
        if not head:
            continue
        fields = [(int(off), ctype.strip(), name) for off, ctype, name in re.findall(r"^\s*(\d+) \|   (\S.*?)\s*\b(\w+)$", block, flags=re.M)]
        out[head.group(1)] = (int(re.search(r"\[sizeof=(\d+),", block).group(1)), fields)
    return out


def ctype_of(c_type: str, structs: dict):
    """The ctypes type of a C field type as the layout dump spells it: `int32_t`, `float[2][32][32]`, `const uint8_t *`,
    `ce_hop_desc[2]` (`structs`: C struct name -> ctypes mirror)."""
    m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*)?((?:\[\d+\])*)", c_type)
    assert m, c_type
    base = SCALARS.get(m.group(2)) or structs[m.group(2)]
    if m.group(3):
        base = C.POINTER(base)
    for dim in reversed(re.findall(r"\[(\d+)\]", m.group(4))):
        base = base * int(dim)
    return base
