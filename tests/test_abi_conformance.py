"""The ctypes binding (srsran_ce_pytorch_amd/_lib.py) against the public headers of include/, for every header of its
registry alike: the declared functions and their tables, the signatures load() applies, every structure's layout against
the compiler's own record layout, the integer macros, and what build() depends on.  No GPU."""
import ctypes as C
from pathlib import Path

import pytest

import abi_header as H
from srsran_ce_pytorch_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADERS = list(_lib.REGISTRY)
ALL_MIRRORS = {name: cls for entry in _lib.REGISTRY.values() for name, cls in entry.structs.items()}
# the macros the per-stage tests compared one by one before this module: the least the comparison below must cover
MIN_DEFINES = {
    "CE_ABI_VERSION",
    "CE_DMRS_MAX_WORDS", "CE_DMRS_MAX_RE", "CE_EQ_MAX_PORTS", "CE_EQ_CHUNK_SC",
    "CE_DEMOD_MAX_BITS", "CE_DEMOD_BLOCK_WORDS", "CE_DEMOD_TILE_SYMBOLS", "CE_DEMOD_OUT_F32", "CE_DEMOD_OUT_I8",
    "CE_RM_F32", "CE_RM_I8", "CE_RM_MAX_SLOT_ELEMS", "CE_RM_TILE_UNITS", "CE_TP_MAX_PRBS", "CE_TP_MAX_PASSES",
    "CE_LDPC_MAX_ZC", "CE_LDPC_MAX_ROWS", "CE_LDPC_MAX_COLS", "CE_LDPC_MAX_ROW_DEGREE", "CE_LDPC_L_BOUND", "CE_LDPC_LDS_MAX",
    "CE_LDPC_F32", "CE_LDPC_I8", "CE_LDPC_STATE_IDX_SHIFT", "CE_LDPC_STATE_MAG_SHIFT",
    "CE_TB_G24A", "CE_TB_G24B", "CE_TB_G16", "CE_TB_THREADS", "CE_TB_MAX_PIECE",
    "CE_ENC_THREADS", "CE_ENC_CORE_TRIANGULAR", "CE_ENC_CORE_NR", "CE_ENC_CRC_CHUNK",
    "CE_MOD_THREADS", "CE_MOD_TILE_SC", "CE_MOD_GROUP_SYMBOLS", "CE_MOD_MAX_TILE_BLOCKS",
    "CE_MOD_A_QPSK", "CE_MOD_A_16QAM", "CE_MOD_A_64QAM", "CE_MOD_A_256QAM",
}


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_the_registry_is_the_public_headers():
    assert sorted(HEADERS) == sorted(p.name for p in (ROOT / "include").iterdir())
    assert (len(HEADERS), len(ALL_MIRRORS), sum(len(e.structs) for e in _lib.REGISTRY.values())) == (11, 34, 34)
    assert _lib.EXPORTS == list(_lib.REGISTRY["ce_hip.h"].signatures) and _lib.EXPORTS_DENOISE == list(_lib.REGISTRY["ce_denoise.h"].signatures)


@pytest.mark.parametrize("header", HEADERS)
def test_functions_and_their_signatures(lib, header):
    """Items 1 and 2: the header's functions are the table's keys, and load() has put the table's restype and argtypes,
    one argtype per declared parameter, on each."""
    declared, table = H.functions(header), _lib.REGISTRY[header].signatures
    assert set(declared) == set(table), set(declared) ^ set(table)
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert len(argtypes) == declared[name], name


@pytest.mark.parametrize("header", HEADERS)
def test_structure_layouts_are_the_compilers(header):
    """Item 3: per structure the header defines, the mirror's field names in order, each field's offset, size and type,
    and sizeof, against clang's record layout."""
    mirrors, layouts = _lib.REGISTRY[header].structs, H.record_layouts(tuple(HEADERS))
    assert list(mirrors) == H.struct_names(header), (list(mirrors), H.struct_names(header))
    for struct, cls in mirrors.items():
        size, fields = layouts[struct]
        assert [f[0] for f in cls._fields_] == [name for _, _, name in fields], struct
        for (offset, c_type, name), (_, mirror_type) in zip(fields, cls._fields_):
            want = H.ctype_of(c_type, ALL_MIRRORS)
            got = getattr(cls, name)
            assert (got.offset, got.size) == (offset, C.sizeof(want)), f"{struct}.{name}: mirror at {got.offset} of {got.size} bytes, header `{c_type}` at {offset} of {C.sizeof(want)}"
            assert mirror_type is want, f"{struct}.{name}: mirror {mirror_type.__name__}, header `{c_type}`"
        assert C.sizeof(cls) == size, struct


def test_integer_macros():
    """Item 4: every integer-literal CE_* macro of a header that the binding also defines has the header's value."""
    compared = set()
    for header in HEADERS:
        for name, value in H.int_defines(header).items():
            if hasattr(_lib, name):
                assert getattr(_lib, name) == value, (header, name)
                compared.add(name)
    assert MIN_DEFINES <= compared, MIN_DEFINES - compared


def test_exports_are_disjoint_across_headers_and_the_abi_is_3(lib):
    """Items 5 and 6."""
    seen = {}
    for header, entry in _lib.REGISTRY.items():
        for name in entry.signatures:
            assert seen.setdefault(name, header) == header, (name, seen[name], header)
    assert _lib.ALL_EXPORTS == list(seen)
    assert lib.ce_abi_version() == 3 == _lib.CE_ABI_VERSION


def test_every_source_and_header_is_a_build_dependency():
    """Item 7."""
    csrc = ROOT / "srsran_ce_pytorch_amd" / "csrc"
    deps = set(_lib.build_deps())
    files = [p for p in (ROOT / "include").rglob("*") if p.is_file()] + [p for p in csrc.iterdir() if p.suffix in (".hip", ".h", ".inc")]
    assert files and not [str(p) for p in files if p not in deps]
    assert sorted(_lib.SOURCES) == sorted(p.name for p in csrc.glob("*.hip")) and len(set(_lib.SOURCES)) == len(_lib.SOURCES)
