"""CPU-side checks of fronthaul I/Q (de)compression (include/ce_tp.h `ce_fh_decompress`, `ce_fh_compress`, `ce_fh_row_bytes`;
srsran_ce_pytorch_amd/fronthaul.py): the three consequences of the format's definitions on seeded draws for every mantissa
width, the bit-serial oracle of tests/fh_oracle.py against hand-made PRBs and against the numpy host helpers on every case,
`ce_fh_row_bytes`, the exports and their signatures, every refusal of the entry points (they all come before anything touches
a device) and of the wrappers that needs no GPU.  No GPU."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import fh_oracle as X
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, fronthaul as FH

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _draws(W):
    """Seeded float32 components of 40 PRBs: amplitudes from 0.5 to 1e9 quantiser steps, with NaN and the infinities; and one
    PRB of zeros in front."""
    rng = np.random.default_rng(100 + W)
    amp = np.repeat(np.geomspace(0.5, 1e9, 40), 24)
    x = (rng.standard_normal(amp.size) * amp).astype(np.float32)
    x[rng.choice(x.size, 12, replace=False)] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 32767.5, -32767.5, -32768.5, 0.5, 1.5, 2.5, -0.5], np.float32)
    return np.concatenate([np.zeros(24, np.float32), x])


@pytest.mark.parametrize("W", range(1, 17))
def test_the_three_consequences_of_the_definitions(W):
    """e <= 15 and every mantissa fits W bits; 0 <= v - (mantissa << e) < 2^e; compression of mantissa << e is (e, mantissa) again."""
    v = X.quantise(_draws(W), 1.0)
    assert all(-32768 <= a <= 32767 for a in v)
    seen = set()
    for p in range(len(v) // 24):
        v24 = v[24 * p:24 * p + 24]
        raw = X.pack_prb(v24, "bfp", W)
        assert raw.shape == (1 + 3 * W,) and raw[0] <= 15
        e, back = X.unpack_prb(raw, "bfp", W)
        assert e == X.exponent(v24, W) == raw[0]
        seen.add(e)
        for a, b in zip(v24, back):
            m = b >> e
            assert b == m << e and -(1 << (W - 1)) <= m < 1 << (W - 1) and 0 <= a - b < 1 << e
        again = X.pack_prb(back, "bfp", W)
        assert np.array_equal(again, raw)                      # idempotent on its own output
    assert min(seen) == 0 and max(seen) == 16 - W              # from no shift to the largest one of this width


def test_the_oracle_on_hand_made_prbs():
    # W = 9: the largest magnitude 255 / -256 still fits, 256 / -257 shifts by one
    for top, e in ((255, 0), (-256, 0), (256, 1), (-257, 1), (32767, 7), (-32768, 7), (0, 0)):
        assert X.exponent([top] + [0] * 23, 9) == e
    raw = X.pack_prb([1, -1] + [0] * 22, "bfp", 9)
    assert raw.tolist()[:4] == [0, 0b00000000, 0b11111111, 0b11000000] and not raw[4:].any()      # bit 7 of byte 1 is I0's top bit
    raw = X.pack_prb([-3, 5] + [0] * 22, "bfp", 4)
    assert raw.tolist()[:2] == [0, 0xD5]
    raw = X.pack_prb([0x1234, -2] + [0] * 22, "none", 16)
    assert raw.shape == (48,) and raw.tolist()[:4] == [0x12, 0x34, 0xFF, 0xFE]                     # big-endian int16
    assert np.array_equal(X.pack_prb([0x1234, -2] + [0] * 22, "bfp", 16)[1:], raw)                 # "none" is W = 16, e = 0, no byte 0
    assert X.pack_prb([300, -7] + [0] * 22, "bfp", 9).tolist()[:3] == [1, 0b01001011, 0b01111111]   # e = 1: 150 = 0_1001_0110, -4 = 1_1111_1100
    # the reserved nibble is ignored; e comes from the low one
    raw = np.array([0xA3] + [0x7F, 0xC0] + [0] * 25, np.uint8)                                          # 0_1111_1111, 1_0000_0000
    assert X.unpack_prb(raw, "bfp", 9) == (3, [255 << 3, -256 << 3] + [0] * 22)
    # the quantiser: ties to even, NaN, saturation, one float32 multiply by float32(1 / scale)
    got = X.quantise(np.array([0.5, 1.5, 2.5, -0.5, -1.5, np.nan, np.inf, -np.inf, 32767.5, -32768.5, 32766.5, -0.0], np.float32), 1.0)
    assert got == [0, 2, 2, 0, -2, 0, 32767, -32768, 32767, -32768, 32766, 0]
    assert float(X.inv_scale(3.0)) == float(np.float32(1.0 / 3.0)) and X.quantise(np.array([3.0], np.float32), 3.0) == [1]
    out = X.decompress_row(X.compress_row(np.array([1 + 2j] * 12, np.complex64), 0.5, "bfp", 9), 1, 0.5, "bfp", 9)
    assert out.dtype == np.complex64 and np.array_equal(out, np.array([1 + 2j] * 12, np.complex64))


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_host_helpers_against_the_oracle(name):
    d = X.inputs(name)
    c = d.c
    packed = FH.bfp_pack(d.grid, c["scale"], c["W"], c["method"])
    assert packed.dtype == np.uint8 and packed.shape == d.packed.shape == (c["B"], c["R"], c["S"], d.row_bytes) and np.array_equal(packed, d.packed)
    if c["method"] == "bfp":
        assert not (packed.reshape(-1, 1 + 3 * c["W"])[:, 0] >> 4).any()                         # the compressor writes 0 into the reserved nibble
    wide = np.concatenate([d.payload, np.full(d.payload.shape[:3] + (5,), 0xEE, np.uint8)], -1)     # a longer last dimension
    got = FH.bfp_unpack(wide, c["n_prb"], c["scale"], c["W"], c["method"])
    assert got.dtype == np.complex64 and got.shape == d.unpacked.shape and np.array_equal(got.view(np.uint32), d.unpacked.view(np.uint32))
    # compress(decompress(compress(x))) == compress(x)
    back = FH.bfp_unpack(d.packed, c["n_prb"], c["scale"], c["W"], c["method"])
    assert np.array_equal(back.view(np.uint32), d.restored.view(np.uint32)) and np.array_equal(FH.bfp_pack(back, c["scale"], c["W"], c["method"]), d.repacked)
    if float(X.inv_scale(c["scale"])) * c["scale"] == 1.0:                                       # a power of two: the round trip of the scale is exact
        assert np.array_equal(d.repacked, d.packed)


def test_the_cases_reach_every_path():
    cs = X.CASES
    assert {c["n_prb"] for c in cs} == {1, 2, 3, 24, 273, 341} and {c["W"] for c in cs if c["method"] == "bfp"} == {1, 8, 9, 12, 14, 16}
    assert any(c["method"] == "none" for c in cs) and {X.row_bytes(c["method"], c["W"], c["n_prb"]) % 4 for c in cs} == {0, 1, 2, 3}
    assert {(c["B"], c["R"], c["S"]) for c in cs} >= {(1, 1, 1), (3, 2, 14)}
    exps = set()
    for name in X.CASE_NAMES:
        d = X.inputs(name)
        if d.c["method"] == "bfp":
            exps |= set((d.packed.reshape(-1, 1 + 3 * d.c["W"])[:, 0]).tolist())
            assert set((d.payload.reshape(-1, 1 + 3 * d.c["W"])[:, 0] >> 4).tolist()) - {0}      # random reserved nibbles in the payloads
    assert {0, 7, 15} <= exps and any(0 < e < 7 for e in exps)
    d = X.inputs("w9_prb24")
    flat = d.grid.view(np.float32)
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (flat == 32767.5 * np.float32(d.c["scale"])).any()
    assert np.signbit(flat[flat == 0.0]).any() and not np.signbit(flat[flat == 0.0]).all()


def test_row_bytes(lib):
    out = C.c_int64()
    for W in range(1, 17):
        for n in (1, 2, 3, 24, 273, 341):
            assert lib.ce_fh_row_bytes(_lib.CE_FH_BFP, W, n, C.byref(out)) == 0 and out.value == n * (1 + 3 * W) == FH.row_bytes("bfp", W, n)
            assert lib.ce_fh_row_bytes(_lib.CE_FH_NONE, W, n, C.byref(out)) == 0 and out.value == 48 * n == FH.row_bytes("none", W, n)
    for args, code, text in (((_lib.CE_FH_BFP, 0, 1), _lib.CE_ERR_INVALID, "iq_width=0 outside 1..16"), ((_lib.CE_FH_BFP, 17, 1), _lib.CE_ERR_INVALID, "iq_width=17 outside 1..16"),
                             ((2, 9, 1), _lib.CE_ERR_UNSUPPORTED, "method=2 is neither"), ((-1, 9, 1), _lib.CE_ERR_UNSUPPORTED, "method=-1"),
                             ((_lib.CE_FH_BFP, 9, 0), _lib.CE_ERR_INVALID, "n_prb=0 outside 1..341"), ((_lib.CE_FH_NONE, 9, 342), _lib.CE_ERR_INVALID, "n_prb=342 outside 1..341")):
        assert lib.ce_fh_row_bytes(*args, C.byref(out)) == code and text in _lib.last_error(), (args, _lib.last_error())
    assert lib.ce_fh_row_bytes(_lib.CE_FH_BFP, 9, 1, None) == _lib.CE_ERR_INVALID and _lib.last_error() == "null argument"
    fh = FH.PuschFronthaulDecompressor(273)
    assert fh.row_bytes() == 273 * 28 and fh.row_bytes(51) == 51 * 28 and FH.PuschFronthaulDecompressor(24, method="none").row_bytes() == 24 * 48
    with pytest.raises(ValueError, match="n_prb=0 outside 1..341"):
        fh.row_bytes(0)


def test_exports_registry_sources_and_the_package(lib):
    sig = _lib.REGISTRY["ce_tp.h"].signatures
    assert [n for n in sig if n.startswith("ce_fh_")] == ["ce_fh_row_bytes", "ce_fh_decompress", "ce_fh_compress"]
    assert len(sig["ce_fh_decompress"][1]) == len(sig["ce_fh_compress"][1]) == 17 and len(sig["ce_fh_row_bytes"][1]) == 4
    assert sig["ce_fh_decompress"][1][15] is C.c_float and sig["ce_fh_compress"][1] == sig["ce_fh_decompress"][1]
    assert all(n in _lib.ALL_EXPORTS and hasattr(lib, n) for n in sig if n.startswith("ce_fh_"))
    assert "ce_fh.hip" in _lib.SOURCES and (CSRC / "ce_fh.hip").is_file()
    assert (_lib.CE_FH_NONE, _lib.CE_FH_BFP, _lib.CE_FH_MAX_PRBS) == (0, 1, 341) and lib.ce_abi_version() == 3
    assert PKG.PuschFronthaulDecompressor is FH.PuschFronthaulDecompressor and PKG.PuschFronthaulCompressor is FH.PuschFronthaulCompressor
    assert PKG.bfp_pack is FH.bfp_pack and PKG.bfp_unpack is FH.bfp_unpack
    p = inspect.signature(FH.PuschFronthaulDecompressor).parameters
    assert list(p) == ["n_prb_grid", "n_sym", "method", "iq_width", "scale", "device"]
    assert (p["n_sym"].default, p["method"].default, p["iq_width"].default, p["scale"].default) == (14, "bfp", 9, 2.0 ** -11)
    for cls in (FH.PuschFronthaulDecompressor, FH.PuschFronthaulCompressor):
        q = inspect.signature(cls.__call__).parameters
        assert list(q)[2:] == ["start_prb", "n_prb", "out"] and (q["start_prb"].default, q["n_prb"].default, q["out"].default) == (0, None, None)
    fh = FH.PuschFronthaulDecompressor(51, 12, "bfp", 14, 2.0 ** -9)
    comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
    assert (comp.n_prb_grid, comp.n_sym, comp.method, comp.iq_width, comp.scale, comp.n_sc, comp.device) == (51, 12, "bfp", 14, fh.scale, 612, None)
    assert comp.inv_scale == np.float32(2.0 ** 9) and FH.inv_scale(3.0) == np.float32(1.0 / 3.0)
    assert FH.PuschFronthaulDecompressor(24, method="none", iq_width=9).iq_width == 16


def test_refusals_of_the_entry_points_come_before_any_device_call(lib):
    """Every argument error of ce_fh_decompress and ce_fh_compress with its text, on made-up addresses: nothing is dereferenced
    or launched.  B x R x S = 2 x 3 x 4 rows of 5 PRBs at W = 9: 140 bytes and 60 REs a row."""
    B, R, S, n, W = 2, 3, 4, 5, 9
    nb, n_sc = n * 28, 12 * n
    pp, pg = 0x10000, 0x80000

    def call(fn, abi=3, p=pp, ps=(R * S * nb, S * nb, nb), g=pg, gs=(R * S * n_sc, S * n_sc, n_sc), slots=B, ports=R, sym=S, prb=n, method=1, width=W, scale=0.5):
        vp = lambda a: C.c_void_p(a) if a else None
        return getattr(lib, fn)(abi, vp(p), *ps, vp(g), *gs, slots, ports, sym, prb, method, width, scale, None)

    dense_p, dense_g = (R * S * nb, S * nb, nb), (R * S * n_sc, S * n_sc, n_sc)
    both = [
        (dict(abi=2), "ABI version 2 != 3"), (dict(width=0), "iq_width=0 outside 1..16"), (dict(width=17), "iq_width=17 outside 1..16"),
        (dict(prb=0), "n_prb=0 outside 1..341"), (dict(prb=342), "n_prb=342 outside 1..341"), (dict(sym=0), "n_sym=0 must be >= 1"),
        (dict(ports=0), "n_ports=0 must be >= 1"), (dict(slots=-1), "n_slots=-1"), (dict(slots=0, width=0), "iq_width=0 outside 1..16"),
        (dict(scale=float("nan")), "outside 2^-96 .. 2^96"), (dict(scale=float("inf")), "outside 2^-96 .. 2^96"), (dict(scale=0.0), "outside 2^-96 .. 2^96"),
        (dict(scale=-1.0), "outside 2^-96 .. 2^96"), (dict(scale=2.0 ** -97), "outside 2^-96 .. 2^96"), (dict(scale=2.0 ** 97), "outside 2^-96 .. 2^96"),
        (dict(p=0), "null argument"), (dict(g=0), "null argument"),
        (dict(ps=(-4, S * nb, nb)), "strides must be >= 0"), (dict(ps=(R * S * nb, S * nb, -4)), "strides must be >= 0"),
        (dict(gs=(R * S * n_sc, -1, n_sc)), "strides must be >= 0"),
        (dict(p=pp + 2), "multiples of 4 bytes"), (dict(p=pp + 1), "multiples of 4 bytes"), (dict(ps=(R * S * nb + 2, S * nb, nb)), "multiples of 4 bytes"),
        (dict(ps=(R * S * nb, S * nb + 1, nb)), "multiples of 4 bytes"), (dict(ps=(R * S * nb, S * nb, nb + 3)), "multiples of 4 bytes"),
        (dict(g=pg + 4), "grid must be 8-byte aligned"),
        (dict(ps=(1 << 60, S * nb, nb)), "exceeds the address space"), (dict(gs=(R * S * n_sc, 1 << 60, n_sc)), "exceeds the address space"),
        (dict(gs=(R * S * n_sc, S * n_sc, 1 << 60)), "exceeds the address space"),
        (dict(g=pp), "payload overlaps grid"), (dict(g=pp + B * R * S * nb - 8), "payload overlaps grid"), (dict(p=pg + 8 * B * R * S * n_sc - 4), "payload overlaps grid"),
    ]
    for fn in ("ce_fh_decompress", "ce_fh_compress"):
        for kw, text in both:
            assert call(fn, **kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (fn, kw, _lib.last_error())
        for kw in (dict(method=2), dict(method=-1)):
            assert call(fn, **kw) == _lib.CE_ERR_UNSUPPORTED and "is neither CE_FH_NONE (0) nor CE_FH_BFP (1)" in _lib.last_error(), (fn, kw)
        for kw in (dict(slots=1 << 31), dict(ports=1 << 31), dict(slots=1 << 16, ports=1 << 15), dict(slots=1 << 20, ports=1 << 9, sym=4), dict(slots=1 << 20, ports=1 << 8, sym=4, prb=65)):
            zero = dict(ps=(0, 0, 0), gs=(0, 0, 0))
            assert call(fn, **zero, **kw) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error(), (fn, kw, _lib.last_error())
        assert call(fn, slots=0) == 0 and call(fn, slots=0, p=0, g=0) == 0                              # an empty batch launches nothing
    # rows of the WRITTEN side that share elements, in any nesting; the side that is read is free
    grid_overlaps = [(R * S * n_sc, S * n_sc, n_sc - 1), (R * S * n_sc, S * n_sc - 1, n_sc), (R * S * n_sc - 1, S * n_sc, n_sc), (0, S * n_sc, n_sc), (R * S * n_sc, 0, n_sc),
                     (R * S * n_sc, S * n_sc, 0), (n_sc, B * n_sc, B * R * n_sc - 1), (S * n_sc, B * S * n_sc - 1, n_sc), (0, 0, 0)]
    for gs in grid_overlaps:
        assert call("ce_fh_decompress", gs=gs) == _lib.CE_ERR_INVALID and "grid: slot_stride=" in _lib.last_error() and f"the rows of {n_sc} REs of {B} slots x {R} ports x {S} symbols overlap" in _lib.last_error(), gs
    pay_overlaps = [(R * S * nb, S * nb, nb - 4), (R * S * nb, S * nb - 4, nb), (R * S * nb - 4, S * nb, nb), (0, S * nb, nb), (R * S * nb, S * nb, 0), (nb, B * nb, B * R * nb - 4), (0, 0, 0)]
    for ps in pay_overlaps:
        assert call("ce_fh_compress", ps=ps) == _lib.CE_ERR_INVALID and "payload: slot_stride=" in _lib.last_error() and f"the rows of {nb} bytes of" in _lib.last_error(), ps
    # with one entry in a dimension its stride does not matter
    assert call("ce_fh_decompress", slots=0, gs=(0, 0, 0)) == 0
    # the accepted nestings would launch, so they are GPU tests; here: a row of 25 bytes (W = 8, one PRB) against a stride of 28
    assert call("ce_fh_compress", prb=1, width=8, ps=(R * S * 28, S * 28, 24)) == _lib.CE_ERR_INVALID and "the rows of 25 bytes" in _lib.last_error()


def test_wrapper_refusals_that_need_no_device(lib):
    for cls in (FH.PuschFronthaulDecompressor, FH.PuschFronthaulCompressor):
        for args, kw, text in (((0,), {}, "n_prb_grid=0 outside 1..341"), ((342,), {}, "n_prb_grid=342 outside 1..341"), ((24.0,), {}, "n_prb_grid must be an int"),
                               ((True,), {}, "n_prb_grid must be an int"), ((24, 0), {}, "n_sym=0 must be >= 1"), ((24, "14"), {}, "n_sym must be an int"),
                               ((24,), dict(method="mulaw"), "method='mulaw' is none of"), ((24,), dict(method=1), "method=1 is none of"),
                               ((24,), dict(iq_width=0), "iq_width=0 outside 1..16"), ((24,), dict(iq_width=17), "iq_width=17 outside 1..16"),
                               ((24,), dict(iq_width=9.0), "iq_width must be an int"), ((24,), dict(method="none", iq_width=0), "iq_width=0 outside 1..16"),
                               ((24,), dict(scale=0.0), "scale=0.0 must be finite and within"), ((24,), dict(scale=float("nan")), "scale=nan must be finite"),
                               ((24,), dict(scale=float("inf")), "scale=inf must be finite"), ((24,), dict(scale=-1.0), "scale=-1.0 must be finite"),
                               ((24,), dict(scale=2.0 ** -97), "within 2\\^-96 .. 2\\^96"), ((24,), dict(scale=2.0 ** 97), "within"), ((24,), dict(scale=1e300), "must be finite"),
                               ((24,), dict(scale="1"), "scale must be a float")):
            with pytest.raises(ValueError, match=text):
                cls(*args, **kw)
        ok = cls(24, scale=2.0 ** -96)
        assert ok.scale == np.float32(2.0 ** -96) and cls(24, scale=2.0 ** 96).inv_scale == np.float32(2.0 ** -96) and ok.device is None
        # no CPU fallback: the call is refused before it looks at its arguments
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            cls(24, device="cpu")(torch.zeros((1, 1, 14, 24 * 28), dtype=torch.uint8))
        with pytest.raises(RuntimeError, match=f"{cls._NOUN} runs on a ROCm GPU only"):
            cls(24, device=torch.device("cpu"))(None)
    for args, text in (((np.zeros(11, np.complex64), 1.0), "12 n_prb subcarriers"), ((np.zeros(12 * 342, np.complex64), 1.0), "12 n_prb subcarriers"),
                       ((np.zeros(12, np.complex64), 0.0), "scale=0.0"), ((np.zeros(12, np.complex64), 1.0, 17), "iq_width=17")):
        with pytest.raises(ValueError, match=text):
            FH.bfp_pack(*args)
    for args, text in (((np.zeros(27, np.uint8), 1, 1.0), "at least 28 bytes"), ((np.zeros(28, np.int8), 1, 1.0), "payload must be uint8"),
                       ((np.zeros(28, np.uint8), 0, 1.0), "n_prb=0 outside"), ((np.zeros(28, np.uint8), 1, 1.0, 9, "x"), "method='x'")):
        with pytest.raises(ValueError, match=text):
            FH.bfp_unpack(*args)
