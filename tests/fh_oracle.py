"""Bit-serial numpy restatement of the fronthaul I/Q format of include/ce_tp.h (`ce_fh_decompress`, `ce_fh_compress`;
O-RAN.WG4.CUS Annex A.1 with the udCompParam byte), the oracle of tests/test_fh.py and the GPU tests: one PRB at a time,
np.unpackbits / np.packbits for the bits, Python integers for every shift, np.float32 for the two multiplies.  Every
comparison against it is by bits; there is no tolerance.

A row carries n_prb PRBs without padding.  "bfp", mantissa width W in 1..16: a PRB is 1 + 3 W bytes, byte 0 the parameter
(low nibble e, high nibble reserved), then I0, Q0, .., I11, Q11 as W-bit two's complement, MSB first.  "none": 48 bytes of
big-endian int16, no parameter byte.

The case table, and per case the seeded inputs and what both directions must return, computed once and shared."""
import functools
from types import SimpleNamespace

import numpy as np

METHODS = ("none", "bfp")


def width(method, W):
    assert method in METHODS and 1 <= W <= 16
    return W if method == "bfp" else 16


def prb_bytes(method, W):
    return 1 + 3 * W if method == "bfp" else 48


def row_bytes(method, W, n_prb):
    return n_prb * prb_bytes(method, W)


def inv_scale(scale):
    return np.float32(1.0 / float(np.float32(scale)))


def quantise(x, scale):
    """float32 components -> Python integers: q = x * inv_scale (one float32 multiply), rint to even, NaN -> 0, saturated."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.asarray(x, np.float32) * inv_scale(scale)
    assert q.dtype == np.float32
    out = []
    for v in np.rint(q).tolist():
        if v != v:
            out.append(0)
        else:
            out.append(int(max(-32768.0, min(32767.0, v))))
    return out


def exponent(v24, W):
    """e = max(L + 1 - W, 0) with L the bit length of the largest v >= 0 ? v : ~v of the PRB's 24 values."""
    L = max(v if v >= 0 else ~v for v in v24).bit_length()
    return max(L + 1 - W, 0)


def pack_prb(v24, method, W):
    """The bytes of one PRB of 24 quantised values I0, Q0, .., I11, Q11 (Python integers in int16 range)."""
    W = width(method, W)
    assert len(v24) == 24 and all(-32768 <= v <= 32767 for v in v24)
    e = exponent(v24, W) if method == "bfp" else 0
    bits = []
    for v in v24:
        m = (v >> e) & ((1 << W) - 1)                          # an arithmetic shift: Python's >> floors
        bits += [(m >> (W - 1 - k)) & 1 for k in range(W)]     # MSB first
    body = np.packbits(np.array(bits, np.uint8))
    return np.concatenate([np.array([e], np.uint8), body]) if method == "bfp" else body


def unpack_prb(raw, method, W):
    """(e, the 24 integers v = sign_extend(mantissa) << e) of one PRB's bytes; the reserved nibble is ignored."""
    W = width(method, W)
    raw = np.asarray(raw, np.uint8)
    assert raw.shape == (prb_bytes(method, W),)
    e, body = (int(raw[0]) & 15, raw[1:]) if method == "bfp" else (0, raw)
    bits = np.unpackbits(body).tolist()
    out = []
    for i in range(24):
        m = 0
        for b in bits[i * W:(i + 1) * W]:
            m = (m << 1) | b
        if m >= 1 << (W - 1):
            m -= 1 << W
        out.append(m << e)
    return e, out


def compress_row(x, scale, method, W):
    """complex64 [12 n_prb] -> uint8 [row_bytes]."""
    x = np.ascontiguousarray(np.asarray(x, np.complex64))
    assert x.ndim == 1 and x.size % 12 == 0
    v = quantise(x.view(np.float32), scale)
    return np.concatenate([pack_prb(v[24 * p:24 * p + 24], method, W) for p in range(x.size // 12)])


def decompress_row(raw, n_prb, scale, method, W):
    """uint8 [>= row_bytes] -> complex64 [12 n_prb]: float32(v) * scale, one float32 multiply."""
    nb, s = prb_bytes(method, W), np.float32(scale)
    raw = np.asarray(raw, np.uint8)
    vals = []
    for p in range(n_prb):
        vals += unpack_prb(raw[p * nb:(p + 1) * nb], method, W)[1]
    assert all(abs(v) <= 1 << 30 for v in vals)
    out = np.array(vals, np.int32).astype(np.float32) * s
    assert out.dtype == np.float32
    return out.view(np.complex64)


def compress(grid, scale, method, W):
    """complex64 [..., 12 n_prb] (rows) -> uint8 [..., row_bytes]."""
    grid = np.asarray(grid, np.complex64)
    lead, n_sc = grid.shape[:-1], grid.shape[-1]
    rows = grid.reshape(-1, n_sc)
    out = np.stack([compress_row(r, scale, method, W) for r in rows])
    return out.reshape(lead + (out.shape[-1],))


def decompress(payload, n_prb, scale, method, W):
    """uint8 [..., >= row_bytes] -> complex64 [..., 12 n_prb]."""
    payload = np.asarray(payload, np.uint8)
    lead = payload.shape[:-1]
    rows = payload.reshape(-1, payload.shape[-1])
    return np.stack([decompress_row(r, n_prb, scale, method, W) for r in rows]).reshape(lead + (12 * n_prb,))


# B x R x n_sym rows of n_prb PRBs.  n_prb 1, 3, 24, 273, 341; W 1, 8, 9, 12, 14, 16 and "none"; W = 8 with 1, 2, 3 PRBs gives
# rows of 25, 50, 75 bytes (1, 2, 3 mod 4); 341 PRBs fill five tiles of 64 and one of 21; 273 PRBs four and one of 17; the
# smallest batch is one row, the larger ones 3 x 2 x 14.  The long rows come in small batches: the oracle is bit-serial.
def _case(name, B, R, S, n_prb, method, W, scale=2.0 ** -11):
    return dict(name=name, B=B, R=R, S=S, n_prb=n_prb, method=method, W=width(method, W), scale=float(np.float32(scale)))


CASES = [
    _case("w9_prb1_one_row", 1, 1, 1, 1, "bfp", 9),
    _case("w9_prb24", 3, 2, 14, 24, "bfp", 9),
    _case("w9_prb273", 1, 2, 2, 273, "bfp", 9),
    _case("w9_prb341", 2, 1, 1, 341, "bfp", 9, scale=3.1e-4),
    _case("w14_prb3", 3, 2, 14, 3, "bfp", 14, scale=2.0 ** -9),
    _case("w14_prb273", 1, 1, 1, 273, "bfp", 14),
    _case("w8_prb1", 3, 2, 14, 1, "bfp", 8),
    _case("w8_prb2", 3, 2, 14, 2, "bfp", 8, scale=7.3e-5),
    _case("w8_prb3", 3, 2, 14, 3, "bfp", 8),
    _case("w1_prb3", 3, 2, 14, 3, "bfp", 1),
    _case("w1_prb341", 1, 1, 1, 341, "bfp", 1),
    _case("w12_prb24", 3, 2, 14, 24, "bfp", 12, scale=1.7),
    _case("w16_prb24", 1, 2, 3, 24, "bfp", 16),
    _case("w16_prb341", 1, 1, 1, 341, "bfp", 16),
    _case("none_prb3", 3, 2, 14, 3, "none", 16),
    _case("none_prb1_one_row", 1, 1, 1, 1, "none", 16),
    _case("none_prb341", 1, 1, 2, 341, "none", 16, scale=2.0 ** -15),
]
CASE_NAMES = [c["name"] for c in CASES]
CASE_BY_NAME = {c["name"]: c for c in CASES}
AMPLITUDES = (3.0, 900.0, 14000.0)        # in quantiser steps: a PRB of each has e = 0, a mid-range e and the largest e of its W
SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0, 32767.5, -32767.5, 32766.5, -32768.5, 0.5, -0.5, 1.5, 2.5, -1.5, 1e9, -1e9)


def make_grid(rng, shape, scale):
    """complex64 `shape` = [.., 12 n_prb]: a seeded Gaussian whose amplitude cycles per PRB through AMPLITUDES (in quantiser
    steps), and the SPECIALS (times scale; NaN, the infinities, signed zeros, ties, the saturation edges) at seeded places."""
    n = int(np.prod(shape))
    amp = np.asarray(AMPLITUDES)[(np.arange(n) // 12 + rng.integers(0, 3)) % 3]
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp * float(np.float32(scale))
    flat = np.ascontiguousarray(x.astype(np.complex64)).view(np.float32)
    where = rng.choice(flat.size, size=min(len(SPECIALS), flat.size), replace=False)
    with np.errstate(over="ignore", invalid="ignore"):
        flat[where] = (np.asarray(SPECIALS[:where.size]) * float(np.float32(scale))).astype(np.float32)
    return flat.view(np.complex64).reshape(shape)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Per case, read-only: `grid` complex64 [B, R, S, 12 n_prb] (rows: the fast layout) and `packed` = compress(grid);
    `payload` uint8 [B, R, S, row_bytes] of seeded random bytes (every exponent, random reserved nibbles, every mantissa)
    and `unpacked` = decompress(payload); `restored` = decompress(packed) and `repacked` = compress(restored), the round trip."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(1000 + CASE_NAMES.index(name))
    shape = (c["B"], c["R"], c["S"], 12 * c["n_prb"])
    grid = make_grid(rng, shape, c["scale"])
    nb = row_bytes(c["method"], c["W"], c["n_prb"])
    payload = rng.integers(0, 256, shape[:3] + (nb,), dtype=np.uint8)
    d = SimpleNamespace(c=c, name=name, grid=grid, payload=payload, row_bytes=nb,
                        packed=compress(grid, c["scale"], c["method"], c["W"]),
                        unpacked=decompress(payload, c["n_prb"], c["scale"], c["method"], c["W"]))
    d.restored = decompress(d.packed, c["n_prb"], c["scale"], c["method"], c["W"])
    d.repacked = compress(d.restored, c["scale"], c["method"], c["W"])
    for a in (d.grid, d.payload, d.packed, d.unpacked, d.restored, d.repacked):
        a.setflags(write=False)
    return d
