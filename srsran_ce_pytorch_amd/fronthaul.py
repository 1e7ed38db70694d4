"""Fronthaul I/Q (de)compression EXTENSION (include/ce_tp.h `ce_fh_decompress`, `ce_fh_compress`; the reference stops at the
channel estimate): the front door behind an O-RAN 7.2x radio unit, which does the FFT itself and sends, per port and symbol, a
run of PRBs of frequency-domain I/Q -- block floating point (BFP) with a 1..16 bit mantissa, usually 9 and sometimes 14, or
plain big-endian int16 (O-RAN.WG4.CUS Annex A.1).  One launch per direction on the current stream, no plan.

    fh = PuschFronthaulDecompressor(n_prb_grid, n_sym=14, method="bfp", iq_width=9, scale=2.0 ** -11)
    received_rg = fh(payload)                               # uint8 [B, R, n_sym, >= row_bytes] -> [B, R, n_sc, n_sym], fast layout
    fh(payload, start_prb=24, n_prb=51, out=received_rg)    # a section: only those PRBs' REs are written
    comp = PuschFronthaulCompressor.for_decompressor(fh)
    payload = comp(received_rg)                             # -> uint8 [B, R, n_sym, row_bytes]

A row is one (port, symbol) of PRBs in ascending subcarrier order, which is the estimator's fast layout
``[slot][port][symbol][subcarrier]`` as it stands: the decompressor writes ``received_rg`` rows without a transposition.  A
BFP PRB is ``1 + 3 W`` bytes: the parameter byte (low nibble: the exponent ``e``, high nibble reserved), then I0, Q0, .., I11,
Q11 as ``W``-bit two's complement, MSB first without gaps; ``"none"`` is 48 bytes of big-endian int16 without the parameter
byte.  A component decompresses to ``float32(sign_extend(mantissa) << e) * scale`` and compresses as ``v = rint(x *
inv_scale)`` (to even, NaN -> 0, saturated to int16) with, per PRB, ``e = max(bit_length(max(v >= 0 ? v : ~v)) + 1 - W, 0)``
and ``mantissa = v >> e``; every output is defined to the bit.  ``bfp_pack`` and ``bfp_unpack`` are the same operators in
numpy, on the host.

Out of scope: eCPRI and section headers, payloads at unaligned byte offsets, block scaling, mu-law, modulation compression and
selective-RE methods, a per-section ``scale`` as a device tensor, decompression fused into the estimator's loads."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib, _stage

METHODS = {"none": _lib.CE_FH_NONE, "bfp": _lib.CE_FH_BFP}
MAX_PRBS = _lib.CE_FH_MAX_PRBS
SCALE_MIN, SCALE_MAX = 2.0 ** -96, 2.0 ** 96


def _format(method, iq_width):
    """(method code, W) of a validated method name and mantissa width; ``"none"`` is W = 16 whatever `iq_width`."""
    if method not in METHODS:
        raise ValueError(f"method={method!r} is none of {sorted(METHODS)}")
    if isinstance(iq_width, bool) or not isinstance(iq_width, (int, np.integer)):
        raise ValueError(f"iq_width must be an int, got {type(iq_width).__name__}")
    if not 1 <= int(iq_width) <= 16:
        raise ValueError(f"iq_width={int(iq_width)} outside 1..16")
    return METHODS[method], (int(iq_width) if method == "bfp" else 16)


def _scale(scale) -> np.float32:
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
        raise ValueError(f"scale must be a float, got {type(scale).__name__}")
    with np.errstate(over="ignore"):
        s = np.float32(scale)
    if not (math.isfinite(float(s)) and SCALE_MIN <= float(s) <= SCALE_MAX):
        raise ValueError(f"scale={float(scale)!r} must be finite and within 2^-96 .. 2^96")
    return s


def inv_scale(scale) -> np.float32:
    """``float32(1 / double(scale))``, rounded once: what the compressor multiplies by."""
    return np.float32(1.0 / float(_scale(scale)))


def row_bytes(method: str, iq_width: int, n_prb: int) -> int:
    """The bytes of a row of `n_prb` PRBs: ``n_prb (1 + 3 iq_width)`` for ``"bfp"``, ``48 n_prb`` for ``"none"`` (`ce_fh_row_bytes`)."""
    code, W = _format(method, iq_width)
    if isinstance(n_prb, bool) or not isinstance(n_prb, (int, np.integer)):
        raise ValueError(f"n_prb must be an int, got {type(n_prb).__name__}")
    out = C.c_int64()
    rc = _lib.load().ce_fh_row_bytes(code, W, int(n_prb) if -2 ** 31 <= int(n_prb) < 2 ** 31 else -1, C.byref(out))
    if rc != 0:
        _stage.raise_for(rc)
    return int(out.value)


def bfp_pack(grid, scale, iq_width: int = 9, method: str = "bfp") -> np.ndarray:
    """numpy, on the host: complex64 ``[..., 12 n_prb]`` (the last dimension one row's subcarriers) -> uint8 ``[..., row_bytes]``,
    the compressor's bytes."""
    code, W = _format(method, iq_width)
    x = np.ascontiguousarray(np.asarray(grid, np.complex64))
    if x.ndim < 1 or x.shape[-1] < 12 or x.shape[-1] % 12 or x.shape[-1] // 12 > MAX_PRBS:
        raise ValueError(f"grid must hold 12 n_prb subcarriers, n_prb in 1..{MAX_PRBS}, in its last dimension, got {x.shape}")
    lead, n_prb = x.shape[:-1], x.shape[-1] // 12
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(x.view(np.float32).reshape(lead + (n_prb, 24)) * inv_scale(scale))
    v = np.clip(np.where(np.isnan(q), np.float32(0.0), q), -32768.0, 32767.0).astype(np.int32)
    if code == _lib.CE_FH_NONE:
        return np.ascontiguousarray(v.astype(">i2")).view(np.uint8).reshape(lead + (48 * n_prb,))
    peak = np.where(v >= 0, v, ~v).max(-1)
    length = sum((peak >> k) > 0 for k in range(16)).astype(np.int32)                 # bit_length of a value below 2^15
    e = np.maximum(length + 1 - W, 0)
    mant = (v >> e[..., None]) & ((1 << W) - 1)
    bits = ((mant[..., None] >> np.arange(W - 1, -1, -1)) & 1).astype(np.uint8)       # MSB first
    body = np.packbits(bits.reshape(lead + (n_prb, 24 * W)), axis=-1)
    return np.concatenate([e[..., None].astype(np.uint8), body], axis=-1).reshape(lead + (n_prb * (1 + 3 * W),))


def bfp_unpack(payload, n_prb: int, scale, iq_width: int = 9, method: str = "bfp") -> np.ndarray:
    """numpy, on the host: uint8 ``[..., >= row_bytes]`` -> complex64 ``[..., 12 n_prb]``, the decompressor's values."""
    code, W = _format(method, iq_width)
    s, nb = _scale(scale), row_bytes(method, iq_width, n_prb)
    p = np.asarray(payload)
    if p.dtype != np.uint8 or p.ndim < 1 or p.shape[-1] < nb:
        raise ValueError(f"payload must be uint8 with at least {nb} bytes in its last dimension, got {p.dtype} {p.shape}")
    lead = p.shape[:-1]
    rows = p[..., :nb].reshape(lead + (n_prb, nb // n_prb))
    hdr = 1 if code == _lib.CE_FH_BFP else 0
    e = (rows[..., 0].astype(np.int32) & 15) if hdr else np.zeros(lead + (n_prb,), np.int32)
    bits = np.unpackbits(np.ascontiguousarray(rows[..., hdr:]), axis=-1).reshape(lead + (n_prb, 24, W)).astype(np.int32)
    mant = (bits << np.arange(W - 1, -1, -1)).sum(-1)
    mant = mant - ((mant >> (W - 1)) << W)                                            # two's complement of W bits
    v = (mant << e[..., None]).astype(np.float32) * s
    return np.ascontiguousarray(v.reshape(lead + (12 * n_prb, 2))).view(np.complex64).reshape(lead + (12 * n_prb,))


class _Fronthaul:
    """What the two directions share: the validated format (no GPU needed), the device bound at the first call, the checks
    of a payload ``[B, R, n_sym, >= row_bytes]`` and of a grid ``[B, R, n_sc, n_sym]`` in the fast layout, and the launch."""

    _NOUN = _ENTRY = ""

    def __init__(self, n_prb_grid: int, n_sym: int = 14, method: str = "bfp", iq_width: int = 9, scale: float = 2.0 ** -11, device=None):
        for name, v in (("n_prb_grid", n_prb_grid), ("n_sym", n_sym)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an int, got {type(v).__name__}")
        self.n_prb_grid, self.n_sym, self.method = int(n_prb_grid), int(n_sym), method
        self._code, self.iq_width = _format(method, iq_width)
        if not 1 <= self.n_prb_grid <= MAX_PRBS:
            raise ValueError(f"n_prb_grid={self.n_prb_grid} outside 1..{MAX_PRBS}")
        if not 1 <= self.n_sym <= 2 ** 31 - 1:
            raise ValueError(f"n_sym={self.n_sym} must be >= 1")
        self.scale = _scale(scale)
        self.inv_scale = inv_scale(self.scale)
        self.n_sc = 12 * self.n_prb_grid
        self._lib = _lib.load()
        self._device_arg = device
        self.device: Optional[torch.device] = None

    def row_bytes(self, n_prb: Optional[int] = None) -> int:
        """The bytes of a row of `n_prb` PRBs (the whole grid's by default) in this format."""
        return row_bytes(self.method, self.iq_width, self.n_prb_grid if n_prb is None else n_prb)

    def _bind(self) -> torch.device:
        if self.device is None:
            device = self._device_arg
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError(f"{self._NOUN} runs on a ROCm GPU only (no CPU fallback)")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self.device = device
        return self.device

    def _section(self, start_prb, n_prb):
        for name, v in (("start_prb", start_prb), ("n_prb", n_prb)):
            if (v is not None or name == "start_prb") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"{name} must be an int, got {type(v).__name__}")
        start = int(start_prb)
        n = self.n_prb_grid - start if n_prb is None else int(n_prb)
        if start < 0 or n < 1 or start + n > self.n_prb_grid:
            raise ValueError(f"start_prb={start}, n_prb={n}: the section lies outside the {self.n_prb_grid} PRBs of the grid")
        return start, n

    @staticmethod
    def _strides(name: str, t: torch.Tensor, dims, row: int, unit: int):
        """The strides of `dims` of `t` in elements (0 where the dimension has one entry), or ``ValueError`` where a stride is
        negative or the last row's `row` elements lie behind what the tensor's storage holds."""
        s = [int(t.stride(d)) if t.shape[d] > 1 else 0 for d in dims]
        if min(s) < 0:
            raise ValueError("negative strides are not supported")
        held = t.untyped_storage().nbytes() // unit - int(t.storage_offset())
        if sum((int(t.shape[d]) - 1) * st for d, st in zip(dims, s)) + row > held:
            raise ValueError(f"{name}: strides {tuple(s)} put the last row's {row} elements behind the {held} the tensor holds")
        return s

    def _check_payload(self, name: str, p, nb: int, B: Optional[int] = None, R: Optional[int] = None):
        dev = self.device
        if not isinstance(p, torch.Tensor) or p.device != dev:
            raise ValueError(f"{name} must be a tensor on {dev}")
        if (p.dtype != torch.uint8 or p.dim() != 4 or p.shape[2] != self.n_sym or p.shape[1] < 1 or p.shape[3] < nb or (p.shape[3] > 1 and p.stride(3) != 1)
                or (B is not None and tuple(p.shape[:2]) != (B, R))):
            lead = "slots, ports" if B is None else f"{B}, {R}"
            raise ValueError(f"{name} must be a {torch.uint8} tensor [{lead}, {self.n_sym}, >= {nb}] with a contiguous last dimension, got "
                             f"{p.dtype} {tuple(p.shape)} with strides {tuple(p.stride())}")
        if p.shape[0] == 0:
            return [0, 0, 0]
        s = self._strides(name, p, (0, 1, 2), nb, 1)
        if p.data_ptr() % 4 or any(v % 4 for v in s):
            raise ValueError(f"{name}: the first byte and the strides {tuple(s)} must be multiples of 4 bytes")
        return s

    def _check_grid(self, name: str, g, B: Optional[int] = None, R: Optional[int] = None):
        dev = self.device
        if not isinstance(g, torch.Tensor) or g.device != dev:
            raise ValueError(f"{name} must be a tensor on {dev}")
        if g.dtype != torch.complex64 or g.dim() != 4 or tuple(g.shape[2:]) != (self.n_sc, self.n_sym) or g.shape[1] < 1 or (B is not None and tuple(g.shape[:2]) != (B, R)):
            lead = "slots, ports" if B is None else f"{B}, {R}"
            raise ValueError(f"{name} must be a {torch.complex64} tensor [{lead}, {self.n_sc}, {self.n_sym}], got {g.dtype} {tuple(g.shape)}")
        if g.stride(2) != 1:
            raise ValueError(f"{name} must be in the fast layout [slot][port][symbol][subcarrier] (subcarrier stride 1: a permuted view of "
                             f"[B, R, n_sym, n_sc]), got strides {tuple(g.stride())}")
        if g.shape[0] == 0:
            return [0, 0, 0]
        return self._strides(name, g, (0, 1, 3), self.n_sc, 8)

    def _launch(self, payload, ps, grid, gs, start: int, n: int, factor: np.float32):
        B, R = int(grid.shape[0]), int(grid.shape[1])
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = getattr(self._lib, self._ENTRY)(_lib.CE_ABI_VERSION, C.c_void_p(payload.data_ptr()), *ps, C.c_void_p(grid.data_ptr() + 8 * 12 * start), *gs,
                                                 B, R, self.n_sym, n, self._code, self.iq_width, float(factor), C.c_void_p(stream))
        if rc != 0:
            _stage.raise_for(rc)


class PuschFronthaulDecompressor(_Fronthaul):
    """Payload rows -> grid rows.  ``n_prb_grid`` (1..341) PRBs per symbol of the grid, ``n_sym`` symbols, ``method`` ``"bfp"`` or
    ``"none"``, ``iq_width`` 1..16 (``"none"`` is 16 bits), ``scale`` a float32 in 2^-96 .. 2^96; validated on construction."""

    _NOUN, _ENTRY = "the fronthaul decompressor", "ce_fh_decompress"

    def __call__(self, payload: torch.Tensor, start_prb: int = 0, n_prb: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``received_rg[B, R, n_sc, n_sym]`` complex64 in the fast layout, on the current stream.

        ``payload``   uint8 ``[B, R, n_sym, >= row_bytes(n_prb)]``, the last dimension contiguous and possibly longer than a row;
                      the first byte and the slot, port and symbol strides multiples of 4 bytes.
        ``start_prb``, ``n_prb``   the section the rows carry: the PRBs ``start_prb .. start_prb + n_prb - 1`` of the grid (by
                      default from ``start_prb`` to the end of the grid).
        ``out``       complex64 ``[B, R, n_sc, n_sym]`` with subcarrier stride 1 and free slot, port and symbol strides, as long
                      as no two rows share an RE; only the section's REs are written, every other keeps its value.  Without
                      it: a zero-filled grid with the section written into it."""
        self._bind()
        start, n = self._section(start_prb, n_prb)
        nb = self.row_bytes(n)
        if out is None:
            ps = self._check_payload("payload", payload, nb)
            B, R = int(payload.shape[0]), int(payload.shape[1])
            out = torch.zeros((B, R, self.n_sym, self.n_sc), dtype=torch.complex64, device=self.device).permute(0, 1, 3, 2)
            gs = self._check_grid("out", out, B, R)
        else:
            gs = self._check_grid("out", out)
            ps = self._check_payload("payload", payload, nb, int(out.shape[0]), int(out.shape[1]))
        if out.shape[0]:
            self._launch(payload, ps, out, gs, start, n, self.scale)
        return out


class PuschFronthaulCompressor(_Fronthaul):
    """Grid rows -> payload rows: an RU emulator, or a downlink path.  The arguments are the decompressor's."""

    _NOUN, _ENTRY = "the fronthaul compressor", "ce_fh_compress"

    @classmethod
    def for_decompressor(cls, fh: PuschFronthaulDecompressor, device=None) -> "PuschFronthaulCompressor":
        """The compressor of `fh`'s grid, format and scale, on `fh`'s device unless `device` names one."""
        return cls(fh.n_prb_grid, fh.n_sym, fh.method, fh.iq_width, float(fh.scale), device=fh._device_arg if device is None else device)

    def __call__(self, grid: torch.Tensor, start_prb: int = 0, n_prb: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 ``[B, R, n_sym, row_bytes(n_prb)]`` on the current stream.

        ``grid``      complex64 ``[B, R, n_sc, n_sym]`` in the fast layout (subcarrier stride 1); only the section's REs are read.
        ``out``       uint8 ``[B, R, n_sym, >= row_bytes(n_prb)]``, the last dimension contiguous, the first byte and the slot,
                      port and symbol strides multiples of 4 bytes, no two rows sharing a byte; only ``[0, row_bytes)`` of each
                      row is written and returned."""
        self._bind()
        start, n = self._section(start_prb, n_prb)
        nb = self.row_bytes(n)
        gs = self._check_grid("grid", grid)
        B, R = int(grid.shape[0]), int(grid.shape[1])
        if out is None:
            out = torch.empty((B, R, self.n_sym, (nb + 3) // 4 * 4), dtype=torch.uint8, device=self.device)
        ps = self._check_payload("out", out, nb, B, R)
        if B:
            self._launch(out, ps, grid, gs, start, n, self.inv_scale)
        return out[..., :nb]
