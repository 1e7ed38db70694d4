"""Soft demapper EXTENSION (include/ce_demod.h; the reference stops at the channel estimate): exact max-log LLRs of the
equalizer's symbol estimates in codeword order, with the PUSCH scrambling of TS 38.211 6.3.1.1 undone, one launch on the
current stream.

    x_hat, nvar = PuschEqualizer(hop1, hop2, L, n_prb_grid)(rx, ch_est, noise)      # [B, n_data_re, L] each
    dem = PuschDemapper("16qam", eq.n_data_re * L, out_dtype=torch.int8, llr_scale=8.0, descramble=True)
    llr = dem(x_hat, nvar, rnti=rnti, n_id=n_id)                                    # [B, n_data_re * L * 4]

An LLR is positive where bit 0 is likelier; `llr < 0` is the hard decision."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib, _stage

MODULATIONS = {"qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8}
MAX_BITS = _lib.CE_DEMOD_MAX_BITS
_RANGES = {"rnti": (0, 65535), "n_id": (0, 1023)}


def modulation_order(modulation) -> int:
    """``"qpsk" | "16qam" | "64qam" | "256qam"`` or Qm itself -> Qm (the library reports an unsupported order)."""
    if isinstance(modulation, str):
        if modulation.lower() not in MODULATIONS:
            raise ValueError(f"modulation {modulation!r}: expected one of {sorted(MODULATIONS)} or Qm")
        return MODULATIONS[modulation.lower()]
    return int(modulation)


def build_desc(modulation, n_symbols: int, out_dtype=torch.float32, llr_scale: float = 1.0, descramble: bool = False,
               device_index: int = 0) -> _lib.DemodDesc:
    """Fill a ``ce_demod_desc``.  Needs no GPU."""
    if out_dtype not in (torch.float32, torch.int8):
        raise ValueError(f"out_dtype {out_dtype}: torch.float32 or torch.int8")
    desc = _lib.DemodDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.qm, desc.n_symbols = modulation_order(modulation), int(n_symbols)
    desc.out_format = _lib.CE_DEMOD_OUT_I8 if out_dtype == torch.int8 else _lib.CE_DEMOD_OUT_F32
    desc.descramble, desc.llr_scale = int(bool(descramble)), float(llr_scale)
    return desc


def derive_host(modulation, n_symbols: int, out_dtype=torch.float32, llr_scale: float = 1.0, descramble: bool = False) -> _lib.DemodHostView:
    """Host-only view of what a plan holds (``ce_demod_derive_host``); works without a GPU."""
    desc = build_desc(modulation, n_symbols, out_dtype, llr_scale, descramble)
    return _stage.derive_host("ce_demod_derive_host", desc, _lib.DemodHostView())


def gold_tables(modulation, n_symbols: int):
    """``(x1[n_words], jump[n_blocks, 31])`` uint32 arrays of a descrambling plan (``ce_demod_copy_tables``, host only):
    word ``8 blk + k`` of c is ``x1[8 blk + k]`` XOR the k-th word stepped from the x2 state
    ``XOR_{i in bits(c_init)} jump[blk, i]``."""
    lib = _lib.load()
    view = derive_host(modulation, n_symbols, descramble=True)
    desc = build_desc(modulation, n_symbols, descramble=True)
    x1 = np.zeros(view.n_words, np.uint32)
    jump = np.zeros((view.n_blocks, 31), np.uint32)
    rc = lib.ce_demod_copy_tables(C.byref(desc), C.c_void_p(x1.ctypes.data), C.c_void_p(jump.ctypes.data))
    if rc != 0:
        _stage.raise_for(rc)
    return x1, jump


class PuschDemapper(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_demod_plan_create", "ce_demod_plan_destroy", "ce_demod_demap"
    _NOUN = "the demapper"

    def __init__(self, modulation, n_symbols: int, out_dtype=torch.float32, llr_scale: float = 1.0, descramble: bool = False,
                 device=None):
        super().__init__(device)
        self._args = (modulation, int(n_symbols), out_dtype, float(llr_scale), bool(descramble))
        view = derive_host(*self._args)
        self.qm, self.n_symbols, self.n_bits = modulation_order(modulation), int(n_symbols), int(view.n_bits)
        self.out_dtype, self.llr_scale, self.descramble = out_dtype, float(llr_scale), bool(descramble)

    def _build_desc(self, device_index: int):
        return build_desc(*self._args, device_index=device_index)

    def __call__(self, x_hat: torch.Tensor, nvar: torch.Tensor, rnti=None, n_id=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``llr[B, n_symbols * Qm]`` (float32 or int8) on the current stream.  ``x_hat`` (complex64) and ``nvar``
        (float32) are dense ``[B, ...]`` tensors of ``n_symbols`` elements per slot, e.g. exactly as the equalizer
        returns them; ``rnti`` / ``n_id`` (needed with ``descramble=True``) are Python ints for the whole batch or int32
        device tensors of length ``B``; ``out`` may pass the result tensor to be overwritten."""
        self._plan()
        dev = self.device
        for name, t, dt in (("x_hat", x_hat, torch.complex64), ("nvar", nvar, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ValueError(f"{name} must be a tensor on {dev}")
            if t.dtype != dt or t.dim() < 1 or not t.is_contiguous():
                raise ValueError(f"{name} must be a dense {dt} tensor [slots, ...]")
        B = x_hat.shape[0]
        if math.prod(x_hat.shape[1:]) != self.n_symbols or tuple(nvar.shape) != tuple(x_hat.shape):
            raise ValueError(f"x_hat {tuple(x_hat.shape)} / nvar {tuple(nvar.shape)}: both must hold {self.n_symbols} symbols per slot")
        if self.descramble and (rnti is None or n_id is None):
            raise ValueError("descramble=True needs rnti and n_id")
        shape = (B, self.n_bits)
        if out is None:
            out = torch.empty(shape, dtype=self.out_dtype, device=dev)
        else:
            _stage.check_dense("out", out, self.out_dtype, shape, dev)
        params = [_stage.batch_param(n, v, B, dev, *_RANGES[n]) for n, v in (("rnti", rnti), ("n_id", n_id))] if self.descramble else []
        if B == 0:
            return out                                           # empty batch: nothing to launch
        _stage.check_aligned(("x_hat", x_hat), ("nvar", nvar), ("out", out))
        strides = (C.c_int64 * 2)(*[_stage.batch_stride(p) for p in params]) if params else None
        ptrs = [C.c_void_p(p.data_ptr()) for p in params] if params else [None, None]
        self._launch(C.c_void_p(x_hat.data_ptr()), C.c_void_p(nvar.data_ptr()), *ptrs, strides, B, C.c_void_p(out.data_ptr()))
        return out
