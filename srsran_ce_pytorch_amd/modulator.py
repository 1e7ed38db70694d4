"""PUSCH modulator EXTENSION (include/ce_mod.h; the reference stops at the channel estimate): the forward counterpart of
``PuschDemapper`` and of the equalizer's data-RE walk in one stage -- scrambling, QAM and layer mapping, RE mapping and DM-RS
insertion (TS 38.211 6.3.1.1 - 6.3.1.3, 6.3.1.6, 6.4.1.1.3; transform precoding, 6.3.1.4, is ``PuschTransformPrecoder`` on
the grid this stage returns), one launch on the current stream.

    eq = PuschEqualizer(hop1, hop2, L, n_prb_grid, reserved_re_mask=0x555)
    mod = PuschModulator.for_equalizer(eq, "16qam", scramble=True)        # same geometry, mask and device
    g = enc(tb, rv=0)                                                     # PuschTransportEncoder: uint8 [B, g_row_bytes]
    pilots = PuschDmrs(hop1, hop2, L, n_prb_grid)(slot, n_id, n_scid)     # [B, n_re, n_dmrs_total, L]
    tx = mod(g, pilots, beta_dmrs, rnti=rnti, n_id=n_id)                  # [B, L, n_sc, n_sym], subcarrier-contiguous

Every value of ``tx`` is one float32 multiply or +0, so the result is defined to the bit (tests/mod_oracle.py).  Precoding is
the identity: layer l is antenna port l."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib, _stage
from . import equalizer as _eq
from .demod import _RANGES, modulation_order


def build_desc(hop1, hop2, n_layers: int, n_prb_grid: int, modulation, n_sym: int = 14, *, reserved_re_mask: int = 0xFFF,
               scramble: bool = True, device_index: int = 0):
    """Fill a ``ce_mod_desc`` from the duck-typed hop objects ``PuschEqualizer`` and ``PuschDmrs`` take (``DMRSsymbols``,
    ``DMRSREmask``, ``maskPRBs``, ``PRBstart``, ``nPRBs``, ``startSymbol``, ``nAllocatedSymbols``; hop 2 empty or without a
    DM-RS symbol = one hop).  Returns ``(desc, keepalive)``; needs no GPU."""
    eq = _eq.build_desc(hop1, hop2, n_layers, n_prb_grid, n_sym, reserved_re_mask=reserved_re_mask)   # its checks, its texts
    n_cdm = (int(n_layers) + 1) // 2
    desc = _lib.ModDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.n_prb_grid, desc.n_sym, desc.n_layers, desc.n_hops = int(n_prb_grid), int(n_sym), int(n_layers), eq.n_hops
    desc.qm, desc.scramble = modulation_order(modulation), int(bool(scramble))
    keep = []
    for hi, hop in enumerate((hop1, hop2)[:eq.n_hops]):
        hd, eh = desc.hop[hi], eq.hop[hi]
        for s in range(_lib.CE_MAX_SYMBOLS):
            hd.dmrs_symbols[s] = eh.dmrs_symbols[s]
        hd.reserved_re_mask, hd.prb_start, hd.n_prbs = eh.reserved_re_mask, eh.prb_start, eh.n_prbs
        hd.start_symbol, hd.n_alloc_symbols = eh.start_symbol, eh.n_alloc_symbols
        rm, mp = hop.DMRSREmask, hop.maskPRBs
        if isinstance(rm, torch.Tensor):
            rm, mp = rm.detach().cpu().numpy(), mp.detach().cpu().numpy()
        rm, mp = np.asarray(rm).astype(bool), np.asarray(mp).astype(bool).ravel()
        if rm.ndim != 2 or rm.shape[0] != 12 or rm.shape[1] < min(n_cdm, _lib.CE_MAX_CDM):
            raise ValueError(f"hop {hi + 1}: DMRSREmask must be (12, >= {n_cdm}), got {rm.shape}")
        if mp.size != n_prb_grid:
            raise ValueError(f"hop {hi + 1}: maskPRBs has {mp.size} entries, grid has {n_prb_grid} PRBs")
        for c in range(min(n_cdm, _lib.CE_MAX_CDM)):
            hd.re_mask[c] = int(sum(1 << r for r in range(12) if rm[r, c]))
        buf = (C.c_uint8 * max(1, mp.size)).from_buffer_copy(np.ascontiguousarray(mp, np.uint8).tobytes() or b"\0")
        keep.append(buf)
        hd.mask_prbs = C.cast(buf, C.POINTER(C.c_uint8))
    return desc, keep


def derive_host(hop1, hop2, n_layers: int, n_prb_grid: int, modulation, n_sym: int = 14, *, reserved_re_mask: int = 0xFFF,
                scramble: bool = True) -> _lib.ModHostView:
    """Host-only view of what a plan derives (``ce_mod_derive_host``); works without a GPU."""
    desc, keep = build_desc(hop1, hop2, n_layers, n_prb_grid, modulation, n_sym, reserved_re_mask=reserved_re_mask, scramble=scramble)
    view = _stage.derive_host("ce_mod_derive_host", desc, _lib.ModHostView())
    del keep
    return view


class PuschModulator(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_mod_plan_create", "ce_mod_plan_destroy", "ce_mod_modulate"
    _NOUN = "the modulator"

    def __init__(self, hop1, hop2, n_layers: int, n_prb_grid: int, modulation, n_sym: int = 14, reserved_re_mask: int = 0xFFF,
                 scramble: bool = True, device=None):
        super().__init__(device)
        self._geometry = (hop1, hop2, int(n_layers), int(n_prb_grid), modulation, int(n_sym))
        self._options = dict(reserved_re_mask=int(reserved_re_mask), scramble=bool(scramble))
        view = derive_host(*self._geometry, **self._options)
        self.qm, self.n_layers, self.scramble = modulation_order(modulation), int(n_layers), bool(scramble)
        self.n_sc, self.n_sym = 12 * int(n_prb_grid), int(n_sym)
        self.n_bits, self.n_symbols, self.n_data_re, self.g_row_bytes = int(view.n_bits), int(view.n_symbols), int(view.n_data_re), int(view.g_row_bytes)
        self.n_re, self.n_dmrs_total = int(view.n_re), int(view.n_dmrs_total)

    @classmethod
    def for_equalizer(cls, eq, modulation, scramble: bool = True) -> "PuschModulator":
        """The modulator whose data REs a ``PuschEqualizer`` takes back apart: hops, layers, grid, ``reserved_re_mask`` and
        device are the equalizer's."""
        if not isinstance(eq, _eq.PuschEqualizer):
            raise ValueError(f"eq must be a PuschEqualizer, got {type(eq).__name__}")
        hop1, hop2, n_layers, n_prb_grid, n_sym = eq._geometry
        return cls(hop1, hop2, n_layers, n_prb_grid, modulation, n_sym=n_sym, reserved_re_mask=eq._mask, scramble=scramble, device=eq._device_arg)

    def _build_desc(self, device_index: int):
        desc, keep = build_desc(*self._geometry, device_index=device_index, **self._options)
        desc.keepalive = keep                                    # the PRB masks it points to live as long as the descriptor
        return desc

    def __call__(self, g: torch.Tensor, pilots: torch.Tensor, beta_dmrs: float = 1.0, rnti=None, n_id=None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``tx[B, L, n_sc, n_sym]`` complex64 on the current stream: the permuted view of the dense ``[B, L, n_sym, n_sc]``
        buffer the kernel writes (every element, so ``out`` -- that dense buffer -- need not be cleared).  ``g`` is the dense
        uint8 ``[B, g_row_bytes]`` row of ``PuschTransportEncoder`` (bit i < n_bits MSB first; bits behind are ignored);
        ``pilots`` the dense complex64 ``[B, n_re, n_dmrs_total, L]`` tensor of ``PuschDmrs``, or ``[n_re, n_dmrs_total, L]``
        for the whole batch; ``beta_dmrs`` a finite float; ``rnti`` / ``n_id`` (needed with ``scramble=True``) Python ints
        for the whole batch or int32 device tensors of length ``B``."""
        text = f"g must be a dense uint8 tensor [slots, {self.g_row_bytes}]"
        if not isinstance(g, torch.Tensor):
            raise ValueError(text + f", got {type(g).__name__}")
        if g.dtype != torch.uint8 or g.dim() != 2 or g.shape[1] != self.g_row_bytes or not g.is_contiguous():
            raise ValueError(text + f", got {g.dtype} {tuple(g.shape)}" + ("" if g.is_contiguous() else " (not contiguous)"))
        self._plan()
        dev = self.device
        if g.device != dev:
            raise ValueError(f"g must be a tensor on {dev}, got {g.device}")
        B, L = g.shape[0], self.n_layers
        per_slot = (self.n_re, self.n_dmrs_total, L)
        text = f"pilots must be a dense complex64 tensor {list(per_slot)} or {[B, *per_slot]}"
        if not isinstance(pilots, torch.Tensor):
            raise ValueError(text + f", got {type(pilots).__name__}")
        if pilots.dtype != torch.complex64 or tuple(pilots.shape) not in (per_slot, (B, *per_slot)) or not pilots.is_contiguous():
            raise ValueError(text + f", got {pilots.dtype} {tuple(pilots.shape)}" + ("" if pilots.is_contiguous() else " (not contiguous)"))
        if pilots.device != dev:
            raise ValueError(f"pilots must be a tensor on {dev}, got {pilots.device}")
        if (isinstance(beta_dmrs, bool) or not isinstance(beta_dmrs, (int, float, np.integer, np.floating))
                or not abs(float(beta_dmrs)) <= float(np.finfo(np.float32).max)):      # (false for a NaN too)
            raise ValueError(f"beta_dmrs={beta_dmrs!r} must be a finite float32 value")
        if self.scramble and (rnti is None or n_id is None):
            raise ValueError("scramble=True needs rnti and n_id")
        shape = (B, L, self.n_sym, self.n_sc)
        if out is None:
            out = torch.empty(shape, dtype=torch.complex64, device=dev)
        else:
            _stage.check_dense("out", out, torch.complex64, shape, dev, "complex64")
        params = [_stage.batch_param(n, v, B, dev, *_RANGES[n]) for n, v in (("rnti", rnti), ("n_id", n_id))] if self.scramble else []
        if B:
            _stage.check_aligned(("g", g), ("out", out))
            strides = (C.c_int64 * 2)(*[_stage.batch_stride(p) for p in params]) if params else None
            ptrs = [C.c_void_p(p.data_ptr()) for p in params] if params else [None, None]
            pil_stride = math.prod(per_slot) if pilots.dim() == 4 else 0
            self._launch(C.c_void_p(g.data_ptr()), C.c_void_p(pilots.data_ptr()) if pilots.numel() else None, pil_stride,
                         C.c_float(float(beta_dmrs)), *ptrs, strides, B, C.c_void_p(out.data_ptr()))
        return out.permute(0, 1, 3, 2)
