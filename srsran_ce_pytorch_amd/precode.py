"""Transform precoding EXTENSION (include/ce_tp.h `ce_tp_precode`; the reference stops at the channel estimate): the
DFT-s-OFDM precoding of TS 38.211 6.3.1.4 behind the modulator -- per data symbol a DFT of length M = 12 n_prbs scaled by
1 / sqrt(M), what ``PuschTransformDeprecoder`` undoes on the receive side; one launch on the current stream, with the
de-precoder's plan.

    mod = PuschModulator(hop1, hop2, 1, n_prb_grid, "16qam")            # one layer, no data on DM-RS symbols
    tx = mod(g, pilots, beta_dmrs, rnti=rnti, n_id=n_id)                # [B, 1, n_sc, n_sym], CP-OFDM
    tx = PuschTransformPrecoder.for_modulator(mod).grid_(tx)            # the data symbols' allocated REs, in place

    y = PuschTransformPrecoder(n_prbs, n_symbols)(x)                    # dense rows: x, y [B, S * M]

Out of scope: the low-PAPR DM-RS sequences of 6.4.1.1.1.2 (Zadoff-Chu / table based; the pilots stay an input and
``PuschDmrs`` stays Gold based), pi/2-BPSK, and a transform fused into the modulator's kernel (its unit of work is a tile
of 256 subcarriers, a row transform needs the whole row)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib, _stage
from . import modulator as _mod
from .deprecode import _check_dense_rows, _copy_geometry, _data_symbols, build_desc, derive_host


class PuschTransformPrecoder(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_tp_plan_create", "ce_tp_plan_destroy", "ce_tp_precode"
    _NOUN = "the transform precoder"

    def __init__(self, n_prbs: int, n_symbols: int, device=None):
        super().__init__(device)
        self._args = (int(n_prbs), int(n_symbols))
        view = derive_host(*self._args)
        self.n_prbs, self.n_symbols, self.m_sc = int(n_prbs), int(n_symbols), int(view.m_sc)
        _copy_geometry(self, view)
        self.row_offsets, self.slot_stride, self._grid_shape = None, None, None      # set by for_modulator

    @classmethod
    def for_modulator(cls, mod, device=None) -> "PuschTransformPrecoder":
        """The precoder of a ``PuschModulator``'s grid: one row per symbol with data, at ``s n_sc + 12 prb_start`` of its
        hop, slot stride ``n_sym n_sc`` (``row_offsets``, ``slot_stride``).  ``ValueError`` unless the modulator has one
        layer, every symbol with data carries it on all 12 REs of a PRB (no data on DM-RS symbols) and ``n_prbs`` is of the
        form 2^a 3^b 5^c."""
        if not isinstance(mod, _mod.PuschModulator):
            raise ValueError(f"mod must be a PuschModulator, got {type(mod).__name__}")
        if mod.n_layers != 1:
            raise ValueError(f"transform precoding is single-layer, the modulator has {mod.n_layers} layers")
        desc, keep = _mod.build_desc(*mod._geometry, **mod._options)
        view = _stage.derive_host("ce_mod_derive_host", desc, _lib.ModHostView())
        n_prbs = int(desc.hop[0].n_prbs)                         # (the modulator refuses hops of unequal width)
        starts = [int(desc.hop[h].prb_start) for h in range(desc.n_hops)]
        del keep
        offsets = [s * mod.n_sc + 12 * starts[view.sym_hop[s]] for s in _data_symbols(view, mod.n_sym)]
        pre = cls(n_prbs, len(offsets), device=device if device is not None else mod._device_arg)
        pre.row_offsets, pre.slot_stride, pre._grid_shape = tuple(offsets), mod.n_sym * mod.n_sc, (mod.n_sc, mod.n_sym)
        return pre

    def _build_desc(self, device_index: int):
        return build_desc(*self._args, device_index=device_index)

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``y[B, S * M]`` complex64 on the current stream.  ``x`` is a dense complex64 ``[B, S * M]`` or ``[B, S * M, 1]``
        tensor, symbol ascending, subcarrier ascending (the modulation symbols of a one-layer slot).  ``out`` may pass the
        result tensor to be overwritten; it may be ``x`` (viewed to 2-D), any other overlap is refused."""
        self._plan()
        dev = self.device
        n = self.n_symbols * self.m_sc
        _check_dense_rows("x", x, torch.complex64, n, dev)
        B = x.shape[0]
        shape = (B, n)
        if out is None:
            out = torch.empty(shape, dtype=torch.complex64, device=dev)
        else:
            _stage.check_dense("out", out, torch.complex64, shape, dev)
        if B == 0:
            return out                                           # empty batch: nothing to launch
        _stage.check_aligned(("x", x), ("out", out))
        x0, o0, nbytes = x.data_ptr(), out.data_ptr(), 8 * B * n
        if x0 < o0 + nbytes and o0 < x0 + nbytes and x0 != o0:
            raise ValueError("out overlaps x: only out = x (the same memory) is the in-place form")
        self._launch(C.c_void_p(x0), n, None, C.c_void_p(o0), n, None, B)
        return out

    def grid_(self, tx: torch.Tensor) -> torch.Tensor:
        """Transform the data rows of a modulator's ``tx`` IN PLACE and return it.  ``tx`` is what ``PuschModulator`` returns:
        the permuted ``[B, 1, n_sc, n_sym]`` complex64 view of a dense ``[B, 1, n_sym, n_sc]`` buffer.  DM-RS symbols and
        every RE outside the allocation are not touched.  Needs an instance made by ``for_modulator``."""
        if self.row_offsets is None:
            raise ValueError("grid_ needs a precoder made by PuschTransformPrecoder.for_modulator")
        self._plan()
        dev = self.device
        n_sc, n_sym = self._grid_shape
        if not isinstance(tx, torch.Tensor) or tx.device != dev:
            raise ValueError(f"tx must be a tensor on {dev}")
        if (tx.dtype != torch.complex64 or tx.dim() != 4 or tuple(tx.shape[1:]) != (1, n_sc, n_sym)
                or not tx.permute(0, 1, 3, 2).is_contiguous()):
            raise ValueError(f"tx must be the modulator's {torch.complex64} tensor [slots, 1, {n_sc}, {n_sym}] (the permuted view of a dense "
                             f"[slots, 1, {n_sym}, {n_sc}] buffer), got {tx.dtype} {tuple(tx.shape)} with strides {tuple(tx.stride())}")
        B = tx.shape[0]
        if B == 0:
            return tx
        _stage.check_aligned(("tx", tx))
        off = (C.c_int32 * self.n_symbols)(*self.row_offsets)
        p = C.c_void_p(tx.data_ptr())
        self._launch(p, self.slot_stride, off, p, self.slot_stride, off, B)
        return tx
