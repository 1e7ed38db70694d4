"""Transform de-precoding EXTENSION (include/ce_tp.h; the reference stops at the channel estimate): the inverse of the
DFT-s-OFDM precoding of TS 38.211 6.3.1.4 between the equalizer and the demapper -- per data symbol an MMSE-weighted
inverse DFT of length M = 12 n_prbs of the equalizer's per-RE estimates, and the per-symbol noise variance the demapper
needs, one launch on the current stream.

    eq = PuschEqualizer(hop1, hop2, 1, n_prb_grid)                                   # one layer, no data on DM-RS symbols
    x_hat, nvar = eq(rx, ch_est, noise)                                              # [B, S * M, 1] each
    x, nvar = PuschTransformDeprecoder.for_equalizer(eq)(x_hat, nvar)                # [B, S * M] each
    llr = PuschDemapper("16qam", eq.n_data_re, descramble=True)(x, nvar, rnti=rnti, n_id=n_id)"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, _stage


def build_desc(n_prbs: int, n_symbols: int, device_index: int = 0) -> _lib.TpDesc:
    """Fill a ``ce_tp_desc``.  Needs no GPU."""
    desc = _lib.TpDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.n_prbs, desc.n_symbols = int(n_prbs), int(n_symbols)
    return desc


def derive_host(n_prbs: int, n_symbols: int) -> _lib.TpHostView:
    """Host-only view of what a plan holds (``ce_tp_derive_host``); works without a GPU."""
    return _stage.derive_host("ce_tp_derive_host", build_desc(n_prbs, n_symbols), _lib.TpHostView())


def twiddles(n_prbs: int, n_symbols: int = 1) -> np.ndarray:
    """complex64 ``[M]``: the plan's table ``W[n] = exp(+j 2 pi n / M)`` (``ce_tp_copy_twiddles``, host only)."""
    view = derive_host(n_prbs, n_symbols)
    w = np.zeros(view.m_sc, np.complex64)
    rc = _lib.load().ce_tp_copy_twiddles(C.byref(build_desc(n_prbs, n_symbols)), C.c_void_p(w.ctypes.data))
    if rc != 0:
        _stage.raise_for(rc)
    return w


def _copy_geometry(stage, view) -> None:
    """The launch geometry a row-transform stage shows as attributes, from its host view."""
    stage.radix = tuple(int(r) for r in view.radix[:view.n_passes])
    stage.rows_per_workgroup, stage.threads_per_row = int(view.rows_per_workgroup), int(view.threads_per_row)


def _data_symbols(view, n_sym: int) -> list:
    """The symbols with data of an equalizer's or a modulator's host view; ``ValueError`` unless each has it on all 12 REs."""
    syms = [s for s in range(n_sym) if view.sym_hop[s] >= 0 and view.data_res_per_prb[s] != 0]
    for s in syms:
        if view.data_res_per_prb[s] != 12:
            raise ValueError(f"symbol {s} carries data on {view.data_res_per_prb[s]} of 12 REs per PRB: transform precoding "
                             "needs DM-RS symbols without data (reserved_re_mask = 0xFFF)")
    return syms


def _check_dense_rows(name: str, t, dtype, n: int, dev) -> None:
    """``ValueError`` unless ``t`` is a dense ``dtype`` tensor ``[slots, n]`` or ``[slots, n, 1]`` on ``dev``."""
    if not isinstance(t, torch.Tensor) or t.device != dev:
        raise ValueError(f"{name} must be a tensor on {dev}")
    if t.dtype != dtype or not t.is_contiguous() or t.dim() not in (2, 3) or tuple(t.shape[1:]) not in ((n,), (n, 1)):
        raise ValueError(f"{name} must be a dense {dtype} tensor [slots, {n}] or [slots, {n}, 1], got {t.dtype} {tuple(t.shape)}")


class PuschTransformDeprecoder(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_tp_plan_create", "ce_tp_plan_destroy", "ce_tp_deprecode"
    _NOUN = "the transform de-precoder"

    def __init__(self, n_prbs: int, n_symbols: int, device=None):
        super().__init__(device)
        self._args = (int(n_prbs), int(n_symbols))
        view = derive_host(*self._args)
        self.n_prbs, self.n_symbols, self.m_sc = int(n_prbs), int(n_symbols), int(view.m_sc)
        _copy_geometry(self, view)

    @classmethod
    def for_equalizer(cls, eq, device=None) -> "PuschTransformDeprecoder":
        """The de-precoder of a ``PuschEqualizer``'s output; ``ValueError`` unless the equalizer has one layer, every
        symbol with data has exactly ``12 n_prbs`` data REs (no data on DM-RS symbols) and both hops have equal
        ``n_prbs``."""
        if eq.n_layers != 1:
            raise ValueError(f"transform precoding is single-layer, the equalizer has {eq.n_layers} layers")
        widths = {int(eq._desc.hop[h].n_prbs) for h in range(eq._desc.n_hops)}
        if len(widths) != 1:
            raise ValueError(f"the hops have {sorted(widths)} PRBs: transform precoding needs one width")
        return cls(widths.pop(), len(_data_symbols(eq._view, eq.n_sym)), device=device if device is not None else eq._device_arg)

    def _build_desc(self, device_index: int):
        return build_desc(*self._args, device_index=device_index)

    def __call__(self, x_hat: torch.Tensor, nvar: torch.Tensor, out: Optional[torch.Tensor] = None,
                 nvar_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(x[B, S * M] complex64, nvar[B, S * M] float32)`` on the current stream.  ``x_hat`` (complex64) and ``nvar``
        (float32) are dense ``[B, S * M]`` or ``[B, S * M, 1]`` tensors, symbol ascending, subcarrier ascending, as the
        one-layer equalizer returns them.  ``out`` / ``nvar_out`` may pass the result tensors to be overwritten; ``out``
        may be ``x_hat`` and ``nvar_out`` may be ``nvar`` (viewed to 2-D), any other overlap is refused."""
        self._plan()
        dev = self.device
        n = self.n_symbols * self.m_sc
        _check_dense_rows("x_hat", x_hat, torch.complex64, n, dev)
        _check_dense_rows("nvar", nvar, torch.float32, n, dev)
        B = x_hat.shape[0]
        if nvar.shape[0] != B:
            raise ValueError(f"x_hat holds {B} slots, nvar {nvar.shape[0]}")
        shape = (B, n)
        if out is None:
            out = torch.empty(shape, dtype=torch.complex64, device=dev)
        else:
            _stage.check_dense("out", out, torch.complex64, shape, dev)
        if nvar_out is None:
            nvar_out = torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            _stage.check_dense("nvar_out", nvar_out, torch.float32, shape, dev)
        if B == 0:
            return out, nvar_out                                 # empty batch: nothing to launch
        _stage.check_aligned(("x_hat", x_hat), ("nvar", nvar), ("out", out), ("nvar_out", nvar_out))
        spans = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
                 for name, t in (("x_hat", x_hat), ("nvar", nvar), ("out", out), ("nvar_out", nvar_out))]
        for i, (na, a0, a1) in enumerate(spans):
            for nb, b0, b1 in spans[max(i + 1, 2):]:             # an input against an output, and the outputs against each other
                if a0 < b1 and b0 < a1 and not ((na, nb) in (("x_hat", "out"), ("nvar", "nvar_out")) and a0 == b0):
                    raise ValueError(f"{nb} overlaps {na}: only out = x_hat and nvar_out = nvar (the same memory) are in-place forms")
        self._launch(C.c_void_p(x_hat.data_ptr()), C.c_void_p(nvar.data_ptr()), B, C.c_void_p(out.data_ptr()),
                     C.c_void_p(nvar_out.data_ptr()))
        return out, nvar_out
