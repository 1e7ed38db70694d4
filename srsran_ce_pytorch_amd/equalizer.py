"""PUSCH equalizer EXTENSION (include/ce_eq.h; the reference stops at the channel estimate): a noise-whitened, unbiased
LMMSE equalizer over the data REs of a slot batch, one launch on the current stream.

`PuschEqualizer(hop1, hop2, n_layers, n_prb_grid, ...)` resolves the hop geometry `estimate()` takes into the list of data
REs; calling it with `rx`, `ch_est` and `noise` exactly as `estimate()` takes / returns them gives the per-layer symbol
estimates and their post-equalisation noise variances in the codeword's symbol order (TS 38.211 6.3.1.6 / 6.3.1.3):

    ch_est, noise, *_ = estimate(rx, pilots, beta, hop1, hop2, config)
    x_hat, nvar = PuschEqualizer(hop1, hop2, L, n_prb_grid)(rx, ch_est, noise)      # [B, n_data_re, L] each

`ch_est` is used as given: a data / DM-RS power offset (beta) is the caller's to fold in."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, _stage

CHUNK_SC = _lib.CE_EQ_CHUNK_SC      # subcarriers one workgroup of the kernel handles
MAX_PORTS = _lib.CE_EQ_MAX_PORTS


def build_desc(hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, *, reserved_re_mask: int = 0xFFF,
               device_index: int = 0):
    """Fill a ``ce_eq_desc`` from the duck-typed hop objects of ``estimate()`` (``DMRSsymbols``, ``PRBstart``, ``nPRBs``,
    ``startSymbol``, ``nAllocatedSymbols``; hop 2 empty or without a DM-RS symbol = one hop).  Needs no GPU."""
    if not 0 <= int(reserved_re_mask) <= 0xFFF:
        raise ValueError(f"reserved_re_mask=0x{int(reserved_re_mask):x} is not a 12-bit RE mask")
    hops = []
    for hop in (hop1, hop2):
        dm = hop.DMRSsymbols
        dm = dm.detach().cpu().numpy() if isinstance(dm, torch.Tensor) else np.asarray(dm)
        hops.append((dm.astype(bool).ravel(), hop))
    if hops[1][0].size == 0 or int(hops[1][0].sum()) == 0:
        hops.pop()
    desc = _lib.EqDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.n_prb_grid, desc.n_sym, desc.n_layers, desc.n_hops = int(n_prb_grid), int(n_sym), int(n_layers), len(hops)
    for hi, (dm, hop) in enumerate(hops):
        hd = desc.hop[hi]
        if 0 < n_sym <= _lib.CE_MAX_SYMBOLS:                   # (the library reports an n_sym outside that range)
            if dm.size != n_sym:
                raise ValueError(f"hop {hi + 1}: DMRSsymbols has {dm.size} entries, grid has {n_sym} symbols")
            for s in range(n_sym):
                hd.dmrs_symbols[s] = int(dm[s])
        hd.reserved_re_mask = int(reserved_re_mask)
        hd.prb_start, hd.n_prbs = int(hop.PRBstart), int(hop.nPRBs)
        hd.start_symbol, hd.n_alloc_symbols = int(hop.startSymbol), int(hop.nAllocatedSymbols)
    return desc


def derive_host(hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, *, reserved_re_mask: int = 0xFFF) -> _lib.EqHostView:
    """Host-only view of what a plan holds (``ce_eq_derive_host``); works without a GPU."""
    desc = build_desc(hop1, hop2, n_layers, n_prb_grid, n_sym, reserved_re_mask=reserved_re_mask)
    return _stage.derive_host("ce_eq_derive_host", desc, _lib.EqHostView())


class PuschEqualizer(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_eq_plan_create", "ce_eq_plan_destroy", "ce_eq_equalize"
    _NOUN = "the equalizer"

    def __init__(self, hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, reserved_re_mask: int = 0xFFF, device=None):
        super().__init__(device)
        self._geometry = (hop1, hop2, int(n_layers), int(n_prb_grid), int(n_sym))
        self._mask = int(reserved_re_mask)
        self._desc = build_desc(*self._geometry, reserved_re_mask=self._mask)
        self._view = derive_host(*self._geometry, reserved_re_mask=self._mask)
        self.n_data_re, self.n_layers = int(self._view.n_data_re), int(n_layers)
        self.n_sc, self.n_sym = 12 * int(n_prb_grid), int(n_sym)

    def data_re(self) -> np.ndarray:
        """``(n_data_re, 2)`` int array: the ``(sym, sc)`` of every output row, from the plan's host view."""
        v, out = self._view, np.empty((self.n_data_re, 2), np.int64)
        for s in range(self.n_sym):
            if v.sym_hop[s] < 0 or v.data_res_per_prb[s] == 0:
                continue
            hd = self._desc.hop[v.sym_hop[s]]
            for q in range(hd.prb_start, hd.prb_start + hd.n_prbs):
                for re in range(12):
                    if v.data_mask[s] >> re & 1:
                        row = v.first_row[s] + (q - hd.prb_start) * v.data_res_per_prb[s] + bin(v.data_mask[s] & ((1 << re) - 1)).count("1")
                        out[row] = (s, 12 * q + re)
        return out

    def _build_desc(self, device_index: int):
        return build_desc(*self._geometry, reserved_re_mask=self._mask, device_index=device_index)

    def __call__(self, rx: torch.Tensor, ch_est: torch.Tensor, noise: torch.Tensor,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(x_hat[B, n_data_re, L] complex64, nvar[B, n_data_re, L] float32)`` on the current stream.  ``rx`` is
        ``[B, R, n_sc, n_sym]`` complex64 with any non-negative strides, ``ch_est`` the dense ``[B, R, n_sc, n_sym, L]``
        complex64 tensor and ``noise`` the dense ``[B, R]`` float64 tensor ``estimate()`` returns; ``out`` may pass the
        two result tensors to be overwritten."""
        self._plan()
        dev = self.device
        for name, t in (("rx", rx), ("ch_est", ch_est), ("noise", noise)):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ValueError(f"{name} must be a tensor on {dev}")
        if rx.dim() != 4 or rx.dtype != torch.complex64:
            raise ValueError("rx must be a complex64 [slots, ports, n_sc, n_sym] tensor")
        B, R, n_sc, n_sym = rx.shape
        if (n_sc, n_sym) != (self.n_sc, self.n_sym):
            raise ValueError(f"grid is {n_sc}x{n_sym}, the equalizer expects {self.n_sc}x{self.n_sym}")
        if not 1 <= R <= MAX_PORTS:
            raise ValueError(f"{R} Rx ports: 1..{MAX_PORTS} are supported")
        if any(s < 0 for s in rx.stride()):
            raise ValueError("negative strides are not supported")
        L = self.n_layers
        if ch_est.dtype != torch.complex64 or tuple(ch_est.shape) != (B, R, n_sc, n_sym, L) or not ch_est.is_contiguous():
            raise ValueError(f"ch_est must be a dense complex64 tensor of shape {(B, R, n_sc, n_sym, L)}")
        if noise.dtype != torch.float64 or tuple(noise.shape) != (B, R) or not noise.is_contiguous():
            raise ValueError(f"noise must be a dense float64 tensor of shape {(B, R)}")
        shape = (B, self.n_data_re, L)
        if out is None:
            out = (torch.empty(shape, dtype=torch.complex64, device=dev), torch.empty(shape, dtype=torch.float32, device=dev))
        x_hat, nvar = out
        _stage.check_dense("out[0]", x_hat, torch.complex64, shape, dev)
        _stage.check_dense("out[1]", nvar, torch.float32, shape, dev)
        if B == 0:
            return x_hat, nvar                                   # empty batch: nothing to launch
        _stage.check_aligned(("ch_est", ch_est), ("out[0]", x_hat), ("out[1]", nvar))
        strides = (C.c_int64 * 4)(*[int(s) for s in rx.stride()])
        self._launch(C.c_void_p(rx.data_ptr()), strides, C.c_void_p(ch_est.data_ptr()), C.c_void_p(noise.data_ptr()), B, R,
                     C.c_void_p(x_hat.data_ptr()), C.c_void_p(nvar.data_ptr()))
        return x_hat, nvar
