"""PUSCH DM-RS generation EXTENSION (include/ce_dmrs.h; the reference takes `pilots` as an input and has no generator).

`PuschDmrs(hop1, hop2, n_layers, n_prb_grid, ...)` resolves the hop geometry `estimate()` takes into jump tables on the
GPU; calling it with per-slot `(slot, n_id, n_scid)` writes `pilots[B, n_re, n_dmrs_total, L]` in the layout
`estimate()` consumes, one launch on the current stream:

    pilots = PuschDmrs(hop1, hop2, L, n_prb_grid)(slot, n_id, n_scid)
    estimate(rx, pilots, beta, hop1, hop2, config)

TS 38.211 5.2.1 / 6.4.1.1.1.1 (Rel-15 form, transform precoding off, antenna ports 0-3)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib, _stage

_RANGES = {"slot": (0, 2 ** 31 - 1), "n_id": (0, 65535), "n_scid": (0, 1)}


def build_desc(hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, *, grid_start_crb: int = 0,
               n_symb_slot: int = 14, device_index: int = 0):
    """Fill a ``ce_dmrs_desc`` from the duck-typed hop objects of ``estimate()`` (``DMRSsymbols``, ``DMRSREmask``,
    ``maskPRBs``; hop 2 empty or without a DM-RS symbol = one hop).  Returns ``(desc, keepalive)``; needs no GPU."""
    n_cdm = (int(n_layers) + 1) // 2
    hops = []
    for hop in (hop1, hop2):
        if isinstance(hop.DMRSsymbols, torch.Tensor):
            dm, rm, mp = (x.detach().cpu().numpy() for x in (hop.DMRSsymbols, hop.DMRSREmask, hop.maskPRBs))
        else:
            dm, rm, mp = hop.DMRSsymbols, hop.DMRSREmask, hop.maskPRBs
        hops.append((np.asarray(dm).astype(bool).ravel(), np.asarray(rm).astype(bool), np.asarray(mp).astype(bool).ravel()))
    if hops[1][0].size == 0 or int(hops[1][0].sum()) == 0:
        hops.pop()
    desc = _lib.DmrsDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.n_prb_grid, desc.grid_start_crb, desc.n_sym = int(n_prb_grid), int(grid_start_crb), int(n_sym)
    desc.n_symb_slot, desc.n_layers, desc.n_hops = int(n_symb_slot), int(n_layers), len(hops)
    keep = []
    for hi, (dm, rm, mp) in enumerate(hops):
        hd = desc.hop[hi]
        if dm.size != n_sym or n_sym > _lib.CE_MAX_SYMBOLS:
            raise ValueError(f"hop {hi + 1}: DMRSsymbols has {dm.size} entries, grid has {n_sym} symbols (<= {_lib.CE_MAX_SYMBOLS})")
        if rm.ndim != 2 or rm.shape[0] != 12 or rm.shape[1] < min(n_cdm, _lib.CE_MAX_CDM):
            raise ValueError(f"hop {hi + 1}: DMRSREmask must be (12, >= {n_cdm}), got {rm.shape}")
        if mp.size != n_prb_grid:
            raise ValueError(f"hop {hi + 1}: maskPRBs has {mp.size} entries, grid has {n_prb_grid} PRBs")
        for s in range(n_sym):
            hd.dmrs_symbols[s] = int(dm[s])
        for c in range(min(n_cdm, _lib.CE_MAX_CDM)):
            hd.re_mask[c] = int(sum(1 << r for r in range(12) if rm[r, c]))
        buf = (C.c_uint8 * max(1, mp.size)).from_buffer_copy(np.ascontiguousarray(mp, np.uint8).tobytes() or b"\0")
        keep.append(buf)
        hd.mask_prbs = C.cast(buf, C.POINTER(C.c_uint8))
    return desc, keep


def derive_host(hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, *, grid_start_crb: int = 0,
                n_symb_slot: int = 14) -> _lib.DmrsHostView:
    """Host-only view of what a plan holds (``ce_dmrs_derive_host``: jump tables, pilot lists); works without a GPU."""
    desc, keep = build_desc(hop1, hop2, n_layers, n_prb_grid, n_sym, grid_start_crb=grid_start_crb, n_symb_slot=n_symb_slot)
    view = _stage.derive_host("ce_dmrs_derive_host", desc, _lib.DmrsHostView())
    del keep
    return view


class PuschDmrs(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_dmrs_plan_create", "ce_dmrs_plan_destroy", "ce_dmrs_generate"
    _NOUN = "the DM-RS generator"

    def __init__(self, hop1, hop2, n_layers: int, n_prb_grid: int, n_sym: int = 14, *, grid_start_crb: int = 0,
                 n_symb_slot: int = 14, device=None):
        super().__init__(device)
        self._geometry = (hop1, hop2, int(n_layers), int(n_prb_grid), int(n_sym))
        self._options = dict(grid_start_crb=int(grid_start_crb), n_symb_slot=int(n_symb_slot))
        view = derive_host(*self._geometry, **self._options)
        self.n_re, self.n_dmrs_total, self.n_layers = int(view.n_re), int(view.n_dmrs_total), int(n_layers)

    def _build_desc(self, device_index: int):
        desc, keep = build_desc(*self._geometry, device_index=device_index, **self._options)
        desc.keepalive = keep                                    # the PRB masks it points to live as long as the descriptor
        return desc

    def _param(self, name: str, value):
        """-> (value, length or None for a scalar); host values are range-checked here, device tensors taken as they are."""
        if isinstance(value, torch.Tensor) and value.device.type == "cuda":
            if value.dtype != torch.int32 or value.dim() != 1:
                raise ValueError(f"{name}: a device tensor must be int32 of shape [B], got {value.dtype} {tuple(value.shape)}")
            return value, value.shape[0]
        lo, hi = _RANGES[name]
        a = value.numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        if a.dtype.kind not in "iu" or a.ndim > 1:
            raise ValueError(f"{name}: expected an int or a 1-D integer array, got {a.dtype} with {a.ndim} axes")
        if a.size and (int(a.min()) < lo or int(a.max()) > hi):
            raise ValueError(f"{name} outside {lo}..{hi}")
        return a.astype(np.int32), (None if a.ndim == 0 else a.shape[0])

    def __call__(self, slot, n_id, n_scid, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pilots[B, n_re, n_dmrs_total, L]`` complex64 on the current stream.  Each parameter is an int or an int32
        ``[B]`` tensor on the device (CPU tensors / numpy arrays are range-checked and moved); ``B`` is the longest
        parameter's length (1 when all are ints), length-1 parameters and ints hold for the whole batch."""
        params = [self._param(n, v) for n, v in (("slot", slot), ("n_id", n_id), ("n_scid", n_scid))]
        lens = [n for _, n in params if n is not None]
        B = max(lens) if lens else 1
        if any(n not in (1, B) for n in lens):
            raise ValueError(f"parameter lengths {lens} do not broadcast to one batch")
        self._plan()
        dev = self.device
        shape = (B, self.n_re, self.n_dmrs_total, self.n_layers)
        if out is None:
            out = torch.empty(shape, dtype=torch.complex64, device=dev)
        else:
            _stage.check_dense("out", out, torch.complex64, shape, dev, "complex64")
        if B == 0:
            return out                                           # empty batch: nothing to launch
        ptrs, strides = [], (C.c_int64 * 3)()
        for i, (v, n) in enumerate(params):
            if not isinstance(v, torch.Tensor):
                v = torch.from_numpy(np.atleast_1d(v)).to(dev)   # on the current stream, like the launch that reads it
            elif v.device != dev:
                raise ValueError(f"parameter tensors must live on {dev}")
            if v.stride(0) < 0:
                raise ValueError("negative strides are not supported")
            params[i] = (v, n)                                   # alive until the launch is enqueued (stream-ordered allocator)
            ptrs.append(C.c_void_p(v.data_ptr()))
            strides[i] = _stage.batch_stride(v)
        self._launch(*ptrs, strides, B, C.c_void_p(out.data_ptr()))
        return out
