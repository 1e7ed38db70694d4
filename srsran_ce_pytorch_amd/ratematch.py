"""LDPC rate-recovery EXTENSION (include/ce_rm.h; the reference stops at the channel estimate): the demapper's LLR row
split into code blocks, deinterleaved, placed in each block's circular buffer at the redundancy version's k0 around the
filler bits, with repetitions and the HARQ buffer of the earlier transmissions added (TS 38.212 5.4.2, 5.5), one launch on
the current stream.

    llr = PuschDemapper("16qam", n_symbols, out_dtype=torch.int8, llr_scale=8.0, descramble=True)(x_hat, nvar, rnti=rnti, n_id=n_id)
    rm = PuschRateRecovery(select_base_graph(tbs, rate), tbs, "16qam", n_layers, dem.n_bits)          # int8 by default
    soft = rm(llr, rv=0)                  # [B, C, N_cb]: one soft buffer per code block, fillers at +127
    soft = rm(llr2, rv=2, harq=soft, out=soft)   # a retransmission combined in place

The transport block size comes from the MCS and the allocation (TS 38.214 5.1.3.2) and is the caller's to state."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib, _stage
from .demod import modulation_order


def select_base_graph(tbs: int, rate: float) -> int:
    """LDPC base graph of TS 38.212 7.2.2 for a transport block of ``tbs`` bits at code rate ``rate``: 2 if
    ``tbs <= 292``, or ``tbs <= 3824 and rate <= 0.67``, or ``rate <= 0.25``; otherwise 1."""
    if tbs < 1 or not 0.0 < rate <= 1.0:
        raise ValueError(f"tbs={tbs} must be positive and rate={rate} in (0, 1]")
    return 2 if tbs <= 292 or (tbs <= 3824 and rate <= 0.67) or rate <= 0.25 else 1


def build_desc(base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, dtype=torch.int8, n_ref: int = 0,
               filler_llr: float = 127.0, device_index: int = 0) -> _lib.RmDesc:
    """Fill a ``ce_rm_desc``.  Needs no GPU."""
    if dtype not in (torch.float32, torch.int8):
        raise ValueError(f"dtype {dtype}: torch.float32 or torch.int8")
    desc = _lib.RmDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.base_graph, desc.tbs, desc.qm = int(base_graph), int(tbs), modulation_order(modulation)
    desc.n_layers, desc.g_bits, desc.n_ref = int(n_layers), int(n_bits), int(n_ref)
    desc.format = _lib.CE_RM_I8 if dtype == torch.int8 else _lib.CE_RM_F32
    desc.filler_llr = float(filler_llr)
    return desc


def derive_host(base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, dtype=torch.int8, n_ref: int = 0,
                filler_llr: float = 127.0) -> _lib.RmHostView:
    """Host-only view of everything a plan derives (``ce_rm_derive_host``); works without a GPU."""
    desc = build_desc(base_graph, tbs, modulation, n_layers, n_bits, dtype, n_ref, filler_llr)
    return _stage.derive_host("ce_rm_derive_host", desc, _lib.RmHostView())


class PuschRateRecovery(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_rm_plan_create", "ce_rm_plan_destroy", "ce_rm_recover"
    _NOUN = "rate recovery"

    def __init__(self, base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, dtype=torch.int8, n_ref: int = 0,
                 filler_llr: float = 127.0, device=None):
        super().__init__(device)
        self._args = (int(base_graph), int(tbs), modulation, int(n_layers), int(n_bits), dtype, int(n_ref), float(filler_llr))
        view = derive_host(*self._args)
        self.base_graph, self.tbs, self.qm, self.n_layers, self.n_bits = int(base_graph), int(tbs), modulation_order(modulation), int(n_layers), int(n_bits)
        self.dtype, self.n_ref, self.filler_llr = dtype, int(n_ref), float(filler_llr)
        self.n_code_blocks, self.n_cb, self.zc = int(view.c), int(view.n_cb), int(view.zc)
        self.e = [int(view.e_lo)] * int(view.n_lo) + [int(view.e_hi)] * (int(view.c) - int(view.n_lo))
        self.filler_range = (int(view.f0), int(view.f1))
        self.k0 = tuple(int(k) for k in view.k0)

    def _build_desc(self, device_index: int):
        return build_desc(*self._args, device_index=device_index)

    def __call__(self, llr: torch.Tensor, rv, harq: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``soft[B, C, N_cb]`` (the plan's dtype) on the current stream.  ``llr`` is the dense ``[B, n_bits]`` row of the
        demapper; ``rv`` a Python int 0..3 for the whole batch or an int32 device tensor of length ``B``; ``harq`` the
        buffer kept from the earlier transmissions (``None`` = all zero); ``out`` may pass the result tensor to be
        overwritten, and may be ``harq`` itself."""
        self._plan()
        dev = self.device
        if not isinstance(llr, torch.Tensor) or llr.device != dev:
            raise ValueError(f"llr must be a tensor on {dev}")
        if llr.dtype != self.dtype or llr.dim() != 2 or llr.shape[1] != self.n_bits or not llr.is_contiguous():
            raise ValueError(f"llr must be a dense {self.dtype} tensor [slots, {self.n_bits}], got {llr.dtype} {tuple(llr.shape)}")
        B = llr.shape[0]
        shape = (B, self.n_code_blocks, self.n_cb)
        if harq is not None:
            _stage.check_dense("harq", harq, self.dtype, shape, dev)
        if out is None:
            out = torch.empty(shape, dtype=self.dtype, device=dev)
        else:
            _stage.check_dense("out", out, self.dtype, shape, dev)
        rv_t = _stage.batch_param("rv", rv, B, dev, 0, 3, "an int 0..3")   # (the kernel uses ``rv & 3`` of a device tensor)
        if B == 0:
            return out                                           # empty batch: nothing to launch
        _stage.check_aligned(("llr", llr), ("harq", harq), ("out", out))
        self._launch(C.c_void_p(llr.data_ptr()), C.c_void_p(rv_t.data_ptr()), _stage.batch_stride(rv_t), B,
                     C.c_void_p(harq.data_ptr()) if harq is not None else None, C.c_void_p(out.data_ptr()))
        return out
