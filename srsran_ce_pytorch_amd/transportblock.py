"""Transport-block assembly EXTENSION (include/ce_tb.h; the reference stops at the channel estimate): the LDPC decoder's
packed code blocks checked against CRC24B, their payloads spliced at bit granularity into the transport block, and the
residue of its CRC24A / CRC16 (TS 38.212 5.1 and 5.2.2 inverted), on the current stream.

    rm = PuschRateRecovery(bg, tbs, "16qam", n_layers, n_bits)
    dec = PuschLdpcDecoder.for_rate_recovery(rm, graph)
    asm = PuschTransportBlock.for_rate_recovery(rm)
    hard, _ = dec(rm(llr, rv=0))
    tb, tb_status, cb_status = asm(hard)          # tb[B, tb_row_bytes] uint8, tb_status[B, 2], cb_status[B, C, 2] int32
    ack = tb_status[:, 0] == 0                    # the transport-block CRC held
    bits = unpack_bits(tb, tbs)                   # ldpc.unpack_bits: [B, tbs] of 0 / 1

The statuses hold CRC residues, not pass bits: ``cb_status[b, r] = {residue of block r, its share t_r of the
transport-block residue}``, ``tb_status[b] = {XOR of the t_r, number of blocks with a nonzero residue}``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _stage


def build_desc(base_graph: int, tbs: int, device_index: int = 0) -> _lib.TbDesc:
    """Fill a ``ce_tb_desc``.  Needs no GPU."""
    desc = _lib.TbDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.base_graph, desc.tbs = int(base_graph), int(tbs)
    return desc


def derive_host(base_graph: int, tbs: int) -> _lib.TbHostView:
    """Host-only view of everything a plan derives (``ce_tb_derive_host``); works without a GPU."""
    return _stage.derive_host("ce_tb_derive_host", build_desc(base_graph, tbs), _lib.TbHostView())


class PuschTransportBlock(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_tb_plan_create", "ce_tb_plan_destroy", "ce_tb_assemble"
    _NOUN = "transport-block assembly"

    def __init__(self, base_graph: int, tbs: int, device=None):
        super().__init__(device)
        self._args = (int(base_graph), int(tbs))
        view = derive_host(*self._args)
        self.base_graph, self.tbs = self._args
        self.c, self.k_prime, self.payload_bits = int(view.c), int(view.k_prime), int(view.p)
        self.in_row_bytes, self.tb_row_bytes = int(view.in_row_bytes), int(view.tb_row_bytes)
        self.l_tb, self.blocks_per_workgroup = int(view.l_tb), int(view.blocks_per_workgroup)

    @classmethod
    def for_rate_recovery(cls, rm) -> "PuschTransportBlock":
        """The assembly behind a ``PuschRateRecovery`` and its decoder: base graph, ``tbs`` and device are the rate recovery's."""
        return cls(rm.base_graph, rm.tbs, device=rm._device_arg)

    def _build_desc(self, device_index: int):
        return build_desc(*self._args, device_index=device_index)

    def _shape_text(self) -> str:
        one = f" or [slots, {self.in_row_bytes}]" if self.c == 1 else ""
        return f"hard must be a dense uint8 tensor [slots, {self.c}, {self.in_row_bytes}]{one}"

    def __call__(self, hard: torch.Tensor):
        """``(tb, tb_status, cb_status)`` on the current stream.  ``hard`` is the decoder's dense uint8
        ``[B, C, in_row_bytes]`` (``[B, in_row_bytes]`` is accepted when ``C = 1``); bits from ``K'`` on are ignored.
        ``tb[B, tb_row_bytes]`` uint8 holds bit i < tbs MSB first and zeros behind; ``tb_status[B, 2]`` and
        ``cb_status[B, C, 2]`` are int32."""
        if not isinstance(hard, torch.Tensor):
            raise ValueError(self._shape_text() + f", got {type(hard).__name__}")
        shape = tuple(hard.shape)
        ok = (hard.dim() == 3 and shape[1:] == (self.c, self.in_row_bytes)) or (self.c == 1 and hard.dim() == 2 and shape[1] == self.in_row_bytes)
        if hard.dtype != torch.uint8 or not ok or not hard.is_contiguous():
            raise ValueError(self._shape_text() + f", got {hard.dtype} {shape}" + ("" if hard.is_contiguous() else " (not contiguous)"))
        self._plan()
        dev = self.device
        if hard.device != dev:
            raise ValueError(f"hard must be a tensor on {dev}, got {hard.device}")
        B = shape[0]
        tb = torch.empty((B, self.tb_row_bytes), dtype=torch.uint8, device=dev)
        tb_status = torch.empty((B, 2), dtype=torch.int32, device=dev)
        cb_status = torch.empty((B, self.c, 2), dtype=torch.int32, device=dev)
        if B:
            _stage.check_aligned(("hard", hard), ("tb", tb), ("tb_status", tb_status), ("cb_status", cb_status))
            self._launch(C.c_void_p(hard.data_ptr()), B, C.c_void_p(tb.data_ptr()), C.c_void_p(tb_status.data_ptr()),
                         C.c_void_p(cb_status.data_ptr()))
        return tb, tb_status, cb_status
