"""Transport-block encoder EXTENSION (include/ce_enc.h; the reference stops at the channel estimate): the forward counterpart
of ``PuschRateRecovery``, ``PuschLdpcDecoder`` and ``PuschTransportBlock`` in one stage -- transport-block CRC, segmentation
with CRC24B and filler bits, LDPC encoding under the caller's ``LdpcGraph``, bit selection and interleaving (TS 38.212 5.1,
5.2.2, 5.3.2, 5.4.2, 5.5), on the current stream.

    rm = PuschRateRecovery(bg, tbs, "16qam", n_layers, n_bits)
    enc = PuschTransportEncoder.for_rate_recovery(rm, graph)          # same integers, same device
    g = enc(tb, rv=0)                                                 # uint8 [B, g_row_bytes], MSB first
    g, cw = enc(tb, rv=rv_tensor, return_codeword=True)               # cw[B, C, cw_row_bytes]: the whole codewords
    bits = unpack_bits(g, enc.n_bits)                                 # ldpc.unpack_bits: [B, n_bits] of 0 / 1

``tb`` is the row ``PuschTransportBlock`` writes.  The base-graph tables of TS 38.212 5.3.2 are not part of this package:
the graph is data, as for the decoder, and must have one of the two core forms ce_enc.h describes."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _stage
from . import ratematch as _rm
from .demod import modulation_order
from .ldpc import LdpcGraph


def build_desc(base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, graph: LdpcGraph, n_ref: int = 0, device_index: int = 0):
    """Fill a ``ce_enc_desc``; returns ``(desc, keep)`` where ``keep`` holds the host arrays the descriptor points to.
    Needs no GPU."""
    keep = graph.csr()
    desc = _lib.EncDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.base_graph, desc.tbs, desc.qm = int(base_graph), int(tbs), modulation_order(modulation)
    desc.n_layers, desc.g_bits, desc.n_ref = int(n_layers), int(n_bits), int(n_ref)
    desc.n_rows, desc.n_cols = graph.n_rows, graph.n_cols
    desc.row_start, desc.col, desc.shift = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep)
    return desc, keep


def derive_host(base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, graph: LdpcGraph, n_ref: int = 0) -> _lib.EncHostView:
    """Host-only view of everything a plan derives (``ce_enc_derive_host``); works without a GPU."""
    desc, keep = build_desc(base_graph, tbs, modulation, n_layers, n_bits, graph, n_ref)
    view = _stage.derive_host("ce_enc_derive_host", desc, _lib.EncHostView())
    del keep
    return view


class PuschTransportEncoder(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_enc_plan_create", "ce_enc_plan_destroy", "ce_enc_encode"
    _NOUN = "the transport-block encoder"

    def __init__(self, base_graph: int, tbs: int, modulation, n_layers: int, n_bits: int, graph: LdpcGraph, n_ref: int = 0, device=None):
        super().__init__(device)
        if not isinstance(graph, LdpcGraph):
            raise ValueError(f"graph must be an LdpcGraph, got {type(graph).__name__}")
        self._args = (int(base_graph), int(tbs), modulation, int(n_layers), int(n_bits), graph, int(n_ref))
        view = derive_host(*self._args)
        self.base_graph, self.tbs, self.qm, self.n_layers, self.n_bits = int(base_graph), int(tbs), modulation_order(modulation), int(n_layers), int(n_bits)
        self.graph, self.n_ref = graph, int(n_ref)
        self.n_code_blocks, self.n_cb, self.zc, self.k_prime, self.payload_bits = int(view.c), int(view.n_cb), int(view.zc), int(view.k_prime), int(view.p)
        self.tb_row_bytes, self.g_row_bytes, self.cw_row_bytes = int(view.tb_row_bytes), int(view.g_row_bytes), int(view.cw_row_bytes)
        self.core_form = "nr" if view.core_form == _lib.CE_ENC_CORE_NR else "triangular"
        self.codeword_bits = graph.n_cols * self.zc
        self.needs_codeword = bool(view.cw_required)      # two code blocks meet inside a dword of g: g is gathered from cw

    @classmethod
    def for_rate_recovery(cls, rm, graph: LdpcGraph) -> "PuschTransportEncoder":
        """The encoder whose ``g`` a ``PuschRateRecovery`` takes back apart: base graph, ``tbs``, modulation, layers,
        ``n_bits``, ``n_ref`` and device are the rate recovery's."""
        if not isinstance(rm, _rm.PuschRateRecovery):
            raise ValueError(f"rm must be a PuschRateRecovery, got {type(rm).__name__}")
        return cls(rm.base_graph, rm.tbs, rm._args[2], rm.n_layers, rm.n_bits, graph, n_ref=rm.n_ref, device=rm._device_arg)

    def _build_desc(self, device_index: int):
        desc, self._keep = build_desc(*self._args, device_index=device_index)
        return desc

    def __call__(self, tb: torch.Tensor, rv=0, return_codeword: bool = False):
        """``g`` or ``(g, cw)`` on the current stream.  ``tb`` is the dense uint8 ``[B, tb_row_bytes]`` row of
        ``PuschTransportBlock`` (bit i < tbs MSB first; bits from ``tbs`` on are ignored); ``rv`` a Python int 0..3 for the
        whole batch or an int32 device tensor of length ``B``.  ``g[B, g_row_bytes]`` uint8 holds bit i < n_bits MSB first
        and zeros behind; ``cw[B, C, cw_row_bytes]`` the whole codewords, punctured columns included, fillers 0."""
        text = f"tb must be a dense uint8 tensor [slots, {self.tb_row_bytes}]"
        if not isinstance(tb, torch.Tensor):
            raise ValueError(text + f", got {type(tb).__name__}")
        if tb.dtype != torch.uint8 or tb.dim() != 2 or tb.shape[1] != self.tb_row_bytes or not tb.is_contiguous():
            raise ValueError(text + f", got {tb.dtype} {tuple(tb.shape)}" + ("" if tb.is_contiguous() else " (not contiguous)"))
        self._plan()
        dev = self.device
        if tb.device != dev:
            raise ValueError(f"tb must be a tensor on {dev}, got {tb.device}")
        B = tb.shape[0]
        g = torch.empty((B, self.g_row_bytes), dtype=torch.uint8, device=dev)
        cw = torch.empty((B, self.n_code_blocks, self.cw_row_bytes), dtype=torch.uint8, device=dev) if return_codeword or self.needs_codeword else None
        rv_t = _stage.batch_param("rv", rv, B, dev, 0, 3, "an int 0..3")   # (the kernel uses ``rv & 3`` of a device tensor)
        if B:
            _stage.check_aligned(("tb", tb), ("g", g), ("cw", cw))
            self._launch(C.c_void_p(tb.data_ptr()), C.c_void_p(rv_t.data_ptr()), _stage.batch_stride(rv_t), B, C.c_void_p(g.data_ptr()),
                         C.c_void_p(cw.data_ptr()) if cw is not None else None)
        return (g, cw) if return_codeword else g
