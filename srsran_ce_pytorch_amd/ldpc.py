"""LDPC decoder EXTENSION (include/ce_ldpc.h; the reference stops at the channel estimate): layered normalised min-sum
decoding of the per-code-block soft buffers of ``PuschRateRecovery``, every block of the batch in one launch on the current
stream.

The base-graph tables of TS 38.212 5.3.2 are NOT part of this package.  The decoder takes the base graph as data -- rows of
``(column, shift)`` pairs -- and nothing in the kernel depends on which graph it is given; it is tested on seeded random
graphs of the NR shape only.  A caller with their own copy of Tables 5.3.2-2 / 5.3.2-3 loads it through
``LdpcGraph.from_table``, which only applies ``V mod Zc``:

    graph = LdpcGraph.from_table(my_bg1_entries[lifting_set_index(rm.zc)], rm.zc)     # (row, col, V) triples
    dec = PuschLdpcDecoder.for_rate_recovery(rm, graph, max_iters=8)
    hard, status = dec(rm(llr, rv=0))           # hard[B, C, row_bytes] uint8, status[B, C, 2] = {iterations, parity ok}
    bits = unpack_bits(hard, dec.k_out)         # [B, C, K'] of 0 / 1"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _stage
from . import ratematch as _rm

NR_SHAPE = {1: (22, 68), 2: (10, 52)}     # base graph -> (n_sys, n_cols) of TS 38.212 5.3.2


def lifting_set_index(zc: int) -> int:
    """Set index i_LS of TS 38.212 Table 5.3.2-1 for ``zc = a 2^j``, a in (2, 3, 5, 7, 9, 11, 13, 15): 0 .. 7;
    ``ValueError`` for a ``zc`` outside the NR set."""
    zc = int(zc)
    if 2 <= zc <= 384:
        a = zc
        while a % 2 == 0 and a > 2:
            a //= 2
        if a == 2 or (a % 2 == 1 and 3 <= a <= 15):
            return (2, 3, 5, 7, 9, 11, 13, 15).index(a)
    raise ValueError(f"zc={zc} is not a lifting size of TS 38.212 Table 5.3.2-1")


class LdpcGraph:
    """A base graph: ``rows[r]`` is the list of ``(col, shift)`` edges of base row r, ``n_cols`` the number of base
    columns; ``n_sys = n_cols - len(rows)``.  Ranges are checked by the library when a decoder is built."""

    def __init__(self, rows: Sequence[Iterable[Tuple[int, int]]], n_cols: int):
        self.rows: List[List[Tuple[int, int]]] = [[(int(c), int(s)) for c, s in row] for row in rows]
        self.n_cols = int(n_cols)

    n_rows = property(lambda self: len(self.rows))
    n_sys = property(lambda self: self.n_cols - len(self.rows))
    n_edges = property(lambda self: sum(len(r) for r in self.rows))

    @classmethod
    def from_table(cls, entries: Iterable[Tuple[int, int, int]], zc: int, n_cols: int | None = None) -> "LdpcGraph":
        """From ``(row, col, V)`` triples of the caller's own copy of the NR tables (one lifting set): ``shift = V mod zc``.
        ``n_cols`` defaults to the largest column + 1."""
        by_row: dict = {}
        top = -1
        for r, c, v in entries:
            by_row.setdefault(int(r), []).append((int(c), int(v) % int(zc)))
            top = max(top, int(c))
        if not by_row or sorted(by_row) != list(range(len(by_row))):
            raise ValueError("entries must cover the rows 0 .. n_rows - 1 without a gap")
        return cls([sorted(by_row[r]) for r in range(len(by_row))], top + 1 if n_cols is None else n_cols)

    def truncated(self, n_rows: int) -> "LdpcGraph":
        """The first ``n_rows`` rows over ``n_sys + n_rows`` columns (a higher code rate: fewer layers);
        ``ValueError`` if one of them touches a column beyond."""
        n_rows = int(n_rows)
        if not 1 <= n_rows <= self.n_rows:
            raise ValueError(f"n_rows={n_rows} outside 1..{self.n_rows}")
        n_cols = self.n_sys + n_rows
        if any(c >= n_cols for row in self.rows[:n_rows] for c, _ in row):
            raise ValueError(f"the first {n_rows} rows touch columns beyond {n_cols - 1}: not a prefix")
        return LdpcGraph(self.rows[:n_rows], n_cols)

    def csr(self):
        """``(row_start[n_rows + 1], col[n_edges], shift[n_edges])`` as int32 arrays."""
        row_start = np.zeros(self.n_rows + 1, np.int32)
        row_start[1:] = np.cumsum([len(r) for r in self.rows])
        col = np.array([c for r in self.rows for c, _ in r], np.int32)
        shift = np.array([s for r in self.rows for _, s in r], np.int32)
        return row_start, col, shift


def build_desc(graph: LdpcGraph, zc: int, n_in: int, k_out: int, n_punctured_cols: int = 2, dtype=torch.int8, llr_scale: float = 1.0,
               max_iters: int = 8, early_stop: bool = True, device_index: int = 0):
    """Fill a ``ce_ldpc_desc``; returns ``(desc, keep)`` where ``keep`` holds the host arrays the descriptor points to.
    Needs no GPU."""
    if dtype not in (torch.float32, torch.int8):
        raise ValueError(f"dtype {dtype}: torch.float32 or torch.int8")
    if isinstance(early_stop, bool):
        early_stop = int(early_stop)
    keep = graph.csr()
    desc = _lib.LdpcDesc()
    desc.abi_version, desc.device = _lib.CE_ABI_VERSION, int(device_index)
    desc.zc, desc.n_rows, desc.n_cols = int(zc), graph.n_rows, graph.n_cols
    desc.n_punctured_cols, desc.n_in, desc.k_out = int(n_punctured_cols), int(n_in), int(k_out)
    desc.in_format = _lib.CE_LDPC_I8 if dtype == torch.int8 else _lib.CE_LDPC_F32
    desc.max_iters, desc.early_stop, desc.llr_scale = int(max_iters), int(early_stop), float(llr_scale)
    desc.row_start, desc.col, desc.shift = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep)
    return desc, keep


def derive_host(graph: LdpcGraph, zc: int, n_in: int, k_out: int, **kw) -> _lib.LdpcHostView:
    """Host-only view of everything a plan derives (``ce_ldpc_derive_host``); works without a GPU."""
    desc, keep = build_desc(graph, zc, n_in, k_out, **kw)
    view = _stage.derive_host("ce_ldpc_derive_host", desc, _lib.LdpcHostView())
    del keep
    return view


def unpack_bits(hard, k_out: int):
    """``[..., k_out]`` uint8 of 0 / 1 from the packed ``hard[..., row_bytes]`` (MSB first); a tensor or a numpy array."""
    if isinstance(hard, torch.Tensor):
        return torch.from_numpy(unpack_bits(hard.cpu().numpy(), k_out))
    return np.unpackbits(np.ascontiguousarray(hard, dtype=np.uint8), axis=-1)[..., :int(k_out)]


class PuschLdpcDecoder(_stage.Stage):
    _CREATE, _DESTROY, _LAUNCH = "ce_ldpc_plan_create", "ce_ldpc_plan_destroy", "ce_ldpc_decode"
    _NOUN = "the LDPC decoder"

    def __init__(self, graph: LdpcGraph, zc: int, n_in: int, k_out: int, n_punctured_cols: int = 2, dtype=torch.int8,
                 llr_scale: float = 1.0, max_iters: int = 8, early_stop: bool = True, device=None):
        super().__init__(device)
        self._args = (graph, int(zc), int(n_in), int(k_out))
        self._kw = dict(n_punctured_cols=n_punctured_cols, dtype=dtype, llr_scale=llr_scale, max_iters=max_iters, early_stop=early_stop)
        view = derive_host(*self._args, **self._kw)
        self.graph, self.zc, self.n_in, self.k_out, self.dtype = graph, int(zc), int(n_in), int(k_out), dtype
        self.max_iters, self.early_stop = int(max_iters), bool(early_stop)
        self.n_sys, self.n_edges, self.row_bytes, self.n_bits = int(view.n_sys), int(view.n_edges), int(view.row_bytes), int(view.n_bits)
        self.blocks_per_workgroup, self.threads, self.lds_bytes = int(view.blocks_per_workgroup), int(view.threads), int(view.lds_bytes)

    @classmethod
    def for_rate_recovery(cls, rm, graph: LdpcGraph, **kw) -> "PuschLdpcDecoder":
        """The decoder of a ``PuschRateRecovery``'s output: ``zc``, ``n_in = N_cb``, ``k_out = K'`` and the dtype are the
        rate recovery's.  ``ValueError`` unless the graph has the NR shape of the rate recovery's base graph -- ``n_sys``
        / ``n_cols`` = 22 / 68 (BG1) or 10 / 52 (BG2) -- or is a prefix of rows of such a graph."""
        view = _rm.derive_host(*rm._args)
        n_sys, n_cols = NR_SHAPE[rm.base_graph]
        if graph.n_sys != n_sys or graph.n_cols > n_cols or graph.n_rows < 1:
            raise ValueError(f"base graph {rm.base_graph} has n_sys = {n_sys} and at most {n_cols} columns; "
                             f"the graph given has n_sys = {graph.n_sys} and {graph.n_cols} columns")
        if any(c >= n_sys + r + 1 for r, row in enumerate(graph.rows) for c, _ in row if r >= 4) or \
                any(c >= n_sys + 4 for row in graph.rows[:4] for c, _ in row):
            raise ValueError("the graph is not a prefix of rows of an NR-shaped graph: row r >= 4 may touch columns up to n_sys + r only")
        kw.setdefault("device", rm._device_arg)
        return cls(graph, int(view.zc), int(view.n_cb), int(view.k_prime), n_punctured_cols=2, dtype=rm.dtype, **kw)

    def _build_desc(self, device_index: int):
        desc, self._keep = build_desc(*self._args, device_index=device_index, **self._kw)
        return desc

    def __call__(self, soft: torch.Tensor, return_post: bool = False):
        """``(hard, status)`` or ``(hard, status, post)`` on the current stream.  ``soft`` is a dense tensor of the plan's
        dtype, ``[B, C, n_in]`` or ``[n_blocks, n_in]``; the leading dimensions are kept: ``hard[..., row_bytes]`` uint8
        (bit i < k_out of a block MSB first, padding 0), ``status[..., 2]`` int32 = {iterations executed, parity holds},
        ``post[..., n_cols zc]`` int16 (the final L)."""
        self._plan()
        dev = self.device
        if not isinstance(soft, torch.Tensor) or soft.device != dev:
            raise ValueError(f"soft must be a tensor on {dev}")
        if soft.dtype != self.dtype or soft.dim() not in (2, 3) or soft.shape[-1] != self.n_in or not soft.is_contiguous():
            raise ValueError(f"soft must be a dense {self.dtype} tensor [slots, C, {self.n_in}] or [blocks, {self.n_in}], "
                             f"got {soft.dtype} {tuple(soft.shape)}")
        lead = tuple(soft.shape[:-1])
        n_blocks = int(np.prod(lead))
        hard = torch.empty(lead + (self.row_bytes,), dtype=torch.uint8, device=dev)
        status = torch.empty(lead + (2,), dtype=torch.int32, device=dev)
        post = torch.empty(lead + (self.n_bits,), dtype=torch.int16, device=dev) if return_post else None
        if n_blocks:
            _stage.check_aligned(("soft", soft), ("hard", hard), ("status", status), ("post", post))
            self._launch(C.c_void_p(soft.data_ptr()), n_blocks, C.c_void_p(hard.data_ptr()), C.c_void_p(status.data_ptr()),
                         C.c_void_p(post.data_ptr()) if post is not None else None)
        return (hard, status, post) if return_post else (hard, status)
