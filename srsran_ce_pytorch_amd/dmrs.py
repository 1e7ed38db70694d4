"""PUSCH DM-RS generation EXTENSION (include/ce_dmrs.h; the reference takes `pilots` as an input and has no generator).

`PuschDmrs(hop1, hop2, n_layers, n_prb_grid, ...)` resolves the hop geometry `estimate()` takes into jump tables on the
GPU; calling it with per-slot `(slot, n_id, n_scid)` writes `pilots[B, n_re, n_dmrs_total, L]` in the layout
`estimate()` consumes, one launch on the current stream:

    pilots = PuschDmrs(hop1, hop2, L, n_prb_grid)(slot, n_id, n_scid)
    estimate(rx, pilots, beta, hop1, hop2, config)

TS 38.211 5.2.1 / 6.4.1.1.1.1 (Rel-15 form, transform precoding off, antenna ports 0-3).

`PuschLowPaprDmrs(hop1, hop2, n_prb_grid, hopping=...)` is the generator for transform precoding ON (DFT-s-OFDM): the
low-PAPR Zadoff-Chu sequence of 38.211 6.4.1.1.1.2 / 5.2.2 with group or sequence hopping, one layer, from per-slot
`(slot, n_id)`; the same layout, so every consumer of `pilots` takes it as it is:

    pilots = PuschLowPaprDmrs(hop1, hop2, n_prb_grid, hopping="group")(slot, n_id)"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

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


class _PilotGenerator(_stage.Stage):
    """What the two generators share: per-slot parameters (ints, host arrays, int32 device tensors) checked, broadcast to
    one batch and handed to the launch as device pointers and element strides, and the ``pilots`` tensor they fill."""
    _RANGES: dict = {}

    def _param(self, name: str, value):
        """-> (value, length or None for a scalar); host values are range-checked here, device tensors taken as they are."""
        if isinstance(value, torch.Tensor) and value.device.type == "cuda":
            if value.dtype != torch.int32 or value.dim() != 1:
                raise ValueError(f"{name}: a device tensor must be int32 of shape [B], got {value.dtype} {tuple(value.shape)}")
            return value, value.shape[0]
        lo, hi = self._RANGES[name]
        a = value.numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        if a.dtype.kind not in "iu" or a.ndim > 1:
            raise ValueError(f"{name}: expected an int or a 1-D integer array, got {a.dtype} with {a.ndim} axes")
        if a.size and (int(a.min()) < lo or int(a.max()) > hi):
            raise ValueError(f"{name} outside {lo}..{hi}")
        return a.astype(np.int32), (None if a.ndim == 0 else a.shape[0])

    def _launch_args(self, ptrs, strides, B: int, out_ptr):
        raise NotImplementedError

    def _generate(self, named, out: Optional[torch.Tensor]) -> torch.Tensor:
        params = [self._param(n, v) for n, v in named]
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
        ptrs, strides = [], []
        for i, (v, n) in enumerate(params):
            if not isinstance(v, torch.Tensor):
                v = torch.from_numpy(np.atleast_1d(v)).to(dev)   # on the current stream, like the launch that reads it
            elif v.device != dev:
                raise ValueError(f"parameter tensors must live on {dev}")
            if v.stride(0) < 0:
                raise ValueError("negative strides are not supported")
            params[i] = (v, n)                                   # alive until the launch is enqueued (stream-ordered allocator)
            ptrs.append(C.c_void_p(v.data_ptr()))
            strides.append(_stage.batch_stride(v))
        self._launch(*self._launch_args(ptrs, strides, B, C.c_void_p(out.data_ptr())))
        return out


class PuschDmrs(_PilotGenerator):
    _CREATE, _DESTROY, _LAUNCH = "ce_dmrs_plan_create", "ce_dmrs_plan_destroy", "ce_dmrs_generate"
    _NOUN = "the DM-RS generator"
    _RANGES = _RANGES

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

    def _launch_args(self, ptrs, strides, B, out_ptr):
        return (*ptrs, (C.c_int64 * 3)(*strides), B, out_ptr)

    def __call__(self, slot, n_id, n_scid, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pilots[B, n_re, n_dmrs_total, L]`` complex64 on the current stream.  Each parameter is an int or an int32
        ``[B]`` tensor on the device (CPU tensors / numpy arrays are range-checked and moved); ``B`` is the longest
        parameter's length (1 when all are ints), length-1 parameters and ints hold for the whole batch."""
        return self._generate((("slot", slot), ("n_id", n_id), ("n_scid", n_scid)), out)


HOPPING = {"neither": _lib.CE_DMRS_LP_HOP_NEITHER, "group": _lib.CE_DMRS_LP_HOP_GROUP, "sequence": _lib.CE_DMRS_LP_HOP_SEQUENCE}


class LowPaprHostView(NamedTuple):
    """What ``ce_dmrs_lp_derive_host`` hands out (include/ce_dmrs.h)."""
    n_re: int
    n_dmrs_total: int
    form: int              # _lib.CE_DMRS_LP_FORM_*
    n_zc: int              # N of the gather table: N_ZC, 31 for 5 PRB, 0 in the table form
    n_words: int
    v_live: bool
    n_prb: int
    col_sym: list
    q: np.ndarray          # [30, 2] int32
    tri: np.ndarray        # [n_re] int32
    hop_words: np.ndarray  # [32, n_words] uint32: row 0 = c for c_init 0, row 1 + i = the contribution of bit i of c_init


def _lp_args(hop1, hop2, n_prb_grid: int, n_sym: int, n_symb_slot: int, n_layers: int, hopping, slots_per_frame: int, phi_table):
    """The scalars and host arrays of ``ce_dmrs_lp_derive_host`` / ``ce_dmrs_lp_plan_create`` from the duck-typed hop objects of
    ``estimate()``, and what keeps the arrays alive.  The library validates the values; here only what has no C form."""
    desc, keep = build_desc(hop1, hop2, 1, n_prb_grid, n_sym, n_symb_slot=n_symb_slot)    # the shape checks of PuschDmrs
    n_hops = int(desc.n_hops)
    if isinstance(hopping, str):
        if hopping not in HOPPING:
            raise ValueError(f"hopping={hopping!r} is not one of {sorted(HOPPING)}")
        hopping = HOPPING[hopping]
    sym = np.zeros((n_hops, _lib.CE_MAX_SYMBOLS), np.uint8)
    re_mask = np.zeros(n_hops, np.uint16)
    prbs = np.zeros((n_hops, int(n_prb_grid)), np.uint8)
    for h in range(n_hops):
        sym[h] = list(desc.hop[h].dmrs_symbols)
        re_mask[h] = desc.hop[h].re_mask[0]
        prbs[h] = np.ctypeslib.as_array(desc.hop[h].mask_prbs, (int(n_prb_grid),))
    phi = None
    if phi_table is not None:
        phi = np.asarray(phi_table.cpu() if isinstance(phi_table, torch.Tensor) else phi_table)
        m_zc = 6 * int(prbs[0].sum())
        if phi.dtype.kind not in "iu" or phi.shape != (30, m_zc):
            raise ValueError(f"phi_table must be an integer array of shape (30, {m_zc}) = (30, 6 n_prb), got {phi.dtype} {phi.shape}")
        if phi.size and (int(phi.min()) < -128 or int(phi.max()) > 127):
            raise ValueError("phi_table values must be -3, -1, 1 or 3")
        phi = np.ascontiguousarray(phi, np.int8)
    arrays = (sym, re_mask, prbs, phi)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)    # noqa: E731
    return (int(n_prb_grid), int(n_sym), int(n_symb_slot), int(n_layers), n_hops, ptr(sym), ptr(re_mask), ptr(prbs), int(hopping),
            int(slots_per_frame), ptr(phi)), (arrays, keep)


def derive_host_low_papr(hop1, hop2, n_prb_grid: int, n_sym: int = 14, *, hopping="neither", slots_per_frame: int = 10,
                         n_symb_slot: int = 14, phi_table=None, n_layers: int = 1) -> LowPaprHostView:
    """Host-only view of what a low-PAPR plan holds (``ce_dmrs_lp_derive_host``); works without a GPU."""
    args, keep = _lp_args(hop1, hop2, n_prb_grid, n_sym, n_symb_slot, n_layers, hopping, slots_per_frame, phi_table)
    info = np.zeros(_lib.CE_DMRS_LP_INFO_LEN, np.int32)
    col_sym = np.zeros(_lib.CE_MAX_SYMBOLS, np.int32)
    q = np.zeros((30, 2), np.int32)
    tri = np.zeros(_lib.CE_DMRS_MAX_RE, np.int32)
    hop_words = np.zeros(32 * _lib.CE_DMRS_LP_MAX_WORDS, np.uint32)
    rc = _lib.load().ce_dmrs_lp_derive_host(*args, *(C.c_void_p(a.ctypes.data) for a in (info, col_sym, q, tri, hop_words)))
    del keep
    if rc != 0:
        _stage.raise_for(rc)
    n_re, n_cols, form, n_zc, n_words, v_live, n_prb = (int(x) for x in info[:7])
    return LowPaprHostView(n_re, n_cols, form, n_zc, n_words, bool(v_live), n_prb, [int(x) for x in col_sym[:n_cols]], q, tri[:n_re].copy(),
                           hop_words[:32 * n_words].reshape(32, n_words).copy())


def low_papr_twiddles(n: int) -> np.ndarray:
    """complex64 ``[n]``: the gather table ``W_n[e] = exp(-j 2 pi e / n)`` as a plan holds it (``ce_dmrs_lp_copy_twiddles``, host only)."""
    if not 2 <= int(n) <= _lib.CE_DMRS_MAX_RE:
        raise ValueError(f"n={n} outside 2..{_lib.CE_DMRS_MAX_RE}")
    w = np.zeros(int(n), np.complex64)
    rc = _lib.load().ce_dmrs_lp_copy_twiddles(int(n), C.c_void_p(w.ctypes.data))
    if rc != 0:
        _stage.raise_for(rc)
    return w


class PuschLowPaprDmrs(_PilotGenerator):
    """PUSCH DM-RS with transform precoding on (38.211 6.4.1.1.1.2, 5.2.2; include/ce_dmrs.h `ce_dmrs_lp_generate`): one layer,
    configuration type 1, single-symbol DM-RS, cyclic shift 0.  Each hop's active PRBs are one contiguous run of the same
    length ``n_prb``; the sequence has ``n_re = 6 n_prb`` elements and starts at the allocation's first pilot.
    ``phi_table`` is the int8 ``[30, 6 n_prb]`` table of 38.211 5.2.2.2 for allocations of 1 to 4 PRB -- data of the caller's,
    not part of this package; without it such an allocation is ``NotImplementedError``."""
    _CREATE, _DESTROY, _LAUNCH = "ce_dmrs_lp_plan_create", "ce_dmrs_lp_plan_destroy", "ce_dmrs_lp_generate"
    _NOUN = "the low-PAPR DM-RS generator"

    def __init__(self, hop1, hop2, n_prb_grid: int, n_sym: int = 14, *, hopping: str = "neither", slots_per_frame: int = 10,
                 n_symb_slot: int = 14, phi_table=None, device=None):
        super().__init__(device)
        self._geometry = (hop1, hop2, int(n_prb_grid), int(n_sym), int(n_symb_slot), 1, hopping, int(slots_per_frame), phi_table)
        view = derive_host_low_papr(hop1, hop2, n_prb_grid, n_sym, hopping=hopping, slots_per_frame=slots_per_frame,
                                    n_symb_slot=n_symb_slot, phi_table=phi_table)
        self.n_re, self.n_dmrs_total, self.n_layers, self.n_prb = view.n_re, view.n_dmrs_total, 1, view.n_prb
        self.hopping, self.slots_per_frame = hopping, int(slots_per_frame)
        self._RANGES = {"slot": (0, self.slots_per_frame - 1), "n_id": (0, 1007)}

    def _create(self, device_index: int, handle) -> int:
        args, keep = _lp_args(*self._geometry)                   # the host arrays live across the call
        rc = self._lib.ce_dmrs_lp_plan_create(_lib.CE_ABI_VERSION, int(device_index), *args, C.byref(handle))
        del keep
        return rc

    def _launch_args(self, ptrs, strides, B, out_ptr):
        return ptrs[0], strides[0], ptrs[1], strides[1], B, out_ptr

    def __call__(self, slot, n_id, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pilots[B, n_re, n_dmrs_total, 1]`` complex64 on the current stream; the parameter forms of ``PuschDmrs``: an int
        or an int32 ``[B]`` device tensor (CPU tensors / numpy arrays are range-checked -- ``slot`` within
        ``0 .. slots_per_frame - 1``, ``n_id`` within ``0 .. 1007`` -- and moved).  Device values are taken as they are: what an
        out-of-range one yields is stated in include/ce_dmrs.h."""
        return self._generate((("slot", slot), ("n_id", n_id)), out)
