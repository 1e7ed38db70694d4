"""SRS channel estimation EXTENSION (include/ce_tp.h `ce_srs_profile`, `ce_srs_estimate`; the reference has no SRS): the
third kind of uplink I/Q in a section-type-1 grid.  Per item and receive port the power delay profile of the sounding ports
(launch 1), and with the delay taken out the channel per sounding port and 4-PRB block, its wideband mean, the noise from the
residual and the received energy (launch 2).  Two launches on the current stream, nothing read by the host between them.

    est = SrsEstimator(k_tc=2, n_ap=2, n_cs=3, k_bar=1, m_srs=48, n_prb_grid=52, n_fft=512, l0=13, hopping="group")
    grid = PuschFronthaulDecompressor(52, n_sym=14, ...)(payload)                 # [B, R, 624, 14], fast layout
    y = grid.permute(0, 1, 3, 2)                                                  # a view, no copy: [B, R, 14, 624]
    prof = est.profile(y, slot, n_id)           # SrsProfile(profile [B, R, win_len], delay int32 [B], ta_s float64 [B])
    out = est(y, slot, n_id, delay=prof.delay)  # SrsEstimate(h_sb [B, R, n_ap, n_symb, n_blocks], h_wb, noise, epre)

``start_prb`` per symbol is the caller's (frequency hopping: Table 6.4.1.4.3-1 is not here), like the ``phi_table`` of the
one-PRB-pair sequences (M = 12 or 24).  ``h_sb`` is referred to each symbol's first comb element: of a channel delayed by
`delay` it keeps the constant phase ``exp(-j 2 pi (12 start_prb[s] + comb_i) delay / (N k_tc))``; `srs_band_response` takes it
out, so that the channel on subcarrier k of the grid is ``srs_band_response(..) exp(-j 2 pi k delay / (N k_tc))``.

`srs_ports`, `srs_sequence` and `srs_map` are the transmit side in numpy, for emulators and tests.  Out of scope: comb 8 and
partial-frequency sounding, per-item geometry, a device-side generator, fractional or per-port delays, interpolation of
``h_sb`` to every subcarrier, coherent combining over symbols, fixed-point input."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, _stage
from .dmrs import HOPPING

FFT_SIZES = (128, 256, 512, 1024, 2048, 4096)
MAX_RX, MAX_AP, MAX_SYMB, INFO_LEN = 64, 4, 4, 10
N_ID_MAX = 65535


def _int(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an int, got {type(v).__name__}")
    if not -2 ** 31 <= int(v) < 2 ** 31:
        raise ValueError(f"{name}={int(v)} does not fit int32")
    return int(v)


def _hopping(hopping) -> int:
    if isinstance(hopping, str):
        if hopping not in HOPPING:
            raise ValueError(f"hopping={hopping!r} is not one of {sorted(HOPPING)}")
        return HOPPING[hopping]
    return _int("hopping", hopping)


def n_cs_max(k_tc: int) -> int:
    if k_tc not in (2, 4):
        raise ValueError(f"k_tc={k_tc} is not 2 or 4")
    return 8 if k_tc == 2 else 12


def srs_ports(k_tc: int, n_ap: int, n_cs: int, k_bar: int):
    """``[(comb_i, cs_i)]`` of the ports ``i < n_ap`` (TS 38.211 6.4.1.4.2, 6.4.1.4.3): ``cs_i = (n_cs + n_cs_max i / n_ap) mod
    n_cs_max`` on comb ``k_bar``; with four ports and ``n_cs`` in the upper half ``cs_i = (n_cs + n_cs_max floor(i / 2) / 2) mod
    n_cs_max`` and ports 1 and 3 on comb ``(k_bar + k_tc / 2) mod k_tc``."""
    k_tc, n_ap, n_cs, k_bar = _int("k_tc", k_tc), _int("n_ap", n_ap), _int("n_cs", n_cs), _int("k_bar", k_bar)
    ncs = n_cs_max(k_tc)
    if n_ap not in (1, 2, 4):
        raise ValueError(f"n_ap={n_ap} is not 1, 2 or 4")
    if not 0 <= n_cs < ncs:
        raise ValueError(f"n_cs={n_cs} outside 0..{ncs - 1}")
    if not 0 <= k_bar < k_tc:
        raise ValueError(f"k_bar={k_bar} outside 0..{k_tc - 1}")
    if n_ap == 4 and n_cs >= ncs // 2:
        return [((k_bar + k_tc // 2) % k_tc if i & 1 else k_bar, (n_cs + ncs * (i // 2) // 2) % ncs) for i in range(4)]
    return [(k_bar, (n_cs + ncs * i // n_ap) % ncs) for i in range(n_ap)]


def _gold_bits(c_init: int, n: int) -> np.ndarray:
    """c(0 .. n - 1) of TS 38.211 5.2.1, bit by bit."""
    nc = 1600
    x1, x2 = np.zeros(nc + n + 31, np.uint8), np.zeros(nc + n + 31, np.uint8)
    x1[0] = 1
    for i in range(31):
        x2[i] = (c_init >> i) & 1
    for i in range(nc + n):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    return x1[nc:nc + n] ^ x2[nc:nc + n]


def _largest_prime_below(m: int) -> int:
    for n in range(m - 1, 1, -1):
        if all(n % d for d in range(2, int(n ** 0.5) + 1)):
            return n
    raise ValueError(m)


def srs_base_sequence(u: int, v: int, m: int, phi_table=None) -> np.ndarray:
    """complex128 ``[m]``: ``rbar_{u,v}(n)`` of TS 38.211 5.2.2 for ``m`` a multiple of 12 (12 and 24 from `phi_table` ``[30, m]``)."""
    if m >= 36:
        n_zc = _largest_prime_below(m)
        q_bar = n_zc * (u + 1) / 31.0
        q = int(np.floor(q_bar + 0.5)) + v * (-1) ** int(np.floor(2.0 * q_bar))
        t = np.arange(m, dtype=np.int64) % n_zc
        return np.exp(-1j * np.pi * ((q * t * (t + 1)) % (2 * n_zc)) / n_zc)
    if phi_table is None:
        raise NotImplementedError(f"M={m} needs the phi table of 38.211 5.2.2.2, which the caller provides")
    return np.exp(1j * np.pi * np.asarray(phi_table, np.float64)[u] / 4.0)


def srs_hopping(hopping, n_id: int, slot: int, l0: int, n_symb: int, m: int, n_symb_slot: int = 14, slots_per_frame: int = 10):
    """``[(u, v)]`` of the symbols ``l0 .. l0 + n_symb - 1`` (6.4.1.4.2): ``c_init = n_id`` for group and for sequence hopping."""
    mode = _hopping(hopping)
    out = []
    c = _gold_bits(int(n_id) & 0x7FFFFFFF, 8 * n_symb_slot * slots_per_frame) if mode else None
    for s in range(n_symb):
        p = n_symb_slot * (int(slot) % slots_per_frame) + l0 + s
        f_gh = v = 0
        if mode == _lib.CE_DMRS_LP_HOP_GROUP:
            f_gh = sum(int(c[8 * p + k]) << k for k in range(8)) % 30
        elif mode == _lib.CE_DMRS_LP_HOP_SEQUENCE and m >= 72:
            v = int(c[p])
        out.append(((f_gh + int(n_id)) % 30, v))
    return out


def srs_sequence(k_tc: int, n_ap: int, n_cs: int, k_bar: int, m_srs: int, n_symb: int = 1, l0: int = 0, slot: int = 0, n_id: int = 0,
                 hopping="neither", n_symb_slot: int = 14, slots_per_frame: int = 10, phi_table=None) -> np.ndarray:
    """complex128 ``[n_ap, n_symb, M]``: ``r^(p_i)(n, l') = exp(j 2 pi cs_i n / n_cs_max) rbar_{u,v}(n)``, ``M = 12 m_srs / k_tc``."""
    ports = srs_ports(k_tc, n_ap, n_cs, k_bar)
    ncs, m = n_cs_max(k_tc), 12 * int(m_srs) // k_tc
    n = np.arange(m, dtype=np.int64)
    out = np.zeros((n_ap, n_symb, m), np.complex128)
    for s, (u, v) in enumerate(srs_hopping(hopping, n_id, slot, l0, n_symb, m, n_symb_slot, slots_per_frame)):
        base = srs_base_sequence(u, v, m, phi_table)
        for i, (_, cs) in enumerate(ports):
            out[i, s] = base * np.exp(2j * np.pi * ((cs * n) % ncs) / ncs)
    return out


def _start_prbs(start_prb, n_symb: int):
    if isinstance(start_prb, (int, np.integer)) and not isinstance(start_prb, bool):
        return [int(start_prb)] * max(int(n_symb), 0)
    if isinstance(start_prb, (str, bytes)) or not hasattr(start_prb, "__iter__"):
        raise ValueError(f"start_prb must be an int or a sequence of ints, got {type(start_prb).__name__}")
    sp = [_int(f"start_prb[{i}]", v) for i, v in enumerate(start_prb)]
    if len(sp) != n_symb:
        raise ValueError(f"start_prb holds {len(sp)} entries for n_symb={n_symb}")
    return sp


def srs_map(seq: np.ndarray, k_tc: int, n_ap: int, n_cs: int, k_bar: int, start_prb, l0: int, n_prb_grid: int, n_sym: int = 14,
            beta: float = 1.0) -> np.ndarray:
    """complex128 transmit grid ``[n_ap, 12 n_prb_grid, n_sym]`` with ``beta seq[i, s, n]`` on subcarrier
    ``12 start_prb[s] + comb_i + k_tc n`` of symbol ``l0 + s``, zero elsewhere."""
    seq = np.asarray(seq)
    n_symb, m = seq.shape[1], seq.shape[2]
    sp = _start_prbs(start_prb, n_symb)
    grid = np.zeros((n_ap, 12 * n_prb_grid, n_sym), np.complex128)
    for i, (comb, _) in enumerate(srs_ports(k_tc, n_ap, n_cs, k_bar)):
        for s in range(n_symb):
            k0 = 12 * sp[s] + comb
            if sp[s] < 0 or k0 + k_tc * (m - 1) >= 12 * n_prb_grid or not 0 <= l0 + s < n_sym:
                raise ValueError(f"symbol {s}: the sequence does not lie inside the grid")
            grid[i, k0:k0 + k_tc * m:k_tc, l0 + s] = beta * seq[i, s]
    return grid


def srs_band_response(h_sb, delay, k_tc: int, n_fft: int, ports, start_prb):
    """``h_sb [B, R, n_ap, n_symb, n_blocks]`` (numpy) with the constant phases of a delayed channel taken out:
    ``h_sb exp(+j 2 pi (12 start_prb[s] + comb_i) delay[b] / (N k_tc))``.  `ports` as `srs_ports` returns them."""
    h = np.asarray(h_sb).astype(np.complex128)
    d = np.broadcast_to(np.asarray(delay, np.float64).reshape(-1), (h.shape[0],))
    k0 = 12.0 * np.asarray(start_prb, np.float64)[None, :] + np.array([c for c, _ in ports], np.float64)[:, None]       # [n_ap, n_symb]
    return h * np.exp(2j * np.pi * k0[None, None, :, :, None] * d[:, None, None, None, None] / (float(n_fft) * k_tc))


class SrsHostView(NamedTuple):
    """What ``ce_srs_derive_host`` hands out (include/ce_tp.h)."""
    view: object           # _lib.TpHostView of the N-point transform
    m: int
    q_len: int
    n_blocks: int
    n_combs: int
    form: int              # _lib.CE_DMRS_LP_FORM_*
    n_zc: int
    guard: int
    default_win_len: int
    n_words: int
    v_live: bool
    port_comb: list
    port_cs: list
    q: np.ndarray          # [30, 2] int32
    tri: np.ndarray        # [M] int32
    hop_words: np.ndarray  # [32, n_words] uint32


def _phi(phi_table, m: int):
    if phi_table is None:
        return None
    phi = np.asarray(phi_table.cpu() if isinstance(phi_table, torch.Tensor) else phi_table)
    if m in (12, 24):
        if phi.dtype.kind not in "iu" or phi.shape != (30, m):
            raise ValueError(f"phi_table must be an integer array of shape (30, {m}), got {phi.dtype} {phi.shape}")
        if int(phi.min()) < -128 or int(phi.max()) > 127:
            raise ValueError("phi_table values must be -3, -1, 1 or 3")
        return np.ascontiguousarray(phi, np.int8)
    return None                                                   # ignored where the sequence is Zadoff-Chu


def _plan_args(k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, l0, start_prb, n_prb_grid, n_sym, n_symb_slot, hopping, slots_per_frame, n_fft, win_len,
               phi_table):
    names = ("k_tc", "n_ap", "n_cs", "k_bar", "m_srs", "n_symb", "l0")
    head = [_int(n, v) for n, v in zip(names, (k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, l0))]
    sp = _start_prbs(start_prb, head[5])
    arr = (C.c_int32 * max(len(sp), MAX_SYMB))(*sp)
    m = 12 * head[4] // head[0] if head[0] in (2, 4) else 0
    phi = _phi(phi_table, m)
    tail = [_int(n, v) for n, v in zip(("n_prb_grid", "n_sym", "n_symb_slot"), (n_prb_grid, n_sym, n_symb_slot))]
    tail += [_hopping(hopping), _int("slots_per_frame", slots_per_frame), _int("n_fft", n_fft), _int("win_len", win_len)]
    return (*head, C.cast(arr, C.c_void_p), *tail, None if phi is None else C.c_void_p(phi.ctypes.data)), (arr, phi)


def derive_host(k_tc: int, n_ap: int, n_cs: int, k_bar: int, m_srs: int, n_prb_grid: int, n_fft: int, *, n_symb: int = 1, l0: int = 0, start_prb=0,
                n_sym: int = 14, n_symb_slot: int = 14, hopping="neither", slots_per_frame: int = 10, win_len: Optional[int] = None,
                phi_table=None) -> SrsHostView:
    """The library's own validation and derivation (``ce_srs_derive_host``; works without a GPU), or ``ValueError`` /
    ``NotImplementedError`` for whatever it refuses.  ``win_len=None`` stands for the default window."""
    args, keep = _plan_args(k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, l0, start_prb, n_prb_grid, n_sym, n_symb_slot, hopping, slots_per_frame, n_fft,
                            1 if win_len is None else win_len, phi_table)
    view, info = _lib.TpHostView(), np.zeros(INFO_LEN, np.int32)
    comb, cs, q = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros((30, 2), np.int32)
    tri, hop = np.zeros(_lib.CE_DMRS_MAX_RE, np.int32), np.zeros(32 * _lib.CE_DMRS_LP_MAX_WORDS, np.uint32)
    rc = _lib.load().ce_srs_derive_host(*args, C.byref(view), *(C.c_void_p(a.ctypes.data) for a in (info, comb, cs, q, tri, hop)))
    del keep
    if rc != 0:
        _stage.raise_for(rc)
    m, q_len, n_blocks, n_combs, form, n_zc, guard, dwl, nw, v_live = (int(x) for x in info)
    return SrsHostView(view, m, q_len, n_blocks, n_combs, form, n_zc, guard, dwl, nw, bool(v_live), [int(x) for x in comb[:int(n_ap)]],
                       [int(x) for x in cs[:int(n_ap)]], q, tri[:m].copy(), hop[:32 * nw].reshape(32, nw).copy())


def tables(k_tc: int, n_ap: int, n_cs: int, k_bar: int, m_srs: int, n_fft: int):
    """(twiddles complex64 ``[N]``, gather table complex64 ``[N_ZC]`` or ``[4]``, rho complex64 ``[n_ap, n_cs_max]``): the plan's
    tables (``ce_srs_copy_tables``, host only)."""
    args = [_int(n, v) for n, v in zip(("k_tc", "n_ap", "n_cs", "k_bar", "m_srs", "n_fft"), (k_tc, n_ap, n_cs, k_bar, m_srs, n_fft))]
    ok = args[0] in (2, 4) and args[1] in (1, 2, 4) and 4 <= args[4] <= 272 and args[4] % 4 == 0 and args[5] in FFT_SIZES
    m = 12 * args[4] // args[0] if ok else 0
    n_w = (_largest_prime_below(m) if m >= 36 else 4) if ok else 1
    tw, w = np.zeros(args[5] if ok else 1, np.complex64), np.zeros(n_w, np.complex64)
    rho = np.zeros((args[1], n_cs_max(args[0])) if ok else (1, 1), np.complex64)
    rc = _lib.load().ce_srs_copy_tables(*args, *(C.c_void_p(a.ctypes.data) for a in (tw, w, rho)))
    if rc != 0:
        _stage.raise_for(rc)
    return tw, w, rho


class SrsProfile(NamedTuple):
    profile: torch.Tensor      # float32 [B, R, win_len]
    delay: torch.Tensor        # int32   [B], on the N grid
    ta_s: torch.Tensor         # float64 [B], delay / (N k_tc scs_hz)


class SrsEstimate(NamedTuple):
    h_sb: torch.Tensor         # complex64 [B, R, n_ap, n_symb, n_blocks]
    h_wb: torch.Tensor         # complex64 [B, R, n_ap]
    noise: torch.Tensor        # float32 [B, R]
    epre: torch.Tensor         # float32 [B, R]


class SrsEstimator(_stage.Stage):
    """``k_tc`` 2 or 4; ``n_ap`` 1, 2 or 4; ``n_cs`` below 8 (comb 2) or 12 (comb 4); ``k_bar`` below ``k_tc``; ``m_srs`` a multiple of
    4 in 4..272; ``n_symb`` 1, 2 or 4 symbols from ``l0`` inside the grid's ``n_sym``; ``start_prb`` an int or one per symbol;
    ``n_fft`` 128 .. 4096 above ``M = 12 m_srs / k_tc``; ``win_len`` defaults to ``floor(N gap / n_cs_max) - ceil(N / M)``.
    Validated on construction by the library's own host entry point; no GPU needed until the first call."""
    _CREATE, _DESTROY = "ce_srs_plan_create", "ce_srs_plan_destroy"
    _NOUN = "the SRS estimator"

    def __init__(self, k_tc: int, n_ap: int, n_cs: int, k_bar: int, m_srs: int, n_prb_grid: int, n_fft: int, *, n_symb: int = 1, l0: int = 0,
                 start_prb=0, n_sym: int = 14, n_symb_slot: int = 14, hopping="neither", slots_per_frame: int = 10, win_len: Optional[int] = None,
                 phi_table=None, scs_hz: float = 30e3, device=None):
        super().__init__(device)
        kw = dict(n_symb=n_symb, l0=l0, start_prb=start_prb, n_sym=n_sym, n_symb_slot=n_symb_slot, hopping=hopping, slots_per_frame=slots_per_frame,
                  phi_table=phi_table)
        hv = derive_host(k_tc, n_ap, n_cs, k_bar, m_srs, n_prb_grid, n_fft, win_len=win_len, **kw)
        self.win_len = hv.default_win_len if win_len is None else int(win_len)
        self.host_view = hv
        self.k_tc, self.n_ap, self.n_cs, self.k_bar, self.m_srs = int(k_tc), int(n_ap), int(n_cs), int(k_bar), int(m_srs)
        self.n_prb_grid, self.n_fft, self.n_symb, self.l0, self.n_sym = int(n_prb_grid), int(n_fft), int(n_symb), int(l0), int(n_sym)
        self.n_symb_slot, self.slots_per_frame, self.hopping = int(n_symb_slot), int(slots_per_frame), _hopping(hopping)
        self.start_prb = tuple(_start_prbs(start_prb, self.n_symb))
        self.ports = list(zip(hv.port_comb, hv.port_cs))
        self.m, self.q_len, self.n_blocks, self.guard, self.n_sc = hv.m, hv.q_len, hv.n_blocks, hv.guard, 12 * self.n_prb_grid
        self._phi = _phi(phi_table, hv.m)
        self.scs_hz = float(scs_hz)
        if isinstance(scs_hz, bool) or not (np.isfinite(self.scs_hz) and self.scs_hz > 0):
            raise ValueError(f"scs_hz={scs_hz!r} must be finite and > 0")
        self.threads_per_row, self.rows_per_workgroup, self.lds_bytes = int(hv.view.threads_per_row), int(hv.view.rows_per_workgroup), int(hv.view.lds_bytes)
        self.radix = tuple(int(r) for r in hv.view.radix[:hv.view.n_passes])

    def _create(self, device_index: int, handle) -> int:
        args, keep = _plan_args(self.k_tc, self.n_ap, self.n_cs, self.k_bar, self.m_srs, self.n_symb, self.l0, self.start_prb, self.n_prb_grid, self.n_sym,
                                self.n_symb_slot, self.hopping, self.slots_per_frame, self.n_fft, self.win_len, self._phi)
        rc = self._lib.ce_srs_plan_create(_lib.CE_ABI_VERSION, int(device_index), *args, C.byref(handle))
        del keep
        return rc

    def _call(self, entry: str, *args):
        dev = self.device
        with torch.cuda.device(dev):
            rc = getattr(self._lib, entry)(self._handle, *args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            _stage.raise_for(rc)

    def _inputs(self, y, slot, n_id):
        """The checks both launches share: (B, R, the launch's leading arguments)."""
        self._plan()
        dev = self.device
        if not isinstance(y, torch.Tensor) or y.device != dev:
            raise ValueError(f"y must be a tensor on {dev}")
        if (y.dtype != torch.complex64 or y.dim() != 4 or y.shape[2] != self.n_sym or y.shape[3] < self.n_sc or (y.shape[3] > 1 and y.stride(3) != 1)):
            raise ValueError(f"y must be a {torch.complex64} tensor [items, ports, {self.n_sym}, >= {self.n_sc}] with a contiguous last dimension, got "
                             f"{y.dtype} {tuple(y.shape)} with strides {tuple(y.stride())}")
        B, R = int(y.shape[0]), int(y.shape[1])
        if not 1 <= R <= MAX_RX:
            raise ValueError(f"y holds {R} receive ports: 1..{MAX_RX} are supported")
        st = [int(y.stride(d)) if y.shape[d] > 1 else 0 for d in range(3)]
        if B:
            if min(st) < 0:
                raise ValueError("negative strides are not supported")
            held = y.untyped_storage().nbytes() // 8 - int(y.storage_offset())
            if sum((n - 1) * s for n, s in zip((B, R, self.n_sym), st)) + self.n_sc > held:
                raise ValueError(f"y: strides {tuple(st)} put the last row's {self.n_sc} elements behind the {held} the tensor holds")
            if y.data_ptr() % 8:
                raise ValueError("y must be 8-byte aligned")
        slot_t = _stage.batch_param("slot", slot, B, dev, 0, 2 ** 31 - 1)
        id_t = _stage.batch_param("n_id", n_id, B, dev, 0, N_ID_MAX)
        lead = (C.c_void_p(y.data_ptr()), *st, B, R, C.c_void_p(slot_t.data_ptr()), _stage.batch_stride(slot_t), C.c_void_p(id_t.data_ptr()),
                _stage.batch_stride(id_t))
        return B, R, lead, (slot_t, id_t)

    def profile(self, y: torch.Tensor, slot, n_id) -> SrsProfile:
        """Launch 1.  ``y`` is complex64 ``[B, R, n_sym, >= 12 n_prb_grid]`` with a contiguous last dimension and free strides
        otherwise; ``slot`` and ``n_id`` are ints or device int32 tensors ``[B]``.  ``delay = argmax_d' sum_r profile - g`` and
        ``ta_s = delay / (N k_tc scs_hz)`` are torch operations on the kernel's output."""
        B, R, lead, keep = self._inputs(y, slot, n_id)
        prof = torch.empty((B, R, self.win_len), dtype=torch.float32, device=self.device)
        if B:
            self._call("ce_srs_profile", *lead, C.c_void_p(prof.data_ptr()))
        delay = (prof.sum(1).argmax(-1) - self.guard).to(torch.int32)
        return SrsProfile(prof, delay, delay.to(torch.float64) / (self.n_fft * self.k_tc * self.scs_hz))

    def __call__(self, y: torch.Tensor, slot, n_id, delay: Optional[torch.Tensor] = None) -> SrsEstimate:
        """Launch 2.  ``delay`` is a device int32 tensor ``[B]`` of any stride >= 0 (``expand`` of one value included) and any
        values (taken mod N), or None for 0."""
        B, R, lead, keep = self._inputs(y, slot, n_id)
        dev = self.device
        d_ptr, d_st = None, 0
        if delay is not None:
            if not isinstance(delay, torch.Tensor) or delay.dtype != torch.int32 or delay.dim() != 1 or delay.shape[0] != B or delay.device != dev:
                raise ValueError(f"delay must be an int32 tensor of shape [{B}] on {dev}")
            if delay.stride(0) < 0:
                raise ValueError("negative strides are not supported")
            d_ptr, d_st = delay.data_ptr(), (int(delay.stride(0)) if B > 1 else 0)
        h_sb = torch.empty((B, R, self.n_ap, self.n_symb, self.n_blocks), dtype=torch.complex64, device=dev)
        h_wb = torch.empty((B, R, self.n_ap), dtype=torch.complex64, device=dev)
        noise = torch.empty((B, R), dtype=torch.float32, device=dev)
        epre = torch.empty((B, R), dtype=torch.float32, device=dev)
        if B:
            self._call("ce_srs_estimate", *lead, C.c_void_p(d_ptr), d_st, *(C.c_void_p(t.data_ptr()) for t in (h_sb, h_wb, noise, epre)))
        return SrsEstimate(h_sb, h_wb, noise, epre)
