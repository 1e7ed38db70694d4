"""PRACH preamble detection EXTENSION (include/ce_tp.h `ce_prach_detect`; the reference stops at the channel estimate): the
other kind of uplink frequency-domain I/Q an O-RAN 7.2x radio unit sends.  Per PRACH occasion and Zadoff-Chu root: the
correlation with the root in the frequency domain, an inverse transform of length N, the power delay profile summed over
ports and repetitions, and per cyclic-shift window its maximum and where it lies; one launch on the current stream.

    det = PrachDetector(139, 256, roots=[1, 138, 70], n_cs=13, n_shifts=10)       # format A/B/C, unrestricted set
    grid = PuschFronthaulDecompressor(12, n_sym=S, ...)(payload)                  # [B, R, 144, S], fast layout
    out = det(grid.permute(0, 1, 3, 2)[..., :139], threshold=12.0)                # a view, no copy: [B, R, S, 139]
    out.detected                     # bool  [B, n_roots, n_shifts]: peak > threshold mean
    out.arrival_s[out.detected]      # seconds after the occasion's reference: the timing advance

``roots`` are PHYSICAL root indices u; the logical-to-physical table of TS 38.211 Tables 6.3.3.1-3/-4 and the N_CS tables are
the caller's data.  ``combine`` is ``"noncoherent"`` (every (port, repetition) adds its power) or ``"coherent"`` (the
repetitions of a port are added before the transform: 10 log10(S) dB more for a channel that holds still over them).

``prach_preamble_freq`` is the transmit side, for emulators and tests.  Out of scope: restricted sets (high-speed cyclic
shifts), the time-domain front end (decimation and the long FFT stay with the radio unit), a noise estimate that excludes
the detected windows, successive cancellation, frequency-offset hypotheses, fixed-point input."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, _stage

L_RA = (139, 571, 839, 1151)
FFT_SIZES = (256, 512, 1024, 2048, 4096)
MAX_ROOTS, MAX_SHIFTS, MAX_PORTS, MAX_REPS = 64, 64, 64, 12
COMBINE = {"noncoherent": 0, "coherent": 1}
DEFAULT_SCS_RA_HZ = {839: 1.25e3, 139: 15e3, 571: 30e3, 1151: 15e3}


def _int(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an int, got {type(v).__name__}")
    if not -2 ** 31 <= int(v) < 2 ** 31:
        raise ValueError(f"{name}={int(v)} does not fit int32")
    return int(v)


def _l_ra(l_ra) -> int:
    L = _int("l_ra", l_ra)
    if L not in L_RA:
        raise ValueError(f"l_ra={L} is none of {L_RA}")
    return L


def _roots(roots):
    if isinstance(roots, (str, bytes)) or not hasattr(roots, "__iter__"):
        raise ValueError(f"roots must be a sequence of ints, got {type(roots).__name__}")
    r = [_int(f"roots[{i}]", u) for i, u in enumerate(roots)]
    return r, (C.c_int32 * max(len(r), 1))(*r)


def _zc(u: int, L: int) -> np.ndarray:
    """x_u(n) = exp(-j 2 pi ((u n (n + 1) / 2) mod L) / L), the index reduced in integers (TS 38.211 6.3.3.1)."""
    n = np.arange(L, dtype=np.int64)
    return np.exp(-2j * np.pi * ((n * (n + 1) // 2 % L * u) % L).astype(np.float64) / L)


def prach_root_freq(u: int, l_ra: int) -> np.ndarray:
    """complex128 ``[L]``: ``X_u[k] = sum_n x_u(n) exp(-j 2 pi n k / L)`` of the physical root `u` in ``1 .. L - 1``; every
    entry has modulus ``sqrt(L)``."""
    L, u = _l_ra(l_ra), _int("u", u)
    if not 1 <= u < L:
        raise ValueError(f"u={u} outside 1..{L - 1}")
    return np.fft.fft(_zc(u, L))


def prach_preamble_freq(u: int, c_v: int, l_ra: int, delay: float = 0.0) -> np.ndarray:
    """The transmit side: complex128 ``[L]``, the unit-modulus frequency-domain preamble of root `u` and cyclic shift `c_v`
    (``x_{u,v}(n) = x_u((n + C_v) mod L)``), ``X_u[k] / sqrt(L) exp(+j 2 pi k (c_v - delay) / L)``, arriving `delay`
    sequence samples (units of ``1 / (L delta_f_RA)`` seconds, fractions allowed) late.  The detector finds it in the window
    of shift ``c_v`` at the index ``((L - c_v + delay) mod L) N / L`` of the N grid."""
    L, c = _l_ra(l_ra), _int("c_v", c_v)
    if not 0 <= c < L:
        raise ValueError(f"c_v={c} outside 0..{L - 1}")
    x = prach_root_freq(u, L)
    return x / np.abs(x) * np.exp(2j * np.pi * np.arange(L) * ((c - float(delay)) / L))


def derive_host(l_ra: int, n_fft: int, roots: Sequence[int], n_cs: int, n_shifts: int, combine: str = "noncoherent"):
    """(``TpHostView`` of the N-point transform, ``win_start`` int32 ``[n_shifts]``, ``win_len``) as the library derives them
    (``ce_prach_derive_host``; works without a GPU), or ``ValueError`` for whatever the library refuses."""
    if combine not in COMBINE:
        raise ValueError(f"combine={combine!r} is none of {sorted(COMBINE)}")
    r, arr = _roots(roots)
    ns = _int("n_shifts", n_shifts)
    view, ws, wl = _lib.TpHostView(), (C.c_int32 * max(min(ns, MAX_SHIFTS), 1))(), C.c_int32()
    rc = _lib.load().ce_prach_derive_host(_int("l_ra", l_ra), _int("n_fft", n_fft), len(r), arr, _int("n_cs", n_cs), ns, COMBINE[combine],
                                          C.byref(view), ws, C.byref(wl))
    if rc != 0:
        _stage.raise_for(rc)
    return view, np.array(ws[:ns], np.int32), int(wl.value)


def tables(l_ra: int, n_fft: int, roots: Sequence[int]):
    """(twiddles complex64 ``[N]``, root table ``T_i[k]`` complex64 ``[n_roots, L]``): the plan's tables
    (``ce_prach_copy_tables``, host only)."""
    r, arr = _roots(roots)
    L, N = _int("l_ra", l_ra), _int("n_fft", n_fft)
    ok = L in L_RA and N in FFT_SIZES and 1 <= len(r) <= MAX_ROOTS
    tw, tab = np.zeros(N if ok else 1, np.complex64), np.zeros((len(r), L) if ok else (1, 1), np.complex64)
    rc = _lib.load().ce_prach_copy_tables(L, N, len(r), arr, C.c_void_p(tw.ctypes.data), C.c_void_p(tab.ctypes.data))
    if rc != 0:
        _stage.raise_for(rc)
    return tw, tab


def prach_windows(l_ra: int, n_fft: int, n_cs: int, n_shifts: int):
    """(``win_start`` int32 ``[n_shifts]``, ``win_len``): window v holds the indices ``(win_start[v] + d) mod N``,
    ``d < win_len``, of the N grid."""
    _, ws, wl = derive_host(l_ra, n_fft, [1], n_cs, n_shifts)
    return ws, wl


def prach_arrival_seconds(l_ra: int, n_fft: int, n_cs: int, shift, delay, scs_ra_hz: float):
    """Seconds by which the preamble of cyclic shift ``C_v = shift n_cs`` arrived late, from the detector's `delay` (the index
    inside window `shift`): ``(win_start + delay - ((L - C_v) mod L) N / L) / (N scs_ra_hz)`` with the window start taken
    before its reduction mod N, ``floor(((L - C_v) mod L) N / L) - ceil(N / L)`` (0 where ``n_cs = 0``).  `shift` and `delay`
    broadcast (numpy)."""
    L, N, ncs = _l_ra(l_ra), _int("n_fft", n_fft), _int("n_cs", n_cs)
    c = (L - np.asarray(shift, np.int64) * ncs) % L
    start = (c * N) // L - (-(-N // L) if ncs else 0)           # n_cs = 0: the one window starts at 0, without a guard
    return (start + np.asarray(delay, np.float64) - c * N / L) / (N * float(scs_ra_hz))


class PrachDetection(NamedTuple):
    peak: torch.Tensor                    # float32 [B, n_roots, n_shifts]
    delay: torch.Tensor                   # int32   [B, n_roots, n_shifts]
    mean: torch.Tensor                    # float32 [B, n_roots]
    detected: Optional[torch.Tensor]      # bool    [B, n_roots, n_shifts], with a threshold
    arrival_s: Optional[torch.Tensor]     # float64 [B, n_roots, n_shifts], with a threshold
    profile: Optional[torch.Tensor]       # float32 [B, n_roots, N], with return_profile


class PrachDetector(_stage.Stage):
    """``l_ra`` 139, 571, 839 or 1151; ``n_fft`` 256 .. 4096 above it; ``roots`` 1..64 distinct physical root indices in
    ``1 .. L - 1``; ``n_cs`` 0 .. L - 1; ``n_shifts`` 1..64 windows with ``n_shifts n_cs <= L`` (``n_cs = 0``: one window round the
    circle).  ``scs_ra_hz`` (for ``arrival_s``) defaults to 1.25 kHz for 839, 15 kHz for 139 and 1151, 30 kHz for 571.
    Validated on construction by the library's own host entry point; no GPU needed until the first call."""
    _CREATE, _DESTROY, _LAUNCH = "ce_prach_plan_create", "ce_prach_plan_destroy", "ce_prach_detect"
    _NOUN = "the PRACH detector"

    def __init__(self, l_ra: int, n_fft: int, roots: Sequence[int], n_cs: int, n_shifts: int, combine: str = "noncoherent", device=None,
                 scs_ra_hz: Optional[float] = None):
        super().__init__(device)
        view, self.win_start, self.win_len = derive_host(l_ra, n_fft, roots, n_cs, n_shifts, combine)
        self.l_ra, self.n_fft, self.n_cs, self.n_shifts, self.combine = int(l_ra), int(n_fft), int(n_cs), int(n_shifts), combine
        self.roots = tuple(int(u) for u in roots)
        self.n_roots = len(self.roots)
        self.scs_ra_hz = float(DEFAULT_SCS_RA_HZ[self.l_ra] if scs_ra_hz is None else scs_ra_hz)
        if not (np.isfinite(self.scs_ra_hz) and self.scs_ra_hz > 0):
            raise ValueError(f"scs_ra_hz={scs_ra_hz!r} must be finite and > 0")
        self.threads_per_row, self.rows_per_workgroup, self.lds_bytes = int(view.threads_per_row), int(view.rows_per_workgroup), int(view.lds_bytes)
        self.radix = tuple(int(r) for r in view.radix[:view.n_passes])
        # seconds per index of the N grid, and per window what puts the fractional window start back
        self._offset_s = prach_arrival_seconds(self.l_ra, self.n_fft, self.n_cs, np.arange(self.n_shifts), 0.0, self.scs_ra_hz)
        self._offset_dev = None

    def _create(self, device_index: int, handle) -> int:
        return self._lib.ce_prach_plan_create(_lib.CE_ABI_VERSION, int(device_index), self.l_ra, self.n_fft, self.n_roots,
                                              (C.c_int32 * self.n_roots)(*self.roots), self.n_cs, self.n_shifts, COMBINE[self.combine], C.byref(handle))

    def __call__(self, y: torch.Tensor, threshold: Optional[float] = None, return_profile: bool = False) -> PrachDetection:
        """``y`` is complex64 ``[B, R, S, >= L]`` -- occasions, ports (1..64), repetitions (1..12), subcarriers -- with a
        contiguous last dimension and free strides otherwise: a view of the decompressor's grid included.  Only the first ``L``
        elements of each row are read.  With a ``threshold``, ``detected = peak > threshold mean`` and ``arrival_s`` (seconds,
        meaningful where detected) come along, both torch operations on the kernel's outputs."""
        self._plan()
        dev, L = self.device, self.l_ra
        if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating))
                                      or not np.isfinite(float(threshold)) or float(threshold) < 0):
            raise ValueError(f"threshold={threshold!r} must be a finite float >= 0")
        if not isinstance(y, torch.Tensor) or y.device != dev:
            raise ValueError(f"y must be a tensor on {dev}")
        if y.dtype != torch.complex64 or y.dim() != 4 or y.shape[3] < L or (y.shape[3] > 1 and y.stride(3) != 1):
            raise ValueError(f"y must be a {torch.complex64} tensor [occasions, ports, repetitions, >= {L}] with a contiguous last dimension, got "
                             f"{y.dtype} {tuple(y.shape)} with strides {tuple(y.stride())}")
        B, R, S = (int(n) for n in y.shape[:3])
        if not 1 <= R <= MAX_PORTS or not 1 <= S <= MAX_REPS:
            raise ValueError(f"y holds {R} ports and {S} repetitions: 1..{MAX_PORTS} and 1..{MAX_REPS} are supported")
        shape = (B, self.n_roots, self.n_shifts)
        peak = torch.empty(shape, dtype=torch.float32, device=dev)
        delay = torch.empty(shape, dtype=torch.int32, device=dev)
        mean = torch.empty(shape[:2], dtype=torch.float32, device=dev)
        profile = torch.empty((B, self.n_roots, self.n_fft), dtype=torch.float32, device=dev) if return_profile else None
        if B:
            st = [int(y.stride(d)) if y.shape[d] > 1 else 0 for d in range(3)]
            if min(st) < 0:
                raise ValueError("negative strides are not supported")
            held = y.untyped_storage().nbytes() // 8 - int(y.storage_offset())
            if sum((n - 1) * s for n, s in zip((B, R, S), st)) + L > held:
                raise ValueError(f"y: strides {tuple(st)} put the last row's {L} elements behind the {held} the tensor holds")
            if y.data_ptr() % 8:
                raise ValueError("y must be 8-byte aligned")
            self._launch(C.c_void_p(y.data_ptr()), *st, B, R, S, C.c_void_p(peak.data_ptr()), C.c_void_p(delay.data_ptr()), C.c_void_p(mean.data_ptr()),
                         C.c_void_p(profile.data_ptr() if profile is not None else None))
        detected = arrival = None
        if threshold is not None:
            if self._offset_dev is None:
                self._offset_dev = torch.as_tensor(self._offset_s, dtype=torch.float64).to(dev)
            detected = peak > float(threshold) * mean[..., None]
            arrival = delay.to(torch.float64) / (self.n_fft * self.scs_ra_hz) + self._offset_dev
        return PrachDetection(peak, delay, mean, detected, arrival, profile)
