"""OFDM demodulation and modulation EXTENSION (include/ce_tp.h `ce_ofdm_demodulate`, `ce_ofdmtx_modulate`; the reference
stops at the channel estimate).  ``PuschOfdmDemodulator`` is the step in front of the estimator -- time-domain I/Q samples of
a slot to the resource grid: cyclic-prefix removal, a DFT of length N = 2^n per symbol, the bins around DC onto the grid's
subcarriers, the window advance and the per-symbol phase of TS 38.211 5.4 compensated; one launch on the current stream.

    cp = nr_cp_lengths(30e3, 4096)                                            # 352, 288 x 13
    dem = PuschOfdmDemodulator(4096, 273, cp, window_advance=cp[1] // 2,
                               sym_phasor=nr_symbol_phasors(f0, 30e3, 4096, cp))
    received_rg = dem(samples)                                                # [B, R, >= 61440] -> [B, R, 3276, 14]
    ch_est, noise, *_ = estimate(received_rg, pilots, beta, hop1, hop2, cfg)

``PuschOfdmModulator`` is the transmit direction behind ``PuschModulator`` (and ``PuschTransformPrecoder``), on the same plan:
the grid's subcarriers onto the bins around DC, the transform, the cyclic prefix in front of every symbol; one launch.

    tx = PuschModulator(...)(g, pilots, beta_dmrs, rnti=rnti, n_id=n_id)      # [B, R, 3276, 14], one grid row per port
    samples = PuschOfdmModulator.for_demodulator(dem)(tx)                     # [B, R, 61440]

Out of scope: a layer-to-port precoding matrix (identity: one grid row per port), windowing or overlap-add between symbols,
int16 or fp16 time samples (frequency-domain int16 and block floating point from a 7.2x radio unit: fronthaul.py), a k0 or 7.5 kHz
shift, the time-domain PRACH front end (the detector over frequency-domain rows: prach.py)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, _stage, deprecode

FFT_SIZES = (128, 256, 512, 1024, 2048, 4096)


def min_fft_size(n_prb_grid: int) -> int:
    """The smallest supported transform length that holds ``12 n_prb_grid`` subcarriers."""
    n_sc = 12 * int(n_prb_grid)
    for n in FFT_SIZES:
        if 1 <= n_sc <= n:
            return n
    raise ValueError(f"n_prb_grid={n_prb_grid}: 12 n_prb_grid must lie in 12..{FFT_SIZES[-1]}")


def _mu(scs_hz: float) -> int:
    mu = int(round(np.log2(float(scs_hz) / 15e3)))
    if not 0 <= mu <= 6 or 15e3 * 2 ** mu != float(scs_hz):
        raise ValueError(f"scs_hz={scs_hz} is not 15 kHz times a power of two")
    return mu


def nr_cp_lengths(scs_hz: float, n_fft: int, n_sym: int = 14, slot: int = 0) -> list:
    """Normal cyclic prefix of TS 38.211 5.3.1 in samples at ``fs = scs_hz n_fft``, per symbol of slot `slot` of a subframe:
    ``9 N / 128``, plus ``2^mu N / 128`` for the first symbol of every half subframe, ``(14 slot + l) mod (7 2^mu) == 0``."""
    mu, n_fft = _mu(scs_hz), int(n_fft)
    if n_fft < 128 or n_fft % 128:
        raise ValueError(f"n_fft={n_fft} must be a multiple of 128 for whole-sample cyclic prefixes")
    return [9 * n_fft // 128 + ((n_fft // 128) << mu if (14 * int(slot) + l) % (7 << mu) == 0 else 0) for l in range(int(n_sym))]


def nr_symbol_phasors(f0_hz: float, scs_hz: float, n_fft: int, cp_len: Sequence[int]) -> np.ndarray:
    """complex64 ``[n_sym]``: ``phi_l = exp(-j 2 pi f0 (t_l + cp_l) / fs)`` with ``fs = scs_hz n_fft`` and ``t_l`` the first
    sample of symbol l's cyclic prefix, computed in double and rounded once -- the ``sym_phasor`` of a demodulator.

    The sign is the receiver's: the exponent is negative.  A transmitter that follows TS 38.211 5.4 with the phase of its
    carrier counted from the start of the slot sends symbol l rotated by ``conj(phi_l) = exp(+j 2 pi f0 (t_l + cp_l) / fs)``
    (the pre-compensation of tests/ofdm_oracle.py ``modulate``), and the demodulator's product with ``phi_l`` takes it out.
    For a link that counts the phase the other way round pass ``-f0_hz``."""
    cp = np.asarray(cp_len, np.int64)
    n_fft = int(n_fft)
    start = np.concatenate([[0], np.cumsum(cp + n_fft)[:-1]]) + cp          # t_l + cp_l: the first sample of the useful part
    return np.exp(-2j * np.pi * float(f0_hz) * start.astype(np.float64) / (float(scs_hz) * n_fft)).astype(np.complex64)


def _cp_array(cp_len, n_sym: int):
    cp = [int(c) for c in cp_len]
    if len(cp) != n_sym:
        raise ValueError(f"cp_len holds {len(cp)} lengths for n_sym={n_sym} symbols")
    if any(not -2 ** 31 <= c < 2 ** 31 for c in cp):
        raise ValueError("cp_len does not fit int32")
    return (C.c_int32 * max(n_sym, 1))(*cp)


def derive_host(n_fft: int, n_prb_grid: int, cp_len: Sequence[int], n_sym: int = 14, window_advance: int = 0) -> _lib.TpHostView:
    """Host-only view of what a plan holds (``ce_ofdm_derive_host``; ``m_sc`` holds ``n_fft``); works without a GPU."""
    view = _lib.TpHostView()
    rc = _lib.load().ce_ofdm_derive_host(int(n_fft), int(n_prb_grid), int(n_sym), _cp_array(cp_len, int(n_sym)), int(window_advance), C.byref(view))
    if rc != 0:
        _stage.raise_for(rc)
    return view


def twiddles(n_fft: int) -> np.ndarray:
    """complex64 ``[N]``: the plan's table ``W[n] = exp(+j 2 pi n / N)`` (``ce_ofdm_copy_twiddles``, host only)."""
    if int(n_fft) not in FFT_SIZES:
        raise ValueError(f"n_fft={n_fft} is not one of {FFT_SIZES}")
    w = np.zeros(int(n_fft), np.complex64)
    rc = _lib.load().ce_ofdm_copy_twiddles(int(n_fft), C.c_void_p(w.ctypes.data))
    if rc != 0:
        _stage.raise_for(rc)
    return w


def _row_strides(name: str, t: torch.Tensor, T: int):
    """(slot stride, port stride) in elements of the complex64 rows ``t[B, R, >= T]``, 0 where the dimension has one entry,
    or ``ValueError`` where the last row's T samples lie behind what the tensor's storage holds."""
    B, R = int(t.shape[0]), int(t.shape[1])
    ss, ps = (int(t.stride(0)) if B > 1 else 0), (int(t.stride(1)) if R > 1 else 0)
    if ss < 0 or ps < 0:
        raise ValueError("negative strides are not supported")
    held = t.untyped_storage().nbytes() // 8 - int(t.storage_offset())
    if (B - 1) * ss + (R - 1) * ps + T > held:
        raise ValueError(f"{name}: strides ({ss}, {ps}) put the last row's {T} samples behind the {held} the tensor holds")
    return ss, ps


class _OfdmStage(_stage.Stage):
    """What the demodulator and the modulator share: the validated plan values and the ``ce_ofdm_plan`` made of them."""
    _CREATE, _DESTROY = "ce_ofdm_plan_create", "ce_ofdm_plan_destroy"

    def __init__(self, n_fft: int, n_prb_grid: int, cp_len: Sequence[int], n_sym: int, window_advance: int, sym_phasor, device):
        super().__init__(device)
        self.n_fft, self.n_prb_grid, self.n_sym, self.window_advance = int(n_fft), int(n_prb_grid), int(n_sym), int(window_advance)
        view = derive_host(self.n_fft, self.n_prb_grid, cp_len, self.n_sym, self.window_advance)
        self.cp_len = tuple(int(c) for c in cp_len)
        self.n_sc, self.n_samples = 12 * self.n_prb_grid, sum(self.cp_len) + self.n_sym * self.n_fft
        deprecode._copy_geometry(self, view)
        self.sym_phasor = None
        if sym_phasor is not None:
            phi = np.asarray(sym_phasor.cpu() if isinstance(sym_phasor, torch.Tensor) else sym_phasor)
            if phi.shape != (self.n_sym,) or phi.dtype.kind not in "fc":
                raise ValueError(f"sym_phasor must hold {self.n_sym} complex values, got {phi.dtype} {phi.shape}")
            phi = phi.astype(np.complex64)
            if not np.all(np.isfinite(phi.view(np.float32))):
                raise ValueError(f"sym_phasor[{int(np.flatnonzero(~np.isfinite(phi))[0])}] is not finite")
            self.sym_phasor = phi

    def _create(self, device_index: int, handle) -> int:
        phi = None if self.sym_phasor is None else self.sym_phasor.ctypes.data_as(C.POINTER(C.c_float))
        return self._lib.ce_ofdm_plan_create(_lib.CE_ABI_VERSION, int(device_index), self.n_fft, self.n_prb_grid, self.n_sym,
                                             _cp_array(self.cp_len, self.n_sym), self.window_advance, phi, C.byref(handle))


class PuschOfdmDemodulator(_OfdmStage):
    _LAUNCH = "ce_ofdm_demodulate"
    _NOUN = "the OFDM demodulator"

    def __init__(self, n_fft: int, n_prb_grid: int, cp_len: Sequence[int], n_sym: int = 14, window_advance: int = 0,
                 sym_phasor=None, device=None):
        super().__init__(n_fft, n_prb_grid, cp_len, n_sym, window_advance, sym_phasor, device)

    def __call__(self, samples: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``received_rg[B, R, n_sc, n_sym]`` complex64 on the current stream: the permuted view of the dense
        ``[B, R, n_sym, n_sc]`` buffer the kernel writes (every element, so ``out`` -- that dense buffer -- need not be
        cleared), the layout of ``PuschModulator``'s ``tx`` and the estimator's fast one.  ``samples`` is complex64
        ``[B, R, >= n_samples]`` with a contiguous last dimension; the slot and port strides are free (a view into a longer
        capture), and only the ``n_fft`` samples of each symbol's window are read.  ``out`` may not overlap ``samples``."""
        self._plan()
        dev, T = self.device, self.n_samples
        if not isinstance(samples, torch.Tensor) or samples.device != dev:
            raise ValueError(f"samples must be a tensor on {dev}")
        if samples.dtype != torch.complex64 or samples.dim() != 3 or samples.shape[2] < T or (samples.shape[2] > 1 and samples.stride(2) != 1):
            raise ValueError(f"samples must be a {torch.complex64} tensor [slots, ports, >= {T}] with a contiguous last dimension, got "
                             f"{samples.dtype} {tuple(samples.shape)} with strides {tuple(samples.stride())}")
        B, R = int(samples.shape[0]), int(samples.shape[1])
        shape = (B, R, self.n_sym, self.n_sc)
        if out is None:
            out = torch.empty(shape, dtype=torch.complex64, device=dev)
        else:
            _stage.check_dense("out", out, torch.complex64, shape, dev, "complex64")
        if B == 0 or R == 0:
            return out.permute(0, 1, 3, 2)                       # empty batch: nothing to launch
        ss, ps = _row_strides("samples", samples, T)
        _stage.check_aligned(("out", out))
        self._launch(C.c_void_p(samples.data_ptr()), ss, ps, B, R, C.c_void_p(out.data_ptr()))
        return out.permute(0, 1, 3, 2)


class PuschOfdmModulator(_OfdmStage):
    """The transmit direction (include/ce_tp.h `ce_ofdmtx_modulate`): the resource grid to the samples of a slot -- the
    subcarriers onto the bins around DC, a transform of length N per symbol scaled by 1 / sqrt(N), the cyclic prefix in front.
    ``sym_phasor`` is the DEMODULATOR's (``nr_symbol_phasors``): the modulator applies its conjugate, so a demodulator of the
    same values returns the grid through an ideal channel, whatever its window advance."""
    _LAUNCH = "ce_ofdmtx_modulate"
    _NOUN = "the OFDM modulator"

    def __init__(self, n_fft: int, n_prb_grid: int, cp_len: Sequence[int], n_sym: int = 14, sym_phasor=None, device=None):
        super().__init__(n_fft, n_prb_grid, cp_len, n_sym, 0, sym_phasor, device)

    @classmethod
    def for_demodulator(cls, dem: PuschOfdmDemodulator, device=None) -> "PuschOfdmModulator":
        """The modulator whose samples `dem` turns back into the grid: its transform length, grid width, cyclic prefixes,
        symbol count and phasors (the window advance is the receiver's alone)."""
        if not isinstance(dem, PuschOfdmDemodulator):
            raise ValueError(f"dem must be a PuschOfdmDemodulator, got {type(dem).__name__}")
        return cls(dem.n_fft, dem.n_prb_grid, dem.cp_len, n_sym=dem.n_sym, sym_phasor=dem.sym_phasor,
                   device=device if device is not None else dem._device_arg)

    def __call__(self, grid: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``samples[B, R, n_samples]`` complex64 on the current stream.  ``grid`` is what ``PuschModulator`` and
        ``PuschTransformPrecoder.grid_`` return: the permuted complex64 ``[B, R, n_sc, n_sym]`` view of a dense
        ``[B, R, n_sym, n_sc]`` buffer, one row per port.  ``out`` is a complex64 ``[B, R, >= n_samples]`` tensor with a
        contiguous last dimension; its slot and port strides are free (a view into a longer stream, the ports inside a slot
        or the slots of a port one behind the other) as long as no two rows share a sample.  Only the first ``n_samples``
        samples of each row are written, each exactly once, and they are what is returned; ``out`` may not overlap ``grid``."""
        self._plan()
        dev, T = self.device, self.n_samples
        if not isinstance(grid, torch.Tensor) or grid.device != dev:
            raise ValueError(f"grid must be a tensor on {dev}")
        if (grid.dtype != torch.complex64 or grid.dim() != 4 or tuple(grid.shape[2:]) != (self.n_sc, self.n_sym)
                or not grid.permute(0, 1, 3, 2).is_contiguous()):
            raise ValueError(f"grid must be a {torch.complex64} tensor [slots, ports, {self.n_sc}, {self.n_sym}] (the permuted view of a dense "
                             f"[slots, ports, {self.n_sym}, {self.n_sc}] buffer), got {grid.dtype} {tuple(grid.shape)} with strides {tuple(grid.stride())}")
        B, R = int(grid.shape[0]), int(grid.shape[1])
        if out is None:
            out = torch.empty((B, R, T), dtype=torch.complex64, device=dev)
        elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.complex64 or out.dim() != 3
              or tuple(out.shape[:2]) != (B, R) or out.shape[2] < T or (out.shape[2] > 1 and out.stride(2) != 1)):
            got = f"{out.dtype} {tuple(out.shape)} with strides {tuple(out.stride())} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
            raise ValueError(f"out must be a {torch.complex64} tensor [{B}, {R}, >= {T}] with a contiguous last dimension on {dev}, got {got}")
        if B == 0 or R == 0:
            return out[:, :, :T]                                 # empty batch: nothing to launch
        ss, ps = _row_strides("out", out, T)
        _stage.check_aligned(("grid", grid))
        self._launch(C.c_void_p(grid.data_ptr()), B, R, C.c_void_p(out.data_ptr()), ss, ps)
        return out[:, :, :T]
