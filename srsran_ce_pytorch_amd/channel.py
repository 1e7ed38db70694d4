"""Time-domain channel emulator EXTENSION (include/ce_tp.h `ce_chan_apply`; the reference stops at the channel estimate): what
lies between ``PuschOfdmModulator`` and ``PuschOfdmDemodulator`` -- a FIR channel from the transmit to the receive ports, a
carrier frequency offset from a numerically controlled oscillator and seeded white Gaussian noise; one launch on the current
stream, no plan.

    ch = PuschChannelEmulator(n_tx=1, n_rx=4, n_taps=12)
    h = torch.as_tensor(taps_from_delays([0, 100e-9, 300e-9], [1, 0.5, 0.2], fs, 12))      # one tx-rx pair; [1, R, P, K] in all
    rx = ch(samples, taps, cfo=cfo_word(350.0, fs), sigma=0.05, seed=7, first_slot=slot)  # [B, 1, T] -> [B, 4, T]
    received_rg = dem(rx)

For slot b, receive port r, sample t:  ``y[b][r][t] = exp(j 2 pi w_b(t) / 2^32) sum_p sum_k h[b][r][p][k] x[b][p][t - k] +
sigma_b n[b][r][t]`` with ``w_b(t) = (phase0_b + cfo_b t) mod 2^32`` and ``x[b][p][t - k] = 0`` for ``t < k``: each slot row is
convolved on its own.  The noise of a sample depends on ``(seed, first_slot + b, r, t)`` alone (Philox4x32-10, counter based),
so a slot run on its own with ``first_slot = b`` reproduces its row of the batch bit for bit.

Out of scope: taps that vary inside a slot (Doppler), tails carried from one slot into the next, fixed-point samples, a
sample-rate offset, coloured noise or interference."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, _stage
from .ofdm import _row_strides

MAX_TAPS, MAX_TX = 128, 4
SINC_HALF_WIDTH, SINC_KAISER_BETA = 8, 6.0
SINC_RIPPLE, SINC_BAND = 1e-3, 0.3          # taps_from_delays: the stated accuracy and the band it holds over (cycles per sample)


def cfo_word(f_hz: float, sample_rate: float) -> int:
    """The frequency control word of `f_hz` at `sample_rate`: ``round(f_hz / sample_rate 2^32)`` as a signed 32-bit value, the
    unit being ``2^-32`` cycles per sample.  ``ValueError`` outside +-half the sample rate (the word would wrap)."""
    fs, f = float(sample_rate), float(f_hz)
    if not (math.isfinite(fs) and fs > 0.0) or not math.isfinite(f):
        raise ValueError(f"cfo_word: f_hz={f_hz}, sample_rate={sample_rate} must be finite, the rate positive")
    word = int(round(f / fs * 2.0 ** 32))
    if not -2 ** 31 <= word <= 2 ** 31 - 1:
        raise ValueError(f"cfo_word: f_hz={f_hz} outside +-half the sample rate {sample_rate}")
    return word


def cfo_hz(word: int, sample_rate: float) -> float:
    """The frequency a control word stands for: ``word 2^-32 sample_rate``."""
    return int(word) * 2.0 ** -32 * float(sample_rate)


def taps_from_delays(delays_s: Sequence[float], gains: Sequence[complex], sample_rate: float, n_taps: int) -> np.ndarray:
    """complex64 ``[n_taps]``: the FIR of the paths ``gains[i] delta(t - delays_s[i])`` at `sample_rate`, each path a
    windowed-sinc fractional-delay filter ``g sinc(k - d) kaiser(k - d)`` with ``d = delay sample_rate`` in samples, the Kaiser
    window of beta = 6 over ``|k - d| <= 8`` samples.  An integer `d` gives the unit tap ``g`` at ``k = d`` exactly.  By Kaiser's
    design formulas the window's ripple is 63 dB down (7e-4) and the transition around Nyquist 0.24 cycles per sample wide
    (0.38 .. 0.62), so a path's response is ``g exp(-j 2 pi f d)`` to within 1e-3 |g| (``SINC_RIPPLE``) for ``|f| <= 0.3`` cycles
    per sample (``SINC_BAND``; a 24-PRB grid in a 512-point transform occupies +-0.28) -- where the whole
    window lies inside the taps, ``8 <= d <= n_taps - 9``; closer to either end the path loses the coefficients that fall
    outside ``0 .. n_taps - 1`` (add a common delay to every path where that matters).  A delay outside ``0 .. n_taps - 1``
    samples is refused.  Computed in double, rounded once."""
    d = np.atleast_1d(np.asarray(delays_s, np.float64)) * float(sample_rate)
    g = np.atleast_1d(np.asarray(gains, np.complex128))
    n_taps = int(n_taps)
    if not 1 <= n_taps <= MAX_TAPS:
        raise ValueError(f"n_taps={n_taps} outside 1..{MAX_TAPS}")
    if d.ndim != 1 or d.shape != g.shape or d.size == 0:
        raise ValueError(f"delays_s and gains must hold the same number (>= 1) of paths, got {d.shape} and {g.shape}")
    if not np.all(np.isfinite(d)) or not np.all(np.isfinite(g)):
        raise ValueError("delays_s and gains must be finite")
    if d.min() < 0.0 or d.max() > n_taps - 1:
        raise ValueError(f"a delay of {d.min() if d.min() < 0 else d.max():g} samples lies outside 0..{n_taps - 1}")
    u = np.arange(n_taps, dtype=np.float64)[None, :] - d[:, None]                     # [path, tap]: k - d
    inside = np.abs(u) <= SINC_HALF_WIDTH
    win = np.where(inside, np.i0(SINC_KAISER_BETA * np.sqrt(np.where(inside, 1.0 - (u / SINC_HALF_WIDTH) ** 2, 0.0))) / np.i0(SINC_KAISER_BETA), 0.0)
    sinc = np.where(u == np.rint(u), (u == 0.0).astype(np.float64), np.sinc(u))      # exact zeros at the other integers
    return (g[:, None] * sinc * win).sum(0).astype(np.complex64)


class PuschChannelEmulator:
    """``n_tx`` (1..4) transmit ports, ``n_rx`` receive ports, ``n_taps`` (1..128) taps per pair; validated on construction (no
    GPU needed), bound to its device at the first call."""

    _NOUN = "the channel emulator"

    def __init__(self, n_tx: int, n_rx: int, n_taps: int, device=None):
        for name, v in (("n_tx", n_tx), ("n_rx", n_rx), ("n_taps", n_taps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an int, got {type(v).__name__}")
        self.n_tx, self.n_rx, self.n_taps = int(n_tx), int(n_rx), int(n_taps)
        if not 1 <= self.n_tx <= MAX_TX:
            raise ValueError(f"n_tx={self.n_tx} outside 1..{MAX_TX}")
        if not 1 <= self.n_rx <= 2 ** 31 - 1:
            raise ValueError(f"n_rx={self.n_rx} must be >= 1")
        if not 1 <= self.n_taps <= MAX_TAPS:
            raise ValueError(f"n_taps={self.n_taps} outside 1..{MAX_TAPS}")
        self._lib = _lib.load()
        self._device_arg = device
        self.device: Optional[torch.device] = None

    def _bind(self) -> torch.device:
        if self.device is None:
            device = self._device_arg
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError(f"{self._NOUN} runs on a ROCm GPU only (no CPU fallback)")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self.device = device
        return self.device

    def __call__(self, samples: torch.Tensor, taps: torch.Tensor, cfo=None, phase0=0, sigma=None, seed: int = 0, first_slot: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``y[B, n_rx, T]`` complex64 on the current stream.

        ``samples``  complex64 ``[B, n_tx, T]`` with a contiguous last dimension; the slot and port strides are free (a view
                     into a longer stream, as ``PuschOfdmModulator(out=)`` writes it).
        ``taps``     complex64 ``[B, n_rx, n_tx, n_taps]``, or ``[1, n_rx, n_tx, n_taps]`` for one channel for the whole batch; dense.
        ``cfo``      ``None`` (no rotation at all), or the frequency control word (``cfo_word``): an int in the int32 range for
                     the whole batch or an int32 device tensor ``[B]``.  ``phase0``: the phase word at sample 0 of every row,
                     an int in ``0 .. 2^32 - 1`` or an int32 device tensor ``[B]`` holding the 32 bits; ignored without ``cfo``.
        ``sigma``    ``None`` (no noise, no generator call), a float ``>= 0`` or a float32 device tensor ``[B]``: the noise's
                     standard deviation, ``E |sigma n|^2 = sigma^2`` per complex sample.
        ``seed``     ``0 .. 2^64 - 1``; ``first_slot``: the slot number of ``samples[0]``, an int64.
        ``out``      complex64 ``[B, n_rx, >= T]`` with a contiguous last dimension and free strides, as long as no two rows
                     share a sample; only ``[0, T)`` of each row is written and returned.  It may not overlap ``samples`` or ``taps``."""
        dev = self._bind()
        P, R, K = self.n_tx, self.n_rx, self.n_taps
        if not isinstance(samples, torch.Tensor) or samples.device != dev:
            raise ValueError(f"samples must be a tensor on {dev}")
        if (samples.dtype != torch.complex64 or samples.dim() != 3 or samples.shape[1] != P or samples.shape[2] < 1
                or (samples.shape[2] > 1 and samples.stride(2) != 1)):
            raise ValueError(f"samples must be a {torch.complex64} tensor [slots, {P}, >= 1] with a contiguous last dimension, got "
                             f"{samples.dtype} {tuple(samples.shape)} with strides {tuple(samples.stride())}")
        B, T = int(samples.shape[0]), int(samples.shape[2])
        if (not isinstance(taps, torch.Tensor) or taps.device != dev or taps.dtype != torch.complex64 or taps.dim() != 4
                or tuple(taps.shape[1:]) != (R, P, K) or taps.shape[0] not in (1, B) or not taps.is_contiguous()):
            got = f"{taps.dtype} {tuple(taps.shape)} with strides {tuple(taps.stride())} on {taps.device}" if isinstance(taps, torch.Tensor) else type(taps).__name__
            raise ValueError(f"taps must be a dense {torch.complex64} tensor [{B} or 1, {R}, {P}, {K}] on {dev}, got {got}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed={seed!r} outside 0..2^64-1")
        if isinstance(first_slot, bool) or not isinstance(first_slot, (int, np.integer)) or not -2 ** 63 <= int(first_slot) < 2 ** 63:
            raise ValueError(f"first_slot={first_slot!r} outside the int64 range")
        fcw = ph = sg = None
        if cfo is not None:
            fcw = _stage.batch_param("cfo", cfo, B, dev, -2 ** 31, 2 ** 31 - 1)
            if not isinstance(phase0, torch.Tensor):
                if isinstance(phase0, bool) or not isinstance(phase0, (int, np.integer)) or not 0 <= int(phase0) < 2 ** 32:
                    raise ValueError(f"phase0={phase0!r} outside 0..2^32-1")
                phase0 = int(phase0) - (2 ** 32 if int(phase0) >= 2 ** 31 else 0)      # the 32 bits as an int32
            ph = _stage.batch_param("phase0", phase0, B, dev, -2 ** 31, 2 ** 31 - 1)
        if sigma is not None:
            if isinstance(sigma, torch.Tensor):
                if sigma.dtype != torch.float32 or sigma.dim() != 1 or sigma.shape[0] != B or sigma.device != dev:
                    raise ValueError(f"sigma: a tensor must be float32 of shape [{B}] on {dev}, got {sigma.dtype} {tuple(sigma.shape)} on {sigma.device}")
                if sigma.stride(0) < 0:
                    raise ValueError("negative strides are not supported")
                sg = sigma
            else:
                if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)):
                    raise ValueError(f"sigma: expected a float or a float32 device tensor of shape [{B}]")
                if not math.isfinite(float(sigma)) or float(sigma) < 0.0:
                    raise ValueError(f"sigma={float(sigma)} must be finite and >= 0")
                sg = torch.tensor([float(sigma)], dtype=torch.float32).to(dev)
        if out is None:
            out = torch.empty((B, R, T), dtype=torch.complex64, device=dev)
        elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.complex64 or out.dim() != 3
              or tuple(out.shape[:2]) != (B, R) or out.shape[2] < T or (out.shape[2] > 1 and out.stride(2) != 1)):
            got = f"{out.dtype} {tuple(out.shape)} with strides {tuple(out.stride())} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
            raise ValueError(f"out must be a {torch.complex64} tensor [{B}, {R}, >= {T}] with a contiguous last dimension on {dev}, got {got}")
        if B == 0:
            return out[:, :, :T]                                 # empty batch: nothing to launch
        xss, xps = _row_strides("samples", samples, T)
        yss, yps = _row_strides("out", out, T)

        def arg(t):
            return (None, 0) if t is None else (C.c_void_p(t.data_ptr()), _stage.batch_stride(t))

        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = self._lib.ce_chan_apply(_lib.CE_ABI_VERSION, C.c_void_p(samples.data_ptr()), xss, xps, B, P, R, T, C.c_void_p(taps.data_ptr()),
                                         0 if taps.shape[0] == 1 else R * P * K, K, *arg(fcw), *arg(ph), *arg(sg), int(seed), int(first_slot),
                                         C.c_void_p(out.data_ptr()), yss, yps, C.c_void_p(stream))
        if rc != 0:
            _stage.raise_for(rc)
        return out[:, :, :T]
