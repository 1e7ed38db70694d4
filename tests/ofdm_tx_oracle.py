"""Oracle of the OFDM modulator (include/ce_tp.h `ce_ofdmtx_modulate`, `PuschOfdmModulator`), the seeded inputs its GPU tests
run on, and the tolerance rule they follow.

The float64 reference is `ofdm_oracle.modulate`.  `modulate_f32` restates the kernel's float32 arithmetic -- the product with
(phi_l.re, -phi_l.im) where phasors are given, the scatter of the n_sc subcarriers onto the bins q_k mod N with zeros in the
other N - n_sc, the passes of `tp_oracle.passes_f32` over the radix sequence and the twiddle table of the library's host
entry points (the inverse transform natively: no conjugation), float32(1 / sqrt(N)) in the last pass, the cyclic prefix as a
copy of the symbol's tail -- only to calibrate the tolerance.

Grids have the estimator's shape [..., n_sc, n_sym]; samples are [..., T], T = sum_l (cp_len[l] + N).

Tolerance rule, per sample of symbol l (eps = 2^-24, rms_l = the rms of the N useful samples of the reference symbol):
    |got - ref| <= T_TX eps (log2(N) rms_l + |ref|)
the form of ofdm_oracle's: a float32 FFT of length N errs in proportion to log2(N) times the rms of its N outputs, the product
in front of it and the scaling behind it in proportion to the value itself.  T_TX = 4 C_TX_RECORDED, where C_TX is the largest
ratio of `modulate_f32`'s own error to that unit over the inputs of the GPU tests (`inputs` over ofdm_oracle.CASES); the factor
4 is tp_oracle's, for FMA contraction and pass-internal ordering on the GPU that the restatement cannot mirror.
tests/test_ofdm_tx.py re-measures C_TX and fails if it exceeds C_TX_RECORDED."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import ofdm_oracle as O
import tp_oracle as T

EPS = O.EPS
C_TX_RECORDED = 1.0      # measured 0.89 (test_ofdm_tx.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T_TX = 4.0 * C_TX_RECORDED
F = np.float32
CASES, CASE_BY_NAME, CASE_NAMES = O.CASES, O.CASE_BY_NAME, O.CASE_NAMES      # the demodulator's: N, n_prb_grid, scs, n_sym, slot, phasor, B, R


def symbol_starts(n_fft, cp_len):
    """(t_l, the first sample of symbol l's cyclic prefix; T)."""
    t, out = 0, []
    for c in cp_len:
        out.append(t)
        t += c + n_fft
    return out, t


def symbol_of_sample(n_fft, cp_len) -> np.ndarray:
    """int [T]: the symbol each sample of a slot belongs to."""
    return np.repeat(np.arange(len(cp_len)), [c + n_fft for c in cp_len])


def symbol_rms(ref, n_fft, cp_len) -> np.ndarray:
    """[..., T]: per sample the rms of the N useful samples of its symbol in `ref` [..., T]."""
    ref = np.asarray(ref).astype(np.complex128)
    starts, _ = symbol_starts(n_fft, cp_len)
    rms = np.stack([np.sqrt(np.mean(np.abs(ref[..., t + c:t + c + n_fft]) ** 2, -1)) for t, c in zip(starts, cp_len)], -1)   # [..., n_sym]
    return rms[..., symbol_of_sample(n_fft, cp_len)]


# ---- the kernel's arithmetic in float32 numpy ----

def modulate_f32(grid, view, tw, cp_len, sym_phasor=None) -> np.ndarray:
    """complex64 [..., T] of grid [..., n_sc, n_sym].  `view`: the library's host view (m_sc = N); `tw`: its twiddle table
    (complex64 [N])."""
    N = int(view.m_sc)
    radix = [int(r) for r in view.radix[:view.n_passes]]
    grid = np.asarray(grid).astype(np.complex64)
    n_sc, n_sym = grid.shape[-2:]
    lead = grid.shape[:-2]
    assert n_sym == len(cp_len) and n_sc <= N
    x = np.swapaxes(grid, -1, -2).reshape(-1, n_sym, n_sc)                                 # [items, n_sym, n_sc]
    xr, xi = x.real.astype(F), x.imag.astype(F)
    if sym_phasor is not None:                                                             # 1. conj(phi_l): the sign flip is exact
        phi = np.asarray(sym_phasor).astype(np.complex64)[None, :, None]
        xr, xi = O._cmul_f32(xr, xi, phi.real.astype(F), (-phi.imag).astype(F))
    _, b = O.bins(N, n_sc)
    re, im = np.zeros((x.shape[0], n_sym, N), F), np.zeros((x.shape[0], n_sym, N), F)      # 2. the scatter; the other bins are zero
    re[..., b], im[..., b] = xr, xi
    scale = F(1.0 / np.sqrt(float(N)))                                                     # in double, rounded once
    re, im = T.passes_f32(re.reshape(-1, N), im.reshape(-1, N), radix, tw, scale)          # 3., 4.
    u = np.empty(re.shape, np.complex64)
    u.real, u.imag = re, im
    u = u.reshape(-1, n_sym, N)
    out = []
    for l, c in enumerate(cp_len):                                                         # 5. the prefix: the tail a second time
        out += [u[:, l, N - c:], u[:, l]]
    return np.concatenate(out, axis=-1).reshape(lead + (-1,))


# ---- the rule ----

def ratio(got, ref, rms, n_fft) -> float:
    unit = EPS * (np.log2(n_fft) * rms + np.abs(ref))
    return float((np.abs(np.asarray(got).astype(np.complex128) - ref) / unit).max())


def check(got, ref, rms, n_fft, what="", t=None) -> float:
    """The comparison every GPU test uses.  Prints the largest error ratio first and returns it."""
    t = T_TX if t is None else t
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), f"{what}: non-finite output"
    r = ratio(got, ref, rms, n_fft)
    print(f"{what}: max |s - ref| / (2^-24 (log2(N) rms_symbol + |ref|)) = {r:.2f}  (bound {t:g})")
    assert r <= t, f"{what}: error ratio {r:.2f} > {t:g}"
    return r


# ---- inputs ----

@functools.lru_cache(maxsize=None)
def inputs(name):
    """A case's seeded complex-normal complex64 grid [B, R, n_sc, n_sym], unit-modulus phasors at seeded angles where the case
    has them, ref = ofdm_oracle.modulate in float64 [B, R, T] and the per-sample symbol rms; shared and read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(23000 + CASES.index(c))
    N, n_sc = c["n_fft"], 12 * c["n_prb_grid"]
    cp = O.cp_lengths_ref(c["scs"], N, c["n_sym"], c["slot"])
    starts, T_ = symbol_starts(N, cp)
    shape = (c["B"], c["R"], n_sc, c["n_sym"])
    grid = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    phi = np.exp(2j * np.pi * rng.random(c["n_sym"])).astype(np.complex64) if c["phasor"] else None
    ref = O.modulate(grid, N, cp, phi)
    d = SimpleNamespace(c=c, name=name, cp=cp, T=T_, starts=starts, n_sc=n_sc, grid=grid, phi=phi, ref=ref, rms=symbol_rms(ref, N, cp))
    return O._freeze(d, "grid", "phi", "ref", "rms")
