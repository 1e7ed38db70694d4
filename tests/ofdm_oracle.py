"""Float64 oracle of the OFDM demodulator (include/ce_tp.h `ce_ofdm_demodulate`), the seeded inputs its GPU tests run on,
and the tolerance rule they follow.

`modulate` is the transmit side the project does not have as a kernel: per symbol an IFFT of length N scaled by sqrt(N)
(unitary) with grid subcarrier k on the signed bin q_k = k - n_sc / 2, and the cyclic prefix in front.  `demodulate_ref`
is the operator of include/ce_tp.h in float64 (`np.fft.fft`, or a literal N x N DFT matrix up to N = 512, so that the
sign and the scale do not lean on a library's convention).  `demodulate_f32` restates the kernel's own float32
arithmetic -- `tpre_oracle.precode_f32` (conjugate, the passes of `tp_oracle.passes_f32` over the radix sequence and
the twiddle table of the library's host entry points, float32(1 / sqrt(N)) in the last pass, conjugate), then at the
store the product with W[(q_k a) mod N] where a != 0 and the product with phi_l where phasors are given, in that order --
only to calibrate the tolerance.

Grids have the estimator's shape [..., n_sc, n_sym]; samples are [..., T], T = sum_l (cp_len[l] + N).

Tolerance rule, per output (eps = 2^-24, rms_window = the rms of the N samples of the output's window):
    |got - ref| <= T_OFDM eps (log2(N) rms_window + |ref|)
A float32 FFT of length N errs in proportion to log2(N) times the rms of its N outputs, which the unitary scale makes
the rms of its inputs; the scaling and the one or two products at the store err in proportion to the output itself.
T_OFDM = 4 C_OFDM_RECORDED, where C_OFDM is the largest ratio of `demodulate_f32`'s own error to that unit over the
inputs of the GPU tests (`CASES`, `advance_inputs`); the factor 4 is tp_oracle's, for FMA contraction and pass-internal
ordering on the GPU that the restatement cannot mirror.  tests/test_ofdm.py re-measures C_OFDM and fails if it exceeds
C_OFDM_RECORDED."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import tpre_oracle as P

EPS = 2.0 ** -24
C_OFDM_RECORDED = 1.25   # measured 0.99 (test_ofdm.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T_OFDM = 4.0 * C_OFDM_RECORDED
MATRIX_MAX = 512          # demodulate_ref(): the explicit matrix up to this N
F = np.float32


# ---- the operator ----

def cp_lengths_ref(scs_hz, n_fft, n_sym=14, slot=0):
    """TS 38.211 5.3.1, normal cyclic prefix, by the standard's own constants: N_cp = 144 kappa 2^-mu, plus 16 kappa for
    symbols 0 and 7 2^mu of a subframe, in units of Tc = 1 / (480 kHz x 4096) with kappa = 64; here in samples at
    fs = scs n_fft, i.e. times n_fft / (2048 kappa 2^-mu)."""
    mu = int(round(np.log2(scs_hz / 15e3)))
    out = []
    for l in range(n_sym):
        tc = 144 * 64 // 2 ** mu + (16 * 64 if (14 * slot + l) % (7 * 2 ** mu) == 0 else 0)
        num = tc * n_fft
        den = 2048 * 64 // 2 ** mu
        assert num % den == 0
        out.append(num // den)
    return out


def symbol_phasors_ref(f0_hz, scs_hz, n_fft, cp_len):
    """phi_l = exp(-j 2 pi f0 (t_l + cp_l) / fs), complex128, by a plain loop."""
    out, t = [], 0
    for c in cp_len:
        out.append(np.exp(-2j * np.pi * f0_hz * (t + c) / (scs_hz * n_fft)))
        t += c + n_fft
    return np.array(out)


def geometry(n_fft, cp_len, advance=0):
    """(window starts w_l, slot length T)."""
    w, t = [], 0
    for c in cp_len:
        w.append(t + c - advance)
        t += c + n_fft
    return w, t


def bins(n_fft, n_sc):
    """(signed bins q_k, FFT bins q_k mod N) of the grid subcarriers k < n_sc."""
    q = np.arange(n_sc) - n_sc // 2
    return q, q % n_fft


def modulate(grid, n_fft, cp_len, sym_phasor=None) -> np.ndarray:
    """complex128 [..., T] of grid [..., n_sc, n_sym]: s_l[n] = N^(-1/2) sum_k conj(phi_l) X[k, l] exp(+j 2 pi q_k n / N),
    n = -cp_l .. N - 1.  `sym_phasor` is the DEMODULATOR's phi_l: the transmitter pre-compensates with its conjugate."""
    grid = np.asarray(grid, np.complex128)
    n_sc, n_sym = grid.shape[-2:]
    assert n_sym == len(cp_len) and n_sc <= n_fft
    _, b = bins(n_fft, n_sc)
    out = []
    for l, c in enumerate(cp_len):
        spec = np.zeros(grid.shape[:-2] + (n_fft,), np.complex128)
        spec[..., b] = grid[..., l] * (1.0 if sym_phasor is None else np.conj(complex(sym_phasor[l])))
        u = np.fft.ifft(spec, axis=-1) * np.sqrt(n_fft)
        out += [u[..., n_fft - c:], u]
    return np.concatenate(out, axis=-1)


def dft_matrix(n_fft) -> np.ndarray:
    k = np.arange(n_fft)
    return np.exp(-2j * np.pi * np.outer(k, k) / n_fft) / np.sqrt(n_fft)


def demodulate_ref(samples, n_fft, n_prb_grid, cp_len, advance=0, sym_phasor=None, matrix=None) -> np.ndarray:
    """complex128 [..., n_sc, n_sym] of samples [..., >= T]: the formula of include/ce_tp.h in float64.
    `matrix`: True = the explicit N x N matrix, False = np.fft.fft, None = the matrix up to MATRIX_MAX."""
    s = np.asarray(samples).astype(np.complex128)
    n_sc = 12 * n_prb_grid
    w, T = geometry(n_fft, cp_len, advance)
    assert s.shape[-1] >= T
    q, b = bins(n_fft, n_sc)
    if matrix is None:
        matrix = n_fft <= MATRIX_MAX
    comp = np.exp(2j * np.pi * q * advance / n_fft)
    out = np.empty(s.shape[:-1] + (n_sc, len(cp_len)), np.complex128)
    for l, w_l in enumerate(w):
        x = s[..., w_l:w_l + n_fft]
        y = x @ dft_matrix(n_fft).T if matrix else np.fft.fft(x, axis=-1) / np.sqrt(n_fft)
        out[..., l] = (1.0 if sym_phasor is None else complex(sym_phasor[l])) * comp * y[..., b]
    return out


def window_rms(samples, n_fft, cp_len, advance=0) -> np.ndarray:
    """[..., 1, n_sym]: the rms of each window's N samples (broadcasts against a grid)."""
    s = np.asarray(samples).astype(np.complex128)
    w, _ = geometry(n_fft, cp_len, advance)
    return np.stack([np.sqrt(np.mean(np.abs(s[..., w_l:w_l + n_fft]) ** 2, -1)) for w_l in w], -1)[..., None, :]


# ---- the kernel's arithmetic in float32 numpy ----

def _cmul_f32(vr, vi, wr, wi):
    return ((vr * wr).astype(F) - (vi * wi).astype(F)).astype(F), ((vr * wi).astype(F) + (vi * wr).astype(F)).astype(F)


def demodulate_f32(samples, view, tw, n_prb_grid, cp_len, advance=0, sym_phasor=None) -> np.ndarray:
    """complex64 [..., n_sc, n_sym].  `view`: the library's host view (m_sc = N); `tw`: its twiddle table (complex64 [N])."""
    N, n_sc = int(view.m_sc), 12 * n_prb_grid
    s = np.asarray(samples).astype(np.complex64)
    lead = s.shape[:-1]
    w, _ = geometry(N, cp_len, advance)
    rows = np.stack([s[..., w_l:w_l + N] for w_l in w], -2).reshape(-1, len(w) * N)      # [items, n_sym N]
    y = P.precode_f32(rows, view, tw).reshape(-1, len(w), N)
    q, b = bins(N, n_sc)
    vr, vi = y[..., b].real.astype(F), y[..., b].imag.astype(F)                            # [items, n_sym, n_sc]
    if advance:
        c = tw[(q * advance) % N]                                                          # integer index arithmetic
        vr, vi = _cmul_f32(vr, vi, c.real.astype(F), c.imag.astype(F))
    if sym_phasor is not None:
        phi = np.asarray(sym_phasor).astype(np.complex64)[None, :, None]
        vr, vi = _cmul_f32(vr, vi, phi.real.astype(F), phi.imag.astype(F))
    assert vr.dtype == F and vi.dtype == F
    out = np.empty(vr.shape, np.complex64)
    out.real, out.imag = vr, vi
    return np.swapaxes(out, -1, -2).reshape(lead + (n_sc, len(w)))


# ---- the rule ----

def ratio(got, ref, rms, n_fft) -> float:
    unit = EPS * (np.log2(n_fft) * rms + np.abs(ref))
    return float((np.abs(np.asarray(got).astype(np.complex128) - ref) / unit).max())


def check(got, ref, rms, n_fft, what="", t=None) -> float:
    """The comparison every GPU test uses.  Prints the largest error ratio first and returns it."""
    t = T_OFDM if t is None else t
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    r = ratio(got, ref, rms, n_fft)
    print(f"{what}: max |y - ref| / (2^-24 (log2(N) rms_window + |ref|)) = {r:.2f}  (bound {t:g})")
    assert r <= t, f"{what}: error ratio {r:.2f} > {t:g}"
    return r


# ---- inputs ----

def _case(name, n_fft, n_prb_grid, scs, n_sym=14, slot=0, advance=0, phasor=False, B=2, R=3):
    return dict(name=name, n_fft=n_fft, n_prb_grid=n_prb_grid, scs=scs, n_sym=n_sym, slot=slot, advance=advance, phasor=phasor, B=B, R=R)


# (threads per row, rows per workgroup) = (64, 4) at N <= 256, (128, 2) at 512 and 1024, (256, 1) above; n_sym = 14 leaves
# the last workgroup of a (slot, port) half empty at 4 rows, n_sym = 1 at 2 rows
CASES = [
    _case("n128_p10_15k_a0", 128, 10, 15e3),                                      # cyclic prefixes 10, 9 x 6, 10, 9 x 6: odd window offsets
    _case("n128_p10_15k_a4", 128, 10, 15e3, advance=4, phasor=True),
    _case("n128_p1", 128, 1, 30e3, n_sym=12, advance=9, phasor=True),             # one PRB: 6 + 6 bins, the whole prefix as advance
    _case("n256_p21", 256, 21, 30e3, phasor=True),                                # n_sc = 252 of 256
    _case("n512_p24_s1", 512, 24, 30e3, n_sym=1, advance=22),                     # two rows per workgroup, one of them inactive
    _case("n512_p24_120k_slot1", 512, 24, 120e3, slot=1, advance=5, phasor=True),  # every prefix 36
    _case("n512_p24_120k_slot4", 512, 24, 120e3, slot=4),                         # the half-subframe boundary: 68, 36 x 13
    _case("n1024_p52", 1024, 52, 30e3, n_sym=12, advance=30, phasor=True),
    _case("n2048_p106_15k", 2048, 106, 15e3, advance=72, B=1, R=2),
    _case("n4096_p273", 4096, 273, 30e3, advance=144, phasor=True, B=1, R=2),
    _case("n4096_p341_s12", 4096, 341, 30e3, n_sym=12, B=1, R=1),                # n_sc = 4092 of 4096
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
CASE_NAMES = [c["name"] for c in CASES]


def _freeze(d, *names):
    for n in names:
        a = getattr(d, n)
        if a is not None:
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(name):
    """A case's white complex64 samples [B, R, T] (every bin carries energy, the unstored ones too), unit-modulus phasors
    at seeded angles where the case has them, ref = demodulate_ref in float64 and the window rms; shared and read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(21000 + CASES.index(c))
    cp = cp_lengths_ref(c["scs"], c["n_fft"], c["n_sym"], c["slot"])
    _, T = geometry(c["n_fft"], cp, c["advance"])
    s = (rng.standard_normal((c["B"], c["R"], T)) + 1j * rng.standard_normal((c["B"], c["R"], T))).astype(np.complex64)
    phi = np.exp(2j * np.pi * rng.random(c["n_sym"])).astype(np.complex64) if c["phasor"] else None
    d = SimpleNamespace(c=c, name=name, cp=cp, T=T, samples=s, phi=phi, n_sc=12 * c["n_prb_grid"],
                        ref=demodulate_ref(s, c["n_fft"], c["n_prb_grid"], cp, c["advance"], phi),
                        rms=window_rms(s, c["n_fft"], cp, c["advance"]))
    return _freeze(d, "samples", "phi", "ref", "rms")


ADVANCE_N, ADVANCE_PRB, ADVANCE_SCS = 256, 20, 30e3


@functools.lru_cache(maxsize=None)
def advance_inputs():
    """An oracle-modulated signal (a seeded complex grid X [2, 2, 240, 14] with phasors) through a four-tap integer-delay
    channel by linear convolution, taps inside min cp_len - a for a = cp / 2: samples64 complex128, samples complex64 (what
    the GPU gets), H X in float64."""
    rng = np.random.default_rng(22000)
    N, n_prb = ADVANCE_N, ADVANCE_PRB
    cp = cp_lengths_ref(ADVANCE_SCS, N)
    a = min(cp) // 2
    X = rng.standard_normal((2, 2, 12 * n_prb, 14)) + 1j * rng.standard_normal((2, 2, 12 * n_prb, 14))
    phi = symbol_phasors_ref(7.3e3, ADVANCE_SCS, N, cp)
    taps = np.array([1.0, 0.4j, 0.0, -0.2, 0.1 + 0.1j])
    assert len(taps) - 1 < min(cp) - a
    s = modulate(X, N, cp, phi)
    y = np.apply_along_axis(lambda v: np.convolve(v, taps)[:v.shape[0]], -1, s)
    _, b = bins(N, 12 * n_prb)
    hx = np.fft.fft(taps, N)[b][None, None, :, None] * X
    d = SimpleNamespace(N=N, n_prb=n_prb, cp=cp, a=a, X=X, phi=phi.astype(np.complex64), taps=taps, samples64=y, samples=y.astype(np.complex64), hx=hx)
    return _freeze(d, "X", "phi", "samples64", "samples", "hx")
