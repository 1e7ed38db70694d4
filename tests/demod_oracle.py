"""Float64 oracle of the soft-demapper extension (include/ce_demod.h), the seeded inputs the GPU tests run on, and the
tolerance rule both follow.

The oracle builds the constellations from the formulas of TS 38.211 5.1.3 - 5.1.6 and takes, per bit, the brute-force
minimum of |y - s|^2 over all 2^Qm points with that bit value -- independent of the kernel's per-axis closed form.  The
scrambling sequence is `gold_bits` of tests/dmrs_oracle.py (both recurrences stepped from n = 0).

Tolerance rule, per LLR of bit j of a symbol (y_ax = Re y for even j, Im y for odd j; a_max = the modulation's largest
axis level; all from the float32 inputs promoted to float64, so input rounding is not part of the error):
    |llr - ref| <= T 2^-24 (|y_ax| + a_max)^2 / nvar
The numerator of an LLR is 2 y_ax (s0 - s1) + s1^2 - s0^2 per axis: a float32 evaluation errs in proportion to
(|y_ax| + a_max)^2 / nvar.  T = 4 C, where C is the largest ratio of `llr_f32`'s own error (the kernel's closed form in
float32 numpy) to 2^-24 (|y_ax| + a_max)^2 / nvar over the inputs of the GPU tests; the factor 4 covers FMA contraction
and the division on the GPU.  tests/test_demod.py re-measures C and fails if it exceeds C_RECORDED.
int8 output q with scale = llr_scale:  |q - clamp(ref scale, -127, 127)| <= 0.5 + scale tol  (rounding ties are left open)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from dmrs_oracle import gold_bits

EPS = 2.0 ** -24
C_RECORDED = 3.0     # measured 2.66 (test_demod.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T = 4.0 * C_RECORDED

NORM = {2: 2.0, 4: 10.0, 6: 42.0, 8: 170.0}
BIG_M = 273 * 12 * 13 * 4


def constellation(qm: int) -> np.ndarray:
    """complex128 [2^Qm]: the point of the bit tuple (b0, b1, ...) at index sum_j b_j 2^j (38.211 5.1.3 - 5.1.6)."""
    pts = np.zeros(1 << qm, np.complex128)
    for idx in range(1 << qm):
        b = [(idx >> j) & 1 for j in range(qm)]
        s = lambda j: 1 - 2 * b[j]   # noqa: E731
        if qm == 2:
            re, im = s(0), s(1)
        elif qm == 4:
            re, im = s(0) * (2 - s(2)), s(1) * (2 - s(3))
        elif qm == 6:
            re, im = s(0) * (4 - s(2) * (2 - s(4))), s(1) * (4 - s(3) * (2 - s(5)))
        else:
            re, im = s(0) * (8 - s(2) * (4 - s(4) * (2 - s(6)))), s(1) * (8 - s(3) * (4 - s(5) * (2 - s(7))))
        pts[idx] = complex(re, im) / np.sqrt(NORM[qm])
    return pts


def a_max(qm: int) -> float:
    return ((1 << (qm // 2)) - 1) / np.sqrt(NORM[qm])


def modulate(bits: np.ndarray, qm: int) -> np.ndarray:
    """bits [..., n * Qm] (0 / 1) -> complex128 [..., n]."""
    b = np.asarray(bits).reshape(bits.shape[:-1] + (-1, qm)).astype(np.int64)
    return constellation(qm)[(b << np.arange(qm)).sum(-1)]


def usable(x, nvar) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.isfinite(nvar) & (nvar > 0) & np.isfinite(x.real) & np.isfinite(x.imag)


def llr_ref(x, nvar, qm: int, chunk: int = 1 << 10) -> np.ndarray:
    """float64 [B, M * Qm] from x [B, ...] complex and nvar [B, ...]: brute-force minima over all points; erasures are 0."""
    B = x.shape[0]
    y = np.asarray(x).reshape(-1).astype(np.complex128)
    nv = np.asarray(nvar).reshape(-1).astype(np.float64)
    ok = usable(y, nv)
    y, nv = np.where(ok, y, 0.0), np.where(ok, nv, 1.0)
    pts = constellation(qm)
    idx = np.arange(1 << qm)
    sets = [(np.flatnonzero((idx >> j) & 1 == 1), np.flatnonzero((idx >> j) & 1 == 0)) for j in range(qm)]
    out = np.zeros((len(y), qm))
    for i in range(0, len(y), chunk):
        yc = y[None, i:i + chunk]
        d2 = (yc.real - pts.real[:, None]) ** 2 + (yc.imag - pts.imag[:, None]) ** 2          # [point, symbol]
        for j, (one, zero) in enumerate(sets):
            out[i:i + chunk, j] = (d2[one].min(0) - d2[zero].min(0)) / nv[i:i + chunk]
    out[~ok] = 0.0
    return out.reshape(B, -1)


def unit_tolerance(x, nvar, qm: int) -> np.ndarray:
    """2^-24 (|y_ax| + a_max)^2 / nvar per LLR [B, M * Qm]; 0 at erasures (exact zeros there)."""
    B = x.shape[0]
    y = np.asarray(x).reshape(-1).astype(np.complex128)
    nv = np.asarray(nvar).reshape(-1).astype(np.float64)
    ok = usable(y, nv)
    y, nv = np.where(ok, y, 0.0), np.where(ok, nv, 1.0)
    ax = np.stack([np.abs(y.real), np.abs(y.imag)] * (qm // 2), -1)                      # even bits: real axis, odd: imaginary
    tol = EPS * (ax + a_max(qm)) ** 2 / nv[:, None]
    tol[~ok] = 0.0
    return tol.reshape(B, -1)


def llr_f32(x, nvar, qm: int) -> np.ndarray:
    """The per-axis closed form of include/ce_demod.h in float32 numpy -- only to calibrate the tolerance."""
    f = np.float32
    B = x.shape[0]
    y = np.asarray(x).reshape(-1).astype(np.complex64)
    nv = np.asarray(nvar).reshape(-1).astype(f)
    m = qm // 2
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_a, g = f(np.sqrt(NORM[qm])), (f(1) / f(NORM[qm])) / nv
    out = np.zeros((len(y), qm), f)
    for axis, ya in enumerate((y.real.astype(f), y.imag.astype(f))):
        v = (ya * inv_a).astype(f)
        for k in range(m):
            K = (1 << (m - k)) - 1
            av = np.abs(v)
            if K == 1:
                fk = f(4) * av
            else:
                s = np.minimum(f(2) * np.floor(f(0.5) * av) + f(1), f(K)).astype(f)
                fk = ((s + f(1)) * (f(2) * av + f(1) - s)).astype(f)
            out[:, 2 * k + axis] = (np.copysign(fk, v) * g).astype(f)
            v = (f((K + 1) // 2) - av).astype(f)
    assert out.dtype == f
    return out.reshape(B, -1)


def quantise_ref(ref, scale) -> np.ndarray:
    return np.clip(np.asarray(ref, np.float64) * float(scale), -127.0, 127.0)


def check(got, ref, tol_unit, what="", scale=None, t=None) -> float:
    """The comparison every GPU test uses.  float32 `got` against `ref` under the rule; int8 `got` (scale given) under the
    int8 rule.  Prints the largest error ratio first and returns it (int8: the excess over 0.5 in units of scale tol)."""
    t = T if t is None else t
    got = np.asarray(got)
    assert got.shape == ref.shape == tol_unit.shape, (got.shape, ref.shape, tol_unit.shape)
    zero = tol_unit == 0
    if scale is None:
        assert got.dtype == np.float32
        assert np.all(np.isfinite(got)), f"{what}: non-finite LLR"
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err[zero] == 0), f"{what}: an erasure is not exactly 0"
        ratio = float((err[~zero] / tol_unit[~zero]).max()) if np.any(~zero) else 0.0
        print(f"{what}: max |llr - ref| / (2^-24 (|y_ax| + a_max)^2 / nvar) = {ratio:.2f}  (T = {t:g})")
        assert ratio <= t, f"{what}: error ratio {ratio:.2f} > T = {t:g}"
        return ratio
    assert got.dtype == np.int8
    err = np.abs(got.astype(np.float64) - quantise_ref(ref, scale))
    assert np.all(got[zero] == 0), f"{what}: an erasure is not exactly 0"
    bound = 0.5 + float(scale) * t * tol_unit
    worst = float((err - bound).max())
    print(f"{what}: int8 max |q - clamp(ref scale)| = {err.max():.3f}, closest to its bound by {-worst:.3g}  (scale = {scale:g}, T = {t:g})")
    assert worst <= 0, f"{what}: int8 error exceeds 0.5 + scale tol by {worst:.3g}"
    return float(err.max())


def dm_case(name, qm, M, B=3, sigma2=10.0 ** -1.5, seed=0):
    rnti = [65535, 0, 0x1234 + seed, 4660][:B] if B == 3 else [40000 + seed, 17 + seed]
    n_id = [1023, 0, 77 + seed, 500][:B] if B == 3 else [1000 - seed, 3 + seed]
    return dict(name=name, qm=qm, M=M, B=B, sigma2=sigma2, seed=seed, rnti=rnti, n_id=n_id)


CASES = [
    dm_case("qpsk_1", 2, 1, seed=1),                       # G smaller than a word
    dm_case("16qam_37", 4, 37, seed=2),                    # G = 148: rows misaligned for 16-byte int8 stores, not a word multiple
    dm_case("64qam_1003", 6, 1003, seed=3),   # G = 6018: no multiple of 32 or of a block; Qm = 6 straddles words
    dm_case("256qam_4099", 8, 4099, seed=4),  # several workgroups and Gold blocks per slot, odd tail
    dm_case("qpsk_156", 2, 156, seed=5),                   # 1 PRB x 13 symbols: G % 16 == 8
    dm_case("256qam_largest", 8, BIG_M, B=2, seed=6),   # the largest G: table extent, index width
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
SMALL = [c["name"] for c in CASES[:5]]


def c_init(rnti: int, n_id: int) -> int:
    return ((rnti << 15) + n_id) % (1 << 31)


@functools.lru_cache(maxsize=None)
def scrambling(ci: int, n: int) -> np.ndarray:
    """c(0 .. n-1) of c_init `ci` as uint8, computed once and shared read-only."""
    c = gold_bits(ci, n)
    c.setflags(write=False)
    return c


def flips(c) -> np.ndarray:
    """bool [B, G]: where descrambling changes the sign."""
    G = c["M"] * c["qm"]
    return np.stack([scrambling(c_init(r, i), G) for r, i in zip(c["rnti"], c["n_id"])]).astype(bool)


def draw(c):
    """x_hat = a constellation point of random bits + CN(0, sigma2), nvar = sigma2 U(0.5, 2), as complex64 / float32."""
    rng = np.random.default_rng(2000 + c["seed"])
    B, M, qm, s2 = c["B"], c["M"], c["qm"], c["sigma2"]
    bits = rng.integers(0, 2, (B, M * qm))
    noise = (rng.standard_normal((B, M)) + 1j * rng.standard_normal((B, M))) * np.sqrt(s2 / 2.0)
    x = (modulate(bits, qm) + noise).astype(np.complex64)
    nvar = (s2 * rng.uniform(0.5, 2.0, (B, M))).astype(np.float32)
    return SimpleNamespace(c=c, name=c["name"], qm=qm, M=M, B=B, G=M * qm, bits=bits, x=x, nvar=nvar, rnti=c["rnti"], n_id=c["n_id"])


def int8_scale(ref) -> float:
    """A power of two near 127 / median |ref|: about half of a case's LLRs saturate."""
    return float(2.0 ** np.round(np.log2(127.0 / np.median(np.abs(ref)))))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """draw() of a named case plus its float64 reference and unit tolerance, computed once and shared read-only."""
    d = draw(CASE_BY_NAME[name])
    d.ref = llr_ref(d.x, d.nvar, d.qm)
    d.tol = unit_tolerance(d.x, d.nvar, d.qm)
    d.scale = int8_scale(d.ref)
    for a in (d.bits, d.x, d.nvar, d.ref, d.tol):
        a.setflags(write=False)
    return d


# ---- end to end: the equalizer test's 25-PRB, 2-layer, 4-port noiseless shape with 16QAM data ----
E2E_PORTS, E2E_QM, E2E_SLOT, E2E_N_ID, E2E_N_SCID, E2E_RNTI, E2E_SCR_ID = 4, 4, 13, 421, 1, 0x4601, 333


def e2e_case():
    from srsran_ce_pytorch_amd import synth as S
    return S.case_spec("demod_e2e_25prb", 52, [S.hop_spec([2, 11], 10, 25)], n_layers=2, seed=78)


def e2e_slot(pilots, data_re, rng):
    """One noiseless slot: random bits -> scrambled with c of (E2E_RNTI, E2E_SCR_ID) -> 16QAM on `data_re` (layer fastest),
    `pilots` [n_re, n_dmrs, L] on the DM-RS REs, through a three-tap channel per (port, layer).  Returns (grids
    [R, n_sc, n_sym] complex64, bits [n_data_re * L * Qm] as sent before scrambling, x_tx [n_data_re, L])."""
    from srsran_ce_pytorch_amd import synth as S
    case = e2e_case()
    n_sc, n_sym, L = 12 * case["n_prb_grid"], case["n_sym"], case["n_layers"]
    hop = S.numpy_hops(case)[0]
    G = len(data_re) * L * E2E_QM
    bits = rng.integers(0, 2, G).astype(np.uint8)
    x_tx = modulate(bits ^ scrambling(c_init(E2E_RNTI, E2E_SCR_ID), G), E2E_QM).reshape(len(data_re), L)
    f_sc = np.arange(n_sc) * case["scs"]
    tap_delay = np.array([0.0, 100e-9, 300e-9]) + case["delay_ns"] * 1e-9
    tap_amp = np.array([1.0, 0.35, 0.2])
    grids = np.zeros((E2E_PORTS, n_sc, n_sym), np.complex64)
    res = np.flatnonzero(np.kron(hop.maskPRBs, hop.DMRSREmask[:, 0]))
    for r in range(E2E_PORTS):
        H = np.stack([(tap_amp * np.exp(2j * np.pi * rng.random(3)))[None, :] @ np.exp(-2j * np.pi * tap_delay[:, None] * f_sc[None, :])
                      for _ in range(L)], -1)[0]                                           # [n_sc, L]
        g = np.zeros((n_sc, n_sym), complex)
        for col, sym in enumerate(case["hops"][0]["dmrs_symbols"]):
            g[res, sym] = case["beta"] * np.sum(H[res] * pilots[:, col, :], -1)
        g[data_re[:, 1], data_re[:, 0]] = np.sum(H[data_re[:, 1]] * x_tx, -1)
        grids[r] = g.astype(np.complex64)
    return grids, bits, x_tx
