"""Float64 oracle of the equalizer extension (include/ce_eq.h), the seeded inputs the GPU tests run on, and the
tolerance rule both follow.

The oracle inverts A with np.linalg.inv (LU with pivoting) -- not the kernel's Cholesky route -- and enumerates the data
REs by plain loops over symbols and subcarriers, independent of the library's per-symbol table.

Tolerance rule, per output element, with kappa = cond(A) and b_l = 1 - [A^-1]_ll taken from the float64 oracle:
    |x_hat_l - ref| <= T 2^-24 (kappa + 1 / b_l) max(1, max_l |ref x_hat_l|)
    |nvar_l  - ref| <= T 2^-24 (kappa + 1 / b_l) ref nvar_l
1 / b is the 1 - d cancellation, kappa the solve.  T = 4 C, where C is the largest ratio of `equalize_f32`'s own error (the
same formulas in float32 numpy) to 2^-24 (kappa + 1 / b) over the inputs of the GPU tests; the factor 4 covers FMA
contraction and another summation order on the GPU.  tests/test_eq.py re-measures C and fails if it exceeds C_RECORDED."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from srsran_ce_pytorch_amd import synth as S
from srsran_ce_pytorch_amd.equalizer import CHUNK_SC

EPS = 2.0 ** -24
C_RECORDED = 3.0     # measured 2.84 (test_eq.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T = 4.0 * C_RECORDED

T1 = [S.TYPE1_CDM0, S.TYPE1_CDM1]
T2 = [S.TYPE2_CDM0, S.TYPE2_CDM1]
CHUNK_PRB = CHUNK_SC // 12


def eq_case(name, n_prb_grid, hops, L, R, B=1, mask=0xFFF, n_sym=14, seed=0):
    return dict(name=name, case=S.case_spec(name, n_prb_grid, hops, n_layers=L, n_sym=n_sym, seed=seed), L=L, R=R, B=B, mask=mask)


CASES = [
    eq_case("smallest", 1, [S.hop_spec([2], 0, 1)], 1, 1, seed=1),
    eq_case("offset", 24, [S.hop_spec([2, 11], 3, 5)], 2, 2, B=3, seed=2),
    eq_case("dmrs_data_type1", 24, [S.hop_spec([2, 11], 3, 5)], 1, 4, mask=0x555, seed=3),
    eq_case("dmrs_data_type2", 24, [S.hop_spec([2, 11], 3, 5, re_masks=T2)], 3, 4, mask=0x3CF, seed=4),
    eq_case("hopping", 52, [S.hop_spec([2], 2, 8, 0, 7), S.hop_spec([9], 30, 8, 7, 7)], 2, 4, seed=5),
    eq_case("short_alloc", 24, [S.hop_spec([3, 8], 3, 5, 2, 9, re_masks=T1)], 3, 4, n_sym=12, seed=6),
    eq_case("L4_R4", 24, [S.hop_spec([2, 11], 3, 5, re_masks=T1)], 4, 4, seed=7),
    eq_case("L4_R8", 24, [S.hop_spec([2, 11], 3, 5, re_masks=T1)], 4, 8, seed=8),
    eq_case("chunk_minus_1prb", 8, [S.hop_spec([2], 0, CHUNK_PRB - 1)], 2, 2, seed=9),
    eq_case("chunk_exact", 8, [S.hop_spec([2], 0, CHUNK_PRB)], 2, 2, seed=10),
    eq_case("chunk_plus_1prb", 8, [S.hop_spec([2], 0, CHUNK_PRB + 1)], 2, 2, seed=11),
    eq_case("chunk_straddled", 8, [S.hop_spec([2], 1, CHUNK_PRB)], 1, 2, seed=12),
    eq_case("full_band_273", 273, [S.hop_spec([2, 11], 0, 273)], 1, 2, B=2, seed=13),
    eq_case("batch5", 24, [S.hop_spec([2, 11], 3, 5)], 2, 4, B=5, seed=14),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def data_re_ref(case, reserved_re_mask=0xFFF) -> np.ndarray:
    """(n_data_re, 2) array of (sym, sc) in output order: symbol ascending, subcarrier ascending within a symbol."""
    out = []
    for sym in range(case["n_sym"]):
        for sc in range(12 * case["n_prb_grid"]):
            for h in case["hops"]:
                if not h["start_symbol"] <= sym < h["start_symbol"] + h["n_alloc"]:
                    continue
                if not h["prb_start"] <= sc // 12 < h["prb_start"] + h["n_prbs"]:
                    continue
                if sym in h["dmrs_symbols"] and (reserved_re_mask >> (sc % 12)) & 1:
                    continue
                out.append((sym, sc))
    return np.array(out, np.int64).reshape(-1, 2)


def _gather(rx, ch_est, noise, data_re, ctype, ftype):
    sym, sc = data_re[:, 0], data_re[:, 1]
    H = np.asarray(ch_est)[:, :, sc, sym, :].astype(ctype)                   # [B, R, n, L]
    y = np.asarray(rx)[:, :, sc, sym].astype(ctype)                          # [B, R, n]
    n = np.asarray(noise).astype(ftype)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(np.isfinite(n) & (n > 0), ftype(1) / n, ftype(0)).astype(ftype)   # [B, R]
    return H, y, w


def _solve(H, y, w, ctype, ftype):
    L = H.shape[-1]
    A = np.eye(L, dtype=ctype) + np.einsum("brni,brnj,br->bnij", H.conj(), H, w.astype(ctype)).astype(ctype)
    z = np.einsum("brni,brn,br->bni", H.conj(), y, w.astype(ctype)).astype(ctype)
    Ainv = np.linalg.inv(A)
    assert Ainv.dtype == ctype
    d = np.real(np.einsum("bnii->bni", Ainv)).astype(ftype)
    b = (ftype(1) - d).astype(ftype)
    v = np.einsum("bnij,bnj->bni", Ainv, z).astype(ctype)
    ok = b > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(ok, v / np.where(ok, b, 1), 0).astype(ctype)
        nvar = np.where(ok, d / np.where(ok, b, 1), np.inf).astype(ftype)
    return A, b, x, nvar


def equalize_ref(rx, ch_est, noise, data_re) -> SimpleNamespace:
    """float64 / np.linalg.inv.  Returns x_hat [B, n, L] complex128, nvar [B, n, L] float64, and for the tolerance rule
    kappa [B, n] = cond(A) and b [B, n, L]."""
    H, y, w = _gather(rx, ch_est, noise, data_re, np.complex128, np.float64)
    A, b, x, nvar = _solve(H, y, w, np.complex128, np.float64)
    return SimpleNamespace(x_hat=x, nvar=nvar, kappa=np.linalg.cond(A), b=b)


def equalize_f32(rx, ch_est, noise, data_re):
    """The same formulas in float32 numpy -- only to calibrate the tolerance."""
    H, y, w = _gather(rx, ch_est, noise, data_re, np.complex64, np.float32)
    _, _, x, nvar = _solve(H, y, w, np.complex64, np.float32)
    return x, nvar


def rel_tolerance(ref, t=None) -> np.ndarray:
    """T 2^-24 (kappa + 1 / b) per element [B, n, L]; inf where b <= 0 (those elements are compared exactly)."""
    with np.errstate(divide="ignore"):
        return (T if t is None else t) * EPS * (ref.kappa[..., None] + np.where(ref.b > 0, 1.0 / np.where(ref.b > 0, ref.b, 1.0), np.inf))


def error_ratios(x, nvar, ref):
    """Each output's error divided by 2^-24 (kappa + 1 / b) times its scale, as [B, n, L] arrays (x, nvar); elements with
    b <= 0 must be exact (x = 0, nvar = +inf) and count as ratio 0."""
    ok = ref.b > 0
    assert np.all(np.asarray(x)[~ok] == 0) and np.all(np.asarray(nvar)[~ok] == np.inf), "b <= 0: x_hat must be 0 and nvar +inf"
    unit = rel_tolerance(ref, 1.0)
    scale = np.maximum(1.0, np.abs(ref.x_hat).max(axis=-1, keepdims=True))
    with np.errstate(invalid="ignore"):
        rx_ = np.where(ok, np.abs(np.asarray(x).astype(np.complex128) - ref.x_hat) / (unit * scale), 0.0)
        rn_ = np.where(ok, np.abs(np.where(ok, np.asarray(nvar).astype(np.float64), 0.0) - np.where(ok, ref.nvar, 0.0))
                       / (unit * np.where(ok, ref.nvar, 1.0)), 0.0)
    assert np.all(np.isfinite(rx_)) and np.all(np.isfinite(rn_)), "non-finite output where the oracle is finite"
    return rx_, rn_


def check(x, nvar, ref, what=""):
    """The comparison every GPU test uses: both outputs under the rule with the recorded T.  Prints the figures first."""
    x, nvar = np.asarray(x), np.asarray(nvar)
    assert x.shape == ref.x_hat.shape and nvar.shape == ref.nvar.shape, (x.shape, nvar.shape, ref.x_hat.shape)
    rx_, rn_ = error_ratios(x, nvar, ref)
    print(f"{what}: max error / (2^-24 (kappa + 1/b) scale): x_hat {rx_.max():.2f}, nvar {rn_.max():.2f}  (T = {T:g})")
    assert rx_.max() <= T, f"{what}: x_hat error ratio {rx_.max():.2f} > T = {T:g}"
    assert rn_.max() <= T, f"{what}: nvar error ratio {rn_.max():.2f} > T = {T:g}"


def draw(c):
    """The inputs of one case.  ch_est is iid CN(0, 1) inside the hops' rectangles and zero outside, rx = H x + n with QPSK x
    on the data REs (and unrelated values everywhere else, so a wrong index shows), noise_r = 10^-1.5 U(0.5, 2)."""
    case, L, R, B = c["case"], c["L"], c["R"], c["B"]
    rng = np.random.default_rng(1000 + case["seed"])
    n_sc, n_sym = 12 * case["n_prb_grid"], case["n_sym"]
    cn = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)   # noqa: E731
    data_re = data_re_ref(case, c["mask"])
    sym, sc = data_re[:, 0], data_re[:, 1]
    ch = np.zeros((B, R, n_sc, n_sym, L), np.complex64)
    for h in case["hops"]:
        k0, k1, s0, s1 = 12 * h["prb_start"], 12 * (h["prb_start"] + h["n_prbs"]), h["start_symbol"], h["start_symbol"] + h["n_alloc"]
        ch[:, :, k0:k1, s0:s1, :] = cn(B, R, k1 - k0, s1 - s0, L)
    noise = 10.0 ** -1.5 * rng.uniform(0.5, 2.0, (B, R))
    x_tx = ((2 * rng.integers(0, 2, (B, len(sym), L)) - 1) + 1j * (2 * rng.integers(0, 2, (B, len(sym), L)) - 1)) / np.sqrt(2.0)
    rx = (3.0 * cn(B, R, n_sc, n_sym)).astype(np.complex64)
    Hd = ch[:, :, sc, sym, :].astype(np.complex128)
    rx[:, :, sc, sym] = (np.einsum("brnl,bnl->brn", Hd, x_tx) + cn(B, R, len(sym)) * np.sqrt(noise)[:, :, None]).astype(np.complex64)
    return SimpleNamespace(c=c, case=case, L=L, R=R, B=B, mask=c["mask"], rx=rx, ch_est=ch, noise=noise, data_re=data_re, x_tx=x_tx)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """draw() of a named case plus its float64 reference, computed once and shared read-only."""
    d = draw(CASE_BY_NAME[name])
    d.ref = equalize_ref(d.rx, d.ch_est, d.noise, d.data_re)
    for a in (d.rx, d.ch_est, d.noise, d.data_re, d.x_tx, d.ref.x_hat, d.ref.nvar, d.ref.kappa, d.ref.b):
        a.setflags(write=False)
    return d
