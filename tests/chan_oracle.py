"""Oracle of the time-domain channel emulator (include/ce_tp.h `ce_chan_apply`, `PuschChannelEmulator`), the seeded inputs
its tests run on, and the tolerance rule they follow.

The operator, for slot b < B, receive port r < R, sample t < T (x[b][p][t - k] = 0 for t < k):
    y[b][r][t] = exp(j 2 pi w_b(t) / 2^32) sum_{p<P} sum_{k<K} h[b][r][p][k] x[b][p][t - k]  +  sigma_b n[b][r][t]
    w_b(t) = (phase0_b + fcw_b t) mod 2^32
    n[b][r][t] = sqrt(-ln u1) exp(j 2 pi u2) from the Philox4x32-10 words of (seed, first_slot + b, r, t >> 1)
`apply_ref` runs it literally in float64 (`np.convolve(..)[:T]` per row, the phase word in Python integers, the noise from
`philox` in Python integers).  `apply_f32` restates the kernel's float32 arithmetic -- FMAs in the order p outer, k inner, the
phasor of float32(int32(w)) 2^-31 half turns, float32 log and sqrt -- only to calibrate the tolerance before a GPU run.  An FMA
is emulated as float32(float64(a) float64(b) + float64(c)): the product is exact in float64, the sum is rounded twice, which
differs from a fused operation in rare half-way cases only.

Tolerance rule, per output sample (eps = 2^-24), with A = sum_p sum_k |h_k| |x_{t-k}| and n the float64 noise value:
    |got - ref| <= T_CH eps (log2(2 P K) A + sigma (1 + |n|))
The `1 +` covers an absolute error of the logarithm near u1 = 1, where |n| itself vanishes.  T_CH = 4 C_CHAN_RECORDED (the
project's convention: T_TX, C_PRE_FUZZ), C_CHAN the largest ratio of the error to that unit over the inputs of the GPU tests
(`CASES`) AGAINST THE FLOAT64 ORACLE.  The GPU test re-measures it on every run and fails above C_CHAN_RECORDED and below a
quarter of it; tests/test_chan.py does the same with `apply_f32` against C_CHAN_F32_RECORDED.  The margin of 4 is for the
device's logf / sincospif differing from numpy's by a few ulp, not for covering a defect."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
F = np.float32
# C_CHAN_RECORDED: the DEVICE's figure against the float64 oracle, measured 1.66 on an MI355X (gfx950) by
# test_zzzzzzzzzzzzzzzzz_hip_chan.py::test_c_chan_is_the_recorded_value (case t1023_k2_r4; it prints every case), rounded up.
C_CHAN_RECORDED = 2.0
C_CHAN_F32_RECORDED = 2.0     # apply_f32 on the CPU: measured 1.66 (t1023_k2_r4), rounded up
T_CH = 4.0 * C_CHAN_RECORDED
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


# ---- Philox4x32-10 ----

def philox(counter, key):
    """The four output words of Philox4x32-10 in Python integers."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def noise_words(seed, slot, port, t_pair):
    """The words of the sample pair t_pair = t >> 1: counter (t_pair, r, s low, s high), key (seed low, seed high)."""
    s = int(slot) & 0xFFFFFFFFFFFFFFFF
    return philox((t_pair, port, s & MASK, s >> 32), (int(seed) & MASK, (int(seed) >> 32) & MASK))


def noise_words_row(seed, slot, port, n_pairs) -> np.ndarray:
    """uint64 [n_pairs, 4]: `noise_words` of t_pair = 0 .. n_pairs - 1 at once (the same recurrence on uint64 arrays, every
    value kept below 2^32 and every product below 2^64)."""
    s = int(slot) & 0xFFFFFFFFFFFFFFFF
    m = np.uint64(MASK)
    sh = np.uint64(32)
    c0 = np.arange(n_pairs, dtype=np.uint64) & m
    c1 = np.full(n_pairs, int(port) & MASK, np.uint64)
    c2 = np.full(n_pairs, s & MASK, np.uint64)
    c3 = np.full(n_pairs, s >> 32, np.uint64)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], -1)


def uniforms(words: np.ndarray, T: int):
    """(a >> 8) + 1 and c >> 8 as int64 [T] of the words [ceil(T / 2), 4]: sample 2 i takes (w0, w1), 2 i + 1 (w2, w3)."""
    w = np.asarray(words, np.uint64).reshape(-1, 2)[:T].astype(np.int64)
    return (w[:, 0] >> 8) + 1, w[:, 1] >> 8


def gauss_ref(i1, i2) -> np.ndarray:
    """complex128: n = sqrt(-ln u1) exp(j 2 pi u2) of u1 = i1 2^-24 (i1 = (a >> 8) + 1) and u2 = i2 2^-24 (i2 = c >> 8)."""
    i1, i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
    return np.sqrt(-np.log(i1 * 2.0 ** -24)) * np.exp(2j * np.pi * (i2 * 2.0 ** -24))


def noise_ref(seed, slot, port, T) -> np.ndarray:
    """complex128 [T]: the noise of the samples 0 .. T - 1 of (slot, port)."""
    return gauss_ref(*uniforms(noise_words_row(seed, slot, port, (T + 1) // 2), T))


def _sincospi_f32(a):
    """(sin, cos) of pi a for float32 a: computed in float64 and rounded once."""
    a = np.asarray(a, np.float64)
    return np.sin(np.pi * a).astype(F), np.cos(np.pi * a).astype(F)


def gauss_f32(i1, i2):
    """(re, im) float32 the way the kernel computes them: rad = sqrtf(-logf(u1)), sincospi(2 u2), rad cos, rad sin."""
    i1, i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
    u1 = i1.astype(F) * F(2.0 ** -24)                                        # exact
    rad = np.sqrt(-np.log(u1))                                              # float32 log and sqrt
    assert rad.dtype == F
    sn, cs = _sincospi_f32(i2.astype(F) * F(2.0 ** -23))
    return rad * cs, rad * sn


def noise_f32(seed, slot, port, T):
    return gauss_f32(*uniforms(noise_words_row(seed, slot, port, (T + 1) // 2), T))


# ---- the phase word ----

def phase_words(phase0, fcw, T) -> np.ndarray:
    """int64 [T]: w(t) = (phase0 + fcw t) mod 2^32, in Python integers."""
    return np.array([(int(phase0) + int(fcw) * t) % (1 << 32) for t in range(T)], np.int64)


def _per_slot(v, B):
    """A scalar or a sequence of B values -> a list of B Python numbers."""
    a = np.asarray(v)
    return [a.item()] * B if a.ndim == 0 else [x.item() for x in a.reshape(B)]


# ---- the operator in float64 ----

def apply_ref(x, h, fcw=None, phase0=0, sigma=None, seed=0, first_slot=0):
    """(y, A, n): y complex128 [B, R, T] of x [B, P, T] and h [B or 1, R, P, K]; A = sum_p sum_k |h_k| |x_{t-k}| and the
    float64 noise values n (zeros without sigma) for the tolerance rule.  fcw / phase0 / sigma: None, a scalar or B values."""
    x, h = np.asarray(x).astype(np.complex128), np.asarray(h).astype(np.complex128)
    B, P, T = x.shape
    R, K = h.shape[1], h.shape[3]
    assert h.shape[0] in (1, B) and h.shape[2] == P
    y, A, n = np.zeros((B, R, T), np.complex128), np.zeros((B, R, T)), np.zeros((B, R, T), np.complex128)
    for b in range(B):
        hb = h[b if h.shape[0] > 1 else 0]
        for r in range(R):
            for p in range(P):
                y[b, r] += np.convolve(x[b, p], hb[r, p])[:T]
                A[b, r] += np.convolve(np.abs(x[b, p]), np.abs(hb[r, p]))[:T]
            if fcw is not None:
                w = phase_words(_per_slot(phase0, B)[b], _per_slot(fcw, B)[b], T)
                y[b, r] *= np.exp(2j * np.pi * (w * 2.0 ** -32))
            if sigma is not None:
                n[b, r] = noise_ref(seed, int(first_slot) + b, r, T)
                y[b, r] += float(_per_slot(sigma, B)[b]) * n[b, r]
    return y, A, n


# ---- the kernel's arithmetic in float32 numpy ----

def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def apply_f32(x, h, fcw=None, phase0=0, sigma=None, seed=0, first_slot=0) -> np.ndarray:
    """complex64 [B, R, T]: the kernel's float32 arithmetic (include/ce_tp.h)."""
    x, h = np.asarray(x).astype(np.complex64), np.asarray(h).astype(np.complex64)
    B, P, T = x.shape
    R, K = h.shape[1], h.shape[3]
    out = np.zeros((B, R, T), np.complex64)
    for b in range(B):
        hb = h[b if h.shape[0] > 1 else 0]
        for r in range(R):
            re, im = np.zeros(T, F), np.zeros(T, F)
            for p in range(P):
                xr, xi = x[b, p].real.astype(F), x[b, p].imag.astype(F)
                for k in range(K):
                    vr, vi = np.zeros(T, F), np.zeros(T, F)
                    vr[k:], vi[k:] = xr[:max(T - k, 0)], xi[:max(T - k, 0)]
                    hr, hi = F(hb[r, p, k].real), F(hb[r, p, k].imag)
                    re = _fma(hr, vr, re)
                    re = _fma(-hi, vi, re)
                    im = _fma(hr, vi, im)
                    im = _fma(hi, vr, im)
            if fcw is not None:
                w = phase_words(_per_slot(phase0, B)[b], _per_slot(fcw, B)[b], T)
                signed = np.where(w >= 1 << 31, w - (1 << 32), w)
                s, c = _sincospi_f32(signed.astype(F) * F(2.0 ** -31))                # int32 -> float32 rounds to nearest even
                re, im = _fma(re, c, -(im * s)), _fma(re, s, im * c)
            if sigma is not None:
                nr, ni = noise_f32(seed, int(first_slot) + b, r, T)
                sg = F(_per_slot(sigma, B)[b])
                re, im = _fma(sg, nr, re), _fma(sg, ni, im)
            out[b, r].real, out[b, r].imag = re, im
    return out


# ---- the rule ----

def unit(A, n, sigma, P, K) -> np.ndarray:
    """The rule's right-hand side without T_CH: eps (log2(2 P K) A + sigma (1 + |n|)), [B, R, T]."""
    B = A.shape[0]
    sg = np.zeros(B) if sigma is None else np.array([float(s) for s in _per_slot(sigma, B)])
    return EPS * (np.log2(2.0 * P * K) * A + sg[:, None, None] * (1.0 + np.abs(n)))


def ratio(got, d) -> float:
    """The largest |got - ref| / unit over the case's outputs; where the unit is zero (no noise, and every product of the sum
    has a zero factor) the output has to be the reference's zero."""
    err = np.abs(np.asarray(got).astype(np.complex128) - d.ref)
    u = unit(d.A, d.n, d.sigma, d.c["P"], d.c["K"])
    zero = u == 0
    assert np.all(err[zero] == 0), "a non-zero output where every product of the sum has a zero factor"
    return float((err[~zero] / u[~zero]).max()) if not zero.all() else 0.0


def check(got, d, what="", t=None) -> float:
    """The comparison every test uses.  Prints the largest error ratio first and returns it."""
    t = T_CH if t is None else t
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == d.ref.shape, (what, got.dtype, got.shape, d.ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), f"{what}: non-finite output"
    r = ratio(got, d)
    print(f"{what}: max |y - ref| / (2^-24 (log2(2 P K) A + sigma (1 + |n|))) = {r:.2f}  (bound {t:g})")
    assert r <= t, f"{what}: error ratio {r:.2f} > {t:g}"
    return r


# ---- inputs ----
# T: 1, the tile edge 1023 / 1024 / 1025, 2500 (three tiles, the last partial); an odd T ends in a pair of one sample.
# K: 1 (no window), 2, 3 and 127 (an odd count: the sliding window's remainder step), 12, 128 (the limit; longer than T = 1).
# taps: shared (slot stride 0) or per slot; cfo / sigma: None, "scalar" (one host value) or "tensor" (B device values).
def _case(name, B, P, R, K, T, shared, cfo, sigma, first_slot=0):
    return dict(name=name, B=B, P=P, R=R, K=K, T=T, shared=shared, cfo=cfo, sigma=sigma, first_slot=first_slot)


CASES = [
    _case("t1_k1", 1, 1, 1, 1, 1, True, "scalar", "scalar"),
    _case("t1_k128_p2", 1, 2, 1, 128, 1, False, "tensor", "tensor", first_slot=(1 << 33) + 5),
    _case("t1023_k2_r4", 3, 1, 4, 2, 1023, True, None, "scalar", first_slot=17),
    _case("t1024_k12_p4", 1, 4, 1, 12, 1024, False, "scalar", None),
    _case("t1024_k3_p4", 3, 4, 1, 3, 1024, True, "tensor", None),
    _case("t1025_k128_p2_r4", 3, 2, 4, 128, 1025, False, "tensor", "tensor", first_slot=-2),
    _case("t1025_k1_plain", 3, 1, 1, 1, 1025, False, None, None),
    _case("t1023_k127_r4", 1, 1, 4, 127, 1023, True, None, None),
    _case("t2500_k12_r4", 3, 1, 4, 12, 2500, True, "tensor", "scalar", first_slot=1000),
    _case("t2500_k2_p2", 1, 2, 1, 2, 2500, False, "scalar", "scalar"),
    _case("t2500_k128_p4_r4", 1, 4, 4, 128, 2500, True, "scalar", "tensor"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
CASE_NAMES = [c["name"] for c in CASES]
# scalar control words that wrap the phase many times: the largest positive and the most negative frequency among them
_SCALAR_FCW = {"t1_k1": 123456789, "t1024_k12_p4": 2 ** 31 - 1, "t2500_k2_p2": -(2 ** 31) + 1, "t2500_k128_p4_r4": -40000001}


def _freeze(d, *names):
    for n in names:
        v = getattr(d, n)
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(name):
    """A case's seeded inputs -- x complex64 [B, P, T] complex normal, h complex64 [B or 1, R, P, K] complex normal of unit
    energy per (r, p), fcw (int32 values) / phase0 (uint32 values) / sigma (float32 values) as None, a scalar or B values, a
    64-bit seed -- with ref, A and n of `apply_ref`; shared and read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(31000 + CASES.index(c))
    B, P, R, K, T = c["B"], c["P"], c["R"], c["K"], c["T"]
    x = (rng.standard_normal((B, P, T)) + 1j * rng.standard_normal((B, P, T))).astype(np.complex64)
    hs = (1 if c["shared"] else B, R, P, K)
    h = ((rng.standard_normal(hs) + 1j * rng.standard_normal(hs)) / np.sqrt(2.0 * K)).astype(np.complex64)
    fcw = phase0 = sigma = None
    if c["cfo"] == "scalar":
        fcw, phase0 = _SCALAR_FCW[name], int(rng.integers(0, 1 << 32))
    elif c["cfo"] == "tensor":
        fcw = rng.integers(-2 ** 31, 2 ** 31, B).astype(np.int32)
        phase0 = rng.integers(0, 1 << 32, B).astype(np.uint32)
    if c["sigma"] == "scalar":
        sigma = float(F(0.25 + rng.random()))
    elif c["sigma"] == "tensor":
        sigma = (0.05 + 2.0 * rng.random(B)).astype(F)
    seed = int(rng.integers(0, 1 << 63)) * 2 + 1
    ref, A, n = apply_ref(x, h, fcw, phase0, sigma, seed, c["first_slot"])
    d = SimpleNamespace(c=c, name=name, x=x, h=h, fcw=fcw, phase0=phase0, sigma=sigma, seed=seed, first_slot=c["first_slot"], ref=ref, A=A, n=n)
    return _freeze(d, "x", "h", "fcw", "phase0", "sigma", "ref", "A", "n")
