"""Float64 oracle of the transform de-precoding extension (include/ce_tp.h), the seeded inputs the GPU tests run on, and
the two tolerance rules both follow.

`precode` is TS 38.211 6.3.1.4 literally (an explicit M x M DFT matrix for small M, so that the sign and the scale do not
lean on a library's convention); `deprecode_ref` is the operator of include/ce_tp.h in float64 with `np.fft.ifft`;
`deprecode_f32` restates the kernel's own float32 arithmetic (radix sequence and twiddle table from the library's host
entry points, the same reduction order, the same final scale) -- only to calibrate the tolerance.

Tolerance rule for x_out, per output i of a row (eps = 2^-24, rms_row = the rms of the row's reference outputs):
    |got_i - ref_i| <= T eps (log2(M) rms_row + |ref_i|)
A float32 FFT of length M errs in proportion to log2(M) times the rms of its outputs; the final scaling by
sqrt(M) / sum(beta) errs in proportion to the output itself.  T = 4 C, where C is the largest ratio of `deprecode_f32`'s
own error to eps (log2(M) rms_row + |ref_i|) over the inputs of the GPU tests (`CASES`, `special_inputs`, `chain_inputs`);
the factor 4 covers FMA contraction and pass-internal ordering on the GPU that the restatement cannot mirror.
tests/test_tp.py re-measures C and fails if it exceeds C_RECORDED.

Tolerance rule for nvar_out = (sum gamma) / (sum beta): every summand is non-negative, so there is no conditioning term.
With u = eps the unit roundoff, 1 + nvar carries u, beta = 1 / (1 + nvar) and gamma = nvar / (1 + nvar) carry 2 u each; a sum
whose longest addition chain has `chain` additions adds chain u, and the final division one more: numerator and
denominator (chain + 2) u each, the quotient 2 (chain + 2) u + u, inside
    |got - ref| <= 2 (chain + 4) eps ref
`chain(view)` is the kernel's longest addition chain: thread t of a row adds the 4 values of each of its
ceil((M / 4) / threads_per_row) groups in turn, then the partial sums meet in a balanced tree of log2(threads_per_row)
levels:  chain = 4 ceil(M / 4 / threads_per_row) + log2(threads_per_row), from the host view, per M.
Where ref = +inf (no usable RE in the row), got must be +inf and the row's x_out exactly 0."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import demod_oracle as D

EPS = 2.0 ** -24
C_RECORDED = 1.5     # measured 1.24 (test_tp.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T = 4.0 * C_RECORDED


def smooth(n: int) -> bool:
    """n has only the prime factors 2, 3 and 5."""
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


VALID_PRBS = [n for n in range(1, 274) if smooth(n)]
MATRIX_MAX = 512          # precode(): the explicit matrix up to this M


# ---- the operator ----

def dft_matrix(M: int) -> np.ndarray:
    k = np.arange(M)
    return np.exp(-2j * np.pi * np.outer(k, k) / M) / np.sqrt(M)


def precode(x, M: int, matrix=None) -> np.ndarray:
    """38.211 6.3.1.4: y(l M + k) = (1 / sqrt(M)) sum_i x(l M + i) exp(-j 2 pi i k / M), complex128, for x [..., S M].
    `matrix`: True = the explicit M x M matrix, False = np.fft.fft, None = the matrix up to MATRIX_MAX."""
    x = np.asarray(x, np.complex128)
    rows = x.reshape(x.shape[:-1] + (-1, M))
    if matrix is None:
        matrix = M <= MATRIX_MAX
    y = rows @ dft_matrix(M).T if matrix else np.fft.fft(rows, axis=-1) / np.sqrt(M)
    return y.reshape(x.shape)


def deprecode_ref(x_hat, nvar, M: int):
    """(x_out complex128, nvar_out float64), both [B, S M]: the formulas of include/ce_tp.h in float64."""
    x = np.asarray(x_hat).astype(np.complex128)
    nv = np.asarray(nvar).astype(np.float64)
    B = x.shape[0]
    x, nv = x.reshape(B, -1, M), nv.reshape(B, -1, M)
    ok = D.usable(x, nv)
    nvs = np.where(ok, nv, 1.0)
    beta = np.where(ok, 1.0 / (1.0 + nvs), 0.0)
    gamma = np.where(ok, nvs / (1.0 + nvs), 1.0)
    u = np.where(ok, beta * np.where(ok, x, 0.0), 0.0)
    sb, sg = beta.sum(-1, keepdims=True), gamma.sum(-1, keepdims=True)
    t = np.fft.ifft(u, axis=-1) * np.sqrt(M)                       # (1 / sqrt(M)) sum_k u_k exp(+j 2 pi i k / M)
    some = sb > 0
    sbs = np.where(some, sb, 1.0)
    x_out = np.where(some, t / (sbs / M), 0.0)
    nvar_out = np.broadcast_to(np.where(some, sg / sbs, np.inf), nv.shape)
    return x_out.reshape(B, -1), np.array(nvar_out).reshape(B, -1)


# ---- the kernel's arithmetic in float32 numpy ----

F = np.float32


def chain(view) -> int:
    tpr = int(view.threads_per_row)
    return 4 * -(-(int(view.m_sc) // 4) // tpr) + int(np.log2(tpr))


def _reduce_f32(v, tpr: int):
    """[rows, M] float32 -> [rows]: the kernel's order (per-thread serial over its groups of 4, a butterfly of lane
    exchanges per wave, then the waves pairwise)."""
    rows, M = v.shape
    n_grp = M // 4
    nit = -(-n_grp // tpr)
    pad = np.zeros((rows, nit * tpr * 4), F)                        # x + 0 = x: a thread without a group adds nothing
    pad[:, :M] = v
    pad = pad.reshape(rows, nit, tpr, 4)
    acc = np.zeros((rows, tpr), F)
    for it in range(nit):
        for e in range(4):
            acc = (acc + pad[:, it, :, e]).astype(F)
    acc = acc.reshape(rows, tpr // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lane ^ off]).astype(F)
    w = acc[:, :, 0]
    if tpr == 64:
        return w[:, 0]
    if tpr == 128:
        return (w[:, 0] + w[:, 1]).astype(F)
    return ((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F)


def _butterfly_f32(R, xr, xi):
    """Lists of R float32 arrays (re, im) -> the R outputs, in the kernel's operation order (no FMA)."""
    add = lambda a, b: ((a[0] + b[0]).astype(F), (a[1] + b[1]).astype(F))     # noqa: E731
    sub = lambda a, b: ((a[0] - b[0]).astype(F), (a[1] - b[1]).astype(F))     # noqa: E731
    mul = lambda c, a: ((F(c) * a[0]).astype(F), (F(c) * a[1]).astype(F))     # noqa: E731
    add_j = lambda a, b: ((a[0] - b[1]).astype(F), (a[1] + b[0]).astype(F))   # noqa: E731
    sub_j = lambda a, b: ((a[0] + b[1]).astype(F), (a[1] - b[0]).astype(F))   # noqa: E731
    x = list(zip(xr, xi))
    if R == 2:
        return [add(x[0], x[1]), sub(x[0], x[1])]
    if R == 4:
        t0, t1, t2, t3 = add(x[0], x[2]), sub(x[0], x[2]), add(x[1], x[3]), sub(x[1], x[3])
        return [add(t0, t2), add_j(t1, t3), sub(t0, t2), sub_j(t1, t3)]
    if R == 3:
        t, u = add(x[1], x[2]), sub(x[1], x[2])
        m, v = sub(x[0], mul(0.5, t)), mul(0.8660254037844386, u)
        return [add(x[0], t), add_j(m, v), sub_j(m, v)]
    c1, c2, s1, s2 = 0.30901699437494745, -0.8090169943749475, 0.9510565162951535, 0.5877852522924731
    t1, t2, u1, u2 = add(x[1], x[4]), add(x[2], x[3]), sub(x[1], x[4]), sub(x[2], x[3])
    m1 = add(add(x[0], mul(c1, t1)), mul(c2, t2))
    m2 = add(add(x[0], mul(c2, t1)), mul(c1, t2))
    n1, n2 = add(mul(s1, u1), mul(s2, u2)), sub(mul(s2, u1), mul(s1, u2))
    return [add(add(x[0], t1), t2), add_j(m1, n1), add_j(m2, n2), sub_j(m2, n2), sub_j(m1, n1)]


def passes_f32(re, im, radix, tw, scale):
    """(re, im) float32 [rows, M] through the kernel's passes (csrc/ce_fft.h `tp_passes`) over `radix` with the twiddle table
    `tw` (complex64 [M]); the last pass multiplies by `scale`, a float32 scalar or one per row ([rows, 1])."""
    M = re.shape[1]
    wr, wi = tw.real.astype(F), tw.imag.astype(F)
    s = 1
    for n, R in enumerate(radix):
        last = n == len(radix) - 1
        nb = M // R
        i = np.arange(nb)
        y = _butterfly_f32(R, [re[:, i + k * nb] for k in range(R)], [im[:, i + k * nb] for k in range(R)])
        ps = (i // s) * s
        o = (i - ps) + ps * R
        nre, nim = np.empty_like(re), np.empty_like(im)
        for j in range(R):
            yr, yi = y[j]
            if last:
                yr, yi = (scale * yr).astype(F), (scale * yi).astype(F)
            elif j:
                a, b = wr[ps * j], wi[ps * j]
                yr, yi = ((yr * a).astype(F) - (yi * b).astype(F)).astype(F), ((yr * b).astype(F) + (yi * a).astype(F)).astype(F)
            nre[:, o + s * j], nim[:, o + s * j] = yr, yi
        re, im = nre, nim
        s *= R
    assert re.dtype == F and im.dtype == F
    return re, im


def deprecode_f32(x_hat, nvar, view, tw):
    """(x_out complex64, nvar_out float32), both [B, S M].  `view`: the library's host view of the shape; `tw`: its twiddle
    table (complex64 [M])."""
    M, tpr = int(view.m_sc), int(view.threads_per_row)
    radix = [int(r) for r in view.radix[:view.n_passes]]
    x = np.asarray(x_hat).astype(np.complex64)
    B = x.shape[0]
    x = x.reshape(-1, M)
    nv = np.asarray(nvar).astype(F).reshape(-1, M)
    ok = D.usable(x, nv)
    with np.errstate(all="ignore"):
        d = (F(1) + nv).astype(F)
        beta = np.where(ok, (F(1) / d).astype(F), F(0))
        gamma = np.where(ok, (nv / d).astype(F), F(1))
        re = np.where(ok, (beta * x.real).astype(F), F(0))
        im = np.where(ok, (beta * x.imag).astype(F), F(0))
    sb, sg = _reduce_f32(beta, tpr), _reduce_f32(gamma, tpr)
    some = sb > 0
    with np.errstate(all="ignore"):
        scale = np.where(some, (F(np.sqrt(float(M))) / sb).astype(F), F(0))
        nvo = np.where(some, (sg / sb).astype(F), F(np.inf))
    re, im = passes_f32(re, im, radix, tw, scale[:, None])
    out = (re + 1j * im).astype(np.complex64)
    assert re.dtype == F and nvo.dtype == F
    return out.reshape(B, -1), np.repeat(nvo, M).reshape(B, -1)


# ---- the rules ----

def x_unit(ref_x, M: int) -> np.ndarray:
    """eps (log2(M) rms_row + |ref_i|) per output, [B, S M]; 0 over a fully dropped row."""
    r = np.asarray(ref_x).reshape(ref_x.shape[0], -1, M)
    rms = np.sqrt(np.mean(np.abs(r) ** 2, -1, keepdims=True))
    return (EPS * (np.log2(M) * rms + np.abs(r))).reshape(ref_x.shape)


def x_ratio(got_x, ref_x, M: int) -> float:
    unit = x_unit(ref_x, M)
    err = np.abs(np.asarray(got_x).astype(np.complex128) - ref_x)
    live = unit > 0
    assert np.all(err[~live] == 0), "an output of a fully dropped row is not exactly 0"
    return float((err[live] / unit[live]).max()) if live.any() else 0.0


def check(got_x, got_nv, ref_x, ref_nv, view, what="", t=None):
    """The comparison every GPU test uses: both rules.  Prints the two largest error ratios first and returns them."""
    t = T if t is None else t
    M = int(view.m_sc)
    got_x, got_nv = np.asarray(got_x), np.asarray(got_nv)
    assert got_x.dtype == np.complex64 and got_nv.dtype == np.float32
    assert got_x.shape == ref_x.shape == got_nv.shape == ref_nv.shape, (got_x.shape, ref_x.shape, got_nv.shape, ref_nv.shape)
    dead = ~np.isfinite(ref_nv)
    assert np.all(np.isposinf(got_nv[dead])) and np.all(got_x[dead] == 0), f"{what}: a fully dropped row is not (0, +inf)"
    assert np.all(np.isfinite(got_nv[~dead])) and np.all(np.isfinite(got_x.view(np.float32))), f"{what}: non-finite output"
    rx = x_ratio(got_x, ref_x, M)
    bound = 2.0 * (chain(view) + 4) * EPS
    rel = np.abs(got_nv[~dead].astype(np.float64) - ref_nv[~dead]) / ref_nv[~dead]
    rn = float(rel.max() / bound) if rel.size else 0.0
    print(f"{what}: max |x - ref| / (2^-24 (log2(M) rms_row + |ref|)) = {rx:.2f}  (T = {t:g});  "
          f"max rel. nvar error = {rn:.3f} of 2 (chain + 4) 2^-24, chain = {chain(view)}")
    assert rx <= t, f"{what}: x_out error ratio {rx:.2f} > T = {t:g}"
    assert rn <= 1.0, f"{what}: nvar_out relative error {rn:.3f} of its bound"
    return rx, rn


# ---- inputs ----

SIZES = [12, 24, 60, 108, 300, 972, 1500, 3072, 3240]     # M: the radices and pass counts each exercises are in test_tp.py
SYMBOLS = [1, 3, 14]
N_SLOTS = 3
CASES = [(M, S) for M in SIZES for S in SYMBOLS]


def draw(M: int, S: int, B: int = N_SLOTS, seed: int = 0):
    """x_hat = precode(random 16QAM symbols) + CN(0, nvar_k), nvar_k = 10^U(-3, 0.5) per RE, as complex64 / float32."""
    rng = np.random.default_rng(7000 + 17 * M + S + 1000003 * seed)
    bits = rng.integers(0, 2, (B, S * M * 4))
    x = D.modulate(bits, 4)
    nvar = 10.0 ** rng.uniform(-3.0, 0.5, (B, S * M))
    noise = (rng.standard_normal((B, S * M)) + 1j * rng.standard_normal((B, S * M))) * np.sqrt(nvar / 2.0)
    return SimpleNamespace(M=M, S=S, B=B, bits=bits, x_tx=x, x_hat=(precode(x, M) + noise).astype(np.complex64), nvar=nvar.astype(np.float32))


def _finish(d):
    d.ref_x, d.ref_nv = deprecode_ref(d.x_hat, d.nvar, d.M)
    for a in (d.x_hat, d.nvar, d.ref_x, d.ref_nv):
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(M: int, S: int):
    """draw() of a case plus its float64 reference, computed once and shared read-only."""
    return _finish(draw(M, S))


SPECIAL = [(12, 3), (300, 3), (3240, 1)]


@functools.lru_cache(maxsize=None)
def special_inputs(M: int, S: int):
    """draw() with nvar in {+inf, 0, -1, NaN} and non-finite x_hat parts on scattered REs of slots 0 and 1 (ten, or one RE
    in six), and slot 2's row 0 fully dropped."""
    d = draw(M, S, seed=1)
    rng = np.random.default_rng(99 + M)
    x, nv = d.x_hat.copy(), d.nvar.copy()
    n = S * M
    bad_nv = [np.inf, 0.0, -1.0, np.nan, -np.inf]
    bad_x = [complex(np.inf, 0.5), complex(-0.25, np.inf), complex(np.nan, 1.0), complex(1.0, np.nan), complex(-np.inf, np.nan)]
    d.dropped = np.zeros((d.B, n), bool)
    for b in (0, 1):
        where = rng.choice(n, max(10, n // 6), replace=False)
        for q, k in enumerate(where):
            if q % 2:
                nv[b, k] = bad_nv[(q // 2) % len(bad_nv)]
            else:
                x[b, k] = bad_x[(q // 2) % len(bad_x)]
        d.dropped[b, where] = True
    for q in range(M):                                              # a fully dropped row, by every means in turn
        if q % 2:
            nv[2, q] = bad_nv[(q // 2) % len(bad_nv)]
        else:
            x[2, q] = bad_x[(q // 2) % len(bad_x)]
    d.dropped[2, :M] = True
    d.x_hat, d.nvar = x, nv
    return _finish(d)


# ---- the stage-level chain: bits -> 16QAM -> precode -> selective gains + noise -> de-precoding -> LLRs ----
CHAIN_PRBS, CHAIN_SYMBOLS, CHAIN_RNTI, CHAIN_N_ID, CHAIN_SIGMA2 = 25, 12, 0x4601, 333, 5e-4
CHAIN_MARGIN = 0.5 / np.sqrt(10.0)        # half the distance from a 16QAM point to its nearest decision boundary


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """One slot of 25 PRB x 12 data symbols: random bits, scrambled, 16QAM, precoded, through a one-tap-per-RE channel of a
    three-tap impulse response with noise of variance CHAIN_SIGMA2, equalized per RE (x_hat = rx / h, nvar = sigma2 / |h|^2).
    The float64 reference keeps every output within CHAIN_MARGIN of the symbol sent, per axis (asserted here)."""
    M, S = 12 * CHAIN_PRBS, CHAIN_SYMBOLS
    rng = np.random.default_rng(4242)
    G = S * M * 4
    bits = rng.integers(0, 2, G).astype(np.uint8)
    x_tx = D.modulate((bits ^ D.scrambling(D.c_init(CHAIN_RNTI, CHAIN_N_ID), G))[None], 4)             # [1, S M]
    y = precode(x_tx, M)
    taps = np.array([1.0, 0.5, 0.3]) * np.exp(2j * np.pi * rng.random(3))
    h = (taps[None, :] * np.exp(-2j * np.pi * np.outer(np.arange(M), [0, 3, 7]) / M)).sum(-1)           # [M]: frequency-selective
    h = np.tile(h, S)[None]
    noise = (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)) * np.sqrt(CHAIN_SIGMA2 / 2.0)
    d = SimpleNamespace(M=M, S=S, B=1, bits=bits, x_tx=x_tx, x_hat=((h * y + noise) / h).astype(np.complex64),
                        nvar=(CHAIN_SIGMA2 / np.abs(h) ** 2).astype(np.float32))
    _finish(d)
    dev = d.ref_x - x_tx
    d.margin = float(max(np.abs(dev.real).max(), np.abs(dev.imag).max()))
    assert d.margin <= CHAIN_MARGIN, (d.margin, CHAIN_MARGIN)
    assert np.abs(h).min() < 0.5 * np.abs(h).max()                  # selective indeed
    llr = D.llr_ref(d.ref_x, d.ref_nv, 4)
    d.llr = np.where(D.scrambling(D.c_init(CHAIN_RNTI, CHAIN_N_ID), G).astype(bool)[None], -llr, llr)
    return d
