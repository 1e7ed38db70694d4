"""Oracle of the PRACH preamble detector (include/ce_tp.h `ce_prach_detect`, `PrachDetector`), the seeded inputs its GPU tests
run on, and the rules they follow.

`detect_ref` is the operator of include/ce_tp.h in float64: the root table from a literal L x L DFT matrix, the zero-padded
inverse transform as a literal N x L matrix for N <= 512 and `np.fft.ifft` beyond, the windows from the integer formula.
`detect_f32` restates the kernel's float32 arithmetic -- the coherent sum over repetitions in ascending order, the table
product, the passes of `tp_oracle.passes_f32` over the radix sequence and the twiddle table of the library's host entry
points with float32(1 / L) in the last pass, re re + im im per term, row q of the workgroup summing the terms
q, q + rows_per_workgroup, .. and the rows then folded in ascending order, the sum for the mean in the kernel's order -- only to
calibrate the tolerance.

Tolerance rule for the profile, eps = 2^-24, m = mean_ref[b][i]:
    |P_got[n] - P_ref[n]| <= T_PRACH eps (log2(N) sqrt(P_ref[n] m) + P_ref[n] + eps log2(N)^2 m)
 * first term: the transform errs per term t by e_t with |e_t| ~ eps log2(N) rms_t (rms_t the rms of the term's N outputs), and
   |z_t + e_t|^2 - |z_t|^2 = 2 Re(conj(z_t) e_t) + |e_t|^2; by Cauchy-Schwarz over the terms sum_t |z_t| rms_t <= sqrt(P m);
 * second term: the scaling, the table product, the squares and the sum over the terms, each relative to the value;
 * third term: sum_t |e_t|^2, what is left where P_ref is near 0.
`peak` follows the rule at the index it was found at.  `mean` is (1 / N) sum_n P[n]: the mean of the rule over n is at most
T_PRACH eps m (log2(N) + 1 + eps log2(N)^2) (Cauchy-Schwarz again: mean_n sqrt(P[n] m) <= m), and its own sum of N terms adds
A = N / 256 - 1 + 8 roundings (per thread, per wave, across the waves) of at most eps m each:
    |mean_got - mean_ref| <= T_PRACH eps m (log2(N) + 1 + A + eps log2(N)^2)
T_PRACH = 4 C_PRACH_RECORDED, where C_PRACH is the largest ratio of `detect_f32`'s own error to those units over the inputs of
the GPU tests; the factor 4 is tp_oracle's, for FMA contraction and pass-internal ordering on the GPU that the restatement
cannot mirror.  tests/test_prach.py re-measures C_PRACH and fails if it exceeds C_PRACH_RECORDED.

Delay rule: a returned d is accepted where P_ref at its index is at least peak_ref minus the two tolerances involved (the one
at the returned index and the one at the oracle's).  In every window that carries a transmitted preamble the inputs are such
that the oracle's own gap between the largest and the second-largest value of the window exceeds GAP_TOLERANCES = 100 times
those two tolerances (tests/test_prach.py asserts it for every such window of every case); there d must equal the oracle's.

Detection: with threshold = sqrt(min hit ratio x max miss ratio) of the oracle, `detected` equals the transmitted set; the
inputs are such that min hit / max miss >= MIN_HIT_OVER_MISS = 4 on the oracle (asserted in tests/test_prach.py)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import tp_oracle as T

EPS = 2.0 ** -24
C_PRACH_RECORDED = 3.0     # measured 2.83 (test_prach.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T_PRACH = 4.0 * C_PRACH_RECORDED
GAP_TOLERANCES = 100.0
MIN_HIT_OVER_MISS = 4.0
MATRIX_MAX = 512
F = np.float32
L_RA = (139, 571, 839, 1151)
FFT_SIZES = (256, 512, 1024, 2048, 4096)


# ---- the operator in float64 ----

def zc(u: int, L: int) -> np.ndarray:
    """x_u(n) = exp(-j 2 pi ((u n (n + 1) / 2) mod L) / L), the index reduced in integers."""
    n = np.arange(L, dtype=np.int64)
    return np.exp(-2j * np.pi * (((n * (n + 1) // 2) % L * u) % L) / L)


@functools.lru_cache(maxsize=None)
def dft_matrix(L: int) -> np.ndarray:
    """W[k, n] = exp(-j 2 pi n k / L), the product n k reduced in integers."""
    n = np.arange(L, dtype=np.int64)
    w = np.exp(-2j * np.pi * ((n[:, None] * n[None, :]) % L) / L)
    w.setflags(write=False)
    return w


def root_freq(u: int, L: int) -> np.ndarray:
    """X_u[k] = sum_n x_u(n) exp(-j 2 pi n k / L), complex128 [L], by the literal matrix."""
    return dft_matrix(L) @ zc(u, L)


def root_table(roots, L: int) -> np.ndarray:
    """T_i[k] = conj(X_{u_i}[k]) / |X_{u_i}[k]|, complex128 [n_roots, L]."""
    x = np.stack([root_freq(int(u), L) for u in roots])
    return np.conj(x) / np.abs(x)


def windows(L: int, N: int, n_cs: int, n_shifts: int):
    """(win_start [n_shifts], win_len) by the integer formula of include/ce_tp.h."""
    if n_cs == 0:
        return np.zeros(1, np.int64), N
    g = -(-N // L)
    c = (L - np.arange(n_shifts, dtype=np.int64) * n_cs) % L
    return ((c * N) // L - g) % N, (n_cs * N) // L


def peak_position(L: int, N: int, c_v: int, delay: float) -> float:
    """The index of the N grid, fractional, at which the preamble of shift c_v arriving `delay` sequence samples late peaks."""
    return ((L - c_v + delay) % L) * N / L


def preamble_freq(u: int, c_v: int, L: int, delay: float = 0.0) -> np.ndarray:
    """The transmit side, complex128 [L], unit modulus: X_u[k] / sqrt(L) exp(+j 2 pi k (c_v - delay) / L)."""
    x = root_freq(u, L)
    return x / np.abs(x) * np.exp(2j * np.pi * np.arange(L) * ((c_v - delay) / L))


def terms_ref(y, combine: int) -> np.ndarray:
    """[B, R, S, L] -> the terms [B, n_terms, L] in the kernel's order (port-major), complex128."""
    y = np.asarray(y).astype(np.complex128)
    B, R, S, L = y.shape
    return y.sum(2) if combine else y.reshape(B, R * S, L)


def profile_ref(y, L: int, N: int, roots, combine: int) -> np.ndarray:
    """P[b][i][n] float64 [B, n_roots, N] of y [B, R, S, >= L]."""
    t = terms_ref(np.asarray(y)[..., :L], combine)                                        # [B, T, L]
    z = t[:, None, :, :] * root_table(roots, L)[None, :, None, :]                          # [B, n_roots, T, L]
    if N <= MATRIX_MAX:
        k, n = np.arange(L, dtype=np.int64), np.arange(N, dtype=np.int64)
        e = np.exp(2j * np.pi * ((n[:, None] * k[None, :]) % N) / N)                       # [N, L]
        tz = z @ e.T / L
    else:
        tz = np.fft.ifft(z, n=N, axis=-1) * (N / L)
    return (np.abs(tz) ** 2).sum(2)


def window_search(P, win_start, win_len: int):
    """(peak [.., n_shifts], delay [.., n_shifts] int64) of P [.., N]: the maximum of each window and the smallest d that attains it."""
    N = P.shape[-1]
    idx = (np.asarray(win_start, np.int64)[:, None] + np.arange(win_len)[None, :]) % N       # [n_shifts, win_len]
    w = P[..., idx]
    d = w.argmax(-1)
    return np.take_along_axis(w, d[..., None], -1)[..., 0], d


def detect_ref(y, L: int, N: int, roots, n_cs: int, n_shifts: int, combine: int):
    P = profile_ref(y, L, N, roots, combine)
    ws, wl = windows(L, N, n_cs, n_shifts)
    peak, delay = window_search(P, ws, wl)
    return SimpleNamespace(profile=P, mean=P.mean(-1), peak=peak, delay=delay, win_start=ws, win_len=wl)


# ---- the kernel's arithmetic in float32 numpy ----

def _mean_f32(P, N: int):
    """[rows, N] float32 -> [rows]: thread t adds P[t], P[t + 256], ..; a butterfly per wave; (w0 + w1) + (w2 + w3); times 1 / N."""
    rows = P.shape[0]
    v = P.reshape(rows, N // 256, 256)
    acc = np.zeros((rows, 256), F)
    for j in range(N // 256):
        acc = (acc + v[:, j]).astype(F)
    acc = acc.reshape(rows, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lane ^ off]).astype(F)
    w = acc[:, :, 0]
    return (((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F) * F(1.0 / N)).astype(F)


def detect_f32(y, L: int, view, tw, table, win_start, win_len: int, combine: int):
    """`view`, `tw` (complex64 [N]) and `table` (complex64 [n_roots, L]): the library's host view and tables."""
    N, rpw = int(view.m_sc), int(view.rows_per_workgroup)
    radix = [int(r) for r in view.radix[:view.n_passes]]
    y = np.asarray(y)[..., :L].astype(np.complex64)
    B, R, S, _ = y.shape
    yr, yi = y.real.astype(F), y.imag.astype(F)
    if combine:
        vr, vi = yr[:, :, 0], yi[:, :, 0]
        for s in range(1, S):
            vr, vi = (vr + yr[:, :, s]).astype(F), (vi + yi[:, :, s]).astype(F)
    else:
        vr, vi = yr.reshape(B, R * S, L), yi.reshape(B, R * S, L)
    nt = vr.shape[1]
    scale = F(1.0 / float(L))                                                              # in double, rounded once
    out = np.zeros((B, len(table), N), F)
    for i, t in enumerate(np.asarray(table).astype(np.complex64)):
        tr, ti = t.real.astype(F), t.imag.astype(F)
        re, im = np.zeros((B, nt, N), F), np.zeros((B, nt, N), F)
        re[..., :L] = ((vr * tr).astype(F) - (vi * ti).astype(F)).astype(F)
        im[..., :L] = ((vr * ti).astype(F) + (vi * tr).astype(F)).astype(F)
        re, im = T.passes_f32(re.reshape(-1, N), im.reshape(-1, N), radix, tw, scale)
        p = ((re * re).astype(F) + (im * im).astype(F)).astype(F).reshape(B, nt, N)
        rows = np.zeros((rpw, B, N), F)
        for term in range(nt):                                                             # row q: its terms in ascending order
            rows[term % rpw] = (rows[term % rpw] + p[:, term]).astype(F)
        acc = rows[0]
        for q in range(1, rpw):                                                            # the rows in ascending order
            acc = (acc + rows[q]).astype(F)
        out[:, i] = acc
    peak, delay = window_search(out, win_start, win_len)
    return SimpleNamespace(profile=out, mean=_mean_f32(out.reshape(-1, N), N).reshape(B, len(table)), peak=peak, delay=delay)


# ---- the rules ----

def profile_unit(P_ref, mean_ref, N: int) -> np.ndarray:
    """eps (log2(N) sqrt(P_ref m) + P_ref + eps log2(N)^2 m), the shape of P_ref [.., N] (or of P_ref [.., n_shifts] with the same m)."""
    lg, m = np.log2(N), np.asarray(mean_ref)[..., None]
    return EPS * (lg * np.sqrt(P_ref * m) + P_ref + EPS * lg * lg * m)


def mean_unit(mean_ref, N: int) -> np.ndarray:
    lg = np.log2(N)
    return EPS * np.asarray(mean_ref) * (lg + 1.0 + (N // 256 - 1 + 8) + EPS * lg * lg)


def _ratio(err, unit) -> float:
    """max err / unit, 0 / 0 counting as 0 (an all-zero occasion: exact zeros on both sides)."""
    err, unit = np.asarray(err, np.float64), np.asarray(unit, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / unit)
    return float(r.max()) if r.size else 0.0


def ratios(got, ref, N: int):
    """(profile ratio or None, peak ratio, mean ratio) of `got` (.peak, .delay, .mean and maybe .profile as arrays) against `ref`."""
    idx = (ref.win_start[None, None, :] + np.asarray(got.delay, np.int64)) % N                  # where each peak was found
    at = np.take_along_axis(ref.profile, idx, -1)
    r_peak = _ratio(np.abs(np.asarray(got.peak, np.float64) - at), profile_unit(at, ref.mean, N))
    r_mean = _ratio(np.abs(np.asarray(got.mean, np.float64) - ref.mean), mean_unit(ref.mean, N))
    r_prof = None
    if getattr(got, "profile", None) is not None:
        r_prof = _ratio(np.abs(np.asarray(got.profile, np.float64) - ref.profile), profile_unit(ref.profile, ref.mean, N))
    return r_prof, r_peak, r_mean


def check(got, d, what="", t=None):
    """The comparison every GPU test uses on a case `d` of `inputs`: the value rules, the delay rule, equality of the delay
    in the signal windows.  Prints the largest error ratios first and returns them."""
    t = T_PRACH if t is None else t
    ref, N = d.ref, d.N
    peak, delay, mean = np.asarray(got.peak), np.asarray(got.delay), np.asarray(got.mean)
    assert peak.dtype == np.float32 and mean.dtype == np.float32 and delay.dtype == np.int32, (what, peak.dtype, delay.dtype, mean.dtype)
    assert peak.shape == ref.peak.shape == delay.shape and mean.shape == ref.mean.shape, (what, peak.shape, delay.shape, mean.shape)
    assert np.all(np.isfinite(peak)) and np.all(np.isfinite(mean)), f"{what}: non-finite output"
    assert delay.min() >= 0 and delay.max() < ref.win_len, f"{what}: a delay outside 0..{ref.win_len - 1}"
    if getattr(got, "profile", None) is not None:
        assert np.asarray(got.profile).dtype == np.float32 and np.asarray(got.profile).shape == ref.profile.shape, what
    r_prof, r_peak, r_mean = ratios(got, ref, N)
    print(f"{what}: max error / unit: profile {'-' if r_prof is None else format(r_prof, '.2f')}, peak {r_peak:.2f}, mean {r_mean:.2f}  (bound {t:g})")
    assert (r_prof is None or r_prof <= t) and r_peak <= t and r_mean <= t, f"{what}: error ratios profile {r_prof}, peak {r_peak:.2f}, mean {r_mean:.2f} > {t:g}"
    # the delay rule: the value of the oracle at the returned index is within the two tolerances of the oracle's maximum
    idx = (ref.win_start[None, None, :] + delay.astype(np.int64)) % N
    idx_ref = (ref.win_start[None, None, :] + ref.delay) % N
    at = np.take_along_axis(ref.profile, idx, -1)
    slack = t * (profile_unit(at, ref.mean, N) + profile_unit(np.take_along_axis(ref.profile, idx_ref, -1), ref.mean, N))
    bad = np.argwhere(at < ref.peak - slack)
    assert not len(bad), f"{what}: delay {delay[tuple(bad[0])]} at (occasion, root, window) {tuple(bad[0])} is no maximum of the oracle's window (its delay: {ref.delay[tuple(bad[0])]})"
    for (b, i, v) in d.sent:                                                                     # an unambiguous peak: the oracle's own index
        assert delay[b, i, v] == ref.delay[b, i, v], f"{what}: delay {delay[b, i, v]} of the preamble at {(b, i, v)}, the oracle has {ref.delay[b, i, v]}"
    return r_prof, r_peak, r_mean


def signal_gaps(d):
    """Per transmitted preamble (b, i, v): (the oracle's gap between the largest and the second-largest value of the window,
    the two tolerances involved)."""
    ref, N, out = d.ref, d.N, []
    for (b, i, v) in d.sent:
        idx = (int(ref.win_start[v]) + np.arange(ref.win_len)) % N
        w = ref.profile[b, i, idx]
        o = np.argsort(w)[::-1]
        u = profile_unit(w[o[:2]], ref.mean[b, i], N)
        out.append((float(w[o[0]] - w[o[1]]), float(T_PRACH * (u[0] + u[1]))))
    return out


def hit_miss(d):
    """(min peak / mean over the transmitted (b, i, v), max over every other window of the occasions that carry signal or noise)."""
    ref = d.ref
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = ref.peak / ref.mean[..., None]
    sent = np.zeros(ratio.shape, bool)
    for s in d.sent:
        sent[s] = True
    live = np.array([k != "zero" for k in d.c["occasions"]])
    return float(ratio[sent].min()), float(ratio[~sent & live[:, None, None]].max())


def threshold(d) -> float:
    hit, miss = hit_miss(d)
    return float(np.sqrt(hit * miss))


# ---- the cases ----
# name: L, N, n_cs, n_shifts; R x S; combine; the occasions ("signal": three preambles on three roots plus noise, "noise",
# "zero"); the noise power per RE against unit preambles.  The smallest shapes that reach every path:
#   N = 256: 4 rows per workgroup of one wave each; 512: 2 rows of 2 waves; 1024: 2 rows; 2048, 4096: 1 row of 4 waves
#   3 x 1 and 5 x 1 terms on 4 rows, 3 x 1 on 2 rows: a last row group that is not full; 1 x 1; S = 12; both combine values
CASES = {
    "a_139_256_b3":     dict(L=139, N=256, n_cs=13, n_shifts=10, R=3, S=2, combine=0, occasions=("signal", "noise", "zero"), noise=0.25),
    "b_139_256_3x1":    dict(L=139, N=256, n_cs=13, n_shifts=10, R=3, S=1, combine=0, occasions=("signal",), noise=0.25),
    "c_139_256_5x2_coh": dict(L=139, N=256, n_cs=13, n_shifts=10, R=5, S=2, combine=1, occasions=("signal",), noise=0.25),
    "d_139_256_ncs69_1x1": dict(L=139, N=256, n_cs=69, n_shifts=2, R=1, S=1, combine=0, occasions=("signal",), noise=0.03),
    "e_139_512_circle_b3": dict(L=139, N=512, n_cs=0, n_shifts=1, R=3, S=1, combine=0, occasions=("signal", "zero", "noise"), noise=0.25),
    "f_139_256_1x12_coh": dict(L=139, N=256, n_cs=69, n_shifts=2, R=1, S=12, combine=1, occasions=("signal",), noise=0.25),
    "g_139_512_1x12":   dict(L=139, N=512, n_cs=13, n_shifts=10, R=1, S=12, combine=0, occasions=("signal",), noise=0.25),
    "h_839_1024_64win": dict(L=839, N=1024, n_cs=13, n_shifts=64, R=2, S=2, combine=0, occasions=("signal",), noise=0.25),
    "i_839_2048_b3_coh": dict(L=839, N=2048, n_cs=119, n_shifts=7, R=3, S=2, combine=1, occasions=("signal", "noise", "signal"), noise=0.25),
    "j_571_1024":       dict(L=571, N=1024, n_cs=30, n_shifts=19, R=2, S=1, combine=0, occasions=("signal",), noise=0.1),
    "k_1151_4096":      dict(L=1151, N=4096, n_cs=100, n_shifts=11, R=2, S=1, combine=0, occasions=("signal",), noise=0.1),
}
CASE_NAMES = list(CASES)


def case_roots(L: int):
    """Roots 1, L - 1 and one in between."""
    return (1, L - 1, L // 2 + 1)


def off_half_sample(L: int, N: int, c_v: int, delay: float) -> float:
    """The delay nearest to `delay` whose peak lies 0.2 samples behind an index of the N grid: away from the half-sample
    positions, where two neighbouring indices tie."""
    pos = (L - c_v + delay) * N / L
    return (np.floor(pos) + 0.2) * L / N - (L - c_v)


def case_preambles(c):
    """[(root index, shift v, delay in sequence samples)] of a signal occasion: a preamble in window 0 without delay, one in
    the last window 0.6 n_cs late (a fifth of the circle where n_cs = 0), one in a middle window 0.3 n_cs late; the late ones
    moved off the half-sample positions."""
    L, N, ncs, ns = c["L"], c["N"], c["n_cs"], c["n_shifts"]
    span = ncs if ncs else L / 3.0
    last, mid = ns - 1, ns // 2
    return [(0, 0, 0.0), (1, last, off_half_sample(L, N, last * ncs, 0.6 * span)), (2, mid, off_half_sample(L, N, mid * ncs, 0.3 * span))]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """A case's seeded complex64 y [B, R, S, L] (per preamble and port a seeded phase, the same over the repetitions; complex
    normal noise), the oracle's results `ref`, the transmitted (occasion, root index, window) triples `sent`; shared and read-only."""
    c = CASES[name]
    rng = np.random.default_rng(31000 + CASE_NAMES.index(name))
    L, N, R, S = c["L"], c["N"], c["R"], c["S"]
    roots, B = case_roots(L), len(c["occasions"])
    y = np.zeros((B, R, S, L), np.complex128)
    sent = []
    for b, kind in enumerate(c["occasions"]):
        if kind == "zero":
            continue
        y[b] = np.sqrt(c["noise"] / 2.0) * (rng.standard_normal((R, S, L)) + 1j * rng.standard_normal((R, S, L)))
        if kind == "signal":
            for (i, v, delay) in case_preambles(c):
                y[b] += np.exp(2j * np.pi * rng.random(R))[:, None, None] * preamble_freq(roots[i], v * c["n_cs"], L, delay)[None, None, :]
                sent.append((b, i, v))
    y = y.astype(np.complex64)
    ref = detect_ref(y, L, N, roots, c["n_cs"], c["n_shifts"], c["combine"])
    d = SimpleNamespace(c=c, name=name, L=L, N=N, roots=roots, y=y, ref=ref, sent=tuple(sent))
    for a in (y, ref.profile, ref.mean, ref.peak, ref.delay):
        a.setflags(write=False)
    return d
