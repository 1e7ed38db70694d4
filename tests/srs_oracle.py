"""Oracle of the SRS channel estimator (include/ce_tp.h `ce_srs_profile` / `ce_srs_estimate`, `SrsEstimator`), the seeded inputs
its GPU tests run on, and the rules they follow.

`sequence`, `profile_ref` and `estimate_ref` run the formulas of TS 38.211 6.4.1.4.2 / 5.2.2 / 5.2.1 and of include/ce_tp.h
literally in float64: the Gold sequence bit by bit with c_init = n_id, q from q_bar in floating point as the text has it, the
transform as a literal N x M matrix for N <= 512 and `np.fft.ifft` beyond.  `profile_f32` / `estimate_f32` restate the kernels'
float32 arithmetic in their orders (the products as written without FMA, `tp_oracle.passes_f32` over the library's radix sequence
and twiddles, the row fold, the per-thread / butterfly / four-wave sums) on the library's own tables -- only to calibrate the
tolerances.

Rules, eps = 2^-24:
 h_sb     |d h_sb[b,r,i,s,j]| <= T eps c_h(Q) sqrt(E_block),  E_block the mean |y|^2 over the block's Q elements of comb_i,
          c_h(Q) = Q + 10: every element is a product of y with three table values (three roundings of at most eps and three
          complex products of at most sqrt(5) eps each: below 10 eps), the serial sum of Q terms adds at most (Q - 1) eps of
          sum |g|, the scaling one more; (1 / Q) sum |g| <= sqrt(E_block) (Cauchy-Schwarz, |table values| = 1).
 h_wb     |d h_wb[b,r,i]| <= T eps (c_h(Q) + n_symb n_blocks) sqrt(epre): the mean of the rule above plus its own serial sum.
 noise    |d noise| <= T eps (sqrt(noise epre) + noise + eps epre): e = g - sum h rho errs by ~eps |g| per element, so
          |e + de|^2 - |e|^2 = 2 Re(conj(e) de) + |de|^2 sums to sqrt(noise epre) (Cauchy-Schwarz) and eps epre; the squares,
          the sum and the scaling are relative to the value.
 epre     |d epre| <= T eps c_e epre,  c_e = n_symb n_combs ceil(M / 256) + 10: the serial part of a thread's sum, six butterfly
          steps, two wave sums, the square and the scaling.
 profile  PRACH's rule (prach_oracle) with m the mean of the (b, r)'s full N-point profile:
          |d P[d']| <= T eps (log2(N) sqrt(P m) + P + eps log2(N)^2 m).
T = 4 C_RECORDED[quantity]; C is the largest ratio of the restatement's own error AGAINST THE FLOAT64 ORACLE to those units over
the GPU cases; the factor 4 is the project's margin for FMA contraction and pass-internal order.  tests/test_srs.py re-measures
every C and fails if one exceeds its recorded value or falls below a quarter of it.

Delay rule (as prach_oracle's): the returned delay is accepted where sum_r profile_ref at its index is within the two
tolerances (summed over r) of the maximum.  In every case the oracle's own gap between the largest and the second-largest value
of sum_r profile exceeds GAP_TOLERANCES = 100 such pairs (tests/test_srs.py asserts it for every item of every case), so the
delay must equal the oracle's."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import tp_oracle as T

EPS = 2.0 ** -24
F = np.float32
# measured 0.130, 0.072, 0.562, 0.235, 3.71 on the cases below (test_srs.py::test_float32_restatement_calibrates_the_tolerances
# prints them per case), rounded up
C_RECORDED = {"h_sb": 0.14, "h_wb": 0.08, "noise": 0.6, "epre": 0.25, "profile": 4.0}
TOL = {k: 4.0 * v for k, v in C_RECORDED.items()}
GAP_TOLERANCES = 100.0
MATRIX_MAX = 512
HOP = {"neither": 0, "group": 1, "sequence": 2}


# ---- TS 38.211 in float64 ----

def gold(c_init: int, n: int) -> np.ndarray:
    """c(0 .. n - 1) of 5.2.1, bit by bit: x1(n + 31) = x1(n + 3) + x1(n), x2(n + 31) = x2(n + 3) + x2(n + 2) + x2(n + 1) + x2(n), N_C = 1600."""
    nc = 1600
    x1, x2 = [0] * (nc + n + 31), [0] * (nc + n + 31)
    x1[0] = 1
    for i in range(31):
        x2[i] = (c_init >> i) & 1
    for i in range(nc + n):
        x1[i + 31] = (x1[i + 3] + x1[i]) % 2
        x2[i + 31] = (x2[i + 3] + x2[i + 2] + x2[i + 1] + x2[i]) % 2
    return np.array([(x1[i + nc] + x2[i + nc]) % 2 for i in range(n)], np.int64)


@functools.lru_cache(maxsize=None)
def _gold_cached(c_init: int, n: int):
    return gold(c_init, n)


def n_cs_max(k_tc: int) -> int:
    return {2: 8, 4: 12}[k_tc]


def ports(k_tc: int, n_ap: int, n_cs: int, k_bar: int):
    """[(comb_i, cs_i)], 6.4.1.4.2 (alpha_i) and 6.4.1.4.3 (k_TC^(p_i))."""
    ncs = n_cs_max(k_tc)
    out = []
    for i in range(n_ap):
        if n_ap == 4 and n_cs >= ncs // 2:
            cs = (n_cs + ncs * (i // 2) // 2) % ncs
            comb = (k_bar + k_tc // 2) % k_tc if i in (1, 3) else k_bar
        else:
            cs = (n_cs + ncs * i // n_ap) % ncs
            comb = k_bar
        out.append((comb, cs))
    return out


def largest_prime_below(m: int) -> int:
    n = m - 1
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n -= 1
    return n


def base_sequence(u: int, v: int, m: int, phi=None) -> np.ndarray:
    """rbar_{u,v}(n), 5.2.2.1 (m >= 36) and 5.2.2.2 (m = 12, 24, phi [30, m])."""
    if m >= 36:
        nzc = largest_prime_below(m)
        q_bar = nzc * (u + 1) / 31
        q = int(np.floor(q_bar + 0.5)) + v * (-1) ** int(np.floor(2 * q_bar))
        i = np.arange(m, dtype=np.int64) % nzc
        return np.exp(-1j * np.pi * ((q * i * (i + 1)) % (2 * nzc)) / nzc)        # the phase reduced in integers
    return np.exp(1j * np.asarray(phi, np.float64)[u] * np.pi / 4)


def hopping_uv(c, slot: int, n_id: int):
    """[(u, v)] per symbol of the case `c`; c_init = n_id in both modes."""
    out = []
    for s in range(c.n_symb):
        p = c.n_symb_slot * (int(slot) % c.slots_per_frame) + c.l0 + s
        f_gh = v = 0
        if c.hopping == "group":
            bits = _gold_cached(int(n_id), 8 * c.n_symb_slot * c.slots_per_frame)
            f_gh = sum(int(bits[8 * p + m]) << m for m in range(8)) % 30
        elif c.hopping == "sequence" and c.M >= 72:
            v = int(_gold_cached(int(n_id), 8 * c.n_symb_slot * c.slots_per_frame)[p])
        out.append(((f_gh + int(n_id)) % 30, v))
    return out


def rho(c) -> np.ndarray:
    """[n_ap, M]: exp(+j 2 pi cs_i n / n_cs_max)."""
    n = np.arange(c.M, dtype=np.int64)
    return np.stack([np.exp(2j * np.pi * ((cs * n) % c.n_cs_max) / c.n_cs_max) for _, cs in c.ports])


def base_rows(c, slot: int, n_id: int) -> np.ndarray:
    """[n_symb, M]: rbar of every symbol."""
    return np.stack([base_sequence(u, v, c.M, c.phi) for u, v in hopping_uv(c, slot, n_id)])


def sequence(c, slot: int, n_id: int) -> np.ndarray:
    """[n_ap, n_symb, M]: what port i transmits."""
    return rho(c)[:, None, :] * base_rows(c, slot, n_id)[None, :, :]


def comb_rows(c, y, comb: int) -> np.ndarray:
    """y [.., n_sym, >= n_sc] -> [.., n_symb, M]: the elements k(s, comb, n) of the symbols l0 + s."""
    return np.stack([y[..., c.l0 + s, 12 * c.start_prb[s] + comb:12 * c.start_prb[s] + comb + c.k_tc * c.M:c.k_tc] for s in range(c.n_symb)], -2)


def _item(v, b):
    v = np.asarray(v).reshape(-1)
    return int(v[b if v.size > 1 else 0])


def profile_full(c, y, slot, n_id) -> np.ndarray:
    """float64 [B, R, N]: sum over (s, i) of |z[d]|^2, z[d] = (1 / M) sum_n G_i[n] exp(+j 2 pi n d / N)."""
    y = np.asarray(y).astype(np.complex128)
    B, R = y.shape[:2]
    N, M = c.N, c.M
    out = np.zeros((B, R, N))
    r_all = rho(c)
    for b in range(B):
        base = base_rows(c, _item(slot, b), _item(n_id, b))
        for i, (comb, _) in enumerate(c.ports):
            g = comb_rows(c, y[b], comb) * np.conj(base)[None] * np.conj(r_all[i])[None, None]            # [R, n_symb, M]
            if N <= MATRIX_MAX:
                n, d = np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64)
                z = g @ np.exp(2j * np.pi * ((n[:, None] * d[None, :]) % N) / N) / M
            else:
                z = np.fft.ifft(g, n=N, axis=-1) * (N / M)
            out[b] += (np.abs(z) ** 2).sum(1)
    return out


def window(c, P) -> np.ndarray:
    """[.., N] -> [.., win_len]: the indices (d' - g) mod N."""
    return P[..., (np.arange(c.win_len) - c.g) % c.N]


def delay_of(c, prof) -> np.ndarray:
    """int64 [B]: argmax_d' sum_r profile[b][r][d'] - g."""
    return np.asarray(prof).sum(1).argmax(-1) - c.g


def estimate_ref(c, y, slot, n_id, delay):
    y = np.asarray(y).astype(np.complex128)
    B, R = y.shape[:2]
    M, Q, nb = c.M, c.Q, c.n_blocks
    n = np.arange(M, dtype=np.int64)
    r_all = rho(c)
    h_sb = np.zeros((B, R, c.n_ap, c.n_symb, nb), np.complex128)
    num, en = np.zeros((B, R)), np.zeros((B, R))
    for b in range(B):
        base = base_rows(c, _item(slot, b), _item(n_id, b))
        d = _item(delay, b) % c.N if delay is not None else 0
        w = np.exp(2j * np.pi * ((n * d) % c.N) / c.N)
        for comb in c.combs:
            yc = comb_rows(c, y[b], comb)                                                                   # [R, n_symb, M]
            g = yc * np.conj(base)[None] * w[None, None]
            e = g.copy()
            for i, (ci, _) in enumerate(c.ports):
                if ci == comb:
                    h = (g * np.conj(r_all[i])[None, None]).reshape(R, c.n_symb, nb, Q).sum(-1) / Q
                    h_sb[b, :, i] = h
                    e = e - np.repeat(h, Q, axis=-1) * r_all[i][None, None]
            num[b] += (np.abs(e) ** 2).sum((1, 2))
            en[b] += (np.abs(yc) ** 2).sum((1, 2))
    dof = c.n_symb * c.n_combs * M - c.n_symb * c.n_ap * M // Q
    return SimpleNamespace(h_sb=h_sb, h_wb=h_sb.mean((3, 4)), noise=num / dof, epre=en / (c.n_symb * c.n_combs * M))


def block_energy(c, y) -> np.ndarray:
    """float64 [B, R, n_ap, n_symb, n_blocks]: the mean |y|^2 over each block's Q elements of the port's comb."""
    y = np.asarray(y).astype(np.complex128)
    return np.stack([(np.abs(comb_rows(c, y, comb)) ** 2).reshape(*y.shape[:2], c.n_symb, c.n_blocks, c.Q).mean(-1) for comb, _ in c.ports], 2)


# ---- the kernels' arithmetic in float32 numpy ----

def _mul(a, b):
    return ((a[0] * b[0]).astype(F) - (a[1] * b[1]).astype(F)).astype(F), ((a[0] * b[1]).astype(F) + (a[1] * b[0]).astype(F)).astype(F)


def _mulc(a, b):
    """a conj(b) = (a.re b.re + a.im b.im, a.im b.re - a.re b.im)."""
    return ((a[0] * b[0]).astype(F) + (a[1] * b[1]).astype(F)).astype(F), ((a[1] * b[0]).astype(F) - (a[0] * b[1]).astype(F)).astype(F)


def _ri(z):
    z = np.asarray(z).astype(np.complex64)
    return z.real.astype(F), z.imag.astype(F)


def _sq(a):
    return ((a[0] * a[0]).astype(F) + (a[1] * a[1]).astype(F)).astype(F)


def base_rows_f32(c, lib, slot: int, n_id: int):
    """[n_symb, M] complex64 from the library's tables: W[(q tri[n]) mod N_ZC], or the four values by phi."""
    rows = []
    for u, v in hopping_uv(c, slot, n_id):
        if c.M >= 36:
            rows.append(lib.w[(int(lib.hv.q[u, v]) * lib.hv.tri.astype(np.int64)) % lib.hv.n_zc])
        else:
            rows.append(lib.w[(np.asarray(c.phi)[u].astype(np.int64) + 3) // 2])
    return np.stack(rows)


def _thread_sums_f32(chunks, inv):
    """`chunks`: per (s, comb) in order a float32 [rows, M]; thread t adds n = t, t + 256, .. of each chunk in turn; a butterfly
    per wave; (w0 + w1) + (w2 + w3); times `inv`."""
    rows = chunks[0].shape[0]
    acc = np.zeros((rows, 256), F)
    for ch in chunks:
        M = ch.shape[1]
        pad = np.zeros((rows, -(-M // 256) * 256), F)
        pad[:, :M] = ch
        for j in range(pad.shape[1] // 256):
            acc = (acc + pad[:, 256 * j:256 * (j + 1)]).astype(F)
    acc = acc.reshape(rows, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lane ^ off]).astype(F)
    w = acc[:, :, 0]
    return (((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F) * F(inv)).astype(F)


def profile_f32(c, lib, y, slot, n_id) -> np.ndarray:
    """float32 [B, R, win_len]; `lib`: the library's host view and tables (`library`)."""
    y = np.asarray(y).astype(np.complex64)
    B, R = y.shape[:2]
    N, M, rpw = c.N, c.M, int(lib.hv.view.rows_per_workgroup)
    radix = [int(r) for r in lib.hv.view.radix[:lib.hv.view.n_passes]]
    n = np.arange(M)
    terms = []
    for s in range(c.n_symb):
        for i, (comb, _) in enumerate(c.ports):
            re, im = np.zeros((B, R, N), F), np.zeros((B, R, N), F)
            for b in range(B):
                base = _ri(base_rows_f32(c, lib, _item(slot, b), _item(n_id, b))[s])
                v = _ri(comb_rows(c, y[b], comb)[:, s])
                g = _mulc(_mulc(v, base), _ri(lib.rho[i][n % c.n_cs_max]))
                re[b, :, :M], im[b, :, :M] = g
            zr, zi = T.passes_f32(re.reshape(-1, N), im.reshape(-1, N), radix, lib.tw, F(1.0 / M))
            terms.append(_sq((zr, zi)).reshape(B, R, N))
    rows = np.zeros((rpw, B, R, N), F)
    for t, p in enumerate(terms):
        rows[t % rpw] = (rows[t % rpw] + p).astype(F)
    acc = rows[0]
    for q in range(1, rpw):
        acc = (acc + rows[q]).astype(F)
    return window(c, acc)


def estimate_f32(c, lib, y, slot, n_id, delay):
    y = np.asarray(y).astype(np.complex64)
    B, R = y.shape[:2]
    M, Q, nb, ncs = c.M, c.Q, c.n_blocks, c.n_cs_max
    n = np.arange(M)
    h_sb = np.zeros((B, R, c.n_ap, c.n_symb, nb), np.complex64)
    ch_n, ch_e = [], []
    for s in range(c.n_symb):
        for comb in c.combs:
            gr, gi, v_all = np.zeros((B, R, M), F), np.zeros((B, R, M), F), []
            for b in range(B):
                base = _ri(base_rows_f32(c, lib, _item(slot, b), _item(n_id, b))[s])
                d = _item(delay, b) % c.N if delay is not None else 0
                v = _ri(comb_rows(c, y[b], comb)[:, s])
                v_all.append(_sq(v))
                gr[b], gi[b] = _mul(_mulc(v, base), _ri(lib.tw[(n * d) % c.N]))
            er, ei = gr.copy(), gi.copy()
            for i, (ci, _) in enumerate(c.ports):
                if ci != comb:
                    continue
                rr, ri_ = _ri(lib.rho[i])
                ar, ai = np.zeros((B, R, nb), F), np.zeros((B, R, nb), F)
                g4r, g4i = gr.reshape(B, R, nb, Q), gi.reshape(B, R, nb, Q)
                for k in range(Q):
                    pr, pi = _mulc((g4r[..., k], g4i[..., k]), (rr[k % ncs], ri_[k % ncs]))
                    ar, ai = (ar + pr).astype(F), (ai + pi).astype(F)
                hr, hi = (F(1.0 / Q) * ar).astype(F), (F(1.0 / Q) * ai).astype(F)
                h_sb[:, :, i, s] = hr + 1j * hi
                pr, pi = _mul((np.repeat(hr, Q, -1), np.repeat(hi, Q, -1)), (rr[n % ncs], ri_[n % ncs]))
                er, ei = (er - pr).astype(F), (ei - pi).astype(F)
            ch_n.append(_sq((er, ei)).reshape(B * R, M))
            ch_e.append(np.stack(v_all).reshape(B * R, M))
    dof = c.n_symb * c.n_combs * M - c.n_symb * c.n_ap * M // Q
    noise = _thread_sums_f32(ch_n, 1.0 / dof).reshape(B, R)
    epre = _thread_sums_f32(ch_e, 1.0 / (c.n_symb * c.n_combs * M)).reshape(B, R)
    flat = h_sb.reshape(B, R, c.n_ap, c.n_symb * nb)
    ar, ai = np.zeros((B, R, c.n_ap), F), np.zeros((B, R, c.n_ap), F)
    for k in range(c.n_symb * nb):
        ar, ai = (ar + flat[..., k].real).astype(F), (ai + flat[..., k].imag).astype(F)
    inv = F(1.0 / (c.n_symb * nb))
    return SimpleNamespace(h_sb=h_sb, h_wb=((inv * ar).astype(F) + 1j * (inv * ai).astype(F)).astype(np.complex64), noise=noise, epre=epre)


# ---- the rules ----

def c_h(Q: int) -> float:
    return Q + 10.0


def units(c, d):
    """The rules' units (without T) of a case's inputs `d`: a dict of arrays shaped like the outputs."""
    ref, lg = d.est, np.log2(c.N)
    m = d.full.mean(-1)[..., None]
    return {
        "h_sb": EPS * c_h(c.Q) * np.sqrt(d.e_block),
        "h_wb": EPS * (c_h(c.Q) + c.n_symb * c.n_blocks) * np.sqrt(ref.epre)[..., None] * np.ones((1, 1, c.n_ap)),
        "noise": EPS * (np.sqrt(ref.noise * ref.epre) + ref.noise + EPS * ref.epre),
        "epre": EPS * (c.n_symb * c.n_combs * -(-c.M // 256) + 10.0) * ref.epre,
        "profile": EPS * (lg * np.sqrt(d.prof * m) + d.prof + EPS * lg * lg * m),
    }


def _ratio(err, unit) -> float:
    err, unit = np.asarray(err, np.float64), np.asarray(unit, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / unit)
    return float(r.max()) if r.size else 0.0


def ratios(d, prof=None, est=None) -> dict:
    """Per quantity the largest |got - ref| / unit of a profile [B, R, win_len] and / or an estimate (arrays) against the case's oracle."""
    u, out = units(d.c, d), {}
    if prof is not None:
        out["profile"] = _ratio(np.abs(np.asarray(prof, np.float64) - d.prof), u["profile"])
    if est is not None:
        for k in ("h_sb", "h_wb", "noise", "epre"):
            out[k] = _ratio(np.abs(np.asarray(getattr(est, k)).astype(np.complex128 if k[0] == "h" else np.float64) - getattr(d.est, k)), u[k])
    return out


def check(d, prof=None, delay=None, est=None, what=""):
    """The comparison every GPU test uses on a case's inputs `d`: the value rules, the delay rule, equality of the delay.
    Prints the ratios first and returns them."""
    c = d.c
    r = ratios(d, prof, est)
    print(f"{what}: max error / unit: " + ", ".join(f"{k} {v:.3f} (bound {TOL[k]:g})" for k, v in r.items()))
    if prof is not None:
        assert np.asarray(prof).dtype == np.float32 and np.asarray(prof).shape == d.prof.shape and np.all(np.isfinite(prof)), what
    if est is not None:
        assert est.h_sb.dtype == np.complex64 == est.h_wb.dtype and est.noise.dtype == np.float32 == est.epre.dtype, what
        assert est.h_sb.shape == d.est.h_sb.shape and est.h_wb.shape == d.est.h_wb.shape and est.noise.shape == d.est.noise.shape == est.epre.shape, what
    for k, v in r.items():
        assert v <= TOL[k], f"{what}: {k} error ratio {v:.3f} > {TOL[k]:g}"
    if delay is not None:
        delay = np.asarray(delay)
        assert delay.dtype == np.int32 and delay.shape == d.delay.shape, (what, delay.dtype, delay.shape)
        assert delay.min() >= -c.g and delay.max() < c.win_len - c.g, f"{what}: a delay outside the window"
        tot, unit = d.prof.sum(1), TOL["profile"] * units(c, d)["profile"].sum(1)
        for b in range(len(delay)):
            at, best = int(delay[b]) + c.g, int(d.delay[b]) + c.g
            assert tot[b, at] >= tot[b, best] - (unit[b, at] + unit[b, best]), f"{what}: delay {delay[b]} of item {b} is no maximum of the oracle's profile"
            assert delay[b] == d.delay[b], f"{what}: delay {delay[b]} of item {b}, the oracle has {d.delay[b]}"
    return r


def gaps(d):
    """Per item: (the oracle's gap between the largest and the second-largest value of sum_r profile, the two tolerances involved)."""
    tot, unit = d.prof.sum(1), TOL["profile"] * units(d.c, d)["profile"].sum(1)
    out = []
    for b in range(tot.shape[0]):
        o = np.argsort(tot[b])[::-1]
        out.append((float(tot[b, o[0]] - tot[b, o[1]]), float(unit[b, o[0]] + unit[b, o[1]])))
    return out


# ---- the cases ----
# (k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, N, R, B), and what the geometry leaves open: l0, start_prb per symbol, the grid
GEOMETRIES = {
    "a_c4_4p_one_comb_m36": dict(k_tc=4, n_ap=4, n_cs=0, k_bar=1, m_srs=12, n_symb=2, N=128, R=3, B=2, l0=11, start_prb=(2, 2), n_prb_grid=15),
    "b_c4_4p_two_combs":    dict(k_tc=4, n_ap=4, n_cs=7, k_bar=3, m_srs=16, n_symb=1, N=128, R=2, B=1, l0=13, start_prb=(0,), n_prb_grid=16),
    "c_c2_4p_m144_4sym":    dict(k_tc=2, n_ap=4, n_cs=5, k_bar=0, m_srs=24, n_symb=4, N=256, R=2, B=3, l0=8, start_prb=(3, 0, 5, 2), n_prb_grid=30,
                                 slot=(3, 17, 1033), n_id=(777, 60, 1023)),
    "d_c2_1p_m24_phi":      dict(k_tc=2, n_ap=1, n_cs=0, k_bar=0, m_srs=4, n_symb=1, N=128, R=1, B=1, l0=0, start_prb=(1,), n_prb_grid=6),
    "e_c4_2p_m12_phi":      dict(k_tc=4, n_ap=2, n_cs=11, k_bar=2, m_srs=4, n_symb=2, N=128, R=1, B=2, l0=5, start_prb=(0, 2), n_prb_grid=6),
    "f_c2_2p_m1632":        dict(k_tc=2, n_ap=2, n_cs=3, k_bar=1, m_srs=272, n_symb=1, N=2048, R=2, B=1, l0=12, start_prb=(1,), n_prb_grid=273),
    "g_c2_1p_m408_r5":      dict(k_tc=2, n_ap=1, n_cs=6, k_bar=1, m_srs=68, n_symb=1, N=512, R=5, B=1, l0=3, start_prb=(4,), n_prb_grid=75),
    # beyond the issue's table: N = 4096 fills the profile kernel's 64 KiB with its buffers, so the gather reads W from memory
    "h_c2_2p_m408_n4096":   dict(k_tc=2, n_ap=2, n_cs=1, k_bar=0, m_srs=68, n_symb=2, N=4096, R=1, B=1, l0=6, start_prb=(0, 3), n_prb_grid=72),
}
# every hopping mode where it changes the result: group hopping always, sequence hopping where M >= 72
CASES = [(g, h) for g, v in GEOMETRIES.items() for h in ("neither", "group", "sequence") if h != "sequence" or 12 * v["m_srs"] // v["k_tc"] >= 72]
CASE_IDS = [f"{g}-{h}" for g, h in CASES]
SIGMA = 0.05


def case(geometry: str, hopping: str = "neither", **over):
    """The plan values of a geometry and what follows from them."""
    v = {**GEOMETRIES[geometry], **over}
    c = SimpleNamespace(name=geometry, hopping=hopping, n_sym=14, n_symb_slot=14, slots_per_frame=20, slot=(7,), n_id=(777,), win_len=None, phi=None)
    c.__dict__.update(v)
    c.n_cs_max = n_cs_max(c.k_tc)
    c.M, c.Q, c.n_blocks, c.n_sc = 12 * c.m_srs // c.k_tc, 48 // c.k_tc, c.m_srs // 4, 12 * c.n_prb_grid
    c.ports = ports(c.k_tc, c.n_ap, c.n_cs, c.k_bar)
    c.combs = list(dict.fromkeys(comb for comb, _ in c.ports))
    c.n_combs = len(c.combs)
    c.g = -(-c.N // c.M)
    fullest = max(sum(1 for comb, _ in c.ports if comb == k) for k in c.combs)
    if c.win_len is None:
        c.win_len = c.N * (c.n_cs_max // fullest) // c.n_cs_max - c.g
    if c.M < 36 and c.phi is None:
        c.phi = np.random.default_rng(4100 + c.M).integers(0, 4, (30, c.M)) * 2 - 3                        # seeded, not the standard's table
    return c


def case_delays(c):
    """Per item: 0, a negative delay inside the guard, one near the window's end; by the geometry's position for B = 1."""
    pool = [0, -1, c.win_len - c.g - 2, 1, -(c.g - 1), c.win_len - c.g - 1]
    k = list(GEOMETRIES).index(c.name) if c.name in GEOMETRIES else 0
    return np.array([pool[(k + b) % len(pool)] for b in range(c.B)], np.int64)


def draw(c, seed: int):
    """(y complex64 [B, R, n_sym, n_sc], gains [B, R, n_ap], delays [B]): unit-variance clutter on every RE the estimator must
    not read, and on the used combs sum_i H beta r_i exp(-j 2 pi k delay / (N k_tc)) + noise of sigma = SIGMA."""
    rng = np.random.default_rng(seed)
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)                 # noqa: E731
    y = cn(c.B, c.R, c.n_sym, c.n_sc)
    H = cn(c.B, c.R, c.n_ap) + 0.5
    delays = case_delays(c)
    n = np.arange(c.M)
    for b in range(c.B):
        seq = sequence(c, _item(c.slot, b), _item(c.n_id, b))
        for comb in c.combs:
            for s in range(c.n_symb):
                k = 12 * c.start_prb[s] + comb + c.k_tc * n
                tx = sum(H[b, :, i, None] * seq[i, s][None, :] for i, (ci, _) in enumerate(c.ports) if ci == comb)
                y[b][:, c.l0 + s, k] = tx *np.exp(-2j * np.pi * k * delays[b] / (c.N * c.k_tc))[None, :] + SIGMA * cn(c.R, c.M)
    return y.astype(np.complex64), H, delays


def finish(c, y, H=None, delays=None):
    """The oracle's results on `y`: the full and the windowed profile, the delay, the estimate at that delay, the block energies."""
    slot, n_id = np.array(c.slot, np.int64), np.array(c.n_id, np.int64)
    full = profile_full(c, y, slot, n_id)
    prof = window(c, full)
    delay = delay_of(c, prof)
    est = estimate_ref(c, y, slot, n_id, delay)
    d = SimpleNamespace(c=c, y=y, H=H, sent=delays, slot=slot, n_id=n_id, full=full, prof=prof, delay=delay, est=est, e_block=block_energy(c, y))
    for a in (y, full, prof, delay, est.h_sb, est.h_wb, est.noise, est.epre):
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(geometry: str, hopping: str = "neither"):
    """A case's seeded inputs and the oracle's results; shared and read-only."""
    c = case(geometry, hopping)
    y, H, delays = draw(c, 52000 + 10 * list(GEOMETRIES).index(geometry) + HOP[hopping])
    return finish(c, y, H, delays)


def plan_kwargs(c) -> dict:
    """The keyword arguments of `SrsEstimator` / `srs.derive_host` for the case (without the device)."""
    return dict(k_tc=c.k_tc, n_ap=c.n_ap, n_cs=c.n_cs, k_bar=c.k_bar, m_srs=c.m_srs, n_prb_grid=c.n_prb_grid, n_fft=c.N, n_symb=c.n_symb, l0=c.l0,
                start_prb=list(c.start_prb), n_sym=c.n_sym, n_symb_slot=c.n_symb_slot, hopping=c.hopping, slots_per_frame=c.slots_per_frame,
                win_len=c.win_len, phi_table=c.phi)


@functools.lru_cache(maxsize=None)
def library(geometry: str, hopping: str = "neither"):
    """The library's host view and tables of a case (no GPU)."""
    from srsran_ce_pytorch_amd import srs as S
    c = case(geometry, hopping)
    hv = S.derive_host(**plan_kwargs(c))
    tw, w, rho_t = S.tables(c.k_tc, c.n_ap, c.n_cs, c.k_bar, c.m_srs, c.N)
    return SimpleNamespace(hv=hv, tw=tw, w=w, rho=rho_t)
