"""The low-PAPR PUSCH DM-RS of TS 38.211 6.4.1.1.1.2 / 5.2.2 (transform precoding on) as stated in include/ce_dmrs.h, run
literally: `fractions.Fraction` for q_bar, Python integers for the phase modulo 2 N_ZC, the bit-serial Gold generator of
tests/dmrs_oracle.py for the hopping bits, float64 `exp` rounded to complex64.  Independent of the library's tables: no jump
table, no index table, no twiddle table.

The phi tables of 38.211 5.2.2.2 (M_ZC <= 24) are not in this repository: `random_phi` draws a SEEDED RANDOM table of the right
shape and alphabet, which is all the generator's handling of a table can be tested with."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import dmrs_oracle as D

MODES = ("neither", "group", "sequence")


def largest_prime_below(m: int) -> int:
    return next(n for n in range(m - 1, 1, -1) if all(n % d for d in range(2, int(n ** 0.5) + 1)))


@functools.lru_cache(maxsize=None)
def _gold(c_init: int, n: int):
    return D.gold_bits(c_init, n)


def group_and_sequence(mode: str, n_symb_slot: int, slot: int, l: int, n_id: int, m_zc: int, frame_bits: int = 14 * 160):
    """(u, v) of one DM-RS symbol.  `frame_bits` only sizes the Gold run (the longest frame: 160 slots of 14 symbols)."""
    p = n_symb_slot * slot + l
    f_gh, v = 0, 0
    if mode == "group":
        c = _gold((n_id // 30) % (1 << 31), 8 * frame_bits)
        f_gh = sum((1 << m) * int(c[8 * p + m]) for m in range(8)) % 30
    elif mode == "sequence":
        if m_zc >= 72:
            v = int(_gold(n_id % (1 << 31), frame_bits)[p])
    else:
        assert mode == "neither", mode
    return (f_gh + n_id) % 30, v


def q_of(n_zc: int, u: int, v: int) -> int:
    q_bar = Fraction(n_zc * (u + 1), 31)
    return (q_bar + Fraction(1, 2)).__floor__() + v * (-1) ** ((2 * q_bar).__floor__())


def _unit(theta: np.ndarray) -> np.ndarray:
    r = np.exp(-1j * theta)
    r.imag += 0.0                                   # the phase 0 is (1, +0), not (1, -0)
    return r


def zc_phase(n_zc: int, q: int, n: np.ndarray):
    """The exact integer phase of x_q(n mod N_ZC) in units of pi / N_ZC, reduced modulo 2 N_ZC (Python integers)."""
    return [(q * t * (t + 1)) % (2 * n_zc) for t in (int(x) % n_zc for x in n)]


def base_sequence(m_zc: int, u: int, v: int, phi=None) -> np.ndarray:
    """r(0 .. M_ZC - 1), alpha = 0, complex128 before the one rounding."""
    n = np.arange(m_zc)
    if m_zc >= 36:
        n_zc = largest_prime_below(m_zc)
        ph = np.array(zc_phase(n_zc, q_of(n_zc, u, v), n), np.float64)
        return _unit(np.pi * ph / n_zc)
    if m_zc == 30:
        ph = np.array([((u + 1) * (int(k) + 1) * (int(k) + 2)) % 62 for k in n], np.float64)
        return _unit(np.pi * ph / 31)
    assert phi is not None and np.asarray(phi).shape == (30, m_zc), "M_ZC <= 24 needs a phi table"
    return np.exp(1j * np.asarray(phi, np.float64)[u] * np.pi / 4)


def pilots_ref(case, slot: int, n_id: int, mode: str = "neither", n_symb_slot: int = 14, phi=None) -> np.ndarray:
    """[n_re, n_dmrs_total, 1] complex64 for one slot of a synth.case_spec dict; `slot` is the slot number in the frame."""
    hops = D.hops_of(case)
    m_zc = 6 * int(hops[0][1].sum())
    cols = []
    for syms, mp, _ in hops:
        assert 6 * int(mp.sum()) == m_zc
        for l in syms:
            u, v = group_and_sequence(mode, n_symb_slot, slot, l, n_id, m_zc)
            cols.append(base_sequence(m_zc, u, v, phi))
    return np.stack(cols, 1)[:, :, None].astype(np.complex64)


def random_phi(m_zc: int, seed: int) -> np.ndarray:
    """A seeded random int8 [30, M_ZC] table over {-3, -1, 1, 3}: NOT the table of 38.211 5.2.2.2."""
    return np.random.default_rng(seed).choice(np.array([-3, -1, 1, 3], np.int8), size=(30, m_zc))
