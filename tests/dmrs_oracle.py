"""Bit-serial numpy restatement of PUSCH DM-RS generation, written from TS 38.211 5.2.1 / 6.4.1.1.1.1 / 6.4.1.1.3 as
stated in include/ce_dmrs.h -- independent of the library's jump tables (it steps the two recurrences from n = 0).

No third-party vector ships with this repository: the anchors in test_dmrs.py were computed with this method and
cross-checked against the table method when the operator was specified."""
from __future__ import annotations

import hashlib

import numpy as np

from srsran_ce_pytorch_amd import synth as S

NC = 1600
A = np.array([0x3F3504F3], np.uint32).view(np.float32)[0]      # float32 0.70710677


# The anchor cases the operator was specified with: (case, slot, n_id, n_scid, n_symb_slot, grid_start_crb)
T1 = [S.TYPE1_CDM0, S.TYPE1_CDM1]
T2 = [S.TYPE2_CDM0, S.TYPE2_CDM1]
CASE_A = (S.case_spec("A", 273, [S.hop_spec([2, 11], 270, 3)], n_layers=1), 159, 65535, 1, 14, 0)
CASE_B = (S.case_spec("B", 52, [S.hop_spec([0, 4], 3, 3, 0, 14, T1), S.hop_spec([8, 12], 28, 3, 0, 14, T1)], n_layers=4), 7, 40, 0, 14, 0)
CASE_C = (S.case_spec("C", 25, [S.hop_spec([3], 5, 7, re_masks=T2)], n_layers=3), 19, 1007, 1, 14, 100)


def gold_bits(c_init: int, n: int) -> np.ndarray:
    """c(0) .. c(n-1) as uint8."""
    total = NC + n
    x1 = [1] + [0] * 30                                   # plain lists: the recurrences run element by element
    x2 = [(c_init >> i) & 1 for i in range(31)]
    for i in range(total - 31):
        x1.append(x1[i + 3] ^ x1[i])
        x2.append(x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i])
    return np.array(x1[NC:total], np.uint8) ^ np.array(x2[NC:total], np.uint8)


def gold_words(c_init: int, n_words: int):
    """Bit n of c in bit n % 32 of word n / 32."""
    bits = gold_bits(c_init, 32 * n_words).astype(np.uint64).reshape(n_words, 32)
    return [int((bits[w] << np.arange(32, dtype=np.uint64)).sum()) for w in range(n_words)]


def c_init(n_symb_slot: int, slot: int, sym: int, n_id: int, n_scid: int) -> int:
    return ((1 << 17) * (n_symb_slot * slot + sym + 1) * (2 * n_id + 1) + 2 * n_id + n_scid) % (1 << 31)


def hops_of(case):
    """`case`: a synth.case_spec dict -> the list of (dmrs symbol indices, maskPRBs bool [n_prb_grid], DMRSREmask bool [12, n_cdm])."""
    out = []
    for h in case["hops"]:
        mp = np.zeros(case["n_prb_grid"], bool)
        if h.get("mask_prbs") is not None:
            mp[h["mask_prbs"]] = True
        else:
            mp[h["prb_start"]: h["prb_start"] + h["n_prbs"]] = True
        out.append((sorted(h["dmrs_symbols"]), mp, np.array(h["re_masks"], bool).T.reshape(12, -1)))
    return out


def pilots_ref(case, slot: int, n_id: int, n_scid: int, n_symb_slot: int = 14, grid_start_crb: int = 0) -> np.ndarray:
    """[n_re, n_dmrs_total, L] complex64 for one slot."""
    L = case["n_layers"]
    hops = hops_of(case)
    n_cols = sum(len(sy) for sy, _, _ in hops)
    n_re = int(hops[0][1].sum() * hops[0][2][:, 0].sum())
    n_bits = 2 * 6 * (grid_start_crb + case["n_prb_grid"]) + 2
    out = np.zeros((n_re, n_cols, L), np.complex64)
    col = 0
    for syms, mp, rm in hops:
        for sym in syms:
            c = gold_bits(c_init(n_symb_slot, slot, sym, n_id, n_scid), n_bits).astype(np.int64)
            for l in range(L):
                mask = rm[:, l // 2]
                ppp = int(mask.sum())
                res = np.flatnonzero(np.kron(mp, mask))             # extraction order of the estimator (T:571-576)
                q, r = res // 12, res % 12
                j = np.array([int(mask[:rr].sum()) for rr in r])    # ordinal among the set bits of the PRB
                m = ppp * (grid_start_crb + q) + j
                w_f = np.where(m % 2 == 0, 1, -1) if l % 2 else 1
                out[:, col, l].real = A * (w_f * (1 - 2 * c[2 * m])).astype(np.float32)
                out[:, col, l].imag = A * (w_f * (1 - 2 * c[2 * m + 1])).astype(np.float32)
            col += 1
    return out


def sha16(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.complex64).tobytes()).hexdigest()[:16]
