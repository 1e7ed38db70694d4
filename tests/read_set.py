"""The read set of a slot: the grid REs the estimator's outputs may depend on, and nothing else.

The reference reads, per hop, ``rg[kron(maskPRBs, DMRSREmask[:, c])][:, DMRSsymbols]`` for the CDM groups
``c < ceil(L / 2)`` and never touches another RE of the grid (oracle/ce_oracle.py: process_hop, S1-S3).  Every kernel
variant must honour the same contract: an RE outside the set -- a data RE, another user's PRB, a symbol without DM-RS,
a CDM group the layers do not use -- cannot change any output, whatever it holds, Inf and NaN included.

Used by tests/test_read_set.py (CPU: the set pinned to the oracle) and tests/test_hip_read_set.py (GPU: every kernel
variant poisoned outside the set).  A plain module, not a conftest."""
from __future__ import annotations

import math

import numpy as np

from srsran_ce_pytorch_amd import synth as S


def hop_read_set(case, h) -> np.ndarray:
    """``bool[n_sc, n_sym]``: the REs hop ``h`` (a ``synth.hop_spec``) reads -- its pilot REs of the CDM groups the layers
    use, on its DM-RS symbols."""
    n_sc, n_sym = 12 * case["n_prb_grid"], case["n_sym"]
    ha = S._hop_arrays(case, h)
    out = np.zeros((n_sc, n_sym), bool)
    dmrs_ix = np.flatnonzero(ha.DMRSsymbols)
    for c in range(int(math.ceil(case["n_layers"] / 2))):
        sc = np.flatnonzero(np.kron(ha.maskPRBs, ha.DMRSREmask[:, c]))
        out[np.ix_(sc, dmrs_ix)] = True
    return out


def read_set(case) -> np.ndarray:
    """``bool[n_sc, n_sym]``: the union of the hops' read sets."""
    out = hop_read_set(case, case["hops"][0])
    for h in case["hops"][1:]:
        out |= hop_read_set(case, h)
    return out


def members(case, rng: np.random.Generator, n_random: int = 3):
    """``[(sc, sym)]``: a sample of the read set -- the first and the last RE of each hop on each of its DM-RS symbols,
    plus ``n_random`` members drawn from ``rng``."""
    out = []
    for h in case["hops"]:
        hs = hop_read_set(case, h)
        for sym in np.flatnonzero(hs.any(axis=0)):
            sc = np.flatnonzero(hs[:, sym])
            out += [(int(sc[0]), int(sym)), (int(sc[-1]), int(sym))]
    every = np.argwhere(read_set(case))
    out += [tuple(int(v) for v in every[i]) for i in rng.choice(len(every), size=min(n_random, len(every)), replace=False)]
    return list(dict.fromkeys(out))
