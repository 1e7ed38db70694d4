"""tests/read_set.py pinned to the oracle (CPU): nothing outside the read set changes the oracle's outputs (NaN everywhere
else gives the same bits, complex128 and complex64), and every sampled member is read (a NaN there makes the EPRE NaN).

Cases: every named standard shape of tests/kernel_variants.py, one seeded representative per (smoothing, interpolator)
(in a grid of at most 106 PRB: the oracle's cost),
and slots whose DM-RS RE mask carries both CDM groups while the layers use only the first (a set that wrongly took CDM
group 1 in fails the member test on the band's last RE)."""
import zlib

import numpy as np
import pytest

import ce_oracle as O
import kernel_variants as K
import read_set as RS
from srsran_ce_pytorch_amd import synth as S


def _cases():
    out = [(name, *K.case_of(point, name, seed=7000 + i)) for i, (name, point) in enumerate(K.NAMED.items())]
    rng = np.random.default_rng(20261016)
    reps = K.representatives()
    for smoothing in K.SMOOTHINGS:
        for interp in K.INTERPS:
            # "mean" selects what "none" selects, so no representative carries it: a "none" one is re-run with "mean"
            pool = [r for r in reps if r[2]["smoothing"] == ("none" if smoothing == "mean" else smoothing) and r[3] == interp
                    and r[2]["n_prb_grid"] <= 106]
            vid, _, case, _ = pool[int(rng.integers(len(pool)))]
            out.append((f"{vid}-{smoothing}", dict(case, smoothing=smoothing), interp))
    both = [S.TYPE1_CDM0, S.TYPE1_CDM1]
    out.append(("cdm1_unused_L1", S.case_spec("cdm1_unused_L1", 52, [S.hop_spec([2, 9], 10, 25, re_masks=both)], n_layers=1, seed=41), "linear"))
    out.append(("cdm1_unused_L2_2hop", S.case_spec(
        "cdm1_unused_L2_2hop", 52, [S.hop_spec([0, 3], 0, 6, 0, 7, [S.TYPE2_CDM0, S.TYPE2_CDM1]),
                                    S.hop_spec([7, 10], 40, 6, 7, 7, [S.TYPE2_CDM0, S.TYPE2_CDM1])],
        n_layers=2, smoothing="none", seed=42), "cnn"))
    return out


CASES = _cases()


def _run(b, grid, interp, dtype):
    return O.srs_channel_estimator(grid.astype(dtype), b.pilots.astype(dtype), b.beta, b.hop1, b.hop2, b.config, interp=interp)


def _same_bits(a, b):
    if a is None or b is None:                                        # cfo: "not estimated"
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_read_set_of_a_split_slot():
    """Hand-checked: two 1-PRB hops, type-1 comb (even REs), 2 layers -> 6 REs x 2 symbols per hop; CDM group 1 unused."""
    case = S.case_spec("rs", 4, [S.hop_spec([2, 5], 1, 1, 0, 7, [S.TYPE1_CDM0, S.TYPE1_CDM1]),
                                 S.hop_spec([9, 12], 3, 1, 7, 7, [S.TYPE1_CDM0, S.TYPE1_CDM1])], n_layers=2)
    want = np.zeros((48, 14), bool)
    want[np.ix_(range(12, 24, 2), [2, 5])] = True
    want[np.ix_(range(36, 48, 2), [9, 12])] = True
    assert np.array_equal(RS.read_set(case), want)
    case["n_layers"] = 3
    want[np.ix_(range(13, 24, 2), [2, 5])] = True
    want[np.ix_(range(37, 48, 2), [9, 12])] = True
    assert np.array_equal(RS.read_set(case), want)


@pytest.mark.parametrize("name,case,interp", CASES, ids=[c[0] for c in CASES])
def test_oracle_reads_the_read_set_and_nothing_else(name, case, interp):
    b = S.build_case(case, 1)
    rs = RS.read_set(case)
    clean = b.grids[0]
    poisoned = np.full_like(clean, np.nan)
    poisoned[rs] = clean[rs]
    for dtype in (np.complex128, np.complex64):                       # superset: NaN outside the set changes no bit
        want, got = _run(b, clean, interp, dtype), _run(b, poisoned, interp, dtype)
        for k, (w, g) in enumerate(zip(want, got)):
            assert _same_bits(w, g), f"{name} {np.dtype(dtype).name}: output {k} depends on an RE outside the read set"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for sc, sym in RS.members(case, rng):                             # every sampled member is read
        one = clean.copy()
        one[sc, sym] = np.nan
        epre = _run(b, one, interp, np.complex64)[3]
        assert np.isnan(epre), f"{name}: RE ({sc}, {sym}) is in the read set but the oracle does not read it"
