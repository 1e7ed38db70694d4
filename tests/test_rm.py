"""CPU-side checks of the rate-recovery extension (include/ce_rm.h): the ABI, the host derivation against the oracle's
(the pinned table of the cases and a sweep of the transport block size on both base graphs), every refusal of the
descriptor before any device call, select_base_graph, the Python argument checks that need no device, the oracle against
a plain-loop accumulation, and the kernel's gather arithmetic (rank, k mod P, the float32-reciprocal divisions) restated
in numpy against the oracle's literal walk over every index of every case.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import rm_oracle as R
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, ratematch as RM

IDS = [c["name"] for c in R.CASES]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _lib_derive(c, dtype=torch.int8):
    return RM.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], dtype, c["n_ref"])


def _same(v, d):
    got = dict(B=v.b, K_cb=v.k_cb, C=v.c, Bp=v.b_prime, Kp=v.k_prime, K_b=v.k_b, Zc=v.zc, K=v.k, N=v.n, N_cb=v.n_cb, f0=v.f0, f1=v.f1,
               P=v.p, k0=tuple(v.k0), E=[v.e_lo] * v.n_lo + [v.e_hi] * (v.c - v.n_lo))
    want = {k: getattr(d, k) for k in got}
    assert got == want, (got, want)


def test_library_exports_every_declared_rm_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies."""
    # LP64 sizes implied by the header: desc 9*4 + 4 = 40; info 4*4 + 8 = 24; view 16*4 + 2*16 + 3*4 = 108
    assert (C.sizeof(_lib.RmDesc), C.sizeof(_lib.RmInfo), C.sizeof(_lib.RmHostView)) == (40, 24, 108)
    assert "ce_rm.h" in _lib.REGISTRY and "ce_rm.hip" in _lib.SOURCES and R.MAX_BITS == _lib.CE_DEMOD_MAX_BITS
    assert PKG.PuschRateRecovery is RM.PuschRateRecovery and PKG.select_base_graph is RM.select_base_graph


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_pinned_derivation_of_the_cases(lib, c):
    d = R.case_derive(c)
    for key, val in c["pinned"].items():
        assert getattr(d, key) == val, (key, getattr(d, key), val)
    for dtype in (torch.int8, torch.float32):
        v = _lib_derive(c, dtype)
        _same(v, d)
        assert v.unit_elems == (4 if dtype == torch.int8 else 1)
        assert v.tiles_per_block == -(-((d.N_cb + 2 * (v.unit_elems - 1)) // v.unit_elems) // _lib.CE_RM_TILE_UNITS)
        assert v.n_tiles == d.C * v.tiles_per_block
    rm = RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], n_ref=c["n_ref"])
    assert (rm.n_code_blocks, rm.n_cb, rm.zc, rm.e, rm.filler_range, rm.k0) == (d.C, d.N_cb, d.Zc, d.E, (d.f0, d.f1), d.k0)
    # positions hit more than once / left untouched are as the case says
    for rv in range(4):
        blk, pos, _ = R.slot_map(d, rv)
        hits = np.zeros((d.C, d.N_cb), np.int64)
        np.add.at(hits, (blk, pos), 1)
        assert hits.sum() == d.G and not hits[:, d.f0:d.f1].any()
        live = np.delete(hits, np.s_[d.f0:d.f1], axis=1)
        if c["rep"]:
            assert live.min() >= 1 and live.max() == -(-max(d.E) // d.P) and 3 <= live.max() <= 4
        else:
            assert live.max() == 1 and max(d.E) <= d.P
    if c["name"] == "bg1_a96_k0_in_filler":
        assert d.f0 <= d.k0[1] < d.f1 and live.size - int(live.sum()) == 136
    if c["name"] == "bg1_a8448_lbrm":
        assert d.k0[3] + d.E[0] > d.N_cb                     # rv 3 wraps the shortened buffer


def test_host_derivation_sweep_against_the_oracle(lib):
    """A swept over the thresholds of 5.2.2 on both base graphs: the library derives what the oracle derives, and
    refuses where the oracle refuses."""
    sweep = sorted({*range(1, 700, 7), 176, 177, 544, 545, 624, 625, 292, 293, 3808, 3824, 3825, 3840, 8424, 8425, *range(700, 30000, 331),
                    *range(30000, 1300000, 45007), 1277992})
    n_ok = n_refused = 0
    for bg in (1, 2):
        for A in sweep:
            for qm, L in ((2, 1), (6, 3), (8, 4)):
                B = A + (24 if A > 3824 else 16)
                c_est = max(1, -(-B // ((8448 if bg == 1 else 3840) - 24)))
                G = qm * L * (c_est + 3 + A % 5)
                if G > R.MAX_BITS:
                    continue
                try:
                    d = R.derive(bg, A, qm, L, G)
                except ValueError:
                    with pytest.raises(ValueError):
                        RM.derive_host(bg, A, qm, L, G)
                    n_refused += 1
                    continue
                _same(RM.derive_host(bg, A, qm, L, G), d)
                n_ref = d.K - 2 * d.Zc + (A % 3) * d.Zc
                _same(RM.derive_host(bg, A, qm, L, G, n_ref=n_ref), R.derive(bg, A, qm, L, G, n_ref))
                n_ok += 1
    print(f"sweep: {n_ok} descriptors derived alike, {n_refused} refused alike")
    assert n_ok > 500 and n_refused > 0
    assert R.ZC_SET[:6] == [2, 3, 4, 5, 6, 7] and R.ZC_SET[-1] == 384 and len(R.ZC_SET) == 51


def test_every_refusal_comes_before_any_device_call(lib):
    good = dict(base_graph=1, tbs=8448, modulation=8, n_layers=1, n_bits=12008, dtype=torch.float32, n_ref=0, filler_llr=20.0)
    d = R.derive(1, 8448, 8, 1, 12008)
    assert RM.derive_host(**good).c == 2
    bad = [dict(base_graph=0), dict(base_graph=3), dict(modulation=3), dict(modulation=10), dict(n_layers=0), dict(n_layers=5),
           dict(tbs=0), dict(tbs=-5),
           dict(tbs=8449),                                             # B = 8473 over C = 2 blocks
           dict(base_graph=2, tbs=3825),                               # B = 3849 > K_cb of BG2, C = 2, odd
           dict(n_bits=12004),                                         # no multiple of L Qm
           dict(n_bits=8),                                             # q = 1 < C = 2
           dict(n_bits=0), dict(n_bits=_lib.CE_DEMOD_MAX_BITS + 8),
           dict(n_ref=d.K - 2 * d.Zc - 1), dict(n_ref=1), dict(n_ref=-1),
           dict(filler_llr=0.0), dict(filler_llr=-1.0), dict(filler_llr=float("nan")), dict(filler_llr=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            RM.derive_host(**{**good, **kw})
        with pytest.raises(ValueError):
            RM.PuschRateRecovery(**{**good, **kw})
    assert RM.derive_host(**{**good, "n_ref": d.K - 2 * d.Zc}).n_cb == d.K - 2 * d.Zc
    assert RM.derive_host(**{**good, "n_bits": _lib.CE_DEMOD_MAX_BITS}).e_lo == _lib.CE_DEMOD_MAX_BITS // 2
    assert RM.derive_host(**{**good, "dtype": torch.int8, "filler_llr": float("nan")}).c == 2      # int8 ignores filler_llr
    with pytest.raises(ValueError, match="dtype"):
        RM.derive_host(**{**good, "dtype": torch.float16})
    with pytest.raises(ValueError, match="bpsk"):
        RM.derive_host(**{**good, "modulation": "bpsk"})
    # K' > K_b 384 cannot be reached through segmentation (K' <= K_cb = K_b 384 on both graphs): the check is defensive
    assert 22 * 384 == 8448 and 10 * 384 == 3840
    # plan creation refuses each before it touches a device; the format code has no Python spelling
    for field, val in (("abi_version", _lib.CE_ABI_VERSION + 1), ("format", 2), ("base_graph", 3), ("qm", 5), ("n_layers", 9), ("tbs", 0),
                       ("g_bits", 12004), ("n_ref", 1), ("filler_llr", float("nan"))):
        desc = RM.build_desc(1, 8448, 8, 1, 12008, torch.float32, 0, 20.0)
        setattr(desc, field, val)
        handle, view = C.c_void_p(), _lib.RmHostView()
        assert lib.ce_rm_plan_create(C.byref(desc), C.byref(handle)) == _lib.CE_ERR_INVALID and not handle.value, field
        assert lib.ce_rm_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID, field
    # more outputs per slot than the kernel's index arithmetic covers: unsupported, not invalid
    with pytest.raises(NotImplementedError, match="outputs per slot"):
        RM.derive_host(1, 8424 * 700 - 24, 2, 1, 2 * 700)
    # the host entry points refuse a null plan and accept an empty batch without a device
    assert lib.ce_rm_recover(None, None, None, 0, 0, None, None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_rm_plan_get_info(None, None) == _lib.CE_ERR_INVALID


def test_select_base_graph():
    for tbs, rate, bg in ((292, 0.9, 2), (293, 0.9, 1), (3824, 0.67, 2), (3824, 0.68, 1), (3825, 0.67, 1), (3825, 0.25, 2), (100000, 0.25, 2),
                          (100000, 0.26, 1), (1, 0.01, 2), (24, 1.0, 2)):
        assert RM.select_base_graph(tbs, rate) == bg == R.select_base_graph(tbs, rate), (tbs, rate)
    for tbs, rate in ((0, 0.5), (100, 0.0), (100, 1.5)):
        with pytest.raises(ValueError):
            RM.select_base_graph(tbs, rate)


def test_oracle_accumulates_in_source_order():
    """np.add.at against a plain Python loop on the smallest repetition case, both formats, with a kept buffer."""
    x = R.inputs("bg2_a24_rep")
    for llr, harq in ((x.llr_f32, x.harq_f32), (x.llr_i8, x.harq_i8)):
        a, hits = R.recover(x.d, llr, R.rvs_of(1), harq, R.FILLER)
        b = R.recover_loop(x.d, llr, R.rvs_of(1), harq, R.FILLER)
        assert a.dtype == llr.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) and hits.max() == 4
    # a reversed order gives another float32 result somewhere: the order is observable
    blk, pos, kk = R.slot_map(x.d, 1)
    fwd = np.zeros((x.d.C, x.d.N_cb), np.float32)
    rev = np.zeros_like(fwd)
    order = np.lexsort((kk, blk))
    np.add.at(fwd, (blk[order], pos[order]), x.llr_f32[0][order])
    np.add.at(rev, (blk[order[::-1]], pos[order[::-1]]), x.llr_f32[0][order[::-1]])
    assert not np.array_equal(fwd, rev)


def _divmod_f32(a, d):
    """ce_divmod of csrc/ce_segment.h: a float32 product with the float32 reciprocal, truncated, one correction either way."""
    inv = np.float32(1.0) / np.float32(d)
    q = (a.astype(np.float32) * inv).astype(np.int64)
    m = a - q * d
    q = np.where(m < 0, q - 1, np.where(m >= d, q + 1, q))
    m = a - q * d
    return q, m


def check_gather_arithmetic(d, v, unit, slots, rvs=range(4)):
    """The closed form of include/ce_rm.h exactly as csrc/ce_rm.hip evaluates it -- the buffers of the slots `slots` cut at
    the 4-byte grid of the output into units of 1 (float32) or 4 (int8) elements, (k, j, i) divided out once per unit and
    stepped from element to element, a second hit divided again -- under every rv of `rvs`: each source index lies inside
    the block's part of the row and belongs to that position in the oracle's map, every position of a buffer is visited
    by exactly one unit, and every element of the row is read exactly once.  `d` is the oracle's derivation, `v` the
    library's host view of the same descriptor in the format of `unit`."""
    qm, nf = d.qm, d.f1 - d.f0
    assert v.unit_elems == unit
    for rv in rvs:
        blk, pos, kk = R.slot_map(d, rv)
        s = int(v.s[rv])
        assert s == (d.k0[rv] if d.k0[rv] < d.f0 else d.f0 if d.k0[rv] < d.f1 else d.k0[rv] - nf)
        for b in slots:
            seen = np.zeros(d.G, np.int64)
            for r in range(d.C):
                e_r = v.e_lo if r < v.n_lo else v.e_hi
                base = r * v.e_lo if r < v.n_lo else v.n_lo * v.e_lo + (r - v.n_lo) * v.e_hi
                eq = e_r // qm
                assert e_r == d.E[r] and base == sum(d.E[:r])
                lead = ((b * d.C + r) * d.N_cb) % unit
                n_units = (lead + d.N_cb + unit - 1) // unit
                assert n_units <= v.tiles_per_block * _lib.CE_RM_TILE_UNITS
                n0 = np.arange(n_units, dtype=np.int64) * unit - lead
                first = np.maximum(n0, 0)
                rank = np.where(first < d.f0, first, np.where(first < d.f1, d.f0, first - nf))
                k = np.where(rank >= s, rank - s, rank + d.P - s)
                k = np.where(k >= d.P, k - d.P, k)
                assert k.min() >= 0 and k.max() < d.P
                j, i = _divmod_f32(k, eq)
                assert np.array_equal(j, k // eq) and np.array_equal(i, k % eq)
                visited = np.zeros(d.N_cb, np.int64)
                for el in range(unit):
                    n = n0 + el
                    valid = (n >= 0) & (n < d.N_cb)
                    np.add.at(visited, n[valid], 1)
                    live = valid & ~((n >= d.f0) & (n < d.f1))
                    hit = live & (k < e_r)
                    src = base + i[hit] * qm + j[hit]
                    assert src.size == 0 or (src.min() >= base and src.max() < base + e_r)
                    assert np.all(blk[src] == r) and np.array_equal(pos[src], n[hit]) and np.array_equal(kk[src], k[hit])
                    seen[src] += 1
                    n2, k2 = n[hit], k[hit] + d.P
                    while np.any(k2 < e_r):
                        n2, k2 = n2[k2 < e_r], k2[k2 < e_r]
                        j2, i2 = _divmod_f32(k2, eq)
                        assert np.array_equal(j2, k2 // eq) and np.array_equal(i2, k2 % eq)
                        src = base + i2 * qm + j2
                        assert src.min() >= base and src.max() < base + e_r
                        assert np.all(blk[src] == r) and np.array_equal(pos[src], n2) and np.array_equal(kk[src], k2)
                        seen[src] += 1
                        k2 = k2 + d.P
                    # the step to the next non-filler position
                    k = np.where(live, k + 1, k)
                    i = np.where(live, i + 1, i)
                    carry = live & (i == eq)
                    i, j = np.where(carry, 0, i), np.where(carry, j + 1, j)
                    wrap = live & (k == d.P)
                    k, i, j = np.where(wrap, 0, k), np.where(wrap, 0, i), np.where(wrap, 0, j)
                assert np.all(visited == 1)
            assert np.all(seen == 1)


@pytest.mark.parametrize("unit", [1, 4], ids=["f32", "i8"])
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_kernel_gather_arithmetic_against_the_literal_walk(lib, c, unit):
    """check_gather_arithmetic over every index of every case: three slots, every rv, both formats."""
    check_gather_arithmetic(R.case_derive(c), _lib_derive(c, torch.int8 if unit == 4 else torch.float32), unit, range(R.N_SLOTS))


def test_reciprocal_division_is_exact_below_2_pow_21():
    """ce_divmod at the multiples of d and their predecessors, where a truncated estimate is most likely to be off by
    more than the one step it corrects: a sample of divisors up to 2^20, every multiple below 2^21 (the dividend is a
    k < max(P, E_r) <= 2^21)."""
    rng = np.random.default_rng(5)
    for d in sorted({1, 2, 3, 5, 7, 350, 396, 9000, 13728, 25344, 2 ** 20, *rng.integers(1, 2 ** 20, 40).tolist()}):
        top = 2 ** 21
        m = np.arange(1, (top - 1) // d + 1, dtype=np.int64) * d
        a = np.unique(np.concatenate([m, m - 1, np.array([0, top - 1])]))
        q, rem = _divmod_f32(a, d)
        assert np.array_equal(q, a // d) and np.array_equal(rem, a % d), d
