"""CPU-side checks of the low-PAPR DM-RS generator (include/ce_dmrs.h `ce_dmrs_lp_*`, `PuschLowPaprDmrs`): the library's host
derivation (N_ZC, q[u][v], the triangular index table, the hopping tables combined as the kernel combines them) against the
literal oracle of tests/dmrs_lp_oracle.py, the twiddle table bit for bit, the oracle's own properties, every refusal with
its text, the registry and the wrapper's parameter checks.  No GPU.

The phi tables of 38.211 5.2.2.2 are not in this repository: where an allocation of 1 to 4 PRB is tested, the table is a
seeded random one (dmrs_lp_oracle.random_phi)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import dmrs_lp_oracle as LP
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, dmrs, synth as S

N_PRBS = [5, 6, 7, 12, 24, 273, 341]
TWIDDLE_N = [31, 41, 61, 71, 139, 1637, 2039]      # every N the CPU and GPU tests of this generator use


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def hops(n_prb, n_prb_grid=None, start=0, syms=(2, 11), mask=S.TYPE1_CDM0, syms2=None, start2=None, n_sym=14):
    specs = [S.hop_spec(list(syms), start, n_prb, re_masks=[mask])]
    if syms2 is not None:
        specs.append(S.hop_spec(list(syms2), start if start2 is None else start2, n_prb, re_masks=[mask]))
    case = S.case_spec(f"lp{n_prb}", n_prb_grid or n_prb + start, specs, n_sym=n_sym)
    return case, S.numpy_hops(case)[:2]


@pytest.mark.parametrize("n_prb", N_PRBS)
def test_sequence_tables_against_the_oracle(lib, n_prb):
    case, (h1, h2) = hops(n_prb)
    view = dmrs.derive_host_low_papr(h1, h2, n_prb, hopping="sequence")
    m_zc = 6 * n_prb
    assert (view.n_re, view.n_dmrs_total, view.n_prb, view.col_sym) == (m_zc, 2, n_prb, [2, 11]) and view.v_live == (m_zc >= 72)
    if n_prb == 5:                                                           # the length-30 form: W_31[(u + 1) (n + 1) (n + 2) / 2]
        assert (view.form, view.n_zc) == (_lib.CE_DMRS_LP_FORM_30, 31)
        assert [list(r) for r in view.q] == [[u + 1, u + 1] for u in range(30)]
        assert list(view.tri) == [((k + 1) * (k + 2) // 2) % 31 for k in range(30)]
        return
    n_zc = LP.largest_prime_below(m_zc)
    assert (view.form, view.n_zc) == (_lib.CE_DMRS_LP_FORM_ZC, n_zc)
    assert [list(r) for r in view.q] == [[LP.q_of(n_zc, u, v) for v in (0, 1)] for u in range(30)]       # all 60 pairs, exact fractions
    assert list(view.tri) == [((k % n_zc) * (k % n_zc + 1) // 2) % n_zc for k in range(m_zc)]
    for u, v in ((0, 0), (7, 1), (29, 1)):                                   # the index form is the exact integer phase
        e = (int(view.q[u][v]) * view.tri.astype(np.int64)) % n_zc
        assert list(2 * e) == LP.zc_phase(n_zc, LP.q_of(n_zc, u, v), np.arange(m_zc))


@pytest.mark.parametrize("spf,nss", [(10, 14), (160, 14), (20, 12), (40, 14), (80, 12)])
def test_hopping_tables_against_the_bit_serial_oracle(lib, spf, nss):
    """(f_gh, v) from the library's tables -- row 0 XOR the rows of the set bits of c_init, the kernel's combination -- for every
    slot of the frame, every symbol and a seeded set of n_id."""
    n_ids = [0, 29, 30, 1007] + [int(x) for x in np.random.default_rng(11).integers(0, 1008, 4)]
    case, (h1, h2) = hops(12, n_sym=nss)
    for mode in ("group", "sequence"):
        view = dmrs.derive_host_low_papr(h1, h2, 12, nss, hopping=mode, slots_per_frame=spf, n_symb_slot=nss)
        n_pos = nss * spf
        assert view.n_words == (-(-n_pos // 4) if mode == "group" else -(-n_pos // 32)) <= _lib.CE_DMRS_LP_MAX_WORDS
        for n_id in n_ids:
            c_init = n_id // 30 if mode == "group" else n_id
            words = view.hop_words[0].copy()
            for i in range(31):
                if c_init >> i & 1:
                    words ^= view.hop_words[1 + i]
            p = np.arange(n_pos)
            if mode == "group":
                got = ((words[p >> 2] >> (8 * (p & 3)).astype(np.uint32)) & 0xFF) % 30
            else:
                got = (words[p >> 5] >> (p & 31).astype(np.uint32)) & 1
            want = [LP.group_and_sequence(mode, nss, slot, l, n_id, 72) for slot in range(spf) for l in range(nss)]
            if mode == "group":
                assert [((f + n_id) % 30, 0) for f in got.tolist()] == want, (mode, n_id)
            else:
                assert [(n_id % 30, v) for v in got.tolist()] == want, (mode, n_id)
    assert dmrs.derive_host_low_papr(h1, h2, 12, nss, n_symb_slot=nss).n_words == 0
    # below 72 subcarriers the sequence number stays 0 and the plan says so
    _, (g1, g2) = hops(11)
    assert not dmrs.derive_host_low_papr(g1, g2, 11, hopping="sequence").v_live


def _tie_distance(x: np.ndarray) -> np.ndarray:
    """Distance of the float64 values x from the nearest float32 rounding tie, in float32 ulps."""
    ulp = np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    return np.abs(np.mod(x / ulp, 1.0) - 0.5)


@pytest.mark.parametrize("n", TWIDDLE_N)
def test_twiddles_bitwise_and_clear_of_rounding_ties(lib, n):
    """W_N against numpy's float64 cos / -sin rounded to float32, bit for bit.  A bitwise claim must not rest on a libm: two
    correct libms differ by an ulp of float64, 2^-29 of a float32 ulp, so every entry is required to lie at least 1e-6 ulp
    from a float32 rounding tie."""
    th = 2 * np.pi * np.arange(n) / n
    re, im = np.cos(th), -np.sin(th)
    im[0] = 0.0
    want = (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)
    got = dmrs.low_papr_twiddles(n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.view(np.uint32)[0] == 0x3F800000 and got.view(np.uint32)[1] == 0           # W[0] = (1, +0)
    d = min(_tie_distance(re[1:]).min(), _tie_distance(im[1:]).min())
    print(f"N={n}: closest float32 rounding tie at {d:.3e} ulp")
    assert d >= 1e-6


def test_oracle_self_checks():
    for m_zc, phi in ((12, LP.random_phi(12, 1)), (30, None), (36, None), (72, None), (1638, None)):
        for u, v in ((0, 0), (13, 1), (29, 0)):
            assert np.abs(np.abs(LP.base_sequence(m_zc, u, v, phi)) - 1).max() < 1e-12
    for n_zc in (31, 71, 1637):                                              # one period of x_q: constant amplitude, flat spectrum
        for q in (1, n_zc // 2, n_zc - 1):
            x = np.exp(-1j * np.pi * np.array(LP.zc_phase(n_zc, q, np.arange(n_zc)), np.float64) / n_zc)
            mag = np.abs(np.fft.fft(x))
            assert mag.max() / mag.min() - 1 < 1e-9, (n_zc, q)
    # the rows behind one period repeat it: r(n) = x_q(n mod N_ZC)
    r = LP.base_sequence(36, 4, 0)
    assert np.array_equal(r[31:], r[:5])
    # Why the design reduces the phase index in integers: pi q m (m + 1) / N_ZC formed in float32 is off by far more than
    # rounding at 273 PRB (the float32 product m (m + 1) q has lost its low bits long before the division).
    n_zc, q = 1637, LP.q_of(1637, 29, 0)
    m = np.arange(1638) % n_zc
    f = np.float32
    naive = np.exp(-1j * (f(np.pi) * f(q) * m.astype(f) * (m.astype(f) + f(1)) / f(n_zc)).astype(np.float64))
    assert np.abs(naive - LP.base_sequence(1638, 29, 0)).max() > 0.1
    # the length-30 form and q: anchors worked by hand
    assert LP.q_of(31, 0, 0) == 1 and LP.q_of(31, 29, 1) == 31 and LP.largest_prime_below(1638) == 1637 and LP.largest_prime_below(2046) == 2039
    assert LP.q_of(71, 0, 0) == 2 and LP.q_of(71, 0, 1) == 3 and LP.q_of(71, 1, 1) == 4    # q_bar = 71/31: 2 q_bar = 4.58 even; 142/31: 9.16 odd


def _c_derive(lib, n_prb_grid=24, n_sym=14, nss=14, n_layers=1, n_hops=1, sym=None, re_mask=(0x555, 0x555), prbs=None,
              hopping=0, spf=10, phi=None, null=()):
    sym = np.zeros((2, 14), np.uint8) if sym is None else sym
    if not sym.any():
        sym[0, [2, 11]] = 1
    if prbs is None:
        prbs = np.zeros((2, n_prb_grid), np.uint8)
        prbs[:, 3:9] = 1
    rm = np.array(re_mask, np.uint16)
    ptr = lambda name, a: None if name in null or a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    info = np.zeros(8, np.int32)
    rc = lib.ce_dmrs_lp_derive_host(n_prb_grid, n_sym, nss, n_layers, n_hops, ptr("sym", sym), ptr("re_mask", rm), ptr("prbs", prbs),
                                    hopping, spf, ptr("phi", phi), C.c_void_p(info.ctypes.data), None, None, None, None)
    return rc, _lib.last_error() if rc else "", info


def test_every_refusal_with_its_text(lib):
    rc, _, info = _c_derive(lib)
    assert rc == 0 and list(info[:4]) == [36, 2, 0, 31]
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    gap = np.zeros((2, 24), np.uint8)
    gap[:, [3, 4, 5, 7, 8, 9]] = 1
    unequal = np.zeros((2, 24), np.uint8)
    unequal[0, 3:9], unequal[1, 3:10] = 1, 1
    two = np.zeros((2, 14), np.uint8)
    two[0, 2], two[1, 11] = 1, 1
    same = np.zeros((2, 14), np.uint8)
    same[0, 2], same[1, 2] = 1, 1
    small = np.zeros((2, 24), np.uint8)
    small[:, 3:5] = 1
    bad_phi = LP.random_phi(12, 3)
    bad_phi[17, 5] = 2
    refused = [
        (dict(prbs=gap), UNS, "hop 0: the 6 active PRBs are not one contiguous run"),
        (dict(prbs=unequal, sym=two, n_hops=2), INV, "hop 1 has 7 active PRBs, hop 0 has 6"),
        (dict(re_mask=(0x0C3, 0x555)), INV, "hop 0: re_mask=0x0c3 is not a configuration type 1 mask (0x555 0xAAA)"),
        (dict(re_mask=(0x555, 0x554), sym=two.copy(), n_hops=2), INV, "hop 1: re_mask=0x554"),
        (dict(n_layers=2), UNS, "n_layers=2: low-PAPR DM-RS is single-layer"),
        (dict(n_layers=0), UNS, "n_layers=0"),
        (dict(hopping=3), INV, "hopping=3 is not one of neither (0), group (1), sequence (2)"),
        (dict(hopping=-1), INV, "hopping=-1"),
        (dict(spf=15), INV, "slots_per_frame=15, expected 10, 20, 40, 80 or 160"),
        (dict(spf=0), INV, "slots_per_frame=0"),
        (dict(spf=320), INV, "slots_per_frame=320"),
        (dict(null=("sym",)), INV, "null argument"),
        (dict(null=("re_mask",)), INV, "null argument"),
        (dict(null=("prbs",)), INV, "null argument"),
        (dict(n_hops=3), INV, "n_hops=3 outside 1..2"),
        (dict(n_prb_grid=342, prbs=np.ones((2, 342), np.uint8)), UNS, "grid of 342 PRB"),
        (dict(nss=13), INV, "n_symb_slot=13, expected 14 or 12"),
        (dict(nss=12), INV, "n_sym=14 outside 1..n_symb_slot=12"),
        (dict(sym=same, n_hops=2), INV, "Hops should not overlap."),
        (dict(prbs=np.zeros((2, 24), np.uint8)), INV, "hop 0: mask_prbs has no active PRB"),
        (dict(prbs=small), UNS, "M_ZC=12 (2 PRB) needs the phi table of 38.211 5.2.2.2"),
        (dict(prbs=small, phi=bad_phi), INV, "phi[17][5]=2 is not one of -3, -1, 1, 3"),
    ]
    for kw, code, text in refused:
        rc, err, _ = _c_derive(lib, **kw)
        assert rc == code and text in err, (kw.keys(), rc, err)
    rc, _, info = _c_derive(lib, prbs=small, phi=LP.random_phi(12, 3))
    assert rc == 0 and list(info[:4]) == [12, 2, _lib.CE_DMRS_LP_FORM_PHI, 0]
    # plan creation refuses the same values, and a foreign ABI, before any device call; generate refuses a null plan
    handle = C.c_void_p()
    sym, rm, prbs = np.zeros((1, 14), np.uint8), np.array([0x555], np.uint16), np.ones((1, 6), np.uint8)
    sym[0, 3] = 1
    args = (6, 14, 14, 1, 1, C.c_void_p(sym.ctypes.data), C.c_void_p(rm.ctypes.data), C.c_void_p(prbs.ctypes.data))
    assert lib.ce_dmrs_lp_plan_create(_lib.CE_ABI_VERSION + 1, 0, *args, 0, 10, None, C.byref(handle)) == INV and "ABI" in _lib.last_error()
    assert lib.ce_dmrs_lp_plan_create(_lib.CE_ABI_VERSION, 0, *args, 5, 10, None, C.byref(handle)) == INV and "hopping=5" in _lib.last_error()
    assert lib.ce_dmrs_lp_plan_create(_lib.CE_ABI_VERSION, 0, *args, 0, 10, None, None) == INV and not handle.value
    assert lib.ce_dmrs_lp_generate(None, None, 0, None, 0, 1, None, None) == INV and "null argument" in _lib.last_error()
    assert lib.ce_dmrs_lp_copy_twiddles(1, None) == INV and lib.ce_dmrs_lp_copy_twiddles(31, None) == INV
    w = np.zeros(4, np.complex64)
    assert lib.ce_dmrs_lp_copy_twiddles(1, C.c_void_p(w.ctypes.data)) == INV and "n=1 outside 2..2048" in _lib.last_error()


def test_the_wrapper_maps_the_refusals_to_exceptions(lib):
    _, (h1, h2) = hops(6, 24, 3)
    gen = dmrs.PuschLowPaprDmrs(h1, h2, 24)
    assert (gen.n_re, gen.n_dmrs_total, gen.n_layers, gen.n_prb) == (36, 2, 1, 6)
    scattered = S.case_spec("s", 24, [S.hop_spec([2], 0, 3, mask_prbs=[1, 2, 5])])
    with pytest.raises(NotImplementedError, match="not one contiguous run"):
        dmrs.PuschLowPaprDmrs(*S.numpy_hops(scattered)[:2], 24)
    unequal = S.case_spec("u", 24, [S.hop_spec([2], 0, 6), S.hop_spec([11], 8, 7)])
    with pytest.raises(ValueError, match="hop 1 has 7 active PRBs, hop 0 has 6"):
        dmrs.PuschLowPaprDmrs(*S.numpy_hops(unequal)[:2], 24)
    type2 = S.case_spec("t2", 24, [S.hop_spec([2], 0, 6, re_masks=[S.TYPE2_CDM0])])
    with pytest.raises(ValueError, match="re_mask=0x0c3"):
        dmrs.PuschLowPaprDmrs(*S.numpy_hops(type2)[:2], 24)
    with pytest.raises(NotImplementedError, match="n_layers=2"):
        dmrs.derive_host_low_papr(h1, h2, 24, n_layers=2)
    with pytest.raises(ValueError, match="hopping='both'"):
        dmrs.PuschLowPaprDmrs(h1, h2, 24, hopping="both")
    with pytest.raises(ValueError, match="hopping=9"):
        dmrs.PuschLowPaprDmrs(h1, h2, 24, hopping=9)
    with pytest.raises(ValueError, match="slots_per_frame=14"):
        dmrs.PuschLowPaprDmrs(h1, h2, 24, slots_per_frame=14)
    # 1 to 4 PRB: NotImplementedError without a table, accepted with a (seeded random) one
    for n_prb in (1, 2, 3, 4):
        _, (s1, s2) = hops(n_prb, 24, 5)
        with pytest.raises(NotImplementedError, match="needs the phi table"):
            dmrs.PuschLowPaprDmrs(s1, s2, 24)
        gen = dmrs.PuschLowPaprDmrs(s1, s2, 24, phi_table=LP.random_phi(6 * n_prb, n_prb))
        assert gen.n_re == 6 * n_prb
        for bad in (LP.random_phi(6 * n_prb + 6, 0), LP.random_phi(6 * n_prb, 0).astype(np.float32), LP.random_phi(6 * n_prb, 0)[:29]):
            with pytest.raises(ValueError, match="phi_table must be an integer array of shape"):
                dmrs.PuschLowPaprDmrs(s1, s2, 24, phi_table=bad)
        with pytest.raises(ValueError, match="is not one of -3, -1, 1, 3"):
            dmrs.PuschLowPaprDmrs(s1, s2, 24, phi_table=LP.random_phi(6 * n_prb, 0) * 0)
    # 5 PRB and more ignore a table
    _, (f1, f2) = hops(5, 24, 5)
    assert dmrs.PuschLowPaprDmrs(f1, f2, 24, phi_table=None).n_re == 30


def test_registry_exports_and_signature(lib):
    sigs = _lib.REGISTRY["ce_dmrs.h"].signatures
    for name in ("ce_dmrs_lp_derive_host", "ce_dmrs_lp_copy_twiddles", "ce_dmrs_lp_plan_create", "ce_dmrs_lp_plan_destroy", "ce_dmrs_lp_generate"):
        assert name in sigs and name in _lib.ALL_EXPORTS and hasattr(lib, name)
    assert "ce_dmrs_lp.hip" in _lib.SOURCES
    assert PKG.PuschLowPaprDmrs is dmrs.PuschLowPaprDmrs
    assert issubclass(dmrs.PuschLowPaprDmrs, dmrs._PilotGenerator) and issubclass(dmrs.PuschDmrs, dmrs._PilotGenerator)
    assert dmrs.PuschLowPaprDmrs._param is dmrs.PuschDmrs._param and dmrs.PuschLowPaprDmrs._generate is dmrs.PuschDmrs._generate   # shared, not copied
    p = inspect.signature(dmrs.PuschLowPaprDmrs.__init__).parameters
    assert list(p) == ["self", "hop1", "hop2", "n_prb_grid", "n_sym", "hopping", "slots_per_frame", "n_symb_slot", "phi_table", "device"]
    assert (p["n_sym"].default, p["hopping"].default, p["slots_per_frame"].default, p["n_symb_slot"].default) == (14, "neither", 10, 14)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("hopping", "slots_per_frame", "n_symb_slot", "phi_table", "device"))
    assert list(inspect.signature(dmrs.PuschLowPaprDmrs.__call__).parameters) == ["self", "slot", "n_id", "out"]


def test_host_parameters_are_range_checked_before_any_device_use(lib):
    _, (h1, h2) = hops(6)
    gen = dmrs.PuschLowPaprDmrs(h1, h2, 6, hopping="group", slots_per_frame=20)
    for args in ((20, 0), (-1, 0), (0, 1008), (0, -1), (np.array([3, 20]), 0), (0, np.array([1, 5000])), (0, 1.0), (0.5, 0),
                 (np.zeros((2, 2), np.int64), 0)):
        with pytest.raises(ValueError):
            gen(*args)
    with pytest.raises(ValueError, match="slot outside 0..19"):
        gen(20, 0)
    with pytest.raises(ValueError, match="n_id outside 0..1007"):
        gen(19, 1008)
    with pytest.raises(ValueError, match="broadcast"):
        gen(np.arange(3), np.arange(2))
    with pytest.raises(ValueError, match="slot outside 0..9"):
        dmrs.PuschLowPaprDmrs(h1, h2, 6)(10, 0)


def kernel_combination(view, mode, nss, slot, n_id, phi=None):
    """The kernel's arithmetic on the host view: the hopping word from the table rows, (u, v), q, e = (q tri[k]) mod N, a gather."""
    out = np.zeros((view.n_re, view.n_dmrs_total, 1), np.complex64)
    for s, l in enumerate(view.col_sym):
        p, f_gh, v = nss * slot + l, 0, 0
        if mode != "neither":
            c_init = n_id // 30 if mode == "group" else n_id
            wi = p >> 2 if mode == "group" else p >> 5
            x = int(view.hop_words[0][wi])
            for i in range(31):
                if c_init >> i & 1:
                    x ^= int(view.hop_words[1 + i][wi])
            if mode == "group":
                f_gh = ((x >> (8 * (p & 3))) & 0xFF) % 30
            elif view.v_live:
                v = (x >> (p & 31)) & 1
        u = (f_gh + n_id % 30) % 30
        if view.form == _lib.CE_DMRS_LP_FORM_PHI:
            a = LP.D.A
            four = np.array([complex(-a, -a), complex(a, -a), complex(a, a), complex(-a, a)], np.complex64)
            out[:, s, 0] = four[(np.asarray(phi)[u].astype(np.int64) + 3) // 2]
        else:
            out[:, s, 0] = dmrs.low_papr_twiddles(view.n_zc)[(int(view.q[u][v]) * view.tri.astype(np.int64)) % view.n_zc]
    return out


@pytest.mark.parametrize("n_prb,mode,slot,n_id", [(5, "group", 3, 1007), (6, "neither", 0, 0), (6, "group", 9, 29), (11, "sequence", 4, 513),
                                                  (12, "sequence", 7, 30), (2, "group", 1, 77), (4, "neither", 2, 1000), (273, "sequence", 5, 999),
                                                  (341, "group", 8, 444)])
def test_host_tables_combined_as_the_kernel_does_reproduce_the_oracle(lib, n_prb, mode, slot, n_id):
    grid = min(n_prb + 4, 341)
    case, (h1, h2) = hops(n_prb, grid, grid - n_prb, syms=(0, 5, 13))
    phi = LP.random_phi(6 * n_prb, 40 + n_prb) if n_prb <= 4 else None       # a seeded random table, not the specification's
    view = dmrs.derive_host_low_papr(h1, h2, grid, hopping=mode, phi_table=phi)
    got = kernel_combination(view, mode, 14, slot, n_id, phi)
    want = LP.pilots_ref(case, slot, n_id, mode, 14, phi)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
