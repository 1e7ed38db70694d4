"""CPU tests of the SRS channel estimator's host side (include/ce_tp.h `ce_srs_*`, srsran_ce_pytorch_amd/srs.py) and of its oracle
(tests/srs_oracle.py): the port rule, the oracle on hand-made inputs, the library's tables and windows against the oracle, the
hopping against a bit-serial Gold sequence with c_init = n_id, exports, every refusal with nothing written, the calibration of the
tolerances and the gap condition of the delay rule.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import srs_oracle as SO
import srsran_ce_pytorch_amd as pkg
from srsran_ce_pytorch_amd import _lib, srs as S


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


ALL_PORT_ARGS = [(k_tc, n_ap, n_cs, k_bar) for k_tc in (2, 4) for n_ap in (1, 2, 4) for n_cs in range(SO.n_cs_max(k_tc)) for k_bar in range(k_tc)]


def test_ports_follow_the_rule_for_every_configuration():
    moved = 0
    for k_tc, n_ap, n_cs, k_bar in ALL_PORT_ARGS:
        ncs = 8 if k_tc == 2 else 12
        got = S.srs_ports(k_tc, n_ap, n_cs, k_bar)
        upper = n_ap == 4 and n_cs >= ncs // 2
        want = [(((k_bar + k_tc // 2) % k_tc) if upper and i in (1, 3) else k_bar,
                 ((n_cs + ncs * (i // 2) // 2) if upper else (n_cs + ncs * i // n_ap)) % ncs) for i in range(n_ap)]
        assert got == want == SO.ports(k_tc, n_ap, n_cs, k_bar), (k_tc, n_ap, n_cs, k_bar)
        assert len(set(got)) == n_ap, f"(comb, cs) pairs repeat: {got}"
        hv = S.derive_host(k_tc, n_ap, n_cs, k_bar, 12, 14, 128)
        assert list(zip(hv.port_comb, hv.port_cs)) == want
        if upper:
            moved += 1
            assert got[1][0] == got[3][0] != k_bar == got[0][0] == got[2][0] and got[0][1] == got[1][1] and got[2][1] == got[3][1] and hv.n_combs == 2
        else:
            assert all(c == k_bar for c, _ in got) and hv.n_combs == 1
    assert moved == 4 * 2 + 6 * 4


def _flat(c, H, delay=0, sigma=0.0, seed=1):
    """y [1, R, n_sym, n_sc]: zeros but the used combs, which carry sum_i H r_i delayed by `delay` grid steps, plus noise."""
    rng = np.random.default_rng(seed)
    y = np.zeros((1, c.R, c.n_sym, c.n_sc), np.complex128)
    seq, n = SO.sequence(c, c.slot[0], c.n_id[0]), np.arange(c.M)
    for comb in c.combs:
        for s in range(c.n_symb):
            k = 12 * c.start_prb[s] + comb + c.k_tc * n
            tx = sum(H[:, i, None] * seq[i, s][None] for i, (ci, _) in enumerate(c.ports) if ci == comb)
            noise = sigma * (rng.standard_normal((c.R, c.M)) + 1j * rng.standard_normal((c.R, c.M))) / np.sqrt(2)
            y[0][:, c.l0 + s, k] = tx * np.exp(-2j * np.pi * k * delay / (c.N * c.k_tc)) + noise
    return y


@pytest.mark.parametrize("geometry", ["a_c4_4p_one_comb_m36", "b_c4_4p_two_combs", "c_c2_4p_m144_4sym", "e_c4_2p_m12_phi"])
def test_oracle_on_a_flat_noiseless_channel(geometry):
    c = SO.case(geometry, "group", B=1)
    H = np.random.default_rng(5).standard_normal((c.R, c.n_ap)) + 1j * np.random.default_rng(6).standard_normal((c.R, c.n_ap))
    y = _flat(c, H)
    est = SO.estimate_ref(c, y, c.slot, c.n_id, None)
    assert np.abs(est.h_sb - H[None, :, :, None, None]).max() <= 1e-12 and np.abs(est.h_wb - H[None]).max() <= 1e-12
    assert est.noise.max() <= 1e-24 and np.allclose(est.epre[0], (np.abs(H) ** 2).sum(1) / c.n_combs, rtol=1e-12)
    prof = SO.window(c, SO.profile_full(c, y, c.slot, c.n_id))
    assert np.allclose(prof[0, :, c.g], (np.abs(H) ** 2).sum(1) * c.n_symb, rtol=1e-12) and np.all(SO.delay_of(c, prof) == 0)


@pytest.mark.parametrize("delta", [-2, 5, 17])
def test_oracle_finds_a_pure_delay_and_takes_it_out(delta):
    c = SO.case("a_c4_4p_one_comb_m36", "neither", B=1)
    H = np.random.default_rng(7).standard_normal((c.R, c.n_ap)) + 1j * np.random.default_rng(8).standard_normal((c.R, c.n_ap))
    y = _flat(c, H, delay=delta)
    prof = SO.window(c, SO.profile_full(c, y, c.slot, c.n_id))
    assert SO.delay_of(c, prof)[0] == delta
    est = SO.estimate_ref(c, y, c.slot, c.n_id, np.array([delta]))
    back = S.srs_band_response(est.h_sb, [delta], c.k_tc, c.N, c.ports, c.start_prb)
    assert np.abs(back - H[None, :, :, None, None]).max() <= 1e-12 and est.noise.max() <= 1e-24
    phase = np.exp(-2j * np.pi * (12 * c.start_prb[0] + c.ports[0][0]) * delta / (c.N * c.k_tc))
    assert np.abs(est.h_sb[0, :, 0, 0] - (H[:, 0] * phase)[:, None]).max() <= 1e-12            # the constant phase stays in h_sb
    wrapped = SO.estimate_ref(c, y, c.slot, c.n_id, np.array([delta + 3 * c.N]))
    assert np.array_equal(wrapped.h_sb, est.h_sb)                                               # the delay is taken mod N


def test_oracle_noise_estimate_is_unbiased_within_statistical_bounds():
    c = SO.case("c_c2_4p_m144_4sym", "sequence", B=1, R=8)
    H = np.ones((c.R, c.n_ap), np.complex128)
    sigma = 0.05
    est = SO.estimate_ref(c, _flat(c, H, delay=3, sigma=sigma), c.slot, c.n_id, np.array([3]))
    dof = c.n_symb * c.n_combs * c.M - c.n_symb * c.n_ap * c.n_blocks
    # noise dof / sigma^2 is chi-square with 2 dof degrees of freedom over 2: relative standard deviation 1 / sqrt(dof); 5 sigma
    assert np.all(np.abs(est.noise / sigma ** 2 - 1.0) <= 5.0 / np.sqrt(dof)), est.noise / sigma ** 2
    assert abs(est.noise.mean() / sigma ** 2 - 1.0) <= 5.0 / np.sqrt(dof * c.R)
    assert np.abs(est.h_sb - S.srs_band_response(np.ones_like(est.h_sb), [-3], c.k_tc, c.N, c.ports, c.start_prb)).max() <= 6 * sigma / np.sqrt(c.Q)


@pytest.mark.parametrize("geometry,hopping", SO.CASES, ids=SO.CASE_IDS)
def test_library_tables_and_windows_against_the_oracle(geometry, hopping):
    c, lib_ = SO.case(geometry, hopping), SO.library(geometry, hopping)
    hv = lib_.hv
    assert (hv.m, hv.q_len, hv.n_blocks, hv.n_combs, hv.guard, hv.default_win_len) == (c.M, c.Q, c.n_blocks, c.n_combs, c.g, c.win_len)
    assert list(zip(hv.port_comb, hv.port_cs)) == c.ports and hv.v_live == (hopping == "sequence" and c.M >= 72)
    assert int(hv.view.m_sc) == c.N and int(hv.view.n_workgroups_per_slot) == 1 and int(np.prod([int(r) for r in hv.view.radix[:hv.view.n_passes]])) == c.N
    n = np.arange(c.N)
    assert np.array_equal(lib_.tw, np.exp(2j * np.pi * n / c.N).astype(np.complex64))
    assert np.abs(lib_.rho - SO.rho(c)[:, :c.n_cs_max]).max() <= SO.EPS
    if c.M >= 36:
        nzc = SO.largest_prime_below(c.M)
        assert hv.form == _lib.CE_DMRS_LP_FORM_ZC and hv.n_zc == nzc == len(lib_.w)
        assert np.array_equal(lib_.w, np.exp(-2j * np.pi * np.arange(nzc) / nzc).astype(np.complex64).real + 1j * (-np.sin(2 * np.pi * np.arange(nzc) / nzc)).astype(np.float32))
        i = np.arange(c.M) % nzc
        assert np.array_equal(hv.tri, (i * (i + 1) // 2) % nzc)
        for u in range(30):
            for v in range(2):
                q_bar = nzc * (u + 1) / 31
                assert hv.q[u, v] == int(np.floor(q_bar + 0.5)) + v * (-1) ** int(np.floor(2 * q_bar))
    else:
        assert hv.form == _lib.CE_DMRS_LP_FORM_PHI and hv.n_zc == 0 and len(lib_.w) == 4
        assert np.abs(lib_.w - np.exp(1j * np.pi * np.array([-3, -1, 1, 3]) / 4)).max() <= SO.EPS
    for b in range(c.B):                                                   # the sequences, to float32 rounding
        slot, n_id = SO._item(c.slot, b), SO._item(c.n_id, b)
        assert np.abs(SO.base_rows_f32(c, lib_, slot, n_id) - SO.base_rows(c, slot, n_id)).max() <= 2 * SO.EPS
        mine = S.srs_sequence(c.k_tc, c.n_ap, c.n_cs, c.k_bar, c.m_srs, c.n_symb, c.l0, slot, n_id, hopping, c.n_symb_slot, c.slots_per_frame, c.phi)
        assert np.abs(mine - SO.sequence(c, slot, n_id)).max() <= 1e-12
        grid = S.srs_map(mine, c.k_tc, c.n_ap, c.n_cs, c.k_bar, c.start_prb, c.l0, c.n_prb_grid, c.n_sym, beta=0.5)
        assert grid.shape == (c.n_ap, c.n_sc, c.n_sym) and np.count_nonzero(grid) == c.n_ap * c.n_symb * c.M
        for i, (comb, _) in enumerate(c.ports):
            assert np.array_equal(SO.comb_rows(c, grid[i].T, comb), 0.5 * mine[i])


def _fold(words, c_init):
    """The words of c for `c_init` from the library's table [32, nw]: row 0 and the rows 1 + i of the set bits."""
    out = words[0].copy()
    for i in range(31):
        if (c_init >> i) & 1:
            out ^= words[1 + i]
    return out


@pytest.mark.parametrize("hopping", ["group", "sequence"])
def test_hopping_words_against_the_bit_serial_gold_sequence_with_c_init_n_id(hopping):
    c = SO.case("c_c2_4p_m144_4sym", hopping)
    hv = SO.library("c_c2_4p_m144_4sym", hopping).hv
    n_pos = c.n_symb_slot * c.slots_per_frame
    assert hv.n_words == (-(-n_pos // 4) if hopping == "group" else -(-n_pos // 32)) and hv.hop_words.shape == (32, hv.n_words)
    differs = 0
    for n_id in (0, 1, 29, 30, 777, 1023, 65535):
        bits = SO.gold(n_id, 32 * hv.n_words)
        words = (bits.reshape(-1, 32) << np.arange(32)).sum(1).astype(np.uint32)
        assert np.array_equal(_fold(hv.hop_words, n_id), words), n_id
        other = SO.gold(n_id // 30, 32 * hv.n_words)                        # PUSCH's rule: not SRS's
        for slot in (0, 7, 19):
            for (u, v), s in zip(SO.hopping_uv(c, slot, n_id), range(c.n_symb)):
                p = c.n_symb_slot * slot + c.l0 + s
                if hopping == "group":
                    assert u == (int(sum(int(bits[8 * p + m]) << m for m in range(8))) % 30 + n_id) % 30 and v == 0
                    differs += u != (int(sum(int(other[8 * p + m]) << m for m in range(8))) % 30 + n_id) % 30
                else:
                    assert u == n_id % 30 and v == int(bits[p])
        assert S.srs_hopping(hopping, n_id, 7, c.l0, c.n_symb, c.M, c.n_symb_slot, c.slots_per_frame) == SO.hopping_uv(c, 7, n_id)
    if hopping == "group":
        assert differs > 0, "no case where floor(n_id / 30) would give another u"
        assert SO.hopping_uv(c, 3, 777) != [((int(sum(int(SO.gold(25, 8 * n_pos)[8 * (14 * 3 + c.l0 + s) + m]) << m for m in range(8))) % 30 + 777) % 30, 0)
                                            for s in range(c.n_symb)]                                 # the GPU case's own (slot, n_id)


def test_sequence_hopping_is_live_from_72_elements_only():
    assert not S.derive_host(4, 1, 0, 0, 20, 30, 128, hopping="sequence").v_live          # M = 60
    assert S.derive_host(4, 1, 0, 0, 24, 30, 128, hopping="sequence").v_live              # M = 72
    assert not S.derive_host(4, 1, 0, 0, 24, 30, 128, hopping="group").v_live


def test_exports_and_argument_counts(lib):
    for name in ("SrsEstimator", "SrsProfile", "SrsEstimate", "srs_ports", "srs_sequence", "srs_map", "srs_band_response"):
        assert getattr(pkg, name) is getattr(S, name)
    sig = _lib.REGISTRY["ce_tp.h"].signatures
    counts = {"ce_srs_derive_host": 23, "ce_srs_copy_tables": 9, "ce_srs_plan_create": 19, "ce_srs_plan_destroy": 1, "ce_srs_profile": 13, "ce_srs_estimate": 18}
    for name, n in counts.items():
        assert len(sig[name][1]) == n and hasattr(lib, name), name
    assert "ce_srs.hip" in _lib.SOURCES and _lib.CE_ABI_VERSION == 3
    assert S.SrsProfile._fields == ("profile", "delay", "ta_s") and S.SrsEstimate._fields == ("h_sb", "h_wb", "noise", "epre")
    assert list(inspect.signature(S.SrsEstimator.profile).parameters) == ["self", "y", "slot", "n_id"]
    assert list(inspect.signature(S.SrsEstimator.__call__).parameters) == ["self", "y", "slot", "n_id", "delay"]


GOOD = dict(k_tc=4, n_ap=4, n_cs=7, k_bar=3, m_srs=16, n_prb_grid=20, n_fft=128, n_symb=2, l0=3, start_prb=[0, 4], n_sym=14, n_symb_slot=14,
            hopping="group", slots_per_frame=20, win_len=20)
BAD_PLANS = [
    (dict(k_tc=3), ValueError), (dict(k_tc=8), ValueError), (dict(n_ap=3), ValueError), (dict(n_ap=0), ValueError), (dict(n_ap=8), ValueError),
    (dict(n_cs=-1), ValueError), (dict(n_cs=12), ValueError), (dict(k_tc=2, k_bar=1, n_cs=8), ValueError), (dict(k_bar=4), ValueError), (dict(k_bar=-1), ValueError),
    (dict(m_srs=0), ValueError), (dict(m_srs=6), ValueError), (dict(m_srs=276, n_prb_grid=300, n_fft=4096), ValueError), (dict(m_srs=-4), ValueError),
    (dict(n_symb=3, start_prb=[0, 0, 0]), ValueError), (dict(n_symb=0, start_prb=[]), ValueError), (dict(n_symb=8, start_prb=[0] * 8), ValueError),
    (dict(l0=-1), ValueError), (dict(l0=13), ValueError), (dict(n_sym=4, l0=3), ValueError), (dict(n_sym=15), ValueError), (dict(n_sym=0), ValueError),
    (dict(n_sym=13, n_symb_slot=12), ValueError), (dict(n_symb_slot=13), ValueError),
    (dict(start_prb=[0, 5]), ValueError), (dict(start_prb=[-1, 0]), ValueError), (dict(start_prb=[0]), ValueError), (dict(start_prb="01"), ValueError),
    (dict(n_prb_grid=15), ValueError), (dict(n_prb_grid=0), ValueError), (dict(n_prb_grid=342), ValueError),
    (dict(hopping="both"), ValueError), (dict(hopping=3), ValueError), (dict(slots_per_frame=15), ValueError),
    (dict(n_fft=64), ValueError), (dict(n_fft=192), ValueError), (dict(n_fft=8192), ValueError), (dict(m_srs=44, n_prb_grid=50, start_prb=[0, 4]), ValueError),   # M = 132 > 128
    (dict(win_len=0), ValueError), (dict(win_len=129), ValueError), (dict(win_len=-3), ValueError),
    (dict(m_srs=4), NotImplementedError), (dict(m_srs=8), NotImplementedError),                                             # M = 12, 24 without phi
    (dict(m_srs=4, phi_table=np.zeros((30, 12), np.int64)), ValueError), (dict(m_srs=4, phi_table=np.ones((30, 11), np.int64)), ValueError),
    (dict(m_srs=4, phi_table=np.ones((30, 12))), ValueError), (dict(k_tc=True), ValueError), (dict(n_fft=128.0), ValueError), (dict(m_srs=2 ** 31), ValueError),
]


@pytest.mark.parametrize("over,exc", BAD_PLANS, ids=[",".join(f"{k}={v if np.isscalar(v) else '..'}" for k, v in o.items()) for o, _ in BAD_PLANS])
def test_refused_plans(over, exc):
    S.derive_host(**GOOD)
    with pytest.raises(exc):
        S.derive_host(**{**GOOD, **over})
    with pytest.raises(exc):
        S.SrsEstimator(**{**GOOD, **over})


def test_a_refusal_writes_nothing(lib):
    view, marks = _lib.TpHostView(), [np.full(n, 0x5A5A5A5A, np.int32) for n in (10, 4, 4, 60, 2048, 32 * 560)]
    C.memset(C.byref(view), 0x5A, C.sizeof(view))
    sp = (C.c_int32 * 4)(0, 4, 0, 0)
    ptrs = [C.c_void_p(a.ctypes.data) for a in marks]
    bad = [(4, 4, 12, 3, 16, 2, 3), (4, 4, 7, 3, 16, 2, 13), (4, 4, 7, 3, 4, 2, 3)]                 # n_cs; l0; M = 12 without phi
    for head, code in zip(bad, (_lib.CE_ERR_INVALID, _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED)):
        rc = lib.ce_srs_derive_host(*head, C.cast(sp, C.c_void_p), 20, 14, 14, 1, 20, 128, 20, None, C.byref(view), *ptrs)
        assert rc == code and _lib.last_error()
        assert bytes(view) == b"\x5a" * C.sizeof(view) and all(np.all(a == 0x5A5A5A5A) for a in marks)
    tabs = [np.full(64, np.float32(7.5)) for _ in range(3)]
    assert lib.ce_srs_copy_tables(4, 3, 0, 0, 16, 128, *(C.c_void_p(a.ctypes.data) for a in tabs)) == _lib.CE_ERR_INVALID
    assert all(np.all(a == np.float32(7.5)) for a in tabs)
    out = C.c_void_p(0x1234)
    assert lib.ce_srs_plan_create(2, 0, 4, 4, 7, 3, 16, 2, 3, C.cast(sp, C.c_void_p), 20, 14, 14, 1, 20, 128, 20, None, C.byref(out)) == _lib.CE_ERR_INVALID
    assert "ABI" in _lib.last_error() and out.value == 0x1234
    assert lib.ce_srs_plan_create(3, 0, 4, 4, 7, 3, 16, 2, 3, C.cast(sp, C.c_void_p), 20, 14, 14, 1, 20, 64, 20, None, C.byref(out)) == _lib.CE_ERR_INVALID
    assert out.value == 0x1234 and lib.ce_srs_plan_create(3, 0, 4, 4, 7, 3, 16, 2, 3, C.cast(sp, C.c_void_p), 20, 14, 14, 1, 20, 128, 20, None, None) == _lib.CE_ERR_INVALID
    # the launches refuse a null plan before they look at anything else
    assert lib.ce_srs_profile(None, None, 0, 0, 0, 1, 1, None, 0, None, 0, None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_srs_estimate(None, None, 0, 0, 0, 1, 1, None, 0, None, 0, None, 0, None, None, None, None, None) == _lib.CE_ERR_INVALID
    lib.ce_srs_plan_destroy(None)


def test_wrapper_refuses_a_cpu_device_and_bad_helper_arguments():
    import torch
    est = S.SrsEstimator(**GOOD, device="cpu")
    with pytest.raises(RuntimeError):
        est.profile(torch.zeros((1, 1, 14, 240), dtype=torch.complex64), 0, 0)
    for bad in ((3, 1, 0, 0), (2, 3, 0, 0), (2, 1, 8, 0), (2, 1, 0, 2), (4, 4, 12, 0), (2.0, 1, 0, 0)):
        with pytest.raises(ValueError):
            S.srs_ports(*bad)
    with pytest.raises(ValueError):
        S.SrsEstimator(**GOOD, scs_hz=0.0)
    with pytest.raises(ValueError):
        S.srs_map(np.zeros((1, 1, 48)), 4, 1, 0, 0, [17], 0, 20)
    assert est.win_len == 20 and S.SrsEstimator(**{**GOOD, "win_len": None}).win_len == 128 * 6 // 12 - 3


def test_float32_restatement_calibrates_the_tolerances():
    """C per quantity: the restatement's largest error against the float64 oracle in the rules' units over the GPU cases.  Each
    must lie in (C_RECORDED / 4, C_RECORDED]."""
    worst = {k: 0.0 for k in SO.C_RECORDED}
    for geometry, hopping in SO.CASES:
        d, lib_ = SO.inputs(geometry, hopping), SO.library(geometry, hopping)
        prof = SO.profile_f32(d.c, lib_, d.y, d.slot, d.n_id)
        assert np.array_equal(SO.delay_of(d.c, prof), d.delay), (geometry, hopping)
        est = SO.estimate_f32(d.c, lib_, d.y, d.slot, d.n_id, d.delay)
        r = SO.ratios(d, prof, est)
        print(f"{geometry}-{hopping}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        for k, v in r.items():
            worst[k] = max(worst[k], v)
    print("C measured:", {k: round(v, 4) for k, v in worst.items()}, "recorded:", SO.C_RECORDED)
    for k, v in worst.items():
        assert SO.C_RECORDED[k] / 4.0 < v <= SO.C_RECORDED[k], f"{k}: measured C {v:.4f}, recorded {SO.C_RECORDED[k]}"


@pytest.mark.parametrize("geometry,hopping", SO.CASES, ids=SO.CASE_IDS)
def test_gap_condition_of_the_delay_rule_holds_for_every_item(geometry, hopping):
    d = SO.inputs(geometry, hopping)
    assert np.array_equal(d.delay, d.sent), (d.delay, d.sent)                   # the oracle finds what was sent
    got = SO.gaps(d)
    assert len(got) == d.c.B
    for b, (gap, pair) in enumerate(got):
        print(f"{geometry}-{hopping} item {b}: gap {gap:.4g} = {gap / d.prof.sum(1)[b].max():.3f} of the peak = {gap / pair:.3g} tolerance pairs")
        assert gap > SO.GAP_TOLERANCES * pair, (b, gap, pair)
    seen = {int(x) for g, h in SO.CASES for x in SO.inputs(g, h).sent}
    c = d.c
    assert 0 in seen and min(seen) < 0 and d.sent.min() >= -(c.g - 1) and d.sent.max() <= c.win_len - c.g - 1
