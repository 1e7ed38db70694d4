"""CPU-side checks of the equalizer extension (include/ce_eq.h): the ABI, the library's host derivation (the per-symbol
table and the row formula the kernel uses) against the plain-loop enumeration of tests/eq_oracle.py, descriptor errors
before any device call, and the calibration of the tolerance rule the GPU tests apply.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import eq_oracle as Q
from srsran_ce_pytorch_amd import _lib, equalizer as EQ, synth as S

IDS = [c["name"] for c in Q.CASES]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_every_declared_eq_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies."""
    assert "ce_eq.h" in _lib.REGISTRY and "ce_eq.hip" in _lib.SOURCES
    # LP64 sizes implied by the header: hop 14 + 2 + 4*4 = 32; desc 6*4 + 2*32 = 88; info 4 + 4 + 8 = 16; view 4*14*4 + 4 = 228
    assert (C.sizeof(_lib.EqHopDesc), C.sizeof(_lib.EqDesc), C.sizeof(_lib.EqInfo), C.sizeof(_lib.EqHostView)) == (32, 88, 16, 228)
    assert EQ.CHUNK_SC == _lib.CE_EQ_CHUNK_SC and EQ.CHUNK_SC % 12 == 0


@pytest.mark.parametrize("c", Q.CASES, ids=IDS)
def test_host_derivation_reproduces_the_plain_loop_enumeration(lib, c):
    case = c["case"]
    h1, h2, _ = S.numpy_hops(case)
    ref = Q.data_re_ref(case, c["mask"])
    eq = EQ.PuschEqualizer(h1, h2, c["L"], case["n_prb_grid"], case["n_sym"], reserved_re_mask=c["mask"])
    view = EQ.derive_host(h1, h2, c["L"], case["n_prb_grid"], case["n_sym"], reserved_re_mask=c["mask"])
    assert eq.n_data_re == view.n_data_re == len(ref)
    count = 0
    for s in range(14):
        hops = [i for i, h in enumerate(case["hops"]) if h["start_symbol"] <= s < h["start_symbol"] + h["n_alloc"]] if s < case["n_sym"] else []
        assert view.sym_hop[s] == (hops[0] if hops else -1)
        if s < case["n_sym"]:
            assert view.first_row[s] == count
        on_sym = ref[ref[:, 0] == s, 1]
        count += len(on_sym)
        if hops:
            h = case["hops"][hops[0]]
            mask = sum(1 << r for r in range(12) if 12 * h["prb_start"] + r in on_sym)
            assert view.data_mask[s] == mask == (0xFFF & ~c["mask"] if s in h["dmrs_symbols"] else 0xFFF)
            assert view.data_res_per_prb[s] == bin(mask).count("1") and len(on_sym) == h["n_prbs"] * bin(mask).count("1")
        else:
            assert view.data_mask[s] == 0 and view.data_res_per_prb[s] == 0 and len(on_sym) == 0
    assert np.array_equal(eq.data_re(), ref)


def test_default_mask_leaves_dmrs_symbols_out_and_counts_rows(lib):
    h1, h2, _ = S.numpy_hops(S.bench_case("filter"))
    assert EQ.PuschEqualizer(h1, h2, 1, 273).n_data_re == 3276 * 12
    assert EQ.PuschEqualizer(h1, h2, 4, 273, reserved_re_mask=0x555).n_data_re == 3276 * 12 + 2 * 273 * 6
    assert EQ.PuschEqualizer(h1, h2, 4, 273, reserved_re_mask=0).n_data_re == 3276 * 14


def test_descriptor_errors_come_before_any_device_call(lib):
    good = S.case_spec("g", 52, [S.hop_spec([2, 11], 4, 6)], n_layers=2)
    h1, h2, _ = S.numpy_hops(good)
    assert EQ.derive_host(h1, h2, 2, 52, 14).n_data_re == 72 * 12
    for L in (0, 5):
        with pytest.raises(NotImplementedError, match=f"n_layers={L}"):
            EQ.derive_host(h1, h2, L, 52, 14)
    two = S.case_spec("t", 52, [S.hop_spec([2], 4, 6), S.hop_spec([11], 20, 6)])            # both described over the whole slot
    a, b, _ = S.numpy_hops(two)
    with pytest.raises(NotImplementedError, match="share OFDM symbol 0"):
        EQ.derive_host(a, b, 1, 52, 14)
    touching = S.case_spec("t", 52, [S.hop_spec([2], 4, 6, 0, 8), S.hop_spec([11], 20, 6, 7, 7)])   # symbol 7 in both
    a, b, _ = S.numpy_hops(touching)
    with pytest.raises(NotImplementedError, match="share OFDM symbol 7"):
        EQ.derive_host(a, b, 1, 52, 14)
    beyond = S.numpy_hops(S.case_spec("b", 52, [S.hop_spec([2], 47, 6)]))
    with pytest.raises(ValueError, match="outside the grid of 52 PRB"):
        EQ.derive_host(beyond[0], beyond[1], 1, 52, 14)
    late = S.numpy_hops(S.case_spec("l", 52, [S.hop_spec([2], 4, 6, 6, 9)]))
    with pytest.raises(ValueError, match="outside the grid of 14 symbols"):
        EQ.derive_host(late[0], late[1], 1, 52, 14)
    with pytest.raises(ValueError, match="n_sym=15"):
        EQ.derive_host(h1, h2, 1, 52, 15)
    with pytest.raises(NotImplementedError, match="grid of 342 PRB"):
        EQ.derive_host(h1, h2, 1, 342, 14)
    with pytest.raises(ValueError, match="12-bit"):
        EQ.derive_host(h1, h2, 1, 52, 14, reserved_re_mask=0x1000)
    desc = EQ.build_desc(h1, h2, 2, 52, 14)
    view, handle = _lib.EqHostView(), C.c_void_p()
    assert lib.ce_eq_derive_host(C.byref(desc), C.byref(view)) == 0
    desc.abi_version = _lib.CE_ABI_VERSION + 1
    assert lib.ce_eq_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID and b"ABI" in lib.ce_last_error()
    for bad in ("abi", "layers", "hops", "prbs", "n_sym"):            # plan creation refuses each before it touches a device
        desc = EQ.build_desc(h1, h2, 2, 52, 14)
        if bad == "abi":
            desc.abi_version += 1
        elif bad == "layers":
            desc.n_layers = 5
        elif bad == "hops":
            desc.n_hops, desc.hop[1] = 2, desc.hop[0]
        elif bad == "prbs":
            desc.hop[0].n_prbs = 49
        else:
            desc.n_sym = 15
        code = lib.ce_eq_plan_create(C.byref(desc), C.byref(handle))
        assert code in (_lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED) and not handle.value, bad
        assert code == (_lib.CE_ERR_UNSUPPORTED if bad in ("layers", "hops") else _lib.CE_ERR_INVALID), bad


def test_float32_restatement_calibrates_the_tolerance(lib):
    """C = the largest ratio of equalize_f32's own error to 2^-24 (kappa + 1 / b) over the GPU tests' inputs; T = 4 C is
    recorded in eq_oracle.py.  Fails when the re-measured C exceeds the recorded one."""
    worst = 0.0
    for c in Q.CASES:
        d = Q.inputs(c["name"])
        x, nvar = Q.equalize_f32(d.rx, d.ch_est, d.noise, d.data_re)
        rx_, rn_ = Q.error_ratios(x, nvar, d.ref)
        print(f"{c['name']:>18}: L={d.L} R={d.R}  C_x = {rx_.max():6.2f}  C_nvar = {rn_.max():6.2f}")
        worst = max(worst, float(rx_.max()), float(rn_.max()))
    print(f"C = {worst:.2f} (recorded {Q.C_RECORDED:g}, T = {Q.T:g})")
    assert worst <= Q.C_RECORDED and Q.T == 4.0 * Q.C_RECORDED


@pytest.mark.parametrize("c", Q.CASES, ids=IDS)
def test_the_draw_keeps_the_rule_tight(c):
    """From the oracle alone, with T = 64: no element's relative tolerance above 5e-2, at most 2 % of a case's elements
    above 1e-3 -- an indexing error (an O(1) difference) cannot hide under the rule."""
    d = Q.inputs(c["name"])
    assert np.all(d.ref.b > 0)
    tol = Q.rel_tolerance(d.ref, 64.0)
    frac = float(np.mean(tol > 1e-3))
    print(f"{c['name']}: max relative tolerance {tol.max():.2e}, {100 * frac:.2f} % of elements above 1e-3; max kappa {d.ref.kappa.max():.0f}")
    assert tol.max() <= 5e-2 and frac <= 0.02
    assert Q.T <= 64.0
    # the noiseless part of the draw is what the test says it is: hard decisions of the oracle's x_hat give the QPSK symbols sent
    agree = np.mean((np.sign(d.ref.x_hat.real) == np.sign(d.x_tx.real)) & (np.sign(d.ref.x_hat.imag) == np.sign(d.x_tx.imag)))
    assert agree > 0.9
