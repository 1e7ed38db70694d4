"""CPU-side checks of the transform de-precoding extension (include/ce_tp.h): the ABI, the valid sizes and every refusal
before any device call, the host derivation (radix sequences, the stride constants of the kernel's division, launch
geometry, twiddles), the oracle against itself (matrix form against FFT form, round trip, a Monte-Carlo check of the noise
prediction and of the bias), the calibration of the float32 restatement that sets the GPU tolerance, and the stage-level
chain through the CPU oracles.  No GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import demod_oracle as D
import tp_oracle as T
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, deprecode as DP

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_every_declared_tp_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies, the
    package's re-export and the header's place in the chain."""
    # LP64 sizes implied by the header: desc 4*4; info 2*4 + 8; view 2*4 + 8*4 + 8*4 + 6*4 = 96
    assert (C.sizeof(_lib.TpDesc), C.sizeof(_lib.TpInfo), C.sizeof(_lib.TpHostView)) == (16, 16, 96)
    assert "ce_tp.hip" in _lib.SOURCES and "ce_tp.h" in _lib.REGISTRY
    assert PKG.PuschTransformDeprecoder is DP.PuschTransformDeprecoder
    assert "ce_tp.h" in (ROOT / "include" / "ce_demod.h").read_text()


def test_valid_sizes_against_brute_force_and_every_refusal(lib):
    def brute(n):
        return all(p in (2, 3, 5) for p in range(2, n + 1) if n % p == 0 and all(p % q for q in range(2, p)))
    valid = [n for n in range(1, 274) if brute(n)]
    assert valid == T.VALID_PRBS and len(valid) == 53 and valid[-1] == 270 and 12 * 270 == 3240
    for n in range(-2, 300):
        for S in (1, 14):
            if n in valid:
                v = DP.derive_host(n, S)
                assert v.m_sc == 12 * n
            else:
                with pytest.raises(ValueError):
                    DP.derive_host(n, S)
                with pytest.raises(ValueError):
                    DP.PuschTransformDeprecoder(n, S)
    for n in (7, 11, 14, 273, 0, 275, 276):
        assert n not in valid
    for S in (0, -1, 15):
        with pytest.raises(ValueError):
            DP.derive_host(6, S)
    # plan creation refuses each before it touches a device
    for field, val in (("abi_version", _lib.CE_ABI_VERSION + 1), ("n_prbs", 7), ("n_prbs", 0), ("n_prbs", 276), ("n_symbols", 0), ("n_symbols", 15)):
        desc = DP.build_desc(6, 12)
        setattr(desc, field, val)
        handle, view, tw = C.c_void_p(), _lib.TpHostView(), np.zeros(2 * 72, np.float32)
        assert lib.ce_tp_plan_create(C.byref(desc), C.byref(handle)) == _lib.CE_ERR_INVALID and not handle.value, field
        assert lib.ce_tp_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID, field
        assert lib.ce_tp_copy_twiddles(C.byref(desc), C.c_void_p(tw.ctypes.data)) == _lib.CE_ERR_INVALID and not tw.any(), field
    # the host entry points refuse null arguments
    assert lib.ce_tp_deprecode(None, None, None, 0, None, None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_tp_plan_get_info(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_tp_derive_host(None, None) == _lib.CE_ERR_INVALID and lib.ce_tp_copy_twiddles(None, None) == _lib.CE_ERR_INVALID


def test_host_view_of_all_53_sizes(lib):
    settings = set()
    for n in T.VALID_PRBS:
        for S in (1, 3, 12, 14):
            v = DP.derive_host(n, S)
            M = 12 * n
            radix = list(v.radix[:v.n_passes])
            assert int(np.prod(radix)) == M == v.m_sc and set(radix) <= {2, 3, 4, 5} and 2 <= v.n_passes <= 7, (n, radix)
            assert radix.count(2) <= 1 and all(r == 0 for r in v.radix[v.n_passes:])
            assert radix[-1] in (3, 5)
            s = 1
            for p, r in enumerate(radix):                       # the kernel's floor(i / s) = (i magic) >> 32 over every butterfly
                i = np.arange(M // r, dtype=np.uint64)
                magic = int(v.stride_magic[p])
                assert (magic == 0) == (s == 1)
                got = i if magic == 0 else (i * np.uint64(magic)) >> np.uint64(32)
                assert np.array_equal(got, i // np.uint64(s)), (n, p)
                # every twiddle index and every output index of the pass stays inside the row
                ps = (i // np.uint64(s)) * np.uint64(s)
                assert int((ps * np.uint64(r - 1)).max()) < M and int(((i - ps) + ps * np.uint64(r) + np.uint64(s * (r - 1))).max()) < M
                s *= r
            assert v.threads == 256 == v.threads_per_row * v.rows_per_workgroup and v.threads_per_row in (64, 128, 256)
            assert v.lds_bytes == v.rows_per_workgroup * 16 * M <= 51840 and v.twiddle_bytes == 8 * M
            assert v.n_workgroups_per_slot == -(-S // v.rows_per_workgroup)
            assert T.chain(v) == 4 * -(-(M // 4) // v.threads_per_row) + {64: 6, 128: 7, 256: 8}[v.threads_per_row] <= 24
            settings.add(v.rows_per_workgroup)
        tp = DP.PuschTransformDeprecoder(n, 12)
        assert (tp.m_sc, tp.n_symbols, tp.radix, tp.rows_per_workgroup) == (M, 12, tuple(radix), v.rows_per_workgroup)
    assert settings == {1, 2, 4}
    # the sizes of the GPU tests: what each exercises
    want = {12: [4, 3], 24: [4, 2, 3], 60: [4, 3, 5], 108: [4, 3, 3, 3], 300: [4, 3, 5, 5], 972: [4, 3, 3, 3, 3, 3], 1500: [4, 3, 5, 5, 5],
            3072: [4, 4, 4, 4, 4, 3], 3240: [4, 2, 3, 3, 3, 3, 5]}
    assert sorted(want) == T.SIZES
    for M, radix in want.items():
        v = DP.derive_host(M // 12, 1)
        assert list(v.radix[:v.n_passes]) == radix
    assert {DP.derive_host(M // 12, 1).rows_per_workgroup for M in T.SIZES} == {1, 2, 4}


def test_twiddles_are_float64_values_rounded_once(lib):
    for n in (1, 25, 81, 256, 270):
        M = 12 * n
        w = DP.twiddles(n)
        k = np.arange(M)
        want = np.exp(2j * np.pi * k / M)
        assert w.dtype == np.complex64 and w.shape == (M,)
        assert np.array_equal(w.real, np.cos(2 * np.pi * k / M).astype(np.float32)) and np.array_equal(w.imag, np.sin(2 * np.pi * k / M).astype(np.float32))
        assert np.abs(w - want).max() <= 2.0 ** -24


def test_precode_matrix_form_equals_fft_form():
    rng = np.random.default_rng(3)
    for M in (12, 24, 60, 108, 300, 972):
        x = rng.standard_normal((2, 3 * M)) + 1j * rng.standard_normal((2, 3 * M))
        a, b = T.precode(x, M, matrix=True), T.precode(x, M, matrix=False)
        assert a.shape == b.shape == x.shape and np.abs(a - b).max() <= 1e-11 * np.sqrt(M)
        # unitary, and the sign of 6.3.1.4: a single symbol at i = 1 gives exp(-j 2 pi k / M) / sqrt(M)
        assert abs(np.linalg.norm(a) - np.linalg.norm(x)) <= 1e-9 * np.linalg.norm(x)
        e = np.zeros(M, complex)
        e[1] = 1.0
        assert np.allclose(T.precode(e[None], M, matrix=True)[0], np.exp(-2j * np.pi * np.arange(M) / M) / np.sqrt(M), atol=1e-14)
    assert T.MATRIX_MAX >= 300


@pytest.mark.parametrize("M", [12, 60, 300, 3240])
def test_deprecode_ref_inverts_precode(M):
    rng = np.random.default_rng(M)
    x = D.modulate(rng.integers(0, 2, (2, 3 * M * 4)), 4)
    got, nv = T.deprecode_ref(T.precode(x, M), np.full(x.shape, 1e-9), M)
    assert np.abs(got - x).max() <= 1e-9 and np.allclose(nv, 1e-9, rtol=1e-6)
    # a fully dropped row is erased, the others are untouched by it
    bad = np.full(x.shape, 1e-9)
    bad[0, :M] = np.inf
    got2, nv2 = T.deprecode_ref(T.precode(x, M), bad, M)
    assert np.all(got2[0, :M] == 0) and np.all(np.isposinf(nv2[0, :M])) and np.array_equal(got2[0, M:], got[0, M:]) and np.array_equal(got2[1], got[1])


def _views(M, S):
    return DP.derive_host(M // 12, S), DP.twiddles(M // 12)


def _calibrate(d, what):
    view, tw = _views(d.M, d.S)
    gx, gn = T.deprecode_f32(d.x_hat, d.nvar, view, tw)
    ratio, _ = T.check(gx, gn, d.ref_x, d.ref_nv, view, what, t=T.C_RECORDED)
    return ratio


def test_float32_restatement_calibrates_the_tolerance(lib):
    """C of tp_oracle's tolerance rule, re-measured over exactly the inputs the GPU tests use: `deprecode_f32` against
    `deprecode_ref` in the rule's unit, printed per case; a value above C_RECORDED fails (inside T.check, with t = C)."""
    worst = 0.0
    for M, S in T.CASES:
        worst = max(worst, _calibrate(T.inputs(M, S), f"M={M} S={S}"))
    for M, S in T.SPECIAL:
        worst = max(worst, _calibrate(T.special_inputs(M, S), f"special M={M} S={S}"))
    worst = max(worst, _calibrate(T.chain_inputs(), "chain"))
    print(f"C = {worst:.2f}  (C_RECORDED = {T.C_RECORDED:g}, T = {T.T:g})")
    assert worst <= T.C_RECORDED and T.T == 4.0 * T.C_RECORDED
    assert worst >= 0.25                                        # the restatement is float32 indeed


def test_float32_restatement_on_all_53_sizes(lib):
    worst = 0.0
    for n in T.VALID_PRBS:
        d = T._finish(T.draw(12 * n, 1, seed=2))
        worst = max(worst, _calibrate(d, f"n_prbs={n}"))
    print(f"all 53 sizes at S = 1: C = {worst:.2f}")
    assert worst <= T.C_RECORDED


def test_special_inputs_are_what_they_say():
    for M, S in T.SPECIAL:
        d = T.special_inputs(M, S)
        ok = D.usable(d.x_hat, d.nvar)
        assert np.array_equal(~ok, d.dropped) and d.dropped[:2].any(1).all() and not d.dropped[:2].reshape(2, S, M).all(-1).any()
        assert np.all(d.ref_x[2, :M] == 0) and np.all(np.isposinf(d.ref_nv[2, :M])) and np.all(np.isfinite(d.ref_nv[:2]))
        assert np.all(np.isfinite(d.ref_x))
        for bad in (np.isposinf(d.nvar), d.nvar == 0, d.nvar == -1, np.isnan(d.nvar), ~np.isfinite(d.x_hat.real), ~np.isfinite(d.x_hat.imag)):
            assert bad[:2].any()


@pytest.mark.parametrize("drop", [0.0, 0.1], ids=["all_res", "10pct_dropped"])
@pytest.mark.parametrize("M", [12, 72, 300])
def test_monte_carlo_nvar_out_predicts_the_error_power_and_the_bias_is_one(M, drop):
    """A fixed three-tap channel, fresh 16QAM symbols and noise per trial: the error power of x_out, averaged over trials,
    is nvar_out within four standard errors of the trial means, and the coefficient of the transmitted symbol is 1."""
    rng = np.random.default_rng(1000 + M + int(100 * drop))
    n_trials, sigma2 = 4000, 0.05
    taps = np.array([1.0, 0.6, 0.4]) * np.exp(2j * np.pi * rng.random(3))
    h = (taps[None, :] * np.exp(-2j * np.pi * np.outer(np.arange(M), [0, 1, 3]) / M)).sum(-1)
    x = D.modulate(rng.integers(0, 2, (n_trials, M * 4)), 4)
    noise = (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * np.sqrt(sigma2 / 2.0)
    x_hat = (h * T.precode(x, M, matrix=M <= 72) + noise) / h
    nvar = np.broadcast_to(sigma2 / np.abs(h) ** 2, x.shape).copy()
    nvar[rng.random(x.shape) < drop] = np.inf
    got, nv_out = T.deprecode_ref(x_hat, nvar, M)
    live = np.isfinite(nv_out[:, 0])
    assert live.mean() > 0.99
    got, nv_out, x = got[live], nv_out[live], x[live]
    diff = (np.abs(got - x) ** 2).mean(-1) - nv_out[:, 0]
    se = diff.std() / np.sqrt(len(diff))
    pred = nv_out[:, 0].mean()
    bias = ((got * x.conj()).real.sum(-1) / (np.abs(x) ** 2).sum(-1))
    bse = bias.std() / np.sqrt(len(bias))
    print(f"M={M} drop={drop}: predicted {pred:.5f}, measured {pred + diff.mean():.5f} (+- {se:.5f}); bias {bias.mean():.4f} +- {bse:.4f}")
    assert abs(diff.mean()) <= 4.0 * se and se <= 0.02 * pred and pred > 0.02
    assert abs(bias.mean() - 1.0) <= 4.0 * bse and bse <= 0.004


def test_stage_chain_through_the_cpu_oracles():
    """bits -> scrambled -> 16QAM -> precode -> selective gains + noise -> deprecode_ref -> llr_ref -> descrambled: every hard
    decision is the bit sent, with the margin the oracle asserts."""
    d = T.chain_inputs()
    assert d.margin <= T.CHAIN_MARGIN and d.llr.shape == (1, d.S * d.M * 4)
    assert np.array_equal((d.llr[0] < 0).astype(np.uint8), d.bits)
    assert np.all(d.llr != 0)
    # a plain IDFT of the zero-forcing estimates is the worse estimate on this channel: the MMSE combination matters
    plain = np.fft.ifft(d.x_hat.astype(np.complex128).reshape(d.S, d.M), axis=-1).reshape(1, -1) * np.sqrt(d.M)
    assert np.mean(np.abs(plain - d.x_tx) ** 2) > np.mean(np.abs(d.ref_x - d.x_tx) ** 2)


def test_python_argument_checks_that_need_no_device():
    with pytest.raises(ValueError):
        DP.PuschTransformDeprecoder(7, 12)
    with pytest.raises(ValueError):
        DP.PuschTransformDeprecoder(6, 0)
    tp = DP.PuschTransformDeprecoder(6, 12)
    assert tp.m_sc == 72 and tp.radix == (4, 2, 3, 3) and tp.device is None
