"""CPU-side checks of the OFDM demodulator (include/ce_tp.h `ce_ofdm_*`, srsran_ce_pytorch_amd/ofdm.py): the exports, the
normal cyclic prefix and the symbol phasors against the standard's constants, the host view of the six transform lengths,
every refusal that needs no plan with its text, the oracle pair of tests/ofdm_oracle.py against each other (modulator
then demodulator returns the grid, and H X behind an integer-tap channel), the matrix form against the FFT form, the
calibration of the float32 restatement that sets the GPU tolerance, the kernel's code, and the de-precoder's host view
after the move of its derivation into csrc/ce_fft.h.  No GPU.

The refusals of `ce_ofdm_demodulate` behind the null-plan check (strides, alignment, overlap, counts) need a plan handle,
which only a device gives: tests/test_zzzzzzzzzzzz_hip_ofdm.py `test_refusals_of_the_entry_point_and_the_wrapper`."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ofdm_oracle as O
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, deprecode as DP, ofdm as OF

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_and_the_package_the_class(lib):
    names = ["ce_ofdm_derive_host", "ce_ofdm_copy_twiddles", "ce_ofdm_plan_create", "ce_ofdm_plan_destroy", "ce_ofdm_demodulate"]
    assert [n for n in _lib.REGISTRY["ce_tp.h"].signatures if n.startswith("ce_ofdm_")] == names and "ce_ofdm.hip" in _lib.SOURCES
    assert all(hasattr(lib, n) for n in names) and len(lib.ce_ofdm_demodulate.argtypes) == 8
    assert PKG.PuschOfdmDemodulator is OF.PuschOfdmDemodulator
    # no plan: refused before anything else, whatever the other arguments
    assert lib.ce_ofdm_demodulate(None, None, 0, 0, 0, 0, None, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    lib.ce_ofdm_plan_destroy(None)


def test_normal_cyclic_prefix_lengths():
    assert OF.nr_cp_lengths(15e3, 2048) == [160] + [144] * 6 + [160] + [144] * 6
    assert OF.nr_cp_lengths(30e3, 4096) == [352] + [288] * 13
    total = 0
    for slot in range(8):                                        # 120 kHz: 8 slots per subframe, the long prefix in slots 0 and 4
        cp = OF.nr_cp_lengths(120e3, 512, slot=slot)
        assert cp == ([68] + [36] * 13 if slot in (0, 4) else [36] * 14), (slot, cp)
        total += sum(cp) + 14 * 512
    assert total == 61440                                        # 1 ms at 61.44 MHz
    assert OF.nr_cp_lengths(15e3, 128)[:9] == [10, 9, 9, 9, 9, 9, 9, 10, 9]
    assert OF.nr_cp_lengths(30e3, 512, n_sym=3, slot=1) == [44, 36, 36]
    for scs, n, n_sym, slot in [(15e3, 128, 14, 0), (30e3, 256, 12, 1), (60e3, 1024, 14, 2), (120e3, 512, 14, 4), (240e3, 256, 14, 8), (30e3, 4096, 1, 0)]:
        assert OF.nr_cp_lengths(scs, n, n_sym, slot) == O.cp_lengths_ref(scs, n, n_sym, slot), (scs, n, n_sym, slot)
    for bad in (dict(scs_hz=20e3, n_fft=128), dict(scs_hz=15e3, n_fft=192), dict(scs_hz=15e3, n_fft=64)):
        with pytest.raises(ValueError):
            OF.nr_cp_lengths(**bad)


def test_min_fft_size_and_symbol_phasors():
    assert [OF.min_fft_size(n) for n in (1, 10, 11, 21, 22, 24, 52, 106, 273, 341)] == [128, 128, 256, 256, 512, 512, 1024, 2048, 4096, 4096]
    for bad in (0, 342):
        with pytest.raises(ValueError, match="12 n_prb_grid must lie"):
            OF.min_fft_size(bad)
    cp = OF.nr_cp_lengths(30e3, 512)
    phi = OF.nr_symbol_phasors(10e3, 30e3, 512, cp)
    ref = O.symbol_phasors_ref(10e3, 30e3, 512, cp)
    assert phi.dtype == np.complex64 and phi.shape == (14,) and np.abs(phi - ref).max() <= 2.0 ** -24           # in double, rounded once
    # the sign: the exponent is negative, phi_0 = exp(-j 2 pi f0 cp_0 / fs), and the oracle's modulator sends the conjugate
    assert np.isclose(np.angle(ref[0]), -2 * np.pi * 10e3 * 44 / (30e3 * 512)) and ref[0].imag < 0
    X = np.ones((12, 14), complex)
    s = O.modulate(X, 512, cp, ref)
    plain = O.modulate(X, 512, cp)
    _, T = O.geometry(512, cp)
    assert s.shape == (T,) == (7680,)
    t = 0
    for l, c in enumerate(cp):
        assert np.allclose(s[t:t + c + 512], np.conj(ref[l]) * plain[t:t + c + 512], atol=1e-14)
        t += c + 512
    assert np.abs(O.demodulate_ref(s, 512, 1, cp, 0, ref) - X).max() < 1e-12
    assert np.abs(O.demodulate_ref(s, 512, 1, cp, 0, None) - X).max() > 0.5


def test_host_view_of_the_six_sizes(lib):
    want = {128: ([4, 4, 4, 2], 64, 4), 256: ([4, 4, 4, 4], 64, 4), 512: ([4, 4, 4, 4, 2], 128, 2), 1024: ([4, 4, 4, 4, 4], 128, 2),
            2048: ([4, 4, 4, 4, 4, 2], 256, 1), 4096: ([4, 4, 4, 4, 4, 4], 256, 1)}
    assert tuple(want) == OF.FFT_SIZES
    for N, (radix, tpr, rpw) in want.items():
        for n_sym in (1, 12, 14):
            cp = OF.nr_cp_lengths(30e3, N, n_sym)
            v = OF.derive_host(N, N // 12, cp, n_sym, cp[-1])
            assert v.m_sc == N and list(v.radix[:v.n_passes]) == radix and int(np.prod(radix)) == N and not any(v.radix[v.n_passes:])
            assert (v.threads_per_row, v.rows_per_workgroup, v.threads) == (tpr, rpw, 256) and tpr * rpw == 256
            assert v.lds_bytes == rpw * 2 * 8 * N <= 65536 and v.twiddle_bytes == 8 * N and v.n_workgroups_per_slot == -(-n_sym // rpw)
            s = 1
            for p in range(v.n_passes):                          # floor(i / s) = (i magic) >> 32 for every i < N
                i = np.arange(N, dtype=np.uint64)
                magic = np.uint64(v.stride_magic[p])
                assert (magic == 0) == (s == 1) and (s == 1 or np.array_equal((i * magic) >> np.uint64(32), i // np.uint64(s)))
                s *= radix[p]
        tw = OF.twiddles(N)
        assert np.abs(tw - np.exp(2j * np.pi * np.arange(N) / N)).max() <= 2.0 ** -24 and tw[0] == 1                          # rounded once
        d = OF.PuschOfdmDemodulator(N, N // 12, OF.nr_cp_lengths(30e3, N))
        assert (d.n_samples, d.n_sc, d.radix, d.rows_per_workgroup, d.threads_per_row) == (15 * N, 12 * (N // 12), tuple(radix), rpw, tpr)


def test_every_refusal_without_a_plan(lib):
    cp = OF.nr_cp_lengths(15e3, 128)
    ok = dict(n_fft=128, n_prb_grid=10, cp_len=cp, n_sym=14, window_advance=0)
    assert OF.derive_host(**ok).m_sc == 128
    refused = [
        (dict(n_fft=192), "n_fft=192 is not 128, 256, 512, 1024, 2048 or 4096"),
        (dict(n_fft=64), "n_fft=64 is not"),
        (dict(n_fft=8192), "n_fft=8192 is not"),
        (dict(n_fft=0), "n_fft=0 is not"),
        (dict(n_prb_grid=11), "n_prb_grid=11: n_sc = 12 n_prb_grid must lie in 12..n_fft=128"),
        (dict(n_prb_grid=0), "n_prb_grid=0: n_sc"),
        (dict(n_prb_grid=-3), "n_prb_grid=-3: n_sc"),
        (dict(n_sym=0, cp_len=[]), "n_sym=0 outside 1..14"),
        (dict(n_sym=15, cp_len=cp + [9]), "n_sym=15 outside 1..14"),
        (dict(cp_len=cp[:3] + [-1] + cp[4:]), "cp_len[3]=-1 is negative"),
        (dict(cp_len=cp[:13] + [129]), "cp_len[13]=129 is longer than the symbol, n_fft=128"),
        (dict(window_advance=-1), "window_advance=-1 outside 0..9 (the shortest cyclic prefix)"),
        (dict(window_advance=10), "window_advance=10 outside 0..9 (the shortest cyclic prefix)"),
    ]
    for kw, text in refused:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            OF.derive_host(**args)
        assert text in str(e.value), (kw, str(e.value))
        with pytest.raises(ValueError) as e:                     # the class is validated on construction, without a GPU
            OF.PuschOfdmDemodulator(args["n_fft"], args["n_prb_grid"], args["cp_len"], n_sym=args["n_sym"], window_advance=args["window_advance"])
        assert text in str(e.value), (kw, str(e.value))
    assert OF.derive_host(128, 10, cp, 14, 9).m_sc == 128                                        # a = min cp_len is legal
    with pytest.raises(ValueError, match="cp_len holds 13 lengths for n_sym=14"):
        OF.derive_host(128, 10, cp[:13])
    with pytest.raises(ValueError, match="n_fft=100 is not one of"):
        OF.twiddles(100)
    view = _lib.TpHostView()
    cp_c = (C.c_int32 * 14)(*cp)
    assert lib.ce_ofdm_derive_host(128, 10, 14, None, 0, C.byref(view)) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    assert lib.ce_ofdm_derive_host(128, 10, 14, cp_c, 0, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    assert lib.ce_ofdm_copy_twiddles(128, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    assert lib.ce_ofdm_copy_twiddles(96, C.c_void_p(np.zeros(96, np.complex64).ctypes.data)) == _lib.CE_ERR_INVALID and "n_fft=96" in _lib.last_error()
    # plan creation refuses before it touches a device: the ABI version, every value above, a non-finite phasor
    h = C.c_void_p()
    phi = np.ones(14, np.complex64)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    assert lib.ce_ofdm_plan_create(2, 0, 128, 10, 14, cp_c, 0, None, C.byref(h)) == _lib.CE_ERR_INVALID and "ABI version 2 != 3" in _lib.last_error()
    assert lib.ce_ofdm_plan_create(3, 0, 128, 10, 14, cp_c, 0, None, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    assert lib.ce_ofdm_plan_create(3, 0, 128, 11, 14, cp_c, 0, fp(phi), C.byref(h)) == _lib.CE_ERR_INVALID and "n_prb_grid=11" in _lib.last_error()
    for l, bad in [(0, complex(np.nan, 0)), (5, complex(1, np.inf)), (13, complex(-np.inf, np.nan))]:
        p = phi.copy()
        p[l] = bad
        assert lib.ce_ofdm_plan_create(3, 0, 128, 10, 14, cp_c, 0, fp(p), C.byref(h)) == _lib.CE_ERR_INVALID
        assert f"sym_phasor[{l}] is not finite" in _lib.last_error() and not h.value
        with pytest.raises(ValueError, match=re.escape(f"sym_phasor[{l}] is not finite")):
            OF.PuschOfdmDemodulator(128, 10, cp, sym_phasor=p)
    for bad in (phi[:13], np.ones(14, np.int32), np.ones((14, 1), np.complex64)):
        with pytest.raises(ValueError, match="sym_phasor must hold 14 complex values"):
            OF.PuschOfdmDemodulator(128, 10, cp, sym_phasor=bad)
    assert OF.PuschOfdmDemodulator(128, 10, cp, sym_phasor=list(phi)).sym_phasor.dtype == np.complex64


@pytest.mark.parametrize("N,n_prb,scs,slot,a,with_phi", [(128, 10, 15e3, 0, 0, False), (128, 10, 15e3, 0, 4, True), (256, 21, 30e3, 0, 9, True),
                                                       (512, 24, 120e3, 4, 18, False), (1024, 52, 30e3, 1, 36, True), (4096, 341, 30e3, 0, 100, True)])
def test_oracle_demodulator_inverts_the_oracle_modulator_and_returns_hx_behind_a_channel(N, n_prb, scs, slot, a, with_phi):
    rng = np.random.default_rng(N + n_prb)
    cp = O.cp_lengths_ref(scs, N, 14, slot)
    X = rng.standard_normal((2, 12 * n_prb, 14)) + 1j * rng.standard_normal((2, 12 * n_prb, 14))
    phi = O.symbol_phasors_ref(3.5e9, scs, N, cp) if with_phi else None
    s = O.modulate(X, N, cp, phi)
    assert s.shape == (2, sum(cp) + 14 * N)
    assert np.allclose(np.mean(np.abs(s) ** 2), 12 * n_prb / N * np.mean(np.abs(X) ** 2), rtol=0.1)          # unitary scale
    assert np.abs(O.demodulate_ref(s, N, n_prb, cp, a, phi) - X).max() < 1e-12
    taps = np.zeros(min(cp) - a, complex)                        # the longest channel the advance leaves room for: delays 0 .. min cp - a - 1
    taps[[0, 1, len(taps) // 2, len(taps) - 1]] = [1.0, 0.4j, -0.2, 0.1 + 0.1j]
    y = np.stack([np.convolve(v, taps)[:s.shape[1]] for v in s])
    _, b = O.bins(N, 12 * n_prb)
    hx = np.fft.fft(taps, N)[b][None, :, None] * X
    assert np.abs(O.demodulate_ref(y, N, n_prb, cp, a, phi) - hx).max() < 1e-12
    if a > 0:                                                    # one tap more than fits breaks it: the bound on the taps is tight
        late = np.zeros(min(cp) - a + 2, complex)
        late[[0, -1]] = [1.0, 0.5]
        y = np.stack([np.convolve(v, late)[:s.shape[1]] for v in s])
        assert np.abs(O.demodulate_ref(y, N, n_prb, cp, a, phi) - np.fft.fft(late, N)[b][None, :, None] * X)[..., 1:].max() > 1e-3
    d = O.advance_inputs()
    for adv in (0, d.a):
        assert np.abs(O.demodulate_ref(d.samples64, d.N, d.n_prb, d.cp, adv, d.phi.astype(complex)) - d.hx).max() < 1e-6   # phi rounded to float32


@pytest.mark.parametrize("name", [c["name"] for c in O.CASES if c["n_fft"] <= O.MATRIX_MAX])
def test_matrix_form_equals_fft_form(name):
    d = O.inputs(name)
    c = d.c
    a = O.demodulate_ref(d.samples, c["n_fft"], c["n_prb_grid"], d.cp, c["advance"], d.phi, matrix=True)
    b = O.demodulate_ref(d.samples, c["n_fft"], c["n_prb_grid"], d.cp, c["advance"], d.phi, matrix=False)
    assert np.array_equal(a, d.ref) and np.abs(a - b).max() < 1e-12 * np.sqrt(c["n_fft"])


def test_float32_restatement_calibrates_the_tolerance(lib):
    """C_OFDM of ofdm_oracle's tolerance rule, re-measured over exactly the inputs the GPU tests use: `demodulate_f32` against
    `demodulate_ref` in the rule's unit, printed per case; a value above C_OFDM_RECORDED fails (inside O.check, with t = C)."""
    worst = 0.0
    for c in O.CASES:
        d = O.inputs(c["name"])
        view = OF.derive_host(c["n_fft"], c["n_prb_grid"], d.cp, c["n_sym"], c["advance"])
        got = O.demodulate_f32(d.samples, view, OF.twiddles(c["n_fft"]), c["n_prb_grid"], d.cp, c["advance"], d.phi)
        assert got.shape == (c["B"], c["R"], d.n_sc, c["n_sym"])
        worst = max(worst, O.check(got, d.ref, d.rms, c["n_fft"], c["name"], t=O.C_OFDM_RECORDED))
    d = O.advance_inputs()
    for a in (0, d.a):
        view = OF.derive_host(d.N, d.n_prb, d.cp, 14, a)
        got = O.demodulate_f32(d.samples, view, OF.twiddles(d.N), d.n_prb, d.cp, a, d.phi)
        ref = O.demodulate_ref(d.samples, d.N, d.n_prb, d.cp, a, d.phi)
        worst = max(worst, O.check(got, ref, O.window_rms(d.samples, d.N, d.cp, a), d.N, f"advance a={a}", t=O.C_OFDM_RECORDED))
    print(f"C_OFDM = {worst:.2f}  (C_OFDM_RECORDED = {O.C_OFDM_RECORDED:g}, T_OFDM = {O.T_OFDM:g})")
    assert worst <= O.C_OFDM_RECORDED and O.T_OFDM == 4.0 * O.C_OFDM_RECORDED
    assert worst >= 0.25                                        # the restatement is float32 indeed


def test_the_cases_reach_every_launch_geometry(lib):
    seen = set()
    for c in O.CASES:
        d = O.inputs(c["name"])
        v = OF.derive_host(c["n_fft"], c["n_prb_grid"], d.cp, c["n_sym"], c["advance"])
        seen.add((v.threads_per_row, v.rows_per_workgroup, c["n_sym"] % v.rows_per_workgroup != 0 or v.rows_per_workgroup == 1))
        assert c["B"] <= 2 and c["R"] <= 4 and d.samples.shape == (c["B"], c["R"], d.T)
    assert seen >= {(64, 4, True), (128, 2, True), (256, 1, True)}
    assert {c["n_fft"] for c in O.CASES} == set(OF.FFT_SIZES) and {c["n_sym"] for c in O.CASES} == {14, 12, 1}
    assert any(w % 2 for w in O.geometry(128, O.inputs("n128_p10_15k_a0").cp)[0])                 # a window at an odd sample


def test_no_flat_addressing_no_scratch_8_byte_loads_and_16_byte_stores_in_the_kernel():
    src = CSRC / "ce_ofdm.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^(_ZN12_GLOBAL__N_114ce_ofdm_kernel\w+):\s*;.*?\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert len(kernels) == 1
    body = kernels[0][1]
    assert not re.search(r"\bflat_(load|store)", body) and not re.search(r"\bscratch_(load|store)", body) and not re.search(r"\batomic", body)
    assert re.search(r"\bglobal_load_dwordx2\b", body) and re.search(r"\bglobal_store_dwordx4\b", body)      # 8-byte loads of samples, 16-byte stores of the grid
    assert not re.search(r"\bglobal_store_(dword|dwordx2|dwordx3|byte|short)\b", body), "a narrower store"
    assert not re.search(r"\bglobal_load_(dwordx3|dwordx4|ubyte|sbyte|ushort|sshort)\b", body), "a load that needs more than 8-byte alignment"
    assert re.search(r"\.private_segment_fixed_size: 0\b", text) and re.search(r"\.group_segment_fixed_size: 0\b", text)   # no scratch, no static LDS in front of the dynamic


# what ce_tp_derive_host gave before its derivation moved into csrc/ce_fft.h: (m_sc, n_passes, radix, stride_magic,
# threads_per_row, rows_per_workgroup, threads, lds_bytes, twiddle_bytes, n_workgroups_per_slot) per (n_prbs, n_symbols)
PINNED = {
    (1, 1): (12, 2, [4, 3, 0, 0, 0, 0, 0, 0], [0, 1073741825, 0, 0, 0, 0, 0, 0], 64, 4, 256, 768, 96, 1),
    (2, 14): (24, 3, [4, 2, 3, 0, 0, 0, 0, 0], [0, 1073741825, 536870913, 0, 0, 0, 0, 0], 64, 4, 256, 1536, 192, 4),
    (5, 3): (60, 3, [4, 3, 5, 0, 0, 0, 0, 0], [0, 1073741825, 357913942, 0, 0, 0, 0, 0], 64, 4, 256, 3840, 480, 1),
    (9, 12): (108, 4, [4, 3, 3, 3, 0, 0, 0, 0], [0, 1073741825, 357913942, 119304648, 0, 0, 0, 0], 64, 4, 256, 6912, 864, 3),
    (25, 12): (300, 4, [4, 3, 5, 5, 0, 0, 0, 0], [0, 1073741825, 357913942, 71582789, 0, 0, 0, 0], 64, 4, 256, 19200, 2400, 3),
    (81, 14): (972, 6, [4, 3, 3, 3, 3, 3, 0, 0], [0, 1073741825, 357913942, 119304648, 39768216, 13256072, 0, 0], 128, 2, 256, 31104, 7776, 7),
    (96, 7): (1152, 6, [4, 4, 4, 2, 3, 3, 0, 0], [0, 1073741825, 268435457, 67108865, 33554433, 11184811, 0, 0], 128, 2, 256, 36864, 9216, 4),
    (125, 3): (1500, 5, [4, 3, 5, 5, 5, 0, 0, 0], [0, 1073741825, 357913942, 71582789, 14316558, 0, 0, 0], 256, 1, 256, 24000, 12000, 3),
    (256, 14): (3072, 6, [4, 4, 4, 4, 4, 3, 0, 0], [0, 1073741825, 268435457, 67108865, 16777217, 4194305, 0, 0], 256, 1, 256, 49152, 24576, 14),
    (270, 12): (3240, 7, [4, 2, 3, 3, 3, 3, 5, 0], [0, 1073741825, 536870913, 178956971, 59652324, 19884108, 6628036, 0], 256, 1, 256, 51840, 25920, 12),
}


def test_the_de_precoders_host_view_is_what_it_was_before_the_move(lib):
    for (n_prbs, n_symbols), want in PINNED.items():
        v = DP.derive_host(n_prbs, n_symbols)
        got = (v.m_sc, v.n_passes, list(v.radix), list(v.stride_magic), v.threads_per_row, v.rows_per_workgroup, v.threads, v.lds_bytes,
               v.twiddle_bytes, v.n_workgroups_per_slot)
        assert got == want, (n_prbs, n_symbols)
    for n_prbs, text in [(7, "n_prbs=7 has a prime factor above 5"), (0, "n_prbs=0 outside 1..275"), (276, "n_prbs=276 outside 1..275")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            DP.derive_host(n_prbs, 3)
    assert np.abs(DP.twiddles(25) - np.exp(2j * np.pi * np.arange(300) / 300)).max() <= 2.0 ** -24
