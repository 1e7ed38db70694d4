"""CPU-side checks of the time-domain channel emulator (include/ce_tp.h `ce_chan_apply`, `ce_chan_noise_words`;
srsran_ce_pytorch_amd/channel.py): the exports, the library's Philox against the Random123 known answers and against the
Python-integer restatement of tests/chan_oracle.py, the statistics of the oracle's noise, the float32 restatement against the
float64 operator on every case (the CPU calibration of the tolerance), the phase word, the host helpers, every refusal of the
entry point (they all come before anything touches a device) and of the wrapper that needs no GPU, and the kernels' code-object
figures.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import chan_oracle as X
import ofdm_oracle as O
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, channel as CH

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"

# Random123's known answers for philox4x32_10: (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _lib_words(lib, seed, slot, port, t_pair):
    out = (C.c_uint32 * 4)()
    assert lib.ce_chan_noise_words(seed, slot, port, t_pair, out) == 0
    return tuple(int(w) for w in out)


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def test_exports_registry_sources_and_the_package(lib):
    sig = _lib.REGISTRY["ce_tp.h"].signatures
    assert [n for n in sig if n.startswith("ce_chan_")] == ["ce_chan_apply", "ce_chan_noise_words"]
    assert len(sig["ce_chan_apply"][1]) == 23 and len(sig["ce_chan_noise_words"][1]) == 5
    assert all(n in _lib.ALL_EXPORTS and hasattr(lib, n) for n in ("ce_chan_apply", "ce_chan_noise_words"))
    assert "ce_chan.hip" in _lib.SOURCES and (CSRC / "ce_chan.hip").is_file()
    assert [n for n in sig if n.startswith("ce_ofdm_")] == ["ce_ofdm_derive_host", "ce_ofdm_copy_twiddles", "ce_ofdm_plan_create", "ce_ofdm_plan_destroy", "ce_ofdm_demodulate"]
    assert PKG.PuschChannelEmulator is CH.PuschChannelEmulator and PKG.cfo_word is CH.cfo_word and PKG.taps_from_delays is CH.taps_from_delays
    assert lib.ce_abi_version() == 3


def test_philox_known_answers_in_the_library_and_the_restatement(lib):
    for counter, key, want in KAT:
        assert X.philox(counter, key) == want
        # the issue's layout: counter (t_pair, port, slot low, slot high), key (seed low, seed high)
        seed, slot = key[0] | key[1] << 32, counter[2] | counter[3] << 32
        assert X.noise_words(seed, slot, counter[1], counter[0]) == want
        assert _lib_words(lib, seed, _signed(slot, 64), _signed(counter[1], 32), counter[0]) == want
    rng = np.random.default_rng(5)
    for _ in range(24):
        seed, slot = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(-2 ** 62, 2 ** 62))
        port, t_pair = int(rng.integers(0, 64)), int(rng.integers(0, 1 << 31))
        want = X.noise_words(seed, slot, port, t_pair)
        assert _lib_words(lib, seed, slot, port, t_pair) == want
        assert want == X.philox((t_pair, port, slot & X.MASK, (slot >> 32) & X.MASK), (seed & X.MASK, seed >> 32))
    # each of the four inputs reaches the words; the array form is the scalar one
    base = X.noise_words(7, 9, 2, 100)
    assert len({base, X.noise_words(8, 9, 2, 100), X.noise_words(7 + (1 << 32), 9, 2, 100), X.noise_words(7, 10, 2, 100),
                X.noise_words(7, 9 + (1 << 32), 2, 100), X.noise_words(7, 9, 3, 100), X.noise_words(7, 9, 2, 101)}) == 7
    rows = X.noise_words_row(0x1234567890abcdef, -3, 5, 40)
    assert all(tuple(int(w) for w in rows[i]) == X.noise_words(0x1234567890abcdef, -3, 5, i) == _lib_words(lib, 0x1234567890abcdef, -3, 5, i) for i in range(40))
    assert lib.ce_chan_noise_words(1, 2, 3, 4, None) == _lib.CE_ERR_INVALID and _lib.last_error() == "null argument"


def test_noise_statistics_of_the_oracle():
    """2^20 samples of (seed 0x1234567890abcdef, slot 5, port 3); the bounds are the issue's, the values measured with this
    mapping in the comments."""
    n = X.noise_ref(0x1234567890abcdef, 5, 3, 1 << 20)
    re, im, p = n.real, n.imag, np.abs(n) ** 2
    stats = dict(mean=abs(n.mean()), power=p.mean(), re2=np.mean(re * re), im2=np.mean(im * im), reim=abs(np.mean(re * im)),
                 lag1=abs(np.mean(n[1:] * np.conj(n[:-1]))), m4=np.mean(p * p))
    print(stats)
    assert stats["mean"] <= 0.005                                 # 0.0016
    assert abs(stats["power"] - 1.0) <= 0.005                     # 1.00022
    assert abs(stats["re2"] - 0.5) <= 0.005 and abs(stats["im2"] - 0.5) <= 0.005      # 0.49967 / 0.50056: within 1 % of 0.5
    assert stats["reim"] <= 0.002                                 # 5.6e-5
    assert stats["lag1"] <= 0.005                                 # 3.3e-4
    assert abs(stats["m4"] - 2.0) <= 0.02                         # 2.0022
    # sample 2 i takes (w0, w1), sample 2 i + 1 (w2, w3)
    w = X.noise_words(0x1234567890abcdef, 5, 3, 0)
    assert np.allclose(n[0], X.gauss_ref((w[0] >> 8) + 1, w[1] >> 8)) and np.allclose(n[1], X.gauss_ref((w[2] >> 8) + 1, w[3] >> 8))


def test_noise_extremes_are_finite():
    """a = 0 gives |n| = sqrt(24 ln 2), a = 0xffffffff gives n = 0; both finite in the float32 restatement too."""
    lo, hi = (0 >> 8) + 1, (0xffffffff >> 8) + 1
    for i2 in (0, 1 << 22, (1 << 24) - 1):
        assert abs(abs(X.gauss_ref(lo, i2)) - np.sqrt(24.0 * np.log(2.0))) < 1e-12 and X.gauss_ref(hi, i2) == 0
        for i1, want in ((lo, np.sqrt(24.0 * np.log(2.0))), (hi, 0.0)):
            re, im = X.gauss_f32(i1, i2)
            assert re.dtype == np.float32 and np.isfinite(re) and np.isfinite(im) and abs(np.hypot(float(re), float(im)) - want) < 4e-6


def test_the_restatement_calibrates_the_tolerance():
    """C of chan_oracle's rule for `apply_f32` against `apply_ref`, over exactly the inputs the GPU tests use, printed per
    case: the CPU calibration.  Above C_CHAN_F32_RECORDED or below a quarter of it fails."""
    worst = 0.0
    for name in X.CASE_NAMES:
        d = X.inputs(name)
        c = d.c
        got = X.apply_f32(d.x, d.h, d.fcw, d.phase0, d.sigma, d.seed, d.first_slot)
        assert got.shape == (c["B"], c["R"], c["T"]) == d.ref.shape == d.A.shape
        worst = max(worst, X.check(got, d, name, t=X.C_CHAN_F32_RECORDED))
    print(f"C_CHAN (float32 restatement) = {worst:.2f}  (C_CHAN_F32_RECORDED = {X.C_CHAN_F32_RECORDED:g}, C_CHAN_RECORDED = {X.C_CHAN_RECORDED:g}, T_CH = {X.T_CH:g})")
    assert X.C_CHAN_F32_RECORDED / 4.0 <= worst <= X.C_CHAN_F32_RECORDED and X.T_CH == 4.0 * X.C_CHAN_RECORDED


def test_the_cases_reach_every_path():
    cs = X.CASES
    assert {c["T"] for c in cs} == {1, 1023, 1024, 1025, 2500} and {c["K"] for c in cs} >= {1, 2, 12, 128, 3, 127}
    assert {c["P"] for c in cs} == {1, 2, 4} and {c["R"] for c in cs} == {1, 4} and {c["B"] for c in cs} == {1, 3}
    assert {(c["cfo"], c["sigma"]) for c in cs} >= {(None, None), (None, "scalar"), ("scalar", None), ("tensor", None), ("scalar", "scalar"),
                                                    ("tensor", "tensor"), ("tensor", "scalar"), ("scalar", "tensor")}
    assert {c["shared"] for c in cs if c["B"] > 1} == {True, False}
    assert any(c["first_slot"] >= 1 << 32 for c in cs) and any(c["first_slot"] < 0 for c in cs)
    for name in X.CASE_NAMES:
        d = X.inputs(name)
        c = d.c
        assert d.x.shape == (c["B"], c["P"], c["T"]) and d.h.shape == (1 if c["shared"] else c["B"], c["R"], c["P"], c["K"])
        assert d.x.dtype == d.h.dtype == np.complex64 and (d.sigma is None) == (c["sigma"] is None) and (d.fcw is None) == (c["cfo"] is None)


def test_the_phase_word_wraps_exactly():
    T = 2500
    for fcw in (2 ** 31 - 1, -(2 ** 31) + 1, -(2 ** 31), 1, -1):
        for phase0 in (0, 0xfffffffe, 0x80000000):
            w = X.phase_words(phase0, fcw, T)
            wrapped = (np.uint32(phase0) + np.uint32(fcw & 0xffffffff) * np.arange(T, dtype=np.uint32)).astype(np.int64)      # uint32 arithmetic
            assert np.array_equal(w, wrapped) and w.min() >= 0 and w.max() < 1 << 32
            assert int(w[T - 1]) == (phase0 + fcw * (T - 1)) % (1 << 32)
    assert int(X.phase_words(0, 2 ** 31 - 1, T)[T - 1]) == 2 ** 31 - (T - 1)      # (2^31 - 1) 2499 = 2^31 - 2499 mod 2^32, 2499 being odd


def test_cfo_word_round_trips_and_refuses_beyond_half_the_rate():
    fs = 15.36e6
    assert abs(fs * 2.0 ** -32 - 0.0036) < 1e-4                   # Hz per step
    for f in (0.0, 350.0, -350.0, 1e3, -7.5e3, 3.84e6, -7.68e6, 7.68e6 - 1.0):
        w = CH.cfo_word(f, fs)
        assert isinstance(w, int) and -2 ** 31 <= w <= 2 ** 31 - 1 and abs(CH.cfo_hz(w, fs) - f) <= 0.5 * fs * 2.0 ** -32 + 1e-9
        assert CH.cfo_word(CH.cfo_hz(w, fs), fs) == w
    assert CH.cfo_word(-7.68e6, fs) == -2 ** 31 and CH.cfo_word(1.0, 2.0 ** 32) == 1 and CH.cfo_word(1.5, 2.0 ** 32) == 2
    for f, rate in ((7.68e6, fs), (-7.68e6 - 1.0, fs), (1e9, fs), (1.0, 0.0), (1.0, -fs), (np.nan, fs), (1.0, np.inf)):
        with pytest.raises(ValueError, match="cfo_word"):
            CH.cfo_word(f, rate)


def test_a_control_word_of_one_bin_shifts_the_grid_by_one_subcarrier():
    """fcw = 2^32 / N turns an OFDM symbol of the oracle's modulator into its grid shifted by one bin (float64 throughout)."""
    N, n_prb = 128, 10
    rng = np.random.default_rng(9)
    grid = rng.standard_normal((12 * n_prb, 1)) + 1j * rng.standard_normal((12 * n_prb, 1))
    s = O.modulate(grid, N, [0])                                   # one symbol, no prefix: the phase counts from its first sample
    for sign in (1, -1):
        y, _, _ = X.apply_ref(s[None, None], np.ones((1, 1, 1, 1)), fcw=sign * (2 ** 32 // N), phase0=0)
        back = O.demodulate_ref(y[0, 0], N, n_prb, [0], 0)
        if sign > 0:
            assert np.abs(back[1:] - grid[:-1]).max() < 1e-12
        else:
            assert np.abs(back[:-1] - grid[1:]).max() < 1e-12
    y, _, _ = X.apply_ref(s[None, None], np.ones((1, 1, 1, 1)), fcw=2 ** 32 // N, phase0=1 << 30)       # a quarter turn at sample 0
    assert np.abs(O.demodulate_ref(y[0, 0], N, n_prb, [0], 0)[1:] - 1j * grid[:-1]).max() < 1e-12


def test_taps_from_delays():
    # an integer delay gives a unit tap, exactly
    for d in (0, 3, 11):
        h = CH.taps_from_delays([float(d)], [2.0 - 1.0j], 1.0, 12)
        want = np.zeros(12, np.complex64)
        want[d] = 2.0 - 1.0j
        assert h.dtype == np.complex64 and h.shape == (12,) and np.array_equal(h, want)
    # the 0 / 100 / 300 ns profile at 10 MHz is three unit taps
    h = CH.taps_from_delays([0.0, 100e-9, 300e-9], [1.0, 0.5, 0.25j], 10e6, 8)
    assert np.allclose(h, [1.0, 0.5, 0, 0.25j, 0, 0, 0, 0], atol=1e-7)
    # a half-sample delay (behind a bulk delay that keeps the window inside the taps): the response over the occupied band
    f = np.linspace(-CH.SINC_BAND, CH.SINC_BAND, 601)
    k = np.arange(24)
    for d in (8.5, 8.25, 12.75, 15.0 - 1e-3):
        h = CH.taps_from_delays([d / 15.36e6], [1.0], 15.36e6, 24).astype(np.complex128)
        resp = (h[None, :] * np.exp(-2j * np.pi * f[:, None] * k[None, :])).sum(1)
        err = np.abs(resp - np.exp(-2j * np.pi * f * d)).max()
        print(f"delay {d}: max deviation {err:.2e} over |f| <= {CH.SINC_BAND}")
        assert err <= CH.SINC_RIPPLE
    # paths add; refusals
    a, b = CH.taps_from_delays([8.5], [1.0], 1.0, 24), CH.taps_from_delays([10.25], [0.5j], 1.0, 24)
    assert np.allclose(CH.taps_from_delays([8.5, 10.25], [1.0, 0.5j], 1.0, 24), a + b, atol=1e-7)
    for args, text in ((([0.0], [1.0], 1.0, 0), "n_taps=0 outside 1..128"), (([0.0], [1.0], 1.0, 129), "n_taps=129 outside 1..128"),
                       (([0.0, 1.0], [1.0], 1.0, 4), "the same number"), (([], [], 1.0, 4), "the same number"),
                       (([-0.5], [1.0], 1.0, 4), "outside 0..3"), (([3.5], [1.0], 1.0, 4), "outside 0..3"),
                       (([np.nan], [1.0], 1.0, 4), "finite"), (([1.0], [np.inf], 1.0, 4), "finite")):
        with pytest.raises(ValueError) as e:
            CH.taps_from_delays(*args)
        assert text in str(e.value), (args, str(e.value))


def test_refusals_of_the_entry_point_come_before_any_device_call(lib):
    """Every argument error of ce_chan_apply with its text, on made-up addresses: nothing is dereferenced or launched."""
    B, P, R, K, T = 2, 2, 3, 4, 100
    px, ph, py = 0x10000, 0x80000, 0x100000

    def call(abi=3, x=px, xss=P * T, xps=T, slots=B, tx=P, rx=R, n=T, taps=ph, tss=R * P * K, k=K, fcw=None, fs=0, p0=None, p0s=0, sg=None, sgs=0,
             y=py, yss=R * T, yps=T):
        vp = lambda a: C.c_void_p(a) if a else None
        return lib.ce_chan_apply(abi, vp(x), xss, xps, slots, tx, rx, n, vp(taps), tss, k, vp(fcw), fs, vp(p0), p0s, vp(sg), sgs, 0, 0, vp(y), yss, yps, None)

    refused = [
        (dict(abi=2), "ABI version 2 != 3"), (dict(abi=0), "ABI version 0 != 3"),
        (dict(slots=-1), "n_slots=-1"), (dict(rx=-1), "n_rx=-1"), (dict(n=-5), "n_samples=-5"),
        (dict(tx=0), "n_tx=0 outside 1..4"), (dict(tx=5), "n_tx=5 outside 1..4"), (dict(k=0), "n_taps=0 outside 1..128"),
        (dict(k=129), "n_taps=129 outside 1..128"), (dict(rx=0), "n_rx=0 must be >= 1"), (dict(n=0), "n_samples=0 must be >= 1"),
        (dict(slots=0, tx=9), "n_tx=9 outside 1..4"),                                               # the limits hold for an empty batch too
        (dict(x=0), "null argument"), (dict(y=0), "null argument"), (dict(taps=0), "null argument"), (dict(fcw=0x4000), "null argument"),
        (dict(xss=-1), "strides must be >= 0"), (dict(xps=-1), "strides must be >= 0"), (dict(yss=-1), "strides must be >= 0"),
        (dict(yps=-T), "strides must be >= 0"), (dict(tss=-1), "strides must be >= 0"), (dict(fcw=0x4000, p0=0x5000, fs=-1), "strides must be >= 0"),
        (dict(fcw=0x4000, p0=0x5000, p0s=-1), "strides must be >= 0"), (dict(sg=0x6000, sgs=-1), "strides must be >= 0"),
        (dict(x=px + 4), "x must be 8-byte aligned"), (dict(y=py + 4), "y must be 8-byte aligned"), (dict(taps=ph + 2), "taps must be 8-byte aligned"),
        (dict(n=1 << 60), "exceeds the address space"), (dict(yss=1 << 60), "exceeds the address space"), (dict(yps=1 << 60), "exceeds the address space"),
        (dict(xss=1 << 60), "exceeds the address space"), (dict(xps=1 << 60), "exceeds the address space"), (dict(tss=1 << 60), "exceeds the address space"),
        (dict(tss=R * P * K - 1), f"taps_slot_stride={R * P * K - 1} is neither 0 nor >= n_rx n_tx n_taps = {R * P * K}"), (dict(tss=1), "taps_slot_stride=1"),
        # rows of y that share samples, in either nesting: ce_ofdmtx_modulate's conditions, its text
        (dict(yps=T - 1), f"slot_stride={R * T} and port_stride={T - 1}: the rows of {T} samples of {B} slots x {R} ports overlap"),
        (dict(yss=R * T - 1), "overlap"), (dict(yss=0), "overlap"), (dict(yps=0), "overlap"), (dict(yss=T - 1, yps=B * T), "overlap"),
        (dict(yss=T, yps=B * T - 1), "overlap"), (dict(yss=T, yps=T), "overlap"), (dict(yss=0, yps=0), "overlap"),
        (dict(slots=1, yss=0, yps=T - 1), "overlap"), (dict(rx=1, yss=T - 1, yps=0), "overlap"),
        # the extent of y against x and against the taps
        (dict(y=px), "y overlaps x"), (dict(y=px + 8 * (B * P * T - 1)), "y overlaps x"), (dict(x=py + 8 * (B * R * T - 1)), "y overlaps x"),
        (dict(y=ph), "y overlaps taps"), (dict(y=ph + 8 * (B * R * P * K - 1)), "y overlaps taps"), (dict(taps=py + 8 * (B * R * T - 1)), "y overlaps taps"),
        (dict(tss=0, y=ph + 8 * (R * P * K - 1)), "y overlaps taps"),
    ]
    for kw, text in refused:
        assert call(**kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (kw, _lib.last_error())
    for kw in (dict(slots=1 << 31), dict(rx=1 << 31), dict(slots=1 << 16, rx=1 << 15), dict(slots=1, rx=1, n=1 << 41, yss=0, yps=0), dict(slots=1 << 20, rx=1 << 10, n=2049)):
        assert call(**kw) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error(), kw
    assert call(slots=0) == 0 and call(slots=0, x=0, y=0, taps=0) == 0                              # an empty batch launches nothing


def test_wrapper_refusals_that_need_no_device(lib):
    for args, text in (((0, 1, 1), "n_tx=0 outside 1..4"), ((5, 1, 1), "n_tx=5 outside 1..4"), ((1, 0, 1), "n_rx=0 must be >= 1"),
                       ((1, 1, 0), "n_taps=0 outside 1..128"), ((1, 1, 129), "n_taps=129 outside 1..128"), ((1.0, 1, 1), "n_tx must be an int"),
                       ((1, True, 1), "n_rx must be an int"), ((1, 1, "4"), "n_taps must be an int")):
        with pytest.raises(ValueError) as e:
            CH.PuschChannelEmulator(*args)
        assert text in str(e.value), (args, str(e.value))
    ch = CH.PuschChannelEmulator(1, 4, 12)
    assert (ch.n_tx, ch.n_rx, ch.n_taps, ch.device) == (1, 4, 12, None)
    # no CPU fallback: the call is refused before it looks at its arguments
    x, h = torch.zeros((1, 1, 16), dtype=torch.complex64), torch.zeros((1, 4, 1, 12), dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="the channel emulator runs on a ROCm GPU only"):
        CH.PuschChannelEmulator(1, 4, 12, device="cpu")(x, h)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        CH.PuschChannelEmulator(1, 4, 12, device=torch.device("cpu"))(None, None)


def test_code_object_figures_of_the_kernels():
    """The compiler's record of the four instantiations (cfo x noise): no scratch, no spills, no static LDS (the launch sizes
    it: at most 40 KiB), at most 64 VGPRs (eight waves per SIMD, so the LDS alone sets the occupancy)."""
    src = CSRC / "ce_chan.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    names = re.findall(r"^\s+\.name:\s+(\S*ce_chan_kernel\S*)$", text, flags=re.M)
    assert len(names) == 4 and len(set(names)) == 4
    for name in names:
        meta = re.search(r"\n(  - \.agpr_count:.*?\.name:\s+" + re.escape(name) + r"\n.*?\.wavefront_size:\s+\d+)", text, flags=re.S)
        assert meta, name
        fig = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", meta.group(1).split("  - .agpr_count:")[-1], flags=re.M)}
        print(name, {k: fig[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert fig["private_segment_fixed_size"] == 0 and fig["vgpr_spill_count"] == 0 and fig["sgpr_spill_count"] == 0, name
        assert fig["group_segment_fixed_size"] == 0 and fig["vgpr_count"] <= 64 and fig["max_flat_workgroup_size"] == 256, name
    assert 8 * (CH.MAX_TX * (1024 + CH.MAX_TAPS) + CH.MAX_TX * CH.MAX_TAPS) == 40 * 1024      # the largest launch: P = 4, K = 128
