"""CPU-side checks of the OFDM modulator (include/ce_tp.h `ce_ofdmtx_modulate`, srsran_ce_pytorch_amd/ofdm.py
`PuschOfdmModulator`): the export and the class, the refusals that need no plan, `for_demodulator`, the float32 restatement of
tests/ofdm_tx_oracle.py against the float64 operator `ofdm_oracle.modulate` (the calibration that sets the GPU tolerance), its
cyclic prefixes, the launch geometries the cases reach, and the kernel's code.  No GPU.

The refusals of `ce_ofdmtx_modulate` behind the null-plan check need a plan handle, which only a device gives:
tests/test_zzzzzzzzzzzzzz_hip_ofdm_tx.py `test_refusals_of_the_entry_point_and_the_wrapper`."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import ofdm_oracle as O
import ofdm_tx_oracle as X
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, ofdm as OF

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _f32(name):
    d = X.inputs(name)
    c = d.c
    view = OF.derive_host(c["n_fft"], c["n_prb_grid"], d.cp, c["n_sym"], 0)
    return d, X.modulate_f32(d.grid, view, OF.twiddles(c["n_fft"]), d.cp, d.phi)


def test_library_export_and_the_package_the_class(lib):
    sig = _lib.REGISTRY["ce_tp.h"].signatures
    assert "ce_ofdmtx_modulate" in sig and len(sig["ce_ofdmtx_modulate"][1]) == 8 and not "ce_ofdmtx_modulate".startswith("ce_ofdm_")
    assert hasattr(lib, "ce_ofdmtx_modulate") and len(lib.ce_ofdmtx_modulate.argtypes) == 8 and "ce_ofdm.hip" in _lib.SOURCES
    assert PKG.PuschOfdmModulator is OF.PuschOfdmModulator and issubclass(OF.PuschOfdmModulator, OF._stage.Stage)
    assert OF.PuschOfdmModulator._LAUNCH == "ce_ofdmtx_modulate" and OF.PuschOfdmModulator._CREATE == OF.PuschOfdmDemodulator._CREATE
    assert lib.ce_abi_version() == 3


def test_a_null_plan_is_refused_first(lib):
    a = np.zeros(4, np.complex64).ctypes.data
    for args in ((None, 0, 0, None, 0, 0), (a, 1, 1, a, 0, 0), (a, -1, -1, a + 4, -1, -1), (None, 1 << 40, 1 << 40, None, 1 << 62, 1 << 62)):
        assert lib.ce_ofdmtx_modulate(None, *args, None) == _lib.CE_ERR_INVALID and _lib.last_error() == "null argument", args


def test_argument_errors_that_need_no_device(lib):
    cp = OF.nr_cp_lengths(15e3, 128)
    mod = OF.PuschOfdmModulator(128, 10, cp)
    assert (mod.n_fft, mod.n_prb_grid, mod.n_sym, mod.n_sc, mod.n_samples, mod.window_advance, mod.sym_phasor) == (128, 10, 14, 120, 1920, 0, None)
    assert (mod.radix, mod.threads_per_row, mod.rows_per_workgroup) == ((4, 4, 4, 2), 64, 4)
    # the constructor's validation is the demodulator's: the same refusals with the same texts
    refused = [
        (dict(n_fft=192), "n_fft=192 is not 128, 256, 512, 1024, 2048 or 4096"),
        (dict(n_prb_grid=11), "n_prb_grid=11: n_sc = 12 n_prb_grid must lie in 12..n_fft=128"),
        (dict(n_prb_grid=0), "n_prb_grid=0: n_sc"),
        (dict(n_sym=15, cp_len=cp + [9]), "n_sym=15 outside 1..14"),
        (dict(n_sym=0, cp_len=[]), "n_sym=0 outside 1..14"),
        (dict(cp_len=cp[:3] + [-1] + cp[4:]), "cp_len[3]=-1 is negative"),
        (dict(cp_len=cp[:13] + [129]), "cp_len[13]=129 is longer than the symbol, n_fft=128"),
        (dict(cp_len=cp[:13]), "cp_len holds 13 lengths for n_sym=14"),
        (dict(sym_phasor=np.ones(13, np.complex64)), "sym_phasor must hold 14 complex values"),
        (dict(sym_phasor=np.ones(14, np.int32)), "sym_phasor must hold 14 complex values"),
        (dict(sym_phasor=np.array([1] * 5 + [complex(1, np.inf)] + [1] * 8, np.complex64)), "sym_phasor[5] is not finite"),
    ]
    for kw, text in refused:
        args = dict(n_fft=128, n_prb_grid=10, cp_len=cp, n_sym=14)
        args.update(kw)
        for cls in (OF.PuschOfdmModulator, OF.PuschOfdmDemodulator):
            with pytest.raises(ValueError) as e:
                cls(**args)
            assert text in str(e.value), (cls.__name__, kw, str(e.value))
    with pytest.raises(TypeError):                               # the advance is a receiver value
        OF.PuschOfdmModulator(128, 10, cp, window_advance=4)
    for bad in (None, mod, "dem"):
        with pytest.raises(ValueError, match="dem must be a PuschOfdmDemodulator"):
            OF.PuschOfdmModulator.for_demodulator(bad)
    # no CPU fallback: the call is refused before it looks at its arguments
    grid = torch.zeros((1, 1, 14, 120), dtype=torch.complex64).permute(0, 1, 3, 2)
    with pytest.raises(RuntimeError, match="the OFDM modulator runs on a ROCm GPU only"):
        OF.PuschOfdmModulator(128, 10, cp, device="cpu")(grid)


def test_for_demodulator_copies_the_parameters(lib):
    cp = OF.nr_cp_lengths(120e3, 512, 12, slot=4)
    phi = OF.nr_symbol_phasors(10e3, 120e3, 512, cp)
    dem = OF.PuschOfdmDemodulator(512, 24, cp, n_sym=12, window_advance=18, sym_phasor=phi, device="cuda:0")
    mod = OF.PuschOfdmModulator.for_demodulator(dem)
    assert (mod.n_fft, mod.n_prb_grid, mod.n_sym, mod.cp_len, mod.n_sc, mod.n_samples) == (512, 24, 12, tuple(cp), 288, dem.n_samples)
    assert mod.window_advance == 0 and dem.window_advance == 18 and mod._device_arg == "cuda:0"
    assert mod.sym_phasor.dtype == np.complex64 and np.array_equal(mod.sym_phasor, dem.sym_phasor) and np.array_equal(mod.sym_phasor, phi)
    assert (mod.radix, mod.threads_per_row, mod.rows_per_workgroup) == (dem.radix, dem.threads_per_row, dem.rows_per_workgroup)
    assert OF.PuschOfdmModulator.for_demodulator(dem, device="cuda:1")._device_arg == "cuda:1"
    bare = OF.PuschOfdmModulator.for_demodulator(OF.PuschOfdmDemodulator(128, 1, OF.nr_cp_lengths(30e3, 128)))
    assert bare.sym_phasor is None and bare._device_arg is None and (bare.n_sc, bare.n_samples) == (12, 1920)


def test_float32_restatement_calibrates_the_tolerance(lib):
    """C_TX of ofdm_tx_oracle's tolerance rule, re-measured over exactly the inputs the GPU tests use: `modulate_f32` against
    `ofdm_oracle.modulate` in the rule's unit, printed per case; a value above C_TX_RECORDED fails (inside X.check, with t = C)."""
    worst = 0.0
    for c in X.CASES:
        d, got = _f32(c["name"])
        assert got.shape == (c["B"], c["R"], d.T) == d.ref.shape == d.rms.shape
        worst = max(worst, X.check(got, d.ref, d.rms, c["n_fft"], c["name"], t=X.C_TX_RECORDED))
    print(f"C_TX = {worst:.2f}  (C_TX_RECORDED = {X.C_TX_RECORDED:g}, T_TX = {X.T_TX:g})")
    assert worst <= X.C_TX_RECORDED and X.T_TX == 4.0 * X.C_TX_RECORDED
    assert worst >= 0.25                                         # the restatement is float32 indeed


def test_the_oracles_agree_on_the_operator(lib):
    """The float64 demodulator oracle returns the grid from the restatement's samples, for any advance inside the prefix, and
    the restatement without phasors differs from the one with them by conj(phi_l) per symbol."""
    for name in ("n128_p10_15k_a4", "n512_p24_120k_slot4", "n128_p1"):
        d, got = _f32(name)
        c = d.c
        for a in (0, min(d.cp)):
            back = O.demodulate_ref(got, c["n_fft"], c["n_prb_grid"], d.cp, a, d.phi)
            assert np.abs(back - d.grid).max() < 1e-4 * np.sqrt(c["n_fft"]), (name, a)
        assert d.rms.shape == d.ref.shape and np.all(d.rms > 0)
        t, c0 = d.starts[0], d.cp[0]
        assert np.allclose(d.rms[..., t], np.sqrt(np.mean(np.abs(d.ref[..., t + c0:t + c0 + c["n_fft"]]) ** 2, -1)))


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_cyclic_prefix_of_the_restatement_is_the_symbols_tail_bitwise(name):
    d, got = _f32(name)
    N, bits = d.c["n_fft"], None
    bits = np.ascontiguousarray(got).view(np.uint64)
    assert sum(d.cp) + len(d.cp) * N == d.T == got.shape[-1]
    for t, c in zip(d.starts, d.cp):
        assert c > 0 and np.array_equal(bits[..., t:t + c], bits[..., t + N:t + N + c]), (name, t, c)


def test_the_cases_reach_every_launch_geometry(lib):
    seen = set()
    for c in X.CASES:
        d = X.inputs(c["name"])
        v = OF.derive_host(c["n_fft"], c["n_prb_grid"], d.cp, c["n_sym"], 0)
        seen.add((v.threads_per_row, v.rows_per_workgroup, c["n_sym"] % v.rows_per_workgroup != 0 or v.rows_per_workgroup == 1))
        assert c["B"] <= 2 and c["R"] <= 4 and d.grid.shape == (c["B"], c["R"], 12 * c["n_prb_grid"], c["n_sym"]) and d.grid.dtype == np.complex64
        assert (d.phi is not None) == c["phasor"] and c["n_fft"] - d.n_sc >= 4 and (d.n_sc // 2) % 2 == 0      # guard bins; a pair never straddles DC
    assert seen >= {(64, 4, True), (128, 2, True), (256, 1, True)}
    assert {c["n_fft"] for c in X.CASES} == set(OF.FFT_SIZES) and {c["n_sym"] for c in X.CASES} == {14, 12, 1}
    assert any(t % 2 for t in X.inputs("n128_p10_15k_a0").starts)                                 # a symbol at an odd sample
    assert X.inputs("n512_p24_120k_slot4").cp == [68] + [36] * 13 and X.inputs("n128_p1").n_sc == 12 and X.inputs("n4096_p341_s12").n_sc == 4092
    assert X.inputs("n512_p24_s1").c["n_sym"] == 1                                               # two rows per workgroup, one inactive


def test_no_flat_addressing_no_scratch_16_byte_loads_and_8_byte_stores_in_the_kernel():
    src = CSRC / "ce_ofdm.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^(_ZN12_GLOBAL__N_116ce_ofdmtx_kernel\w+):\s*;.*?\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert len(kernels) == 1
    name, body = kernels[0]
    assert not re.search(r"\bflat_(load|store)", body) and not re.search(r"\bscratch_(load|store)", body) and not re.search(r"\batomic", body)
    assert re.search(r"\bglobal_load_dwordx4\b", body) and re.search(r"\bglobal_store_dwordx2\b", body)      # 16-byte loads of the grid, 8-byte stores of the samples
    assert not re.search(r"\bglobal_store_(dword|byte|short)\b", body), "a narrower store"
    assert not re.search(r"\bglobal_store_(dwordx3|dwordx4)\b", body), "a store that needs more than 8-byte alignment"
    meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)", text)
    assert meta and int(meta.group(1)) == 0                      # no scratch
