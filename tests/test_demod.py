"""CPU-side checks of the soft-demapper extension (include/ce_demod.h): the ABI, descriptor errors before any device
call, the library's Gold tables combined by the documented rule against the bit-serial generator, the calibration of the
tolerance rule the GPU tests apply and the condition on their draw, the constellations, the end-to-end chain's decision
margins through the CPU oracles, and a static check of the kernel instances.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import ce_oracle as O
import demod_oracle as D
import dmrs_oracle
import eq_oracle as Q
from srsran_ce_pytorch_amd import _lib, demod as DM, synth as S

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"
IDS = [c["name"] for c in D.CASES]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_every_declared_demod_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies and
    the relations between its constants."""
    # LP64 sizes implied by the header: desc 6*4 + 4 = 28; info 4 + 4 + 8 = 16; view 6*4 + 8 = 32
    assert (C.sizeof(_lib.DemodDesc), C.sizeof(_lib.DemodInfo), C.sizeof(_lib.DemodHostView)) == (28, 16, 32)
    assert _lib.CE_DEMOD_MAX_BITS >= D.BIG_M * 8 and "ce_demod.hip" in _lib.SOURCES and "ce_demod.h" in _lib.REGISTRY
    # a tile is whole Gold blocks at every modulation order, so a workgroup steps only blocks of its own
    for qm in (2, 4, 6, 8):
        assert (_lib.CE_DEMOD_TILE_SYMBOLS * qm) % (32 * _lib.CE_DEMOD_BLOCK_WORDS) == 0


def test_descriptor_errors_come_before_any_device_call(lib):
    v = DM.derive_host("256qam", D.BIG_M, torch.int8, 2.0, True)
    assert (v.n_bits, v.n_words, v.block_words, v.n_blocks) == (1362816, 42588, 8, 5324) and v.n_tiles == -(-D.BIG_M // 1024)
    assert v.table_bytes == 4 * 8 * 5324 + 4 * 32 * 5324
    v = DM.derive_host(2, 1, descramble=True)
    assert (v.n_bits, v.n_words, v.n_blocks, v.n_tiles) == (2, 1, 1, 1)
    v = DM.derive_host("qpsk", 156)
    assert (v.n_bits, v.n_words, v.n_blocks, v.table_bytes) == (312, 0, 0, 0)           # no descrambling: no tables
    for name, qm in DM.MODULATIONS.items():
        assert DM.PuschDemapper(name, 12).n_bits == DM.PuschDemapper(qm, 12).n_bits == 12 * qm
    with pytest.raises(NotImplementedError, match="qm=3"):
        DM.derive_host(3, 10)
    with pytest.raises(ValueError, match="bpsk"):
        DM.derive_host("bpsk", 10)
    with pytest.raises(ValueError, match="n_symbols=0"):
        DM.derive_host(2, 0)
    with pytest.raises(NotImplementedError, match="bits per slot"):
        DM.derive_host(8, _lib.CE_DEMOD_MAX_BITS // 8 + 1)
    assert DM.derive_host(8, _lib.CE_DEMOD_MAX_BITS // 8).n_bits == _lib.CE_DEMOD_MAX_BITS
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="llr_scale"):
            DM.PuschDemapper("qpsk", 10, out_dtype=torch.int8, llr_scale=bad)
    with pytest.raises(ValueError, match="out_dtype"):
        DM.PuschDemapper("qpsk", 10, out_dtype=torch.float16)
    desc = DM.build_desc(4, 37, torch.int8, 2.0, True)
    view, handle = _lib.DemodHostView(), C.c_void_p()
    assert lib.ce_demod_derive_host(C.byref(desc), C.byref(view)) == 0
    desc.abi_version = _lib.CE_ABI_VERSION + 1
    assert lib.ce_demod_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID and b"ABI" in lib.ce_last_error()
    for bad in ("abi", "qm", "n_symbols", "bits", "scale", "format", "descramble"):   # plan creation refuses each before it touches a device
        desc = DM.build_desc(4, 37, torch.int8, 2.0, True)
        if bad == "abi":
            desc.abi_version += 1
        elif bad == "qm":
            desc.qm = 3
        elif bad == "n_symbols":
            desc.n_symbols = 0
        elif bad == "bits":
            desc.n_symbols = _lib.CE_DEMOD_MAX_BITS // 4 + 1
        elif bad == "scale":
            desc.llr_scale = float("nan")
        elif bad == "format":
            desc.out_format = 2
        else:
            desc.descramble = 2
        code = lib.ce_demod_plan_create(C.byref(desc), C.byref(handle))
        assert not handle.value and code == (_lib.CE_ERR_UNSUPPORTED if bad in ("qm", "bits") else _lib.CE_ERR_INVALID), bad
    x1 = np.zeros(8, np.uint32)
    desc = DM.build_desc(4, 37)
    assert lib.ce_demod_copy_tables(C.byref(desc), C.c_void_p(x1.ctypes.data), C.c_void_p(x1.ctypes.data)) == _lib.CE_ERR_INVALID


def _combine(x1, jump, ci, n_bits):
    """c(0 .. n_bits-1) from the host tables by the rule of include/ce_demod.h, the in-block stepping bit by bit."""
    bw = _lib.CE_DEMOD_BLOCK_WORDS
    state = np.zeros(jump.shape[0], np.uint32)
    for i in range(31):
        if ci >> i & 1:
            state ^= jump[:, i]
    x = np.zeros((jump.shape[0], 31 + 32 * bw), np.uint8)              # every block stepped at once, each from its own state
    x[:, :31] = (state[:, None] >> np.arange(31, dtype=np.uint32)) & 1
    for n in range(32 * bw):
        x[:, n + 31] = x[:, n + 3] ^ x[:, n + 2] ^ x[:, n + 1] ^ x[:, n]
    x2 = x[:, :32 * bw].reshape(-1)[:n_bits]
    x1_bits = ((x1[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)[:n_bits]
    return x1_bits ^ x2


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_host_tables_combine_to_the_bit_serial_sequence(lib, c):
    G = c["M"] * c["qm"]
    v = DM.derive_host(c["qm"], c["M"], descramble=True)
    x1, jump = DM.gold_tables(c["qm"], c["M"])
    assert x1.shape == (v.n_words,) and jump.shape == (v.n_blocks, 31) and v.n_words == -(-G // 32) and v.n_blocks == -(-v.n_words // 8)
    own = [D.c_init(r, i) for r, i in zip(c["rnti"], c["n_id"])]
    assert D.c_init(65535, 1023) == 2 ** 31 - 2 ** 15 + 1023 and D.c_init(0, 0) == 0
    for ci in sorted({0, 2 ** 31 - 1, 1, 1 << 30, *own}):
        assert np.array_equal(_combine(x1, jump, ci, G), D.scrambling(ci, G)), hex(ci)


def test_dmrs_and_descrambling_tables_sample_one_generator(lib):
    """The DM-RS rows and the demapper's jump entries are the one generator of csrc/ce_gold.h sampled two ways: row T[i]
    holds the x2-only words of c for c_init = 1 << i, a jump entry the 31-bit x2 state at a block's first bit -- the low
    31 bits of that block's first word; the x1 words are the same words."""
    from srsran_ce_pytorch_amd import dmrs
    h1, h2, _ = S.numpy_hops(S.bench_case("filter", 1))
    view = dmrs.derive_host(h1, h2, 1, 273, 14)                          # full band from CRB 0: words 0 .. 102
    assert (view.word0[0], view.n_words[0]) == (0, 103)
    x1, jump = DM.gold_tables(2, 1664)
    bw = _lib.CE_DEMOD_BLOCK_WORDS
    assert x1.shape == (104,) and jump.shape == (13, 31) and bw * 12 < 103
    assert np.array_equal(x1[:103], np.array(view.x1[0][:103], np.uint32))
    t = np.array([view.t[0][i][:103] for i in range(31)], np.uint32)     # [i][word]
    assert np.array_equal(jump.T, t[:, ::bw] & np.uint32(0x7FFFFFFF))    # jump[blk, i] == T[i][8 blk] & 0x7FFFFFFF


def test_table_bytes_stay_under_half_of_the_slot_traffic(lib):
    """Qm = 8, int8: a slot reads 12 M bytes and writes 8 M; its workgroups read the x1 words once and 31 jump entries
    per block: M + 124 M / 32 bytes -- under half of 20 M.  A full 31-row table over all words would be 32 M."""
    M = 273 * 12 * 12
    v = DM.derive_host(8, M, torch.int8, 1.0, True)
    read = 4 * v.n_blocks * v.block_words + 4 * 31 * v.n_blocks
    assert read <= (12 * M + 8 * M) / 2 and 4 * 32 * v.n_words > (12 * M + 8 * M) / 2
    print(f"table bytes read per slot {read} = {read / M:.3f} per symbol; input + output {20 * M}")


def test_float32_restatement_calibrates_the_tolerance():
    """C = the largest ratio of llr_f32's own error to 2^-24 (|y_ax| + a_max)^2 / nvar over the GPU tests' inputs; T = 4 C
    is recorded in demod_oracle.py.  Fails when the re-measured C exceeds the recorded one."""
    worst = 0.0
    for c in D.CASES:
        d = D.inputs(c["name"])
        ratio = float((np.abs(D.llr_f32(d.x, d.nvar, d.qm).astype(np.float64) - d.ref) / d.tol).max())
        print(f"{c['name']:>16}: Qm={d.qm} M={d.M}  C = {ratio:5.2f}")
        worst = max(worst, ratio)
    print(f"C = {worst:.2f} (recorded {D.C_RECORDED:g}, T = {D.T:g})")
    assert worst <= D.C_RECORDED and D.T == 4.0 * D.C_RECORDED


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_the_draw_keeps_the_rule_tight(c):
    """The largest absolute tolerance stays below 1e-2 and the median |llr| above 1, so an indexing or bit-order error
    cannot hide; the int8 scale leaves saturated and unsaturated values in the case; the draw is the one stated."""
    d = D.inputs(c["name"])
    assert c["sigma2"] == 10.0 ** -1.5 and d.x.dtype == np.complex64 and d.nvar.dtype == np.float32
    tol = D.T * d.tol
    med = float(np.median(np.abs(d.ref)))
    q = np.abs(d.ref) * d.scale
    n_sat, n_unsat = int(np.sum(q >= 128.0)), int(np.sum(q <= 126.0))
    print(f"{c['name']}: max tolerance {tol.max():.2e}, median |llr| {med:.2f}, int8 scale {d.scale:g}: {n_sat} saturated, {n_unsat} not")
    assert tol.max() < 1e-2 and med > 1.0
    assert n_sat > 0 and n_unsat > 0
    assert len(set(zip(c["rnti"], c["n_id"]))) == c["B"]
    if c["B"] == 3:
        assert (65535, 1023) in zip(c["rnti"], c["n_id"]) and (0, 0) in zip(c["rnti"], c["n_id"])
    # hard decisions of the oracle's LLRs give (nearly all of) the bits that were sent: the sign convention is the stated one
    assert np.mean((d.ref < 0) == d.bits.astype(bool)) > 0.8


@pytest.mark.parametrize("qm,bits,point", [(2, [1, 0], (-1 + 1j) / np.sqrt(2)), (4, [0, 1, 1, 0], (3 - 1j) / np.sqrt(10)),
                                           (6, [1, 0, 0, 1, 1, 0], (-1 + 5j) / np.sqrt(42)),
                                           (8, [0, 1, 1, 0, 0, 1, 1, 1], (9 - 1j) / np.sqrt(170))])
def test_constellations_have_unit_power_and_the_standard_gray_map(qm, bits, point):
    pts = D.constellation(qm)
    assert len(set(np.round(pts, 9))) == 1 << qm and abs(np.mean(np.abs(pts) ** 2) - 1.0) < 1e-12
    assert abs(D.modulate(np.array(bits), qm)[0] - point) < 1e-12
    assert abs(np.abs(pts.real).max() - D.a_max(qm)) < 1e-12
    # Gray: nearest neighbours along an axis differ in one bit
    idx = np.arange(1 << qm)
    for i in idx:
        d = np.abs(pts - pts[i])
        for n in idx[np.isclose(d, 2 / np.sqrt(D.NORM[qm]))]:
            assert bin(i ^ n).count("1") == 1


def test_oracle_special_values_are_erasures():
    x = np.array([[0.3 + 0.1j, np.inf + 0j, 0.2 + np.nan * 1j, 0.1 - 0.2j, 0, 0.5j, -0.5, 1 + 0.45j]], np.complex64)
    nv = np.array([[0.1, 0.1, 0.1, np.inf, 0.0, -1.0, np.nan, 0.2]], np.float32)
    for qm in (2, 4, 6, 8):
        ref, tol = D.llr_ref(x, nv, qm).reshape(8, qm), D.unit_tolerance(x, nv, qm).reshape(8, qm)
        assert np.all(ref[1:7] == 0) and np.all(tol[1:7] == 0) and np.all(ref[[0, 7]] != 0) and np.all(tol[[0, 7]] > 0)
        f32 = D.llr_f32(x[:, [0, 7]], nv[:, [0, 7]], qm).reshape(2, qm)
        assert np.all(np.abs(f32 - ref[[0, 7]]) <= D.T * tol[[0, 7]])


def test_end_to_end_chain_keeps_16qam_clear_of_the_decision_boundaries():
    """The GPU end-to-end test's chain through the CPU oracles: pilots, estimate, equalize.  The equalized 16QAM symbols
    must keep a clear margin to the decision boundaries (0 and +-2 / sqrt(10) per axis), so that hard decisions on the
    GPU's LLRs are a meaningful check."""
    case = D.e2e_case()
    h1, h2, cfg = S.numpy_hops(case)
    pil = dmrs_oracle.pilots_ref(case, D.E2E_SLOT, D.E2E_N_ID, D.E2E_N_SCID)
    data_re = Q.data_re_ref(case)
    grids, bits, x_tx = D.e2e_slot(pil, data_re, np.random.default_rng(78))
    est = [O.srs_channel_estimator(grids[r], pil, case["beta"], h1, h2, cfg) for r in range(D.E2E_PORTS)]
    ch = np.stack([e[0] for e in est])[None]
    noise = np.array([[float(e[1]) for e in est]])
    ref = Q.equalize_ref(grids[None], ch, noise, data_re)
    u = np.stack([ref.x_hat.real, ref.x_hat.imag]).reshape(-1) * np.sqrt(10.0)
    margin = np.minimum(np.abs(u), np.abs(np.abs(u) - 2.0)).min()          # 1.0 = a symbol exactly on its point
    err = np.abs(ref.x_hat[0] - x_tx).max() * np.sqrt(10.0)
    print(f"16QAM end to end on the CPU: smallest distance to a decision boundary {margin:.3f} (1 = on the point), largest symbol error {err:.3f}")
    assert margin > 0.5
    llr = D.llr_ref(ref.x_hat.astype(np.complex64), ref.nvar.astype(np.float32), D.E2E_QM)[0]
    flip = D.scrambling(D.c_init(D.E2E_RNTI, D.E2E_SCR_ID), len(bits)).astype(bool)
    assert np.array_equal(np.where(flip, -llr, llr) < 0, bits.astype(bool))


def test_no_flat_addressing_and_no_scratch_in_any_demapper_instance():
    src = CSRC / "ce_demod.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^(_ZN12_GLOBAL__N_115ce_demod_kernelILi(\d)ELb([01])E\w+):\s*;.*?\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert sorted((int(q), int(i8)) for _, q, i8, _ in kernels) == [(q, f) for q in (2, 4, 6, 8) for f in (0, 1)]
    for _, qm, i8, body in kernels:
        assert not re.search(r"\bflat_(load|store)", body), f"<{qm},{i8}> uses flat addressing"
        assert not re.search(r"\bscratch_(load|store)", body), f"<{qm},{i8}> uses scratch"
        assert re.search(r"\bglobal_load_dwordx4\b", body) and re.search(r"\bglobal_store_dwordx4\b", body)   # 16-byte loads and stores
