"""CPU-side checks of the transform precoding entry point (include/ce_tp.h `ce_tp_precode`): the export and the package's
re-export, the calibration of the float32 restatement that sets the GPU tolerance (tests/tpre_oracle.py), the refusal that
needs no plan, `PuschTransformPrecoder.for_modulator` against a brute-force walk of the data REs, and the DFT-s-OFDM loop
through the CPU oracles.  No GPU.

Every other refusal of `ce_tp_precode` (odd or negative offsets and strides, overlapping rows, offset + M > stride, a
misaligned pointer, partial overlap of x and y, in place with other offsets, negative n_slots, null tensors) comes behind
the null-plan check and so needs a plan handle, which only a device gives: tests/test_zzzzzzzzzzz_hip_precode.py
`test_refusals_empty_batch_and_stream` exercises each with its text."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import demod_oracle as D
import enc_oracle as E
import ldpc_oracle as O
import mod_oracle as MO
import rm_oracle as R
import tb_oracle as TB
import tp_oracle as T
import tpre_oracle as P
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, deprecode as DP, ldpc as LD, modulator as MD, precode as PR, synth as S


ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_ce_tp_precode_and_the_package_the_class(lib):
    assert "ce_tp_precode" in _lib.REGISTRY["ce_tp.h"].signatures and "ce_tp_precode" in _lib.ALL_EXPORTS
    assert lib.ce_tp_precode.restype is C.c_int and len(lib.ce_tp_precode.argtypes) == 9
    assert PKG.PuschTransformPrecoder is PR.PuschTransformPrecoder
    assert (PR.PuschTransformPrecoder._CREATE, PR.PuschTransformPrecoder._DESTROY, PR.PuschTransformPrecoder._LAUNCH) == \
        ("ce_tp_plan_create", "ce_tp_plan_destroy", "ce_tp_precode")
    # no plan: refused before anything else, whatever the other arguments
    assert lib.ce_tp_precode(None, None, 0, None, None, 0, None, 0, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    buf = np.zeros(64, np.complex64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.ce_tp_precode(None, p, 12, None, p, 12, None, 1, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    assert not buf.any()


def test_no_flat_addressing_no_scratch_and_16_byte_accesses_in_the_precode_kernel():
    src = CSRC / "ce_tp.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^(_ZN12_GLOBAL__N_120ce_tp_precode_kernel\w+):\s*;.*?\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert len(kernels) == 1
    body = kernels[0][1]
    assert not re.search(r"\bflat_(load|store)", body) and not re.search(r"\bscratch_(load|store)", body) and not re.search(r"\batomic", body)
    assert re.search(r"\bglobal_load_dwordx4\b", body) and re.search(r"\bglobal_store_dwordx4\b", body)      # 16-byte loads of x, 16-byte stores of y
    assert not re.search(r"\bglobal_store_(dword|dwordx2|dwordx3|byte|short)\b", body), "a narrower store"
    assert not re.search(r"\bglobal_load_(dwordx3|ubyte|sbyte|ushort|sshort)\b", body)


def _views(M, S_):
    return DP.derive_host(M // 12, S_), DP.twiddles(M // 12)


def _calibrate(x, ref, M, S_, what):
    view, tw = _views(M, S_)
    return P.check(P.precode_f32(x, view, tw), ref, M, what, t=P.C_PRE_RECORDED)


def test_float32_restatement_calibrates_the_tolerance(lib):
    """C_PRE of tpre_oracle's tolerance rule, re-measured over exactly the inputs the GPU tests use: `precode_f32` against
    `tp_oracle.precode` in the rule's unit, printed per case; a value above C_PRE_RECORDED fails (inside P.check, with t = C)."""
    worst = 0.0
    for M, S_ in T.CASES:
        d = P.inputs(M, S_)
        worst = max(worst, _calibrate(d.x, d.ref, M, S_, f"M={M} S={S_}"))
    for name in P.GRID_NAMES:
        d = P.grid_inputs(name)
        worst = max(worst, _calibrate(d.x, d.ref, d.M, d.S, f"grid {name} M={d.M} S={d.S}"))
    print(f"C_PRE = {worst:.2f}  (C_PRE_RECORDED = {P.C_PRE_RECORDED:g}, T_PRE = {P.T_PRE:g})")
    assert worst <= P.C_PRE_RECORDED and P.T_PRE == 4.0 * P.C_PRE_RECORDED
    assert worst >= 0.25                                        # the restatement is float32 indeed


def test_float32_restatement_on_all_53_sizes(lib):
    worst = 0.0
    for n in T.VALID_PRBS:
        M = 12 * n
        x = T.draw(M, 1, seed=2).x_tx.astype(np.complex64)
        worst = max(worst, _calibrate(x, T.precode(x, M), M, 1, f"n_prbs={n}"))
    print(f"all 53 sizes at S = 1: C_PRE = {worst:.2f}")
    assert worst <= P.C_PRE_RECORDED


def test_restatement_is_the_de_precoders_passes_between_two_conjugations(lib):
    """precode_f32(x) = conj(the de-precoder restatement's transform of conj(x)) up to the final scale: with nvar = 1 on every
    RE, beta = 1 / 2 exactly, sum beta = M / 2 exactly, and deprecode_f32 scales by sqrt(M) / (M / 2) where precode_f32 scales by
    1 / sqrt(M) -- one definition of the passes for both directions."""
    for M, S_ in ((12, 3), (300, 1), (3240, 1)):
        d = P.inputs(M, S_)
        view, tw = _views(M, S_)
        inv, _ = T.deprecode_f32(np.conj(d.x), np.ones(d.x.shape, np.float32), view, tw)         # (1 / sqrt(M)) IDFT-sum of conj(x), float32
        got = P.precode_f32(d.x, view, tw)
        assert np.abs(np.conj(inv).astype(np.complex128) - got).max() <= 8 * T.EPS * np.abs(got).max()


def _mod(c, **kw):
    args = dict(n_sym=c["case"]["n_sym"], reserved_re_mask=c["mask"])
    args.update(kw)
    return MD.PuschModulator(*MO.hops(c), c["L"], c["case"]["n_prb_grid"], c["qm"], **args)


@pytest.mark.parametrize("name", P.GRID_NAMES)
def test_for_modulator_rows_against_a_walk_of_the_data_res(lib, name):
    c = P.GRID_BY_NAME[name]
    offsets, M, stride = P.grid_rows(c["case"])
    pre = PR.PuschTransformPrecoder.for_modulator(_mod(c))
    assert (list(pre.row_offsets), pre.slot_stride, pre.m_sc, pre.n_symbols) == (offsets, stride, M, len(offsets))
    assert pre.n_prbs == c["case"]["hops"][0]["n_prbs"] and pre.device is None
    assert all(o % 2 == 0 for o in offsets) and stride % 2 == 0
    view = DP.derive_host(pre.n_prbs, pre.n_symbols)
    want = {"bg2_z7_rep": (48, 5, 4), "two_hops": (72, 12, 4), "start2_partial": (24, 7, 4), "270_of_273": (3240, 12, 1)}[name]
    assert (M, len(offsets), view.rows_per_workgroup) == want
    if name == "two_hops":
        n_sc = 12 * c["case"]["n_prb_grid"]
        assert sorted({o % n_sc for o in offsets}) == [48, 360]
    if name == "start2_partial":
        assert len(offsets) % view.rows_per_workgroup != 0 and offsets[0] // (12 * 24) == 2
    if name == "270_of_273":
        assert pre.radix == (4, 2, 3, 3, 3, 3, 5)


def test_for_modulator_refusals(lib):
    c = P.GRID_BY_NAME["two_hops"]
    grid = c["case"]["n_prb_grid"]

    def mod(hops, L=1, mask=0xFFF):
        case = S.case_spec("x", grid, hops, n_layers=L)
        h1, h2, _ = S.numpy_hops(case)
        return MD.PuschModulator(h1, h2, L, grid, "16qam", reserved_re_mask=mask)

    one = [S.hop_spec([2, 11], 10, 6)]
    with pytest.raises(ValueError, match="single-layer, the modulator has 2 layers"):
        PR.PuschTransformPrecoder.for_modulator(mod(one, L=2))
    with pytest.raises(ValueError, match="symbol 2 carries data on 6 of 12 REs per PRB"):
        PR.PuschTransformPrecoder.for_modulator(mod(one, mask=0x555))
    with pytest.raises(ValueError, match="n_prbs=7 has a prime factor above 5"):
        PR.PuschTransformPrecoder.for_modulator(mod([S.hop_spec([2, 11], 10, 7)]))
    with pytest.raises(ValueError, match="PuschModulator"):
        PR.PuschTransformPrecoder.for_modulator(object())
    pre = PR.PuschTransformPrecoder.for_modulator(mod(one))
    assert (pre.n_prbs, pre.n_symbols, len(pre.row_offsets)) == (6, 12, 12)
    # dense-row instances: validated like the de-precoder, and without a grid
    with pytest.raises(ValueError):
        PR.PuschTransformPrecoder(7, 12)
    with pytest.raises(ValueError):
        PR.PuschTransformPrecoder(6, 0)
    dense = PR.PuschTransformPrecoder(6, 12)
    assert dense.m_sc == 72 and dense.radix == (4, 2, 3, 3) and dense.row_offsets is None and dense.device is None
    with pytest.raises(ValueError, match="for_modulator"):
        dense.grid_(None)


def _receive(tx, offsets, M):
    """tx through mod_oracle.loop_channel on 4 ports, per-RE zero forcing with the true channel (x_hat = sum conj(h) y / g,
    nvar = LOOP_NVAR / g, g = sum |h|^2), deprecode_ref, llr_ref, descrambling, int8 LLRs at scale 4, rate recovery, LDPC,
    transport-block assembly.  Returns (tb rows, tb_status, the worst per-axis distance of the de-precoded symbols from a
    QPSK point in units of the point's coordinate)."""
    lp, case = E.LOOPS[P.LOOP_NAME], MO.loop_case(P.LOOP_NAME)
    d, g = E.case_derive(P.LOOP_NAME), E.graph(P.LOOP_NAME)
    B, n_sc = tx.shape[0], 12 * case["n_prb_grid"]
    H = MO.loop_channel(case, np.random.default_rng(81)).astype(np.complex128)[:, :, 0]           # [R, n_sc]
    rx = np.einsum("rk,bsk->brsk", H, tx[:, 0])                                                   # [B, R, n_sym, n_sc]
    x_hat, nvar = [], []
    for o in offsets:
        s, k0 = divmod(o, n_sc)
        h = H[:, k0:k0 + M]
        gain = (np.abs(h) ** 2).sum(0)
        x_hat.append((np.conj(h)[None] * rx[:, :, s, k0:k0 + M]).sum(1) / gain)
        nvar.append(np.broadcast_to(P.LOOP_NVAR / gain, (B, M)))
    x, nv = T.deprecode_ref(np.concatenate(x_hat, 1), np.concatenate(nvar, 1), M)
    u = np.stack([x.real, x.imag]) * np.sqrt(2.0)
    llr = D.llr_ref(x, nv, lp["qm"])
    flip = D.scrambling(D.c_init(MO.LOOP_RNTI, MO.LOOP_SCR_ID), lp["G"]).astype(bool)
    llr = np.where(flip[None], -llr, llr)
    q = np.clip(np.rint(4.0 * llr), -127, 127).astype(np.int8)
    soft, _ = R.recover(d, q, [0] * B)
    L, _, _ = O.decode_ref(g.rows, g.n_cols, d.Zc, O.channel(O.quantise(soft.reshape(-1, d.N_cb)), g.n_cols, d.Zc, 2), 8, True)
    tb, tb_status, _ = TB.assemble_ref(O.pack(L, d.Kp).reshape(B, d.C, -1), TB.derive(d.bg, d.A))
    return tb, tb_status, float(np.abs(np.abs(u) - 1.0).max())


def test_the_dft_s_ofdm_loop_closes_through_the_cpu_oracles(lib):
    """What the GPU loop test leans on, from the references alone: enc_oracle's g -> mod_oracle -> tp_oracle.precode on the
    data rows -> the four-port channel -> zero forcing -> deprecode_ref -> llr_ref -> rate recovery, LDPC and transport-block
    oracles returns the transport block; with the precoding skipped and the de-precoding kept, no slot passes its CRC."""
    d = E.case_derive(P.LOOP_NAME)
    sent = np.array(E.inputs(P.LOOP_NAME)[0])
    tx, offsets, M = P.loop_tx(precoded=True)
    assert (M, len(offsets)) == (48, 5) and len(offsets) * M * 2 == E.LOOPS[P.LOOP_NAME]["G"]
    pre = PR.PuschTransformPrecoder.for_modulator(MD.PuschModulator(*S.numpy_hops(MO.loop_case(P.LOOP_NAME))[:2], 1, 24, "qpsk"))
    assert list(pre.row_offsets) == offsets
    plain, _, _ = P.loop_tx(precoded=False)
    assert np.abs(tx - plain).max() > 0.1                       # precoded indeed, and the DM-RS symbol is not
    assert np.array_equal(tx[:, 0, 2], plain[:, 0, 2])
    tb, status, dist = _receive(tx, offsets, M)
    print(f"DFT-s-OFDM loop: largest per-axis distance from the QPSK point {dist:.4f} (1 = the decision boundary)")
    assert dist < 0.5
    assert np.array_equal(LD.unpack_bits(tb, d.A), sent) and not status.any()
    _, status, _ = _receive(plain, offsets, M)
    assert np.all(status[:, 0] != 0)
