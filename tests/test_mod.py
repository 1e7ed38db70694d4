"""CPU-side checks of the modulator extension (include/ce_mod.h): the ABI, the integers ce_mod_derive_host derives for the
pinned cases, every refusal before any device call, the oracle's constellation points against demod_oracle's, the oracle as
the inverse of what the receiver oracles expect (known channel -> eq_oracle -> demod_oracle with descrambling gives back the
bits of g), the geometries of the GPU loop test through oracle/ce_oracle.py's estimator, and a static check of the kernel
instances.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ce_oracle as O
import demod_oracle as D
import dmrs_oracle
import enc_oracle as E
import eq_oracle as Q
import mod_oracle as M
from srsran_ce_pytorch_amd import _lib, demod as DM, equalizer as EQ, modulator as MO, synth as S

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _view(c, **kw):
    return MO.derive_host(*M.hops(c), c["L"], c["case"]["n_prb_grid"], c["qm"], c["case"]["n_sym"], reserved_re_mask=c["mask"], **kw)


def test_library_exports_every_declared_mod_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies and
    its amplitudes against the oracles'."""
    assert "ce_mod.hip" in _lib.SOURCES and "ce_mod.h" in _lib.REGISTRY
    # LP64 sizes implied by the header: hop 14 + 2*2 + 2 + 4*4 + 4 (pad) + 8 = 48; desc 8*4 + 2*48; info 6*4 + 8; view 6*4 + 5*14*4 + 12*4
    assert (C.sizeof(_lib.ModHopDesc), C.sizeof(_lib.ModDesc), C.sizeof(_lib.ModInfo), C.sizeof(_lib.ModHostView)) == (48, 128, 32, 352)
    assert _lib.CE_MOD_A == {2: _lib.CE_MOD_A_QPSK, 4: _lib.CE_MOD_A_16QAM, 6: _lib.CE_MOD_A_64QAM, 8: _lib.CE_MOD_A_256QAM}
    for qm in (2, 4, 6, 8):
        assert int(M.amplitude(qm).view(np.uint32)) == _lib.CE_MOD_A[qm]
    assert _lib.CE_MOD_A[2] == int(dmrs_oracle.A.view(np.uint32))            # QPSK's constant is the DM-RS amplitude


@pytest.mark.parametrize("name", M.NAMES)
def test_derive_host_integers_of_the_pinned_cases(lib, name):
    c = M.CASE_BY_NAME[name]
    case, L, qm = c["case"], c["L"], c["qm"]
    v = _view(c)
    for k, want in c["pinned"].items():
        assert getattr(v, k) == want, (name, k, getattr(v, k))
    data_re = Q.data_re_ref(case, c["mask"])
    assert (v.n_data_re, v.n_symbols, v.n_bits, v.g_row_bytes) == (len(data_re), len(data_re) * L, len(data_re) * L * qm, 16 * -(-len(data_re) * L * qm // 128))
    ev = EQ.derive_host(*M.hops(c), L, case["n_prb_grid"], case["n_sym"], reserved_re_mask=c["mask"])
    for f in ("sym_hop", "data_mask", "data_res_per_prb", "first_row"):
        assert list(getattr(v, f)) == list(getattr(ev, f)), f
    cols = [s for h in case["hops"] for s in sorted(h["dmrs_symbols"])]
    assert [list(v.dmrs_col).index(i) for i in range(len(cols))] == cols and sorted(v.dmrs_col).count(-1) == 14 - len(cols)
    hs = dmrs_oracle.hops_of(case)
    assert (v.n_re, v.n_dmrs_total) == (int(hs[0][1].sum() * hs[0][2][:, 0].sum()), len(cols))
    dv = DM.derive_host(qm, v.n_symbols, descramble=True)                              # the demapper's tables, to the byte
    assert (v.n_words, v.block_words, v.n_blocks, v.table_bytes) == (dv.n_words, dv.block_words, dv.n_blocks, dv.table_bytes)
    assert (v.tile_sc, v.group_symbols, v.threads, v.lds_bytes) == (256, 7, 256, 7 * 4 * 8 * 35)
    assert v.tiles_per_symbol == -(-12 * case["n_prb_grid"] // 256) and v.n_groups == -(-case["n_sym"] // 7) and v.workgroups_per_slot == v.n_groups * v.tiles_per_symbol
    assert 1 <= v.max_tile_blocks <= _lib.CE_MOD_MAX_TILE_BLOCKS - 1
    off = _view(c, scramble=False)
    assert (off.n_words, off.n_blocks, off.table_bytes, off.n_bits) == (0, 0, 0, v.n_bits)


def _hop(dmrs, prb_start, n_prbs, start=0, n_alloc=14, re_masks=None, mask_prbs=None, n_prb_grid=24, n_sym=14):
    case = S.case_spec("x", n_prb_grid, [S.hop_spec(dmrs, prb_start, n_prbs, start, n_alloc, re_masks, mask_prbs)], n_sym=n_sym)
    return S.numpy_hops(case)[0]


def test_every_refusal(lib):
    none = S.empty_hop_arrays()
    ok = _hop([2, 11], 3, 5)
    assert MO.derive_host(ok, none, 2, 24, "16qam").n_bits == 5 * 12 * 12 * 2 * 4
    with pytest.raises(ValueError, match="scattered"):                                  # scattered PRBs: the reference extractor's quirk
        MO.derive_host(_hop([2, 11], 3, 5, mask_prbs=[3, 4, 6, 7, 8]), none, 1, 24, "qpsk")
    with pytest.raises(ValueError, match="scattered"):
        MO.derive_host(_hop([2, 11], 3, 5, mask_prbs=[3, 4, 5, 6, 7, 9]), none, 1, 24, "qpsk")
    with pytest.raises(ValueError, match="outside reserved_re_mask"):                   # an RE would be pilot and data
        MO.derive_host(ok, none, 1, 24, "qpsk", reserved_re_mask=0xAAA)
    with pytest.raises(ValueError, match="outside reserved_re_mask"):                   # the second CDM group's REs are not reserved
        MO.derive_host(_hop([2], 3, 5, re_masks=M.T1), none, 3, 24, "qpsk", reserved_re_mask=0x555)
    assert MO.derive_host(_hop([2], 3, 5, re_masks=M.T1), none, 2, 24, "qpsk", reserved_re_mask=0x555).n_re == 30    # ... and not in use with 2 layers
    with pytest.raises(ValueError, match="non-empty"):
        MO.derive_host(_hop([2], 3, 5, re_masks=[[0] * 12]), none, 1, 24, "qpsk")
    with pytest.raises(ValueError, match="has 4 REs"):                                  # CDM groups of different sizes
        MO.derive_host(_hop([2], 3, 5, re_masks=[S.TYPE1_CDM0, S.TYPE2_CDM1]), none, 3, 24, "qpsk")
    with pytest.raises(ValueError, match="DM-RS symbol 11 outside its symbols 0..6"):
        MO.derive_host(_hop([2, 11], 3, 5, 0, 7), none, 1, 24, "qpsk")
    with pytest.raises(NotImplementedError, match="share OFDM symbol 6"):               # the equalizer's refusal, in its words
        MO.derive_host(_hop([2], 3, 5, 0, 7), _hop([9], 12, 5, 6, 8), 1, 24, "qpsk")
    with pytest.raises(ValueError, match="hop 1 has 4 PRBs, hop 0 has 5"):
        MO.derive_host(_hop([2], 3, 5, 0, 7), _hop([9], 12, 4, 7, 7), 1, 24, "qpsk")
    with pytest.raises(ValueError, match="outside the grid of 24 PRB"):
        MO.derive_host(_hop([2], 20, 5), none, 1, 24, "qpsk")
    with pytest.raises(NotImplementedError, match="n_layers=5"):
        MO.derive_host(_hop([2, 11], 3, 5, re_masks=M.T1), none, 5, 24, "qpsk")
    # G over the cap: the library checks G <= CE_DEMOD_MAX_BITS, but no geometry it accepts reaches the cap -- the widest grid
    # (341 PRB = 4092 subcarriers <= CE_FFT_SIZE) x 14 symbols without DM-RS x 4 layers x 256QAM stays below it
    widest = MO.derive_host(_hop([], 0, 341, re_masks=M.T1, n_prb_grid=341), none, 4, 341, "256qam")
    assert widest.n_bits == 341 * 12 * 14 * 4 * 8 <= _lib.CE_DEMOD_MAX_BITS and (widest.n_re, widest.n_dmrs_total) == (0, 0)
    with pytest.raises(NotImplementedError, match="12\\*n_prb must be in"):
        MO.derive_host(_hop([2], 0, 342, re_masks=M.T1, n_prb_grid=342), none, 4, 342, "256qam")
    for bad in (1, 3, 10, 0):
        with pytest.raises(NotImplementedError, match="modulation orders 2, 4, 6 and 8"):
            MO.derive_host(ok, none, 1, 24, bad)
    with pytest.raises(ValueError, match="modulation"):
        MO.derive_host(ok, none, 1, 24, "bpsk")
    with pytest.raises(ValueError, match="12-bit RE mask"):
        MO.derive_host(ok, none, 1, 24, "qpsk", reserved_re_mask=0x1000)
    with pytest.raises(ValueError, match="maskPRBs has 24 entries"):
        MO.derive_host(ok, none, 1, 25, "qpsk")
    desc, keep = MO.build_desc(ok, none, 1, 24, "qpsk")
    view = _lib.ModHostView()
    desc.abi_version = 2
    assert lib.ce_mod_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID and "ABI version" in _lib.last_error()
    desc.abi_version, desc.scramble = 3, 2
    assert lib.ce_mod_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID and "scramble=2" in _lib.last_error()
    desc.scramble = 1
    desc.hop[0].mask_prbs = None                                                        # NULL: the contiguous run
    assert lib.ce_mod_derive_host(C.byref(desc), C.byref(view)) == 0 and view.n_bits == 5 * 12 * 12 * 2
    assert lib.ce_mod_derive_host(None, C.byref(view)) == _lib.CE_ERR_INVALID and lib.ce_mod_derive_host(C.byref(desc), None) == _lib.CE_ERR_INVALID
    assert lib.ce_mod_plan_create(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_mod_modulate(None, None, None, 0, 1.0, None, None, None, 0, None, None) == _lib.CE_ERR_INVALID
    del keep


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_the_oracles_points_lie_within_one_ulp_of_the_constellation(qm):
    pts, ref = M.points(qm), D.constellation(qm)
    assert pts.dtype == np.complex64 and len(np.unique(pts)) == 1 << qm
    for got, want in ((pts.real, ref.real), (pts.imag, ref.imag)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
    lv = M.levels(qm)
    assert sorted(set(lv[:, 0])) == sorted(set(lv[:, 1])) == list(range(-(1 << qm // 2) + 1, 1 << qm // 2, 2))
    assert abs(float(np.mean(np.abs(pts.astype(np.complex128)) ** 2)) - 1.0) < 1e-6       # unit mean power


@pytest.mark.parametrize("name", ["qpsk_3prb", "L4_type1", "L2_data_on_dmrs_symbols", "straddle_1prb_64qam", "L3_type2", "256qam_3prb_all_points", "tile_plus_1prb",
                                  "hops_13sym"])
def test_the_oracle_is_the_inverse_of_what_the_receiver_oracles_expect(name):
    """mod_oracle's tx through a known channel, eq_oracle.equalize_ref with the true channel, demod_oracle.llr_ref, the
    scrambling undone: the hard decisions are the bits of g.  Every Qm; 1, 2, 3 and 4 layers; one and two hops."""
    d, tx = M.inputs(name), M.reference(name)
    rng = np.random.default_rng(77)
    B, L, n_sym, n_sc = tx.shape
    R = 8                                                                                # 8 x L iid channels: well conditioned at every RE
    H = (rng.standard_normal((B, R, n_sc, n_sym, L)) + 1j * rng.standard_normal((B, R, n_sc, n_sym, L))) / np.sqrt(2.0)
    rx = np.einsum("brksl,blsk->brks", H, tx.astype(np.complex128))
    data_re = Q.data_re_ref(d.case, d.mask)
    ref = Q.equalize_ref(rx, H, np.full((B, R), 1e-9), data_re)            # (the LMMSE's residual inter-layer term scales with the noise)
    flip = M.scrambling_rows(d.rnti, d.n_id, B, d.G).astype(bool)
    sent = M.points(d.qm)[((d.g_bits ^ flip).reshape(B, -1, d.qm).astype(np.int64) << np.arange(d.qm)).sum(-1)]
    assert np.abs(ref.x_hat.reshape(B, -1) - sent).max() < 1e-4                          # the equalizer's rows are the modulator's symbols
    llr = D.llr_ref(ref.x_hat, ref.nvar, d.qm)
    assert np.array_equal(np.where(flip, -llr, llr) < 0, d.g_bits.astype(bool))
    if name == "256qam_3prb_all_points":
        assert len(np.unique(tx[0, 0][tuple(data_re[:256].T)])) == 256                    # all 256 points occur


@pytest.mark.parametrize("name", sorted(M.LOOP_GEOMETRY))
def test_the_loop_geometries_close_through_the_cpu_oracles(name):
    """What the GPU loop test leans on: the encoder oracle's g -> mod_oracle -> a frequency-selective channel on 4 ports ->
    oracle/ce_oracle.py's estimator with dmrs_oracle's pilots -> eq_oracle -> demod_oracle with descrambling gives the hard
    decisions g, with a margin: a geometry the oracles cannot close is the wrong geometry, not a kernel finding."""
    lp, case = E.LOOPS[name], M.loop_case(name)
    h1, h2, cfg = S.numpy_hops(case)
    qm, L = lp["qm"], lp["L"]
    g_rows = E.reference(name, 0)[0]
    bits = np.unpackbits(g_rows, axis=-1)[:, :lp["G"]]
    pil = dmrs_oracle.pilots_ref(case, M.LOOP_SLOT, M.LOOP_N_ID, M.LOOP_N_SCID)
    tx = M.modulate_ref(case, 0xFFF, qm, bits, pil, case["beta"], M.LOOP_RNTI, M.LOOP_SCR_ID)
    H = M.loop_channel(case, np.random.default_rng(81))
    rx = np.einsum("rkl,blsk->brks", H, tx).astype(np.complex64)
    data_re = Q.data_re_ref(case)
    flip = D.scrambling(D.c_init(M.LOOP_RNTI, M.LOOP_SCR_ID), lp["G"]).astype(bool)
    for b in range(len(bits)):
        est = [O.srs_channel_estimator(rx[b, r], pil, case["beta"], h1, h2, cfg) for r in range(M.LOOP_PORTS)]
        ch = np.stack([e[0] for e in est])[None]
        noise = np.array([[float(e[1]) for e in est]])
        ref = Q.equalize_ref(rx[b][None], ch, noise, data_re)
        u = np.stack([ref.x_hat.real, ref.x_hat.imag]).reshape(-1) * np.sqrt(D.NORM[qm])
        margin = np.abs(u).min() if qm == 2 else np.minimum(np.abs(u), np.abs(np.abs(u) - 2.0)).min()
        print(f"{name} slot {b}: smallest distance to a decision boundary {margin:.3f} (1 = on the point)")
        assert margin > 0.5
        llr = D.llr_ref(ref.x_hat.astype(np.complex64), ref.nvar.astype(np.float32), qm)[0]
        assert np.array_equal(np.where(flip, -llr, llr) < 0, bits[b].astype(bool))


def test_no_flat_addressing_and_no_scratch_in_any_modulator_instance():
    src = CSRC / "ce_mod.hip"
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
           *_lib.EXTRA_FLAGS.get(src.name, []), "-S", "--cuda-device-only", str(src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^(_ZN12_GLOBAL__N_113ce_mod_kernelILi(\d)E\w+):\s*;.*?\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert sorted(int(q) for _, q, _ in kernels) == [2, 4, 6, 8]
    for _, qm, body in kernels:
        assert not re.search(r"\bflat_(load|store)", body), f"<{qm}> uses flat addressing"
        assert not re.search(r"\bscratch_(load|store)", body), f"<{qm}> uses scratch"
        assert not re.search(r"\batomic", body), f"<{qm}> uses atomics"
        assert re.search(r"\bglobal_load_dwordx4\b", body) and re.search(r"\bglobal_store_dwordx4\b", body)   # 16-byte loads of g, 16-byte stores of tx
        assert not re.search(r"\bglobal_store_(dword|dwordx2|dwordx3|byte|short)\b", body), f"<{qm}> has a narrower store"
        assert body.count("s_barrier") == 1
