"""CPU-side checks of the DM-RS generation extension (include/ce_dmrs.h): the ABI, the bit-serial oracle against the
anchors the operator was specified with, the library's host derivation (jump tables + pilot lists, combined here exactly
as the kernel combines them) against that oracle bit for bit, descriptor / parameter errors, and the OCC / CDM
conventions against the estimator's CPU oracle.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ce_oracle as O
import dmrs_oracle as D
from dmrs_oracle import CASE_A, CASE_B, CASE_C, T1, T2
from srsran_ce_pytorch_amd import _lib, dmrs, synth as S

ANCHOR_HASH = {"A": ((18, 2, 1), "d82ca518f1c74f67"), "B": ((18, 4, 4), "bb224eab249c29f3"), "C": ((28, 1, 3), "3ffe9a508323217a")}
CASES = [   # (case, slot, n_id, n_scid, n_symb_slot, grid_start_crb)
    CASE_A, CASE_B, CASE_C,
    (S.case_spec("prb0", 273, [S.hop_spec([2, 11], 0, 1)], n_layers=2), 3, 10, 0, 14, 0),                      # first table word
    (S.case_spec("prb272", 273, [S.hop_spec([2, 11], 272, 1, re_masks=T1)], n_layers=3), 11, 999, 1, 14, 0),   # last table word
    (S.case_spec("scattered", 106, [S.hop_spec([2, 7], 4, 6, re_masks=T1, mask_prbs=[4, 5, 9, 40, 41, 105]),
                                    S.hop_spec([11], 0, 6, re_masks=T1, mask_prbs=[0, 1, 2, 50, 77, 78])], n_layers=4), 17, 513, 1, 14, 3),
    (S.case_spec("crb2000", 52, [S.hop_spec([3, 10], 7, 9, re_masks=T2)], n_layers=2), 79, 65535, 0, 14, 2000),
    (S.case_spec("sym12", 24, [S.hop_spec([2, 9], 2, 5)], n_layers=1, n_sym=12), 39, 77, 1, 12, 0),
]
IDS = [c[0]["name"] for c in CASES]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_every_declared_dmrs_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies."""
    assert "ce_dmrs.h" in _lib.REGISTRY and "ce_dmrs.hip" in _lib.SOURCES
    # LP64 sizes implied by the header: hop 14 + 2*2 (+6 pad) + 8 = 32; desc 8*4 + 2*32 = 96; info 4 + 4 + 8 = 16
    assert (C.sizeof(_lib.DmrsHopDesc), C.sizeof(_lib.DmrsDesc), C.sizeof(_lib.DmrsInfo)) == (32, 96, 16)
    # view: 4*4 + 2*14*4 + 2*2*4 + 2*136*4 (x1) + 2*31*136*4 (t) + 2*2048*4 (m) + 2*2048 (odd_sign)
    assert C.sizeof(_lib.DmrsHostView) == 16 + 112 + 16 + 1088 + 33728 + 16384 + 4096


def test_oracle_reproduces_the_gold_anchors():
    for ci, words in ((0, (0x5e485840, 0x6ac0a9a4)), (1, (0x2ec0c140, 0x47bf59d4)), (123456789, (0x971e2597, 0x5981a05d)),
                      (123863060, (0xe54f4a9b, 0xb5527709)), (1854013439, (0xf050eb3b, 0x9968419f))):
        assert tuple(D.gold_words(ci, 2)) == words, ci
    assert D.c_init(14, 3, 2, 10, 0) == 123863060 and D.c_init(14, 159, 13, 65535, 1) == 1854013439


def test_oracle_reproduces_the_pilot_anchors():
    a = float(D.A)
    ref = {}
    for case, slot, n_id, n_scid, nss, crb in (CASE_A, CASE_B, CASE_C):
        p = D.pilots_ref(case, slot, n_id, n_scid, nss, crb)
        assert (p.shape, D.sha16(p)) == ANCHOR_HASH[case["name"]], case["name"]
        ref[case["name"]] = p
    c = lambda re, im: np.complex64(complex(re * a, im * a))    # noqa: E731
    assert list(ref["A"][:3, 0, 0]) == [c(1, 1), c(-1, 1), c(1, 1)] and ref["A"][-1, 1, 0] == c(1, -1)
    assert list(ref["B"][0, 0]) == [c(1, 1)] * 4 and list(ref["B"][1, 0]) == [c(-1, -1), c(1, 1), c(-1, -1), c(1, 1)]


def kernel_combination(view, n_layers, slot, n_id, n_scid, n_symb_slot):
    """The kernel's arithmetic on the host view, in uint32: c_init, XOR of the table rows its set bits select, two bits
    per pilot, sign flips of float32 0x3f3504f3."""
    u = np.uint32
    n_re, n_cols = view.n_re, view.n_dmrs_total
    out = np.zeros((n_re, n_cols, n_layers, 2), np.uint32)
    with np.errstate(over="ignore"):
        for col in range(n_cols):
            h, sym = view.col_hop[col], view.col_sym[col]
            ci = int(((u(n_symb_slot) * u(slot) + u(sym + 1)) * (u(2) * u(n_id) + u(1))) << u(17)) & 0xFFFFFFFF
            ci = (ci + 2 * n_id + n_scid) & 0x7FFFFFFF
            nw = view.n_words[h]
            words = np.array(view.x1[h][:nw], np.uint32)
            for i in range(31):
                if ci >> i & 1:
                    words ^= np.array(view.t[h][i][:nw], np.uint32)
            m = np.array(view.m[h][:n_re], np.int64)
            assert np.array_equal(np.array(view.odd_sign[h][:n_re]), m & 1)
            br = 2 * m - 32 * view.word0[h]
            assert br.min() >= 0 and (br >> 5).max() < nw
            two = words[br >> 5] >> (br & 31).astype(np.uint32)
            for l in range(n_layers):
                flip = (m & 1).astype(np.uint32) if l % 2 else u(0)
                out[:, col, l, 0] = u(0x3F3504F3) ^ (((two ^ flip) & u(1)) << u(31))
                out[:, col, l, 1] = u(0x3F3504F3) ^ ((((two >> u(1)) ^ flip) & u(1)) << u(31))
    return out.view(np.float32).view(np.complex64)[..., 0]


@pytest.mark.parametrize("case,slot,n_id,n_scid,nss,crb", CASES, ids=IDS)
def test_host_tables_and_pilot_lists_reproduce_the_oracle(lib, case, slot, n_id, n_scid, nss, crb):
    h1, h2, _ = S.numpy_hops(case)
    view = dmrs.derive_host(h1, h2, case["n_layers"], case["n_prb_grid"], case["n_sym"], grid_start_crb=crb, n_symb_slot=nss)
    ref = D.pilots_ref(case, slot, n_id, n_scid, nss, crb)
    assert (view.n_re, view.n_dmrs_total) == ref.shape[:2]
    got = kernel_combination(view, case["n_layers"], slot, n_id, n_scid, nss)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    # X1 = c for c_init 0, T[i] = c for c_init 1 << i XOR X1, at the hop's first kept word
    w0 = view.word0[0]
    if w0 < 40:
        assert view.x1[0][0] == D.gold_words(0, w0 + 1)[w0]
        assert view.t[0][5][0] == D.gold_words(32, w0 + 1)[w0] ^ view.x1[0][0]


def test_full_band_hop_keeps_104_words(lib):
    h1, h2, _ = S.numpy_hops(S.bench_case("filter"))
    view = dmrs.derive_host(h1, h2, 1, 273, 14)
    assert (view.n_re, view.n_dmrs_total, view.ppp, view.word0[0], view.n_words[0]) == (1638, 2, 6, 0, 103)
    view = dmrs.derive_host(h1, h2, 1, 273, 14, grid_start_crb=1)       # 12 bits in: the window straddles one more word
    assert view.n_words[0] == 103 and view.word0[0] == 0
    view = dmrs.derive_host(h1, h2, 1, 273, 14, grid_start_crb=5)       # bits 60 .. 3335
    assert (view.word0[0], view.n_words[0]) == (1, 104)


def test_descriptor_errors(lib):
    good = S.case_spec("g", 52, [S.hop_spec([2, 11], 4, 6, re_masks=T1)], n_layers=2)
    h1, h2, _ = S.numpy_hops(good)
    dmrs.derive_host(h1, h2, 2, 52, 14)
    bad = S.numpy_hops(good)[0]
    bad.DMRSREmask = np.array([[1, 0, 0] * 4], bool).T                       # 0x249: every third RE
    with pytest.raises(ValueError, match="0x249"):
        dmrs.derive_host(bad, h2, 1, 52, 14)
    mixed = S.numpy_hops(good)[0]
    mixed.DMRSREmask = np.array([S.TYPE1_CDM0, S.TYPE2_CDM1], bool).T
    with pytest.raises(ValueError, match="configuration types"):
        dmrs.derive_host(mixed, h2, 3, 52, 14)
    two = S.case_spec("t", 52, [S.hop_spec([2], 4, 6), S.hop_spec([11], 20, 5)])
    a, b, _ = S.numpy_hops(two)
    with pytest.raises(ValueError, match="active PRBs"):
        dmrs.derive_host(a, b, 1, 52, 14)
    with pytest.raises(NotImplementedError, match="n_layers=5"):
        dmrs.derive_host(h1, h2, 5, 52, 14)
    with pytest.raises(ValueError, match="grid_start_crb"):
        dmrs.derive_host(h1, h2, 2, 52, 14, grid_start_crb=-1)
    with pytest.raises(NotImplementedError, match="grid_start_crb"):
        dmrs.derive_host(h1, h2, 2, 52, 14, grid_start_crb=(1 << 20) // 6 - 51)
    with pytest.raises(ValueError, match="n_symb_slot"):
        dmrs.derive_host(h1, h2, 2, 52, 14, n_symb_slot=13)
    with pytest.raises(ValueError, match="n_sym=14"):
        dmrs.derive_host(h1, h2, 2, 52, 14, n_symb_slot=12)
    with pytest.raises(NotImplementedError, match="grid of 342 PRB"):
        big = S.case_spec("b", 342, [S.hop_spec([2], 0, 1)])
        dmrs.derive_host(*S.numpy_hops(big)[:2], 1, 342, 14)
    desc, keep = dmrs.build_desc(h1, h2, 2, 52, 14)
    view = _lib.DmrsHostView()
    assert lib.ce_dmrs_derive_host(C.byref(desc), C.byref(view)) == 0
    desc.abi_version = _lib.CE_ABI_VERSION + 1
    handle = C.c_void_p()
    assert lib.ce_dmrs_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID and b"ABI" in lib.ce_last_error()
    assert lib.ce_dmrs_plan_create(C.byref(desc), C.byref(handle)) == _lib.CE_ERR_INVALID and not handle.value   # before any device call
    del keep


def test_host_parameters_are_range_checked_before_any_device_use(lib):
    h1, h2, _ = S.numpy_hops(CASE_A[0])
    gen = dmrs.PuschDmrs(h1, h2, 1, 273)
    assert (gen.n_re, gen.n_dmrs_total) == (18, 2)
    for args in ((0, 65536, 0), (0, 0, 2), (-1, 0, 0), (np.array([3, -2]), 0, 0), (0, np.array([1, 70000]), 0), (0, 0, 1.0)):
        with pytest.raises(ValueError):
            gen(*args)
    with pytest.raises(ValueError, match="broadcast"):
        gen(np.arange(3), np.arange(2), 0)


def test_conventions_are_the_ones_the_estimator_despreads(lib):
    """Case B through the estimator's CPU oracle: a noiseless grid built from the generated pilots with flat per-layer
    gains must come back as those gains -- the OCC sign and the layer -> CDM column mapping are what the de-spread expects."""
    case, slot, n_id, n_scid, nss, crb = CASE_B
    pil = D.pilots_ref(case, slot, n_id, n_scid, nss, crb)
    gains = np.array([1, 0.5j, -0.7, 0.3 - 0.4j])
    h1, h2, cfg = S.numpy_hops(case)
    cfg.Smoothing, cfg.CFOCompensate = "none", False
    grid = np.zeros((12 * 52, 14), np.complex64)
    col = 0
    for syms, mp, rm in D.hops_of(case):
        for sym in syms:
            for l in range(4):
                res = np.flatnonzero(np.kron(mp, rm[:, l // 2]))
                grid[res, sym] += (gains[l] * pil[:, col, l]).astype(np.complex64)
            col += 1
    ch, noise, *_ = O.srs_channel_estimator(grid, pil, 1.0, h1, h2, cfg)
    for band in (slice(36, 72), slice(336, 372)):
        assert np.abs(ch[band] - gains[None, None, :]).max() <= 1e-6
    assert noise < 1e-10
