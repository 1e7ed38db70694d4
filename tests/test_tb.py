"""CPU-side checks of the transport-block assembly extension (include/ce_tb.h): the ABI, the host derivation against the
oracle and against rate recovery's, every refusal field by field before any device call, the oracle against itself (the
bit-serial CRC against the table form, the catalogue check values, the linearity the kernel's fold rests on, segment ->
assemble_ref as a round trip, assemble_ref against its per-bit loop), the Python wrapper's argument errors, and -- from the
oracles alone -- the conditions the GPU chain test leans on.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import ldpc_oracle as O
import rm_oracle as R
import tb_oracle as T
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, ldpc as LD, ratematch as RM, transportblock as TB

NAMES = [c["name"] for c in T.CASES]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_library_exports_every_declared_tb_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies, the
    polynomials against the oracle's, and the package's re-export."""
    # LP64 sizes implied by the header: desc 4 * 4; info 4 * 4 + 8; view 18 * 4
    assert (C.sizeof(_lib.TbDesc), C.sizeof(_lib.TbInfo), C.sizeof(_lib.TbHostView)) == (16, 24, 72)
    assert (_lib.CE_TB_G24A, _lib.CE_TB_G24B, _lib.CE_TB_G16) == tuple(T.POLY[k][0] for k in ("24A", "24B", "16"))
    assert "ce_tb.hip" in _lib.SOURCES and "ce_tb.h" in _lib.REGISTRY
    assert _lib.CSRC / "ce_segment.h" in _lib.build_deps() and PKG.PuschTransportBlock is TB.PuschTransportBlock


@pytest.mark.parametrize("name", NAMES)
def test_host_view_equals_the_oracle_and_rate_recovery(lib, name):
    c, d = T.CASE_BY_NAME[name], T.case_derive(name)
    v = TB.derive_host(c["bg"], c["A"])
    assert (v.b, v.k_cb, v.c, v.b_prime, v.k_prime, v.l_tb, v.l_cb, v.p, v.g_tb, v.g_cb, v.in_row_bytes, v.tb_row_bytes) == \
        (d.B, d.K_cb, d.C, d.Bp, d.Kp, d.L_tb, d.L_cb, d.P, d.g_tb, d.g_cb, d.in_row_bytes, d.tb_row_bytes)
    rm = RM.derive_host(c["bg"], c["A"], "qpsk", 1, 8192)
    assert (v.b, v.k_cb, v.c, v.b_prime, v.k_prime) == (rm.b, rm.k_cb, rm.c, rm.b_prime, rm.k_prime)
    assert v.p * v.c == v.b == c["A"] + v.l_tb and (v.c == 1 or v.p >= 32)
    assert v.piece_dwords == -(-v.in_row_bytes // 256) <= _lib.CE_TB_MAX_PIECE and 64 * 4 * v.piece_dwords >= v.in_row_bytes
    assert v.threads == _lib.CE_TB_THREADS == 64 * v.blocks_per_workgroup
    assert v.lds_bytes in (2 * 16 * 32 * 4, 2 * 256 * 4) and v.power_bytes == 256 * (v.c + 1)
    assert v.fold_slots_per_workgroup == (v.blocks_per_workgroup if v.c > 1 else 0)
    # the decoder's row at k_out = K' is this stage's input row
    assert v.in_row_bytes == 16 * -(-v.k_prime // 128)


def test_segmentation_is_rate_recoverys_over_a_sweep(lib):
    """One function derives B, C, K' for both stages: the same integers and the same refusals, text included."""
    rng = np.random.default_rng(1)
    sizes = sorted({1, 2, 8, 3824, 3825, 8424, 8425, 1277992, 2 ** 31 - 25} | set(rng.integers(1, 1300000, 300).tolist()))
    refused = 0
    for bg in (1, 2):
        for A in sizes:
            desc, view = TB.build_desc(bg, A), _lib.TbHostView()
            rc = lib.ce_tb_derive_host(C.byref(desc), C.byref(view))
            text = _lib.last_error()
            rdesc, rview = RM.build_desc(bg, A, "qpsk", 1, 8192), _lib.RmHostView()
            rrc = lib.ce_rm_derive_host(C.byref(rdesc), C.byref(rview))
            rtext = _lib.last_error()
            if rc != 0:
                refused += 1
                assert rrc == rc == _lib.CE_ERR_INVALID and text == rtext and ("tbs=" in text or "K'" in text), (bg, A, text, rtext)
            elif rrc == 0:
                assert (view.b, view.c, view.k_prime) == (rview.b, rview.c, rview.k_prime), (bg, A)
            else:                                        # rate recovery alone refuses what concerns its own fields (G, q < C)
                assert "g_bits" in rtext, (bg, A, rtext)
    assert refused > 50


@pytest.mark.parametrize("bg,field,value,word", [(1, "abi_version", 4, "ABI"), (1, "base_graph", 0, "base_graph"), (2, "base_graph", 3, "base_graph"),
                                                 (1, "tbs", 0, "tbs"), (2, "tbs", -5, "tbs"), (1, "tbs", 8449, "tbs"), (2, "tbs", 3833, "tbs")])
def test_every_refusal_names_its_field(lib, bg, field, value, word):
    desc = TB.build_desc(bg, 8448)                        # C = 2 on BG1, C = 3 on BG2
    view, handle = _lib.TbHostView(), C.c_void_p()
    assert lib.ce_tb_derive_host(C.byref(desc), C.byref(view)) == 0 and view.c == 1 + bg
    setattr(desc, field, value)
    assert lib.ce_tb_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID
    text = _lib.last_error()
    assert word in text, text
    assert lib.ce_tb_plan_create(C.byref(desc), C.byref(handle)) == _lib.CE_ERR_INVALID and not handle.value     # before any device call
    if field == "tbs":                                    # what ce_rm_derive_host refuses is refused here, in the same words
        rdesc = RM.build_desc(desc.base_graph, value, "qpsk", 1, 8192)
        assert lib.ce_rm_derive_host(C.byref(rdesc), C.byref(_lib.RmHostView())) == _lib.CE_ERR_INVALID and _lib.last_error() == text
        with pytest.raises(ValueError):
            R.derive(desc.base_graph, value, 2, 1, 8192)


def test_null_arguments_are_refused(lib):
    assert lib.ce_tb_derive_host(None, None) == _lib.CE_ERR_INVALID and lib.ce_tb_plan_create(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_tb_plan_get_info(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_tb_assemble(None, None, 0, None, None, None, None) == _lib.CE_ERR_INVALID
    lib.ce_tb_plan_destroy(None)


# ---- the oracle against itself ----

def test_crc_check_values_and_fast_form():
    for which, want in (("24A", 0xCDE703), ("24B", 0x23EF52), ("16", 0x31C3)):
        assert T.crc_bits(T.CHECK_BITS, which) == want == T.CHECK[which] == int(T.crc_fast(T.CHECK_BITS, which))
    assert T.POLY == {"24A": (0x864CFB, 24), "24B": (0x800063, 24), "16": (0x1021, 16)}
    rng = np.random.default_rng(2)
    for n in list(range(1, 301)):
        bits = rng.integers(0, 2, (2, n)).astype(np.uint8)
        for which in T.POLY:
            fast = T.crc_fast(bits, which)
            assert [T.crc_bits(b, which) for b in bits] == fast.tolist(), (n, which)
    # a string that carries its own CRC has residue 0
    bits = rng.integers(0, 2, 77).astype(np.uint8)
    for which, (_, L) in T.POLY.items():
        assert T.crc_bits(np.concatenate([bits, T._to_bits(T.crc_bits(bits, which), L)]), which) == 0


@pytest.mark.parametrize("name", NAMES)
def test_linearity_and_round_trip(name):
    """XOR of the t_r is the CRC of the whole stream, on random rows and on valid ones; segment -> assemble_ref returns the
    bits sent, the padding 0 and every residue 0."""
    d = T.case_derive(name)
    tb_bits, valid, rand = T.inputs(name)
    for kind in ("valid", "random"):
        tb, status, cb = T.reference(name, kind)
        assert tb.shape == (len(tb_bits), d.tb_row_bytes) and status.shape == (len(tb_bits), 2) and cb.shape == (len(tb_bits), d.C, 2)
        assert np.array_equal(np.bitwise_xor.reduce(cb[..., 1], axis=1), status[:, 0]), (name, kind)
        assert np.array_equal(status[:, 1], (cb[..., 0] != 0).sum(1))
        assert not np.unpackbits(tb, axis=-1)[:, d.A:].any()
    tb, status, cb = T.reference(name, "valid")
    assert np.array_equal(np.unpackbits(tb, axis=-1)[:, :d.A], tb_bits) and not status.any() and not cb[..., 0].any()
    assert np.array_equal(LD.unpack_bits(tb, d.A), tb_bits)
    _, status, cb = T.reference(name, "random")
    assert status[:, 0].all() and np.all(status[:, 1] == d.C)          # random rows fail everywhere
    assert np.unpackbits(rand, axis=-1)[..., d.Kp:].any() or d.Kp % 128 == 0     # and hold bits behind K'


@pytest.mark.parametrize("name", T.SMALL_CASES)
def test_assemble_ref_equals_the_per_bit_loop(name):
    d = T.case_derive(name)
    _, valid, rand = T.inputs(name)
    for rows, kind in ((valid, "valid"), (rand, "random")):
        for got, want in zip(T.assemble_loop(rows, d), T.reference(name, kind)):
            assert np.array_equal(got, want), (name, kind)


@pytest.mark.parametrize("name", T.CORRUPTION_CASES)
def test_corruptions_have_the_stated_properties(name):
    d = T.case_derive(name)
    _, valid, _ = T.inputs(name)
    for s in T.boundary_bits(d):
        r, i = divmod(s, d.P)
        _, status, cb = T.assemble_ref(T.flip(valid, 1, r, i), d)
        bad = cb[1, :, 0] != 0
        assert bad[r] and bad.sum() == 1 and status[1].tolist()[1] == 1 and status[1, 0] != 0 and not status[[0, 2]].any(), (name, s)
        if d.C > 1:
            _, status, cb = T.assemble_ref(T.refresh_cb_crc(T.flip(valid, 1, r, i), d, 1, r), d)
            assert not cb[..., 0].any() and status[1, 0] != 0 and status[1, 1] == 0, (name, s)
    for r in range(d.C if d.C > 1 else 0):
        for i in (d.P, d.Kp - 1):
            _, status, cb = T.assemble_ref(T.flip(valid, 0, r, i), d)
            assert cb[0, r, 0] != 0 and status[0].tolist() == [0, 1], (name, r, i)


# ---- the Python wrapper ----

def test_python_wrapper_without_a_device():
    with pytest.raises(ValueError, match="base_graph"):
        TB.PuschTransportBlock(3, 24)
    with pytest.raises(ValueError, match="tbs"):
        TB.PuschTransportBlock(1, 0)
    with pytest.raises(ValueError, match="no multiple"):
        TB.PuschTransportBlock(1, 8449)
    asm = TB.PuschTransportBlock(1, 8448)
    assert (asm.c, asm.k_prime, asm.payload_bits, asm.in_row_bytes, asm.tb_row_bytes, asm.device) == (2, 4260, 4236, 544, 1056, None)
    rm = RM.PuschRateRecovery(2, 24, "qpsk", 1, 480)
    one = TB.PuschTransportBlock.for_rate_recovery(rm)
    assert (one.base_graph, one.tbs, one.c, one.k_prime, one.payload_bits, one.in_row_bytes, one.tb_row_bytes) == (2, 24, 1, 40, 40, 16, 16)
    for bad, stage in ((torch.zeros((3, 2, 544), dtype=torch.int8), asm), (torch.zeros((3, 2, 543), dtype=torch.uint8), asm),
                       (torch.zeros((3, 544), dtype=torch.uint8), asm), (torch.zeros((3, 1, 544), dtype=torch.uint8), asm),
                       (torch.zeros((3, 2, 1088), dtype=torch.uint8)[:, :, ::2], asm), (np.zeros((3, 2, 544), np.uint8), asm),
                       (torch.zeros((3, 2, 16), dtype=torch.uint8), one), (torch.zeros((16,), dtype=torch.uint8), one)):
        with pytest.raises(ValueError, match=r"\[slots, (2, 544|1, 16)\]"):
            stage(bad)


# ---- the conditions the GPU chain test leans on, from the oracles alone ----

@pytest.mark.parametrize("which", sorted(O.CHAINS))
def test_chain_reference_decodes_every_block_to_the_bits_sent(which):
    x = T.chain_inputs(which)
    d, t, g = x.d, x.t, x.g
    assert T.CHAIN_ESN0_DB == O.ESN0_DB == 1.0                       # the existing chain's Es/N0 suffices: nothing was raised
    ch = O.channel(O.quantise(x.soft.reshape(-1, d.N_cb)), g.n_cols, g.zc, 2)
    L, status, _ = O.decode_ref(g.rows, g.n_cols, g.zc, ch, 8, True)
    assert np.all(status[:, 1] == 1), status.tolist()
    assert np.array_equal((L[:, :d.Kp] < 0).reshape(x.blocks.shape), x.blocks == 1)
    assert x.llr.dtype == np.int8 and x.llr.shape == (O.CHAIN_SLOTS, d.G)
    tb, tb_status, cb = T.assemble_ref(O.pack(L, d.Kp).reshape(O.CHAIN_SLOTS, d.C, -1), t)
    assert np.array_equal(LD.unpack_bits(tb, t.A), x.tb_bits) and not tb_status.any() and not cb[..., 0].any()
    # the last slot's LLR row negated: whatever the decoder makes of it fails the transport-block CRC, the other slot holds
    ch = O.channel(O.quantise(x.soft_neg.reshape(-1, d.N_cb)), g.n_cols, g.zc, 2)
    L, _, _ = O.decode_ref(g.rows, g.n_cols, g.zc, ch, 8, True)
    _, tb_status, _ = T.assemble_ref(O.pack(L, d.Kp).reshape(O.CHAIN_SLOTS, d.C, -1), t)
    assert tb_status[-1, 0] != 0 and not tb_status[:-1].any(), tb_status.tolist()
