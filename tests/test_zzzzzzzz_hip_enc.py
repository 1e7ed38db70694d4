"""GPU tests of the transport-block encoder extension (include/ce_enc.h): `g` and `cw` against tests/enc_oracle.py by value
(np.array_equal -- everything is bits) on the pinned cases: Zc = 2, 6, 7, 15, 36, 72, 104, 176, 208, 352, 384; C = 1, 2, 5, 9
with equal and unequal E_r, a transport block of three CRC chunks, blocks meeting inside a dword of g and at a dword boundary; CRC16 and CRC24A either side of
A = 3824; K_b = 6, 8, 9, 10 (filler columns); G < N_cb and G > 2 N_cb; a limited buffer, rv 1 starting inside the fillers;
all four rv per slot and for a batch; both NR-core variants, three equal shifts, a triangular core, a truncated graph;
garbage behind bit A; guard regions; 8192 slots; an empty batch; a second stream; argument errors; and the loop on the device
encoder -> LLRs -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock.  What the loop leans on is asserted from the
oracles alone in tests/test_enc.py.

The file's name sorts it behind test_zzzzzzz_hip_tb.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import enc_oracle as E
import tb_oracle as T
from srsran_ce_pytorch_amd import _lib, encoder as EN, ldpc as LD, ratematch as RM, transportblock as TB

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _enc(name):
    c, g = E.CASE_BY_NAME[name], E.graph(name)
    return EN.PuschTransportEncoder(c["bg"], c["A"], c["qm"], c["L"], c["G"], LD.LdpcGraph(g.rows, g.n_cols), n_ref=c["n_ref"], device=_dev())


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("name", E.NAMES)
def test_g_and_the_codeword_equal_the_oracle(name):
    d, enc = E.case_derive(name), _enc(name)
    _, tb_rows = E.inputs(name)
    g_ref, cw_ref = E.reference(name, 0)
    rv = _t(E.rvs_of(name, 0), torch.int32)
    g, cw = enc(_t(tb_rows), rv=rv, return_codeword=True)
    alone = enc(_t(tb_rows), rv=rv)                        # without the codeword: only the rows the buffer reaches are computed
    torch.cuda.synchronize()
    _same(cw.cpu().numpy(), cw_ref, (name, "cw"))
    _same(g.cpu().numpy(), g_ref, (name, "g"))
    _same(alone.cpu().numpy(), g_ref, (name, "g without cw"))
    assert not np.unpackbits(g.cpu().numpy(), axis=-1)[:, d.G:].any()
    assert np.array_equal(LD.unpack_bits(g, enc.n_bits).numpy(), LD.unpack_bits(g_ref, d.G))


@pytest.mark.parametrize("name", ["bg2_z7_rep", "bg1_z6_k0_in_filler", "bg1_z15_rows12", "bg1_z208_lbrm", "bg2_z352_c5", "bg2_z208_c2_aligned"])
def test_every_rv_per_slot_and_for_a_batch(name):
    d, enc = E.case_derive(name), _enc(name)
    tb_bits, tb_rows = E.inputs(name)
    tb = _t(tb_rows)
    for shift in (1, 2, 3):
        g = enc(tb, rv=_t(E.rvs_of(name, shift), torch.int32))
        _same(g.cpu().numpy(), E.reference(name, shift)[0], (name, shift))
    wide = _t([4 * b + r for b, r in enumerate(E.rvs_of(name, 1))], torch.int32)     # only rv & 3 is used
    _same(enc(tb, rv=wide).cpu().numpy(), E.reference(name, 1)[0], (name, "rv & 3"))
    bits, _ = E.transmit(d, E.graph(name), tb_bits, [2] * len(tb_bits))
    _same(enc(tb, rv=2).cpu().numpy(), T.pack(bits, enc.g_row_bytes), (name, "rv=2 for the batch"))


@pytest.mark.parametrize("name", ["bg1_z2", "bg1_z15", "bg2_z208_c2", "bg1_z384"])
def test_bits_behind_a_are_ignored(name):
    d, enc = E.case_derive(name), _enc(name)
    tb_bits, tb_rows = E.inputs(name)
    clean = T.pack(tb_bits, enc.tb_row_bytes)
    assert d.A % 128 == 0 or (clean != tb_rows).any()
    a, b = enc(_t(clean), rv=0, return_codeword=True), enc(_t(tb_rows), rv=0, return_codeword=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), name


@pytest.mark.parametrize("name", ["bg2_z7_rep", "bg2_z352_c5", "bg2_z208_c2_aligned"])
def test_guard_regions_round_g_and_cw(name):
    d, enc = E.case_derive(name), _enc(name)
    _, tb_rows = E.inputs(name)
    g_ref, cw_ref = E.reference(name, 0)
    enc._plan()
    S, guard = tb_rows.shape[0], 64
    sizes = (S * enc.g_row_bytes, S * d.C * enc.cw_row_bytes)
    bufs = [torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=_dev()) for n in sizes]
    src, rv = _t(tb_rows), _t(E.rvs_of(name, 0), torch.int32)
    ptr = [C.c_void_p(b.data_ptr() + guard) for b in bufs]
    assert all(p.value % 16 == 0 for p in ptr)
    enc._launch(C.c_void_p(src.data_ptr()), C.c_void_p(rv.data_ptr()), 1, S, *ptr)
    torch.cuda.synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for r, n in zip(raw, sizes):
        assert np.all(r[:guard] == 0xA5) and np.all(r[guard + n:] == 0xA5)
    _same(raw[0][guard:guard + sizes[0]].reshape(S, -1), g_ref, (name, "g"))
    _same(raw[1][guard:guard + sizes[1]].reshape(S, d.C, -1), cw_ref, (name, "cw"))
    assert np.array_equal(src.cpu().numpy(), tb_rows)                 # the input is read only
    if not enc.needs_codeword:                                        # one launch, no codeword: g alone, its guards intact
        buf = torch.full((guard + sizes[0] + guard,), 0xA5, dtype=torch.uint8, device=_dev())
        enc._launch(C.c_void_p(src.data_ptr()), C.c_void_p(rv.data_ptr()), 1, S, C.c_void_p(buf.data_ptr() + guard), None)
        torch.cuda.synchronize()
        r = buf.cpu().numpy()
        assert np.all(r[:guard] == 0xA5) and np.all(r[guard + sizes[0]:] == 0xA5)
        _same(r[guard:guard + sizes[0]].reshape(S, -1), g_ref, (name, "g alone"))


def test_more_workgroups_than_the_chip_holds_at_once():
    """The tiny case at 8192 slots, one workgroup each, every slot its own transport block and rv."""
    name, S = "bg2_z7_rep", 8192
    d, enc = E.case_derive(name), _enc(name)
    assert S > 8 * torch.cuda.get_device_properties(_dev()).multi_processor_count
    rng = np.random.default_rng(6)
    tb_bits = rng.integers(0, 2, (S, d.A)).astype(np.uint8)
    rvs = rng.integers(0, 4, S)
    bits, cw_bits = E.transmit(d, E.graph(name), tb_bits, rvs)
    g, cw = enc(_t(T.pack(tb_bits, enc.tb_row_bytes)), rv=_t(rvs, torch.int32), return_codeword=True)
    _same(g.cpu().numpy(), T.pack(bits, enc.g_row_bytes), "8192 slots: g")
    _same(cw.cpu().numpy(), T.pack(cw_bits, enc.cw_row_bytes), "8192 slots: cw")


def test_empty_batch_and_argument_errors():
    name = "bg2_z208_c2"
    d, enc = E.case_derive(name), _enc(name)
    g, cw = enc(torch.empty((0, enc.tb_row_bytes), dtype=torch.uint8, device=_dev()), rv=0, return_codeword=True)
    assert tuple(g.shape) == (0, enc.g_row_bytes) and tuple(cw.shape) == (0, 2, enc.cw_row_bytes)
    good = _t(E.inputs(name)[1])
    flat = torch.zeros(good.numel() + 16, dtype=torch.uint8, device=_dev())
    off = flat[1:1 + good.numel()].view(good.shape)       # dense, one byte off the 16-byte grid
    assert off.is_contiguous() and off.data_ptr() % 16 == 1
    wide = torch.zeros((2, 2 * enc.tb_row_bytes), dtype=torch.uint8, device=_dev())[:, ::2]
    for bad in (good.to(torch.int8), good.float(), good[:, :-1], good[0], good[:, None], good.cpu(), wide, off, "x"):
        with pytest.raises(ValueError):
            enc(bad)
    for bad_rv in (4, -1, 1.0, True, torch.zeros(2, dtype=torch.int64, device=_dev()), torch.zeros(3, dtype=torch.int32, device=_dev()),
                   torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="rv"):
            enc(good, rv=bad_rv)
    lib, h = enc._lib, enc._handle
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=_dev())
    rv = torch.zeros(2, dtype=torch.int32, device=_dev())
    p = buf.data_ptr()
    assert p % 16 == 0 and enc.needs_codeword
    args = [C.c_void_p(good.data_ptr()), C.c_void_p(rv.data_ptr()), 1, 2, C.c_void_p(p), C.c_void_p(p + 16384)]
    for i in (0, 4, 5):
        bad = list(args)
        bad[i] = C.c_void_p(bad[i].value + 4)
        assert lib.ce_enc_encode(h, *bad, None) == _lib.CE_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert lib.ce_enc_encode(h, *args[:3], -1, *args[4:], None) == _lib.CE_ERR_INVALID and "n_slots" in _lib.last_error()
    assert lib.ce_enc_encode(h, *args[:2], -1, *args[3:], None) == _lib.CE_ERR_INVALID and "strides" in _lib.last_error()
    assert lib.ce_enc_encode(h, None, *args[1:], None) == _lib.CE_ERR_INVALID
    assert lib.ce_enc_encode(h, *args[:5], None, None) == _lib.CE_ERR_INVALID and "cw must be given" in _lib.last_error()
    assert lib.ce_enc_encode(h, None, None, 0, 0, None, None, None) == 0            # n_slots == 0 launches nothing
    info = _lib.EncInfo()
    assert lib.ce_enc_plan_get_info(h, C.byref(info)) == 0
    assert (info.n_code_blocks, info.tb_row_bytes, info.g_row_bytes, info.cw_row_bytes, info.cw_required, info.bytes_per_slot) == \
        (2, 496, 1504, 1360, 1, 496 + 1504)
    torch.cuda.synchronize()


def test_a_non_default_stream_gives_the_same_result():
    name = "bg1_z208_c2"
    enc = _enc(name)
    tb, rv = _t(E.inputs(name)[1]), _t(E.rvs_of(name, 0), torch.int32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        g, cw = enc(tb, rv=rv, return_codeword=True)
    side.synchronize()
    g_ref, cw_ref = E.reference(name, 0)
    _same(g.cpu().numpy(), g_ref, "side stream: g")
    _same(cw.cpu().numpy(), cw_ref, "side stream: cw")


def _llr(g, n_bits, negate_slot=None):
    """+-64 int8 LLRs of the packed bit rows g, on the device: bit 0 -> +64, bit 1 -> -64."""
    shifts = torch.arange(7, -1, -1, device=g.device, dtype=torch.int16)
    bits = ((g.to(torch.int16).unsqueeze(-1) >> shifts) & 1).reshape(g.shape[0], -1)[:, :n_bits]
    llr = (64 - 128 * bits).to(torch.int8)
    if negate_slot is not None:
        llr[negate_slot] = -llr[negate_slot]
    return llr.contiguous()


@pytest.mark.parametrize("name", sorted(E.LOOPS))
def test_the_loop_on_the_device_returns_the_transport_block(name):
    """PuschTransportEncoder -> +-64 LLRs -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock: the block sent and
    residue 0 for rv 0, for rv 0 then rv 2 combined in place, and for a block with one payload bit flipped before encoding;
    a slot whose LLRs are negated fails its CRC."""
    c, d, gr = E.CASE_BY_NAME[name], E.case_derive(name), E.graph(name)
    graph = LD.LdpcGraph(gr.rows, gr.n_cols)
    rm = RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], device=_dev())
    enc = EN.PuschTransportEncoder.for_rate_recovery(rm, graph)
    dec = LD.PuschLdpcDecoder.for_rate_recovery(rm, graph)
    asm = TB.PuschTransportBlock.for_rate_recovery(rm)
    assert (enc.n_code_blocks, enc.n_cb, enc.zc, enc.tb_row_bytes) == (rm.n_code_blocks, rm.n_cb, rm.zc, asm.tb_row_bytes)
    tb_bits = np.array(E.inputs(name)[0])
    tb_bits[1, d.A // 2] ^= 1                                          # slot 1: a flipped payload bit is a valid block too
    sent = T.pack(tb_bits, enc.tb_row_bytes)
    tb = _t(sent)

    def receive(soft):
        hard, status = dec(soft)
        out, tb_status, cb_status = asm(hard)
        torch.cuda.synchronize()
        return out.cpu().numpy(), tb_status.cpu().numpy(), status.cpu().numpy()

    soft = rm(_llr(enc(tb, rv=0), enc.n_bits), rv=0)
    out, tb_status, status = receive(soft)
    assert np.array_equal(out, sent) and not tb_status.any() and (status[..., 1] == 1).all(), (name, tb_status.tolist())
    soft = rm(_llr(enc(tb, rv=2), enc.n_bits), rv=2, harq=soft, out=soft)          # rv 2 combined in place
    out, tb_status, _ = receive(soft)
    assert np.array_equal(out, sent) and not tb_status.any(), (name, "rv 0 + rv 2", tb_status.tolist())
    out, tb_status, _ = receive(rm(_llr(enc(tb, rv=0), enc.n_bits, negate_slot=0), rv=0))
    assert tb_status[0, 0] != 0 and not tb_status[1:].any() and np.array_equal(out[1:], sent[1:]), (name, "negated", tb_status.tolist())
