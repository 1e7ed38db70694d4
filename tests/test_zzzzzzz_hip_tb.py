"""GPU tests of the transport-block assembly extension (include/ce_tb.h): the kernels against the integer oracle of
tests/tb_oracle.py, by value (np.array_equal on tb, tb_status and cb_status -- no tolerance), on the pinned cases: one
partly filled chunk, sizes that are no multiple of 8, the last CRC16 and the first CRC24A size, 66 chunks (two per lane),
block boundaries at bit and at byte offsets into a dword, five blocks with every boundary at another offset, the largest
NR transport block (152 blocks), and three and four dwords per lane in one block and in each of two.  The conditions the chain test leans on are asserted from the oracles alone in
tests/test_tb.py.

The file's name sorts it behind test_zzzzzz_hip_ldpc.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import ldpc_oracle as O
import tb_oracle as T
from srsran_ce_pytorch_amd import _lib, ldpc as LD, ratematch as RM, transportblock as TB

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in T.CASES]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())      # a copy: the shared inputs are read-only


def _asm(name):
    c = T.CASE_BY_NAME[name]
    return T.case_derive(name), TB.PuschTransportBlock(c["bg"], c["A"], device=_dev())


def _run(asm, rows):
    out = asm(_t(rows) if isinstance(rows, np.ndarray) else rows)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _same(got, ref, what=""):
    tb, status, cb = got
    assert tb.dtype == np.uint8 and status.dtype == np.int32 and cb.dtype == np.int32
    assert tb.shape == ref[0].shape and status.shape == ref[1].shape and cb.shape == ref[2].shape, what
    assert np.array_equal(cb, ref[2]), (what, np.argwhere(cb != ref[2])[:4].tolist())
    assert np.array_equal(status, ref[1]), (what, status.tolist()[:4], ref[1].tolist()[:4])
    assert np.array_equal(tb, ref[0]), (what, np.argwhere(tb != ref[0])[:4].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_valid_blocks_give_the_bytes_sent(name):
    d, asm = _asm(name)
    tb_bits, valid, _ = T.inputs(name)
    got = _run(asm, valid)
    _same(got, T.reference(name, "valid"), name)
    tb, status, cb = got
    assert np.array_equal(tb, T.pack(tb_bits, d.tb_row_bytes)) and np.array_equal(LD.unpack_bits(tb, d.A), tb_bits)
    assert not np.unpackbits(tb, axis=-1)[:, d.A:].any() and not status.any() and not cb[..., 0].any()


@pytest.mark.parametrize("name", NAMES)
def test_random_rows_against_the_oracle(name):
    d, asm = _asm(name)
    _, _, rand = T.inputs(name)
    got = _run(asm, rand)
    _same(got, T.reference(name, "random"), name)
    assert got[1][:, 0].all() and np.all(got[1][:, 1] == d.C)
    if d.C == 1:                                          # [B, in_row_bytes] is accepted when C = 1
        assert all(np.array_equal(a, b) for a, b in zip(_run(asm, rand[:, 0]), got))


@pytest.mark.parametrize("name", T.CORRUPTION_CASES)
def test_corruptions_equal_the_oracle_and_have_the_stated_property(name):
    d, asm = _asm(name)
    _, valid, _ = T.inputs(name)
    for s in T.boundary_bits(d):                          # the first bit, the last, and either side of every block boundary
        r, i = divmod(s, d.P)
        rows = T.flip(valid, 1, r, i)                     # a payload bit: block r fails alone, and so does the transport block
        got = _run(asm, rows)
        _same(got, T.assemble_ref(rows, d), (name, s))
        bad = got[2][1, :, 0] != 0
        assert bad[r] and bad.sum() == 1 and got[1][1, 0] != 0 and got[1][1, 1] == 1 and not got[1][[0, 2]].any(), (name, s)
        if d.C > 1:                                       # the same with the block's CRC24B recomputed: only the transport block fails
            rows = T.refresh_cb_crc(rows, d, 1, r)
            got = _run(asm, rows)
            _same(got, T.assemble_ref(rows, d), (name, s, "crc24b recomputed"))
            assert not got[2][..., 0].any() and got[1][1, 0] != 0 and got[1][1, 1] == 0 and not got[1][[0, 2]].any(), (name, s)
    for r in range(d.C if d.C > 1 else 0):                # inside the CRC24B field: the block fails, the transport block holds
        for i in (d.P, d.Kp - 1):
            rows = T.flip(valid, 0, r, i)
            got = _run(asm, rows)
            _same(got, T.assemble_ref(rows, d), (name, r, i))
            assert got[2][0, r, 0] != 0 and got[1][0].tolist() == [0, 1] and np.array_equal(got[0], T.reference(name, "valid")[0]), (name, r, i)


@pytest.mark.parametrize("name", [n for n in NAMES if T.case_derive(n).Kp % 128])      # c1_crc16_top and c1_max fill their rows
def test_bits_behind_k_prime_are_ignored(name):
    d, asm = _asm(name)
    _, valid, rand = T.inputs(name)
    keep = np.unpackbits(np.zeros(d.in_row_bytes, np.uint8))
    keep[:d.Kp] = 1
    keep = np.packbits(keep)
    rng = np.random.default_rng(4)
    for rows in (valid, rand):
        zeros = rows & keep
        noise = zeros | (rng.integers(0, 256, rows.shape).astype(np.uint8) & ~keep)
        assert (noise != zeros).any()
        a, b = _run(asm, zeros), _run(asm, noise)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        _same(a, T.assemble_ref(zeros, d), name)


@pytest.mark.parametrize("name", ["c1_tiny", "c5_bits"])
def test_guard_regions_round_all_three_outputs(name):
    d, asm = _asm(name)
    _, _, rand = T.inputs(name)
    ref = T.reference(name, "random")
    asm._plan()
    S, guard = rand.shape[0], 64
    sizes = (S * d.tb_row_bytes, S * 8, S * d.C * 8)
    bufs = [torch.full((guard + -(-n // 16) * 16 + guard,), 0xA5, dtype=torch.uint8, device=_dev()) for n in sizes]
    src = _t(rand)
    ptr = [C.c_void_p(b.data_ptr() + guard) for b in bufs]
    assert all(p.value % 16 == 0 for p in ptr)
    asm._launch(C.c_void_p(src.data_ptr()), S, *ptr)
    torch.cuda.synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for r, n in zip(raw, sizes):
        assert np.all(r[:guard] == 0xA5) and np.all(r[guard + n:] == 0xA5)
    tb = raw[0][guard:guard + sizes[0]].reshape(S, -1)
    status = raw[1][guard:guard + sizes[1]].view(np.int32).reshape(S, 2)
    cb = raw[2][guard:guard + sizes[2]].view(np.int32).reshape(S, d.C, 2)
    _same((tb, status, cb), ref, name)
    assert np.array_equal(src.cpu().numpy(), rand)                 # the input is read only


def test_more_workgroups_than_the_chip_holds_at_once():
    """c1_tiny at 16384 slots: 4096 workgroups of four waves by the host view's geometry, every third slot corrupted."""
    d, asm = _asm("c1_tiny")
    v = TB.derive_host(2, 24)
    S = 4096 * v.blocks_per_workgroup // v.c
    assert -(-S * v.c // v.blocks_per_workgroup) >= 4096 > 8 * torch.cuda.get_device_properties(_dev()).multi_processor_count
    rng = np.random.default_rng(5)
    tb_bits = rng.integers(0, 2, (S, d.A)).astype(np.uint8)
    rows = T.pack(T.segment(tb_bits, 2), d.in_row_bytes)
    rows[::3, 0, :5] ^= rng.integers(1, 256, (len(rows[::3]), 5)).astype(np.uint8)       # bits below K' = 40 only
    ref = T.assemble_ref(rows, d)
    assert np.all(ref[1][1::3] == 0) and np.all(ref[1][2::3] == 0) and np.count_nonzero(ref[1][::3, 0]) >= len(ref[1][::3]) - 2
    got = _run(asm, rows)
    _same(got, ref, "16384 slots")
    one = _run(asm, rows[:7])                              # two workgroups, the second partly filled
    assert all(np.array_equal(o, w[:7]) for o, w in zip(one, got))


def test_empty_batch_and_argument_errors():
    d, asm = _asm("c2_bits")
    tb, status, cb = asm(torch.empty((0, 2, d.in_row_bytes), dtype=torch.uint8, device=_dev()))
    assert tuple(tb.shape) == (0, d.tb_row_bytes) and tuple(status.shape) == (0, 2) and tuple(cb.shape) == (0, 2, 2)
    good = _t(T.inputs("c2_bits")[2])
    flat = torch.zeros(good.numel() + 16, dtype=torch.uint8, device=_dev())
    off = flat[1:1 + good.numel()].view(good.shape)       # dense, one byte off the 16-byte grid
    assert off.is_contiguous() and off.data_ptr() % 16 == 1
    wide = torch.zeros((3, 2, 2 * d.in_row_bytes), dtype=torch.uint8, device=_dev())[:, :, ::2]
    for bad in (good.to(torch.int8), good.float(), good[:, :, :-1], good[:, :1], good[0], good[:, 0], good.cpu(), wide, off, "x"):
        with pytest.raises(ValueError):
            asm(bad)
    lib, h = asm._lib, asm._handle
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=_dev())
    p = buf.data_ptr()
    assert p % 16 == 0
    args = [C.c_void_p(good.data_ptr()), 3, C.c_void_p(p), C.c_void_p(p + 16384), C.c_void_p(p + 32768)]
    for i in (0, 2, 3, 4):
        bad = list(args)
        bad[i] = C.c_void_p(bad[i].value + 4)
        assert lib.ce_tb_assemble(h, *bad, None) == _lib.CE_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert lib.ce_tb_assemble(h, args[0], -1, *args[2:], None) == _lib.CE_ERR_INVALID and "n_slots" in _lib.last_error()
    assert lib.ce_tb_assemble(h, None, 3, *args[2:], None) == _lib.CE_ERR_INVALID
    assert lib.ce_tb_assemble(h, args[0], 0, None, None, None, None) == 0            # n_slots == 0 launches nothing
    info = _lib.TbInfo()
    assert lib.ce_tb_plan_get_info(h, C.byref(info)) == 0
    assert (info.n_code_blocks, info.in_row_bytes, info.tb_row_bytes, info.bytes_per_slot) == (2, 544, 1056, 2 * 544 + 1056 + 16 + 8)
    torch.cuda.synchronize()


def test_a_non_default_stream_gives_the_same_result():
    d, asm = _asm("c2_bytes")
    _, valid, rand = T.inputs("c2_bytes")
    rows = _t(np.concatenate([valid, rand]))
    ref = _run(asm, rows)
    _same(ref, T.assemble_ref(np.concatenate([valid, rand]), d), "default stream")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        out = asm(rows)
    side.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out, ref))


@pytest.mark.parametrize("which", sorted(O.CHAINS))
def test_chain_behind_the_decoder(which):
    """A random transport block -> segment -> random-graph codewords -> the transmitted positions of rv 0 -> noisy int8 LLRs ->
    PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock: the block sent and every residue 0; with one slot's LLR row
    negated, that slot's residue is nonzero and equals the oracle's for what the decoder actually returned."""
    x = T.chain_inputs(which)
    c, d, t, g = x.c, x.d, x.t, x.g
    rm = RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], device=_dev())
    dec = LD.PuschLdpcDecoder.for_rate_recovery(rm, LD.LdpcGraph(g.rows, g.n_cols))
    asm = TB.PuschTransportBlock.for_rate_recovery(rm)
    assert (asm.c, asm.k_prime, asm.in_row_bytes, asm.tbs) == (d.C, d.Kp, dec.row_bytes, t.A)
    hard, status = dec(rm(_t(x.llr), rv=0))
    tb, tb_status, cb_status = asm(hard)
    torch.cuda.synchronize()
    assert tuple(tb.shape) == (O.CHAIN_SLOTS, t.tb_row_bytes) and tuple(cb_status.shape) == (O.CHAIN_SLOTS, d.C, 2)
    assert np.array_equal(LD.unpack_bits(tb, t.A).numpy(), x.tb_bits) and np.array_equal(tb.cpu().numpy(), T.pack(x.tb_bits, t.tb_row_bytes))
    assert not tb_status.cpu().numpy().any() and not cb_status.cpu().numpy()[..., 0].any() and bool((status[..., 1] == 1).all())
    hard, _ = dec(rm(_t(x.llr_neg), rv=0))
    got = _run(asm, hard)
    _same(got, T.assemble_ref(hard.cpu().numpy(), t), (which, "negated"))
    assert got[1][-1, 0] != 0 and not got[1][:-1].any() and np.array_equal(LD.unpack_bits(got[0][:-1], t.A), x.tb_bits[:-1])
