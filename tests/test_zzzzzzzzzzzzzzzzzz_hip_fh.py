"""GPU tests of fronthaul I/Q (de)compression (include/ce_tp.h `ce_fh_decompress`, `ce_fh_compress`; `PuschFronthaulDecompressor`,
`PuschFronthaulCompressor`), every comparison by bits against the bit-serial oracle of tests/fh_oracle.py: both kernels on
every case of fh_oracle.CASES; the write set (strided `out=` views inside NaN-filled and 0xA5-filled buffers, in three
nestings, with odd and with even strides, sections, padding behind row_bytes); the read set (everything outside the rows
randomised); bitwise independence of a row from its batch; the round trips; a side stream, an empty batch; every refusal of
the entry points and of the wrappers with nothing written; and the loop through the chain: PuschTransportEncoder ->
PuschModulator (-> PuschTransformPrecoder) -> PuschOfdmModulator -> PuschChannelEmulator -> PuschOfdmDemodulator ->
PuschFronthaulCompressor -> PuschFronthaulDecompressor -> estimate -> .. -> PuschTransportBlock.

The file's name sorts it behind test_zzzzzzzzzzzzzzzzz_hip_chan.py: every earlier GPU test keeps its place in the run."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fh_oracle as X
import loop_chain
import mod_oracle as MO
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, channel as CH, fronthaul as FH, ofdm as OF

pytestmark = pytest.mark.gpu

NAN_FILL = np.array([0x7FC12345_7FC54321], np.uint64)       # two quiet NaNs with payloads: the pattern of a grid written into
BYTE_FILL = 0xA5
NESTINGS = {"port_inside_slot": (2, 1, 0), "slot_inside_port": (2, 0, 1), "symbol_outside": (0, 1, 2)}      # dimensions (slot, port, symbol), innermost first
WRITE_CASES = ["w9_prb24", "w8_prb1", "w8_prb3", "w14_prb3", "none_prb3", "w9_prb341"]
SECTION_CASES = WRITE_CASES[:-1] + ["w9_prb273"]            # sections of a grid five PRBs wider: at most 336 PRBs


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)


def _pair(c, n_prb_grid=None, **kw):
    fh = FH.PuschFronthaulDecompressor(c["n_prb"] if n_prb_grid is None else n_prb_grid, c["S"], c["method"], c["W"], c["scale"], device=_dev(), **kw)
    return fh, FH.PuschFronthaulCompressor.for_decompressor(fh)


def _fast(rows):
    """Host rows [B, R, S, n_sc] -> the device grid [B, R, n_sc, S] in the fast layout."""
    return _t(rows).permute(0, 1, 3, 2)


def _rows(grid):
    """The device grid [B, R, n_sc, S] -> host rows [B, R, S, n_sc]."""
    return grid.permute(0, 1, 3, 2).cpu().numpy()


def _strides(nesting, n, row, odd, q=1):
    """Strides (slot, port, symbol) of rows of `row` units nested as `nesting` with a gap behind every row and every group:
    multiples of q; for q = 1 all odd (`odd`) or all even."""
    s, ext = [0, 0, 0], row
    for k, d in enumerate(NESTINGS[nesting]):
        st = -(-(ext + 3 + 2 * k) // q) * q
        if q == 1:
            st += (st & 1) ^ (1 if odd else 0)
        s[d] = st
        ext += (n[d] - 1) * st
    return s, ext


def _pay(a):
    """Host payload rows -> a device tensor whose rows start on 4 bytes: the last dimension padded to a multiple of 4."""
    a = np.asarray(a)
    nb = a.shape[-1]
    wide = np.full(a.shape[:-1] + (nb + (-nb) % 4,), 0xEE, np.uint8)
    wide[..., :nb] = a
    return _t(wide)


def _written(flat, n, s, row, lead):
    """(the rows [B, R, S, row] found in the flat buffer at lead + b s[0] + r s[1] + y s[2], the mask of their elements)."""
    mask, rows = np.zeros(flat.size, bool), np.empty(tuple(n) + (row,), flat.dtype)
    for b in range(n[0]):
        for r in range(n[1]):
            for y in range(n[2]):
                o = lead + b * s[0] + r * s[1] + y * s[2]
                assert not mask[o:o + row].any()
                mask[o:o + row] = True
                rows[b, r, y] = flat[o:o + row]
    return rows, mask


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_decompressor_cases_against_the_oracle(name):
    d = X.inputs(name)
    c = d.c
    fh, _ = _pair(c)
    got = fh(_pay(d.payload))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (c["B"], c["R"], 12 * c["n_prb"], c["S"]) and got.dtype == torch.complex64 and got.device == _dev() and got.stride(2) == 1
    assert np.array_equal(_bits(_rows(got)), _bits(d.unpacked))
    back = fh(_pay(d.packed))                                                # the oracle's own payloads: what a compressor sends
    assert np.array_equal(_bits(_rows(back)), _bits(d.restored))


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_compressor_cases_against_the_oracle(name):
    d = X.inputs(name)
    c = d.c
    _, comp = _pair(c)
    got = comp(_fast(d.grid))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (c["B"], c["R"], c["S"], d.row_bytes) and got.dtype == torch.uint8 and got.device == _dev()
    assert np.array_equal(got.cpu().numpy(), d.packed)


@pytest.mark.parametrize("odd", [True, False])
@pytest.mark.parametrize("nesting", list(NESTINGS))
@pytest.mark.parametrize("name", SECTION_CASES)
def test_decompressor_write_set_of_a_section_in_a_strided_grid(name, nesting, odd):
    """`out` as a strided view of a grid of n_prb + 5 PRBs inside a NaN-filled buffer, the payload a section from PRB 2 on: the
    section's REs carry the oracle's bits; the two PRBs in front, the three behind, the gaps and the guards keep theirs."""
    d = X.inputs(name)
    c = d.c
    dev, n, n_prb = _dev(), (c["B"], c["R"], c["S"]), c["n_prb"]
    n_sc = 12 * (n_prb + 5)
    s, ext = _strides(nesting, n, n_sc, odd)
    lead = 5 if odd else 6
    total = lead + ext + 9
    buf = torch.as_tensor(np.repeat(NAN_FILL, total), device=dev).view(torch.complex64)
    out = buf.as_strided((n[0], n[1], n_sc, n[2]), (s[0], s[1], 1, s[2]), lead)
    assert out.data_ptr() % 16 == (8 if odd else 0)
    fh, _ = _pair(c, n_prb + 5)
    got = fh(_pay(d.payload), start_prb=2, n_prb=n_prb, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == out.shape and got.stride() == out.stride()
    after = _bits(buf)
    rows, mask = _written(after, n, s, 12 * n_prb, lead + 24)
    assert np.array_equal(rows, _bits(d.unpacked))
    assert (~mask).sum() >= 14 + 60 * n[0] * n[1] * n[2] and np.all(after[~mask] == NAN_FILL[0])
    # the complement in two more calls completes the rows of a whole-grid call
    whole = np.concatenate([d.payload[..., :2 * d.row_bytes // n_prb], d.payload, d.payload[..., :3 * d.row_bytes // n_prb]], -1) if n_prb >= 3 else None
    if whole is not None:
        fh(_pay(whole[..., :2 * d.row_bytes // n_prb]), start_prb=0, n_prb=2, out=out)
        fh(_pay(whole[..., -(3 * d.row_bytes // n_prb):]), start_prb=n_prb + 2, n_prb=3, out=out)
        dense = fh(_pay(whole))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(dense))


@pytest.mark.parametrize("nesting", list(NESTINGS))
@pytest.mark.parametrize("name", WRITE_CASES)
def test_compressor_write_set_in_a_strided_byte_buffer(name, nesting):
    """`out` as a strided view with rows longer than row_bytes inside a 0xA5-filled buffer: [0, row_bytes) of every row carries
    the oracle's bytes; the padding behind row_bytes, the gaps and the guards are unchanged."""
    d = X.inputs(name)
    c = d.c
    dev, n, nb = _dev(), (c["B"], c["R"], c["S"]), d.row_bytes
    s, ext = _strides(nesting, n, nb + 3, False, q=4)
    lead, total = 8, 8 + ext + 13
    buf = torch.full((total,), BYTE_FILL, dtype=torch.uint8, device=dev)
    out = buf.as_strided(n + (nb + 3,), tuple(s) + (1,), lead)
    _, comp = _pair(c)
    got = comp(_fast(d.grid), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == n + (nb,) and got.stride() == out.stride()
    after = buf.cpu().numpy()
    rows, mask = _written(after, n, s, nb, lead)
    assert np.array_equal(rows, d.packed)
    assert (~mask).sum() >= 21 + 3 * n[0] * n[1] * n[2] and np.all(after[~mask] == BYTE_FILL)


@pytest.mark.parametrize("name", ["w9_prb24", "w8_prb3", "none_prb3", "w9_prb273"])
def test_read_sets_nothing_outside_the_rows_reaches_the_output(name):
    """The payload rows inside a buffer of random bytes, the grid section inside a grid of random and non-finite REs: with
    everything outside the rows drawn again, both outputs keep the oracle's bits."""
    d = X.inputs(name)
    c = d.c
    dev, n, nb, n_prb = _dev(), (c["B"], c["R"], c["S"]), d.row_bytes, c["n_prb"]
    fh, comp = _pair(c)
    fh_wide, comp_wide = _pair(c, n_prb + 5)
    s, ext = _strides("port_inside_slot", n, nb + 3, False, q=4)
    rng = np.random.default_rng(7)
    for _ in range(2):
        raw = rng.integers(0, 256, 12 + ext + 7, dtype=np.uint8)
        buf = _t(raw)
        view = buf.as_strided(n + (nb,), tuple(s) + (1,), 12)
        view.copy_(_t(d.payload))
        assert np.array_equal(_bits(_rows(fh(view))), _bits(d.unpacked))
        junk = rng.standard_normal(n + (12 * (n_prb + 5), 2)).astype(np.float32) * np.float32(1e6)
        junk[rng.random(junk.shape) < 0.1] = np.nan
        grid = junk.view(np.complex64)[..., 0].copy()
        grid[..., 24:24 + 12 * n_prb] = d.grid
        assert np.array_equal(comp_wide(_fast(grid), start_prb=2, n_prb=n_prb).cpu().numpy(), d.packed)
    assert np.array_equal(comp(_fast(d.grid)).cpu().numpy(), d.packed)


@pytest.mark.parametrize("name", ["w9_prb24", "w8_prb3", "w1_prb3", "none_prb3", "w9_prb273"])
def test_each_row_of_a_batch_equals_its_own_call(name):
    d = X.inputs(name)
    c = d.c
    fh = FH.PuschFronthaulDecompressor(c["n_prb"], 1, c["method"], c["W"], c["scale"], device=_dev())
    comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
    pay, grid = _pay(d.payload), _t(d.grid)
    for b in range(c["B"]):
        for r in range(c["R"]):
            for y in range(c["S"]):
                one = fh(pay[b:b + 1, r:r + 1, y:y + 1])
                assert np.array_equal(_bits(_rows(one))[0, 0, 0], _bits(d.unpacked[b, r, y])), (b, r, y)
                one = comp(grid[b:b + 1, r:r + 1, y:y + 1].permute(0, 1, 3, 2))
                assert np.array_equal(one.cpu().numpy()[0, 0, 0], d.packed[b, r, y]), (b, r, y)


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_round_trip_compress_decompress_compress(name):
    """compress(decompress(compress(x))) == compress(x), on the device, for the power-of-two scales (float32(1 / scale) scale = 1);
    for every scale the second compression is the oracle's of the oracle's decompressed values."""
    d = X.inputs(name)
    c = d.c
    fh, comp = _pair(c)
    first = comp(_fast(d.grid))
    again = comp(fh(first))
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), d.packed)
    assert np.array_equal(again.cpu().numpy(), d.repacked)
    if float(X.inv_scale(c["scale"])) * c["scale"] == 1.0:
        assert np.array_equal(d.repacked, d.packed)


def test_stream_empty_batch_and_defaults():
    d = X.inputs("w9_prb24")
    c = d.c
    dev = _dev()
    fh, comp = _pair(c)
    pay, grid = _t(d.payload), _fast(d.grid)
    e = fh(torch.empty((0, 2, c["S"], d.row_bytes), dtype=torch.uint8, device=dev))           # an empty batch launches nothing
    assert tuple(e.shape) == (0, 2, 288, c["S"])
    e = comp(torch.empty((0, 2, c["S"], 288), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2))
    assert tuple(e.shape) == (0, 2, c["S"], d.row_bytes)
    lib = _lib.load()
    assert lib.ce_fh_decompress(3, None, 0, 0, 0, None, 0, 0, 0, 0, 2, 14, 24, 1, 9, 0.5, None) == 0 and lib.ce_fh_compress(3, None, 0, 0, 0, None, 0, 0, 0, 0, 2, 14, 24, 1, 9, 0.5, None) == 0
    side = torch.cuda.Stream(device=dev)                                    # a non-default stream gives the same bits
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g2, p2 = fh(pay), comp(grid)
    side.synchronize()
    assert np.array_equal(_bits(_rows(g2)), _bits(d.unpacked)) and np.array_equal(p2.cpu().numpy(), d.packed)
    assert fh.device == dev and FH.PuschFronthaulDecompressor(24).device is None
    # without out= the grid outside the section is zero
    wide = FH.PuschFronthaulDecompressor(30, c["S"], c["method"], c["W"], c["scale"], device=dev)
    got = _rows(wide(pay, start_prb=3, n_prb=24))
    assert np.array_equal(_bits(got[..., 36:36 + 288]), _bits(d.unpacked)) and not _bits(got[..., :36]).any() and not _bits(got[..., 36 + 288:]).any()
    # a payload with a longer last dimension and strides of its own
    longer = torch.full((c["B"], c["R"], c["S"], d.row_bytes + 8), 0x5A, dtype=torch.uint8, device=dev)
    longer[..., :d.row_bytes] = pay
    assert np.array_equal(_bits(_rows(fh(longer))), _bits(d.unpacked))


def test_refusals_of_the_entry_points_and_the_wrappers():
    d = X.inputs("w9_prb24")
    c = d.c
    dev, B, R, S, n_prb, nb = _dev(), c["B"], c["R"], c["S"], c["n_prb"], d.row_bytes
    n_sc = 12 * n_prb
    lib = _lib.load()
    fh, comp = _pair(c)
    pay = torch.zeros((B * R * S * nb + 64,), dtype=torch.uint8, device=dev)
    pay[:B * R * S * nb] = _t(d.payload).reshape(-1)
    grid = torch.zeros((B * R * S * n_sc + 8,), dtype=torch.complex64, device=dev)
    pp, pg = pay.data_ptr(), grid.data_ptr()
    dense_p, dense_g = (R * S * nb, S * nb, nb), (R * S * n_sc, S * n_sc, n_sc)

    def call(fn, abi=3, p=pp, ps=dense_p, g=pg, gs=dense_g, slots=B, ports=R, sym=S, prb=n_prb, method=1, width=9, scale=c["scale"]):
        vp = lambda a: C.c_void_p(a) if a else None
        return getattr(lib, fn)(abi, vp(p), *ps, vp(g), *gs, slots, ports, sym, prb, method, width, scale, None)

    refused = [(dict(abi=2), "ABI version 2 != 3"), (dict(width=17), "iq_width=17 outside 1..16"), (dict(prb=342), "n_prb=342 outside 1..341"), (dict(sym=0), "n_sym=0 must be >= 1"),
               (dict(scale=float("nan")), "outside 2^-96 .. 2^96"), (dict(p=0), "null argument"), (dict(g=0), "null argument"), (dict(ps=(-4, S * nb, nb)), "strides must be >= 0"),
               (dict(p=pp + 2), "multiples of 4 bytes"), (dict(ps=(R * S * nb, S * nb + 2, nb)), "multiples of 4 bytes"), (dict(g=pg + 4), "grid must be 8-byte aligned"),
               (dict(gs=(1 << 60, S * n_sc, n_sc)), "exceeds the address space"), (dict(g=pp), "payload overlaps grid"), (dict(p=pg + 8), "payload overlaps grid")]
    for fn in ("ce_fh_decompress", "ce_fh_compress"):
        for kw, text in refused:
            assert call(fn, **kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (fn, kw, _lib.last_error())
        assert call(fn, method=2) == _lib.CE_ERR_UNSUPPORTED and call(fn, slots=1 << 31, ps=(0, 0, 0), gs=(0, 0, 0)) == _lib.CE_ERR_UNSUPPORTED
        assert call(fn, slots=0) == 0
    assert call("ce_fh_decompress", gs=(R * S * n_sc, S * n_sc, n_sc - 1)) == _lib.CE_ERR_INVALID and "overlap" in _lib.last_error()
    assert call("ce_fh_decompress", gs=(0, S * n_sc, n_sc)) == _lib.CE_ERR_INVALID and "overlap" in _lib.last_error()
    assert call("ce_fh_compress", ps=(R * S * nb, S * nb, nb - 4)) == _lib.CE_ERR_INVALID and "overlap" in _lib.last_error()
    assert call("ce_fh_compress", ps=(R * S * nb, 0, nb)) == _lib.CE_ERR_INVALID and "overlap" in _lib.last_error()
    torch.cuda.synchronize()
    assert not grid.any() and not pay[B * R * S * nb:].any() and np.array_equal(pay[:B * R * S * nb].cpu().numpy(), d.payload.reshape(-1))      # nothing was launched
    # what is not refused: the read side with a repeated row (stride 0), the written side dense
    assert call("ce_fh_decompress", ps=(0, 0, 0)) == 0
    torch.cuda.synchronize()
    got = grid[:B * R * S * n_sc].view(B, R, S, n_sc).cpu().numpy()
    assert np.array_equal(_bits(got), np.broadcast_to(_bits(d.unpacked[0, 0, 0]), (B, R, S, n_sc))) and not grid[B * R * S * n_sc:].any()
    # ---- the wrappers' argument errors ----
    p4, g4 = _t(d.payload), _fast(d.grid)
    good_out = torch.zeros((B, R, S, n_sc), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2)
    good_pay = torch.zeros((B, R, S, nb), dtype=torch.uint8, device=dev)
    odd_bytes = torch.zeros((B * R * S * nb + 8,), dtype=torch.uint8, device=dev)
    short = torch.zeros((B, R, S, nb), dtype=torch.uint8, device=dev)
    short.untyped_storage().resize_(B * R * S * nb - 10)
    bad_dec = [
        (dict(payload=p4.to(torch.int8)), "payload must be a torch.uint8 tensor"), (dict(payload=p4[0]), "payload must be"), (dict(payload=p4[..., :-1]), f">= {nb}\\]"),
        (dict(payload=p4[:, :, :-1]), f"payload must be a torch.uint8 tensor \\[{B}, {R}, {S}, >= {nb}\\]"), (dict(payload=p4.cpu()), "payload must be a tensor on"),
        (dict(payload=d.payload), "payload must be a tensor on"), (dict(payload=torch.zeros((B, R, S, 2 * nb), dtype=torch.uint8, device=dev)[..., ::2]), "contiguous last dimension"),
        (dict(payload=odd_bytes[2:2 + B * R * S * nb].view(B, R, S, nb)), "multiples of 4 bytes"),
        (dict(payload=torch.zeros((B, R, S, nb + 2), dtype=torch.uint8, device=dev)[..., :nb]), "multiples of 4 bytes"), (dict(payload=short), "behind the"),
        (dict(payload=p4[:1]), "payload must be"), (dict(start_prb=1, n_prb=24), "the section lies outside the 24 PRBs"), (dict(n_prb=25), "the section lies outside"),
        (dict(start_prb=-1, n_prb=3), "the section lies outside"), (dict(n_prb=0), "the section lies outside"), (dict(start_prb=1.0), "start_prb must be an int"), (dict(start_prb=None), "start_prb must be an int, got NoneType"),
        (dict(out=good_out.to(torch.complex128)), "out must be a torch.complex64 tensor"), (dict(out=good_out[:, :, :-12]), f"out must be a torch.complex64 tensor \\[slots, ports, {n_sc}, {S}\\]"),
        (dict(out=good_out.cpu()), "out must be a tensor on"), (dict(out=torch.zeros((B, R, n_sc, S), dtype=torch.complex64, device=dev)), "fast layout \\[slot\\]\\[port\\]\\[symbol\\]\\[subcarrier\\]"),
        (dict(out=good_out[:1, :1].expand(B, R, n_sc, S)), "overlap"), (dict(out=good_out[:, :1]), "payload must be"),
    ]
    for kw, text in bad_dec:
        args = dict(payload=p4, out=good_out)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            fh(args.pop("payload"), **args)
    bad_comp = [
        (dict(grid=g4.to(torch.complex128)), "grid must be a torch.complex64 tensor"), (dict(grid=g4.contiguous()), "grid must be in the fast layout"),
        (dict(grid=g4[:, :, :-12]), "grid must be a torch.complex64 tensor"), (dict(grid=g4.cpu()), "grid must be a tensor on"), (dict(grid=d.grid), "grid must be a tensor on"),
        (dict(out=good_pay.to(torch.int8)), "out must be a torch.uint8 tensor"), (dict(out=good_pay[..., :-1]), f"out must be a torch.uint8 tensor \\[{B}, {R}, {S}, >= {nb}\\]"),
        (dict(out=good_pay[:1]), "out must be"), (dict(out=good_pay[:1, :1].expand(B, R, S, nb)), "overlap"), (dict(out=good_pay.cpu()), "out must be a tensor on"),
        (dict(n_prb=25), "the section lies outside"),
    ]
    for kw, text in bad_comp:
        args = dict(grid=g4, out=good_pay)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            comp(args.pop("grid"), **args)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        FH.PuschFronthaulDecompressor(n_prb, S, device="cpu")(p4)
    torch.cuda.synchronize()
    assert not good_out.any() and not good_pay.any()                        # none of the refused calls wrote
    assert np.array_equal(_bits(_rows(fh(p4))), _bits(d.unpacked))


LOOP_N, LOOP_SCS, LOOP_ADVANCE, LOOP_F0 = 512, 30e3, 18, 10e3
# the geometry of test_the_loop_through_the_emulator_returns_the_transport_block (test_zzzzzzzzzzzzzzzzz_hip_chan.py)
LOOP_DELAYS, LOOP_AMPS = (0, 2, 5, 11), (1.0, 0.35, 0.2, 0.1)


@pytest.mark.parametrize("W", [9, 14])
def test_the_loop_through_the_fronthaul_returns_the_transport_block(W):
    """loop_chain.build -> loop_chain.modulate (as it is, and through PuschTransformPrecoder.grid_) -> PuschOfdmModulator ->
    PuschChannelEmulator -> PuschOfdmDemodulator -> PuschFronthaulCompressor -> PuschFronthaulDecompressor -> loop_chain.receive
    on the bg2_z7_rep geometry (24-PRB grid, four ports), BFP of W bits at scale = 2^k, the smallest power of two >=
    max|grid| / 32767.  Without noise and at 40 dB the transport block sent comes back with tb_status 0, with and without the
    precoder, and in every one of these runs the wire bytes and the decompressed grid are the oracle's compress and
    compress-then-decompress of the downloaded grid, by bits."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    B, N, a = ch.B, LOOP_N, LOOP_ADVANCE
    cp = OF.nr_cp_lengths(LOOP_SCS, N)
    assert ch.case["scs"] == LOOP_SCS and ch.n_prb_grid == 24 and max(LOOP_DELAYS) < min(cp) - a and ch.L == 1
    dem = OF.PuschOfdmDemodulator(N, ch.n_prb_grid, cp, window_advance=a, sym_phasor=OF.nr_symbol_phasors(LOOP_F0, LOOP_SCS, N, cp), device=dev)
    ofdm = OF.PuschOfdmModulator.for_demodulator(dem)
    K = max(LOOP_DELAYS) + 1
    emu = CH.PuschChannelEmulator(1, MO.LOOP_PORTS, K, device=dev)
    rng = np.random.default_rng(82)
    gains = np.array(LOOP_AMPS)[None] * np.exp(2j * np.pi * rng.random((MO.LOOP_PORTS, len(LOOP_DELAYS))))
    h = np.zeros((1, MO.LOOP_PORTS, 1, K), np.complex64)
    for r in range(MO.LOOP_PORTS):
        h[0, r, 0] = CH.taps_from_delays(LOOP_DELAYS, gains[r], 1.0, K)
    taps = _t(h)
    for precode in (False, True):
        tx = loop_chain.modulate(ch)
        if precode:
            tx = ch.pre.grid_(tx)
        samples = ofdm(tx)
        rms = float(samples.abs().pow(2).mean().sqrt())
        for sigma in (None, 0.01 * rms):
            rx_rg = dem(emu(samples, taps, sigma=sigma, seed=11, first_slot=MO.LOOP_SLOT))
            assert tuple(rx_rg.shape) == (B, MO.LOOP_PORTS, 288, dem.n_sym) and rx_rg.stride(2) == 1
            peak = float(rx_rg.abs().max())
            scale = 2.0 ** math.ceil(math.log2(peak / 32767.0))
            assert scale / 2.0 < peak / 32767.0 <= scale
            fh = FH.PuschFronthaulDecompressor(ch.n_prb_grid, dem.n_sym, "bfp", W, scale, device=dev)
            comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
            wire = comp(rx_rg)
            assert tuple(wire.shape) == (B, MO.LOOP_PORTS, dem.n_sym, 24 * (1 + 3 * W))
            back = fh(wire)
            out, tb_status = loop_chain.receive(ch, back, deprecode=precode)
            assert np.array_equal(out, ch.sent) and not tb_status.any(), (W, precode, sigma, tb_status.tolist())
            rows = _rows(rx_rg)
            packed = X.compress(rows, scale, "bfp", W)
            assert np.array_equal(wire.cpu().numpy(), packed)
            assert np.array_equal(_bits(_rows(back)), _bits(X.decompress(packed, 24, scale, "bfp", W)))
            if sigma is None:
                err = np.abs(_rows(back) - rows)
                print(f"W={W} precode={precode}: scale 2^{int(math.log2(scale))}, SQNR {10 * np.log10((np.abs(rows) ** 2).mean() / (err ** 2).mean()):.1f} dB")
