"""GPU tests of the modulator extension (include/ce_mod.h): `tx` against tests/mod_oracle.py bit for bit (every value is one
float32 multiply or +0) on the pinned cases -- 64QAM symbols straddling dwords on a 1-PRB grid; all four Qm at 3 PRB with all
256 points of 256QAM; 2 layers with data on the DM-RS symbols' odd REs, 3 layers of type 2, 4 layers of type 1; two hops with
symbols in no hop, 12 and 13 symbols, start_symbol > 0; both edges of a 273-PRB grid; an allocation across a tile boundary at
the most bits a tile holds; one full-size slot; 8192 slots -- and scrambling off, shared and per-slot rnti / n_id / pilots,
wrapped c_init, beta 1 and 1.4125, garbage behind bit G, guard regions, the read set, an empty batch, a side stream, out=,
argument errors, and the loop on the device through every stage the project has:
PuschTransportEncoder -> PuschModulator -> channel -> estimate -> PuschEqualizer -> PuschDemapper -> PuschRateRecovery ->
PuschLdpcDecoder -> PuschTransportBlock.  What the loop leans on is asserted from the oracles alone in tests/test_mod.py.

The file's name sorts it behind test_zzzzzzzz_hip_enc.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import eq_oracle as Q
import loop_chain
import mod_oracle as M
from srsran_ce_pytorch_amd import _lib, demod as DM, equalizer as EQ, modulator as MO

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _mod(name, **kw):
    c = M.CASE_BY_NAME[name]
    return MO.PuschModulator(*M.hops(c), c["L"], c["case"]["n_prb_grid"], c["qm"], n_sym=c["case"]["n_sym"], reserved_re_mask=c["mask"], device=_dev(), **kw)


def _np(tx):
    """The wrapper's [B, L, n_sc, n_sym] view -> the oracle's [B, L, n_sym, n_sc], on the host."""
    return tx.permute(0, 1, 3, 2).cpu().numpy()


def _same(got, want, what):
    assert got.dtype == np.complex64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert M.same(got, want), (what, np.argwhere(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))[:4].tolist())


def _run(mod, d, **kw):
    args = dict(rnti=_t(d.rnti), n_id=_t(d.n_id)) if mod.scramble else {}
    args.update(kw)
    return mod(_t(d.g_rows), _t(d.pilots), d.beta, **args)


@pytest.mark.parametrize("name", M.NAMES)
def test_tx_equals_the_oracle(name):
    d, mod = M.inputs(name), _mod(name)
    assert (mod.n_bits, mod.n_symbols, mod.n_data_re, mod.g_row_bytes) == (d.G, d.n_data_re * d.L, d.n_data_re, d.g_rows.shape[1])
    tx = _run(mod, d)
    assert tuple(tx.shape) == (d.B, d.L, 12 * d.case["n_prb_grid"], d.case["n_sym"]) and tx.stride(2) == 1      # subcarrier-contiguous
    _same(_np(tx), M.reference(name), name)
    if name == "256qam_3prb_all_points":
        re = Q.data_re_ref(d.case, d.mask)[:256]
        assert len(np.unique(_np(tx)[0, 0][re[:, 0], re[:, 1]])) == 256


@pytest.mark.parametrize("name", ["straddle_1prb_64qam", "L3_type2", "hops_13sym", "tile_plus_1prb"])
def test_scrambling_parameters_pilots_and_beta(name):
    d, ref = M.inputs(name), M.reference(name)
    mod, plain = _mod(name), _mod(name, scramble=False)
    g, pil = _t(d.g_rows), _t(d.pilots)
    off = M.modulate_ref(d.case, d.mask, d.qm, d.g_bits, d.pilots, d.beta, scramble=False)
    _same(_np(plain(g, pil, d.beta)), off, (name, "scrambling off"))
    _same(_np(plain(g, pil, d.beta, rnti=5, n_id=7)), off, (name, "scrambling off ignores rnti / n_id"))
    assert not M.same(off, ref)
    shared = M.modulate_ref(d.case, d.mask, d.qm, d.g_bits, d.pilots[1], 1.0, 4660, 500)
    _same(_np(mod(g, pil[1].contiguous(), 1.0, rnti=4660, n_id=500)), shared, (name, "shared rnti / n_id / pilots, beta 1"))
    _same(_np(mod(g, pil, d.beta, rnti=_t(d.rnti), n_id=int(d.n_id[0]))), M.modulate_ref(d.case, d.mask, d.qm, d.g_bits, d.pilots, d.beta, d.rnti, int(d.n_id[0])),
          (name, "per-slot rnti, shared n_id"))
    # values above 16 bits: only c_init = (rnti 2^15 + n_id) mod 2^31 matters
    wide_rnti, wide_id = d.rnti.astype(np.int64) + (np.arange(d.B) + 1) * 65536, d.n_id.astype(np.int64) + (np.arange(d.B) + 2) * (1 << 31)
    wrapped = wide_id.astype(np.uint64).astype(np.uint32).view(np.int32)
    _same(_np(mod(g, pil, d.beta, rnti=_t(wide_rnti, torch.int32), n_id=_t(wrapped))), ref, (name, "wrapped c_init"))
    lo = d.n_id.astype(np.int64) + 40000 * 32768                              # n_id carries into the rnti bits
    _same(_np(mod(g, pil, d.beta, rnti=_t(d.rnti), n_id=_t(lo, torch.int32))), M.modulate_ref(d.case, d.mask, d.qm, d.g_bits, d.pilots, d.beta, d.rnti.astype(np.int64) + 40000, d.n_id),
          (name, "n_id above 10 bits"))


@pytest.mark.parametrize("name", ["straddle_1prb_64qam", "qpsk_3prb", "L4_type1"])
def test_bits_behind_g_are_ignored(name):
    d, mod = M.inputs(name), _mod(name)
    clean = M.pack(d.g_bits, mod.g_row_bytes)
    assert (clean != d.g_rows).any()
    a = mod(_t(clean), _t(d.pilots), d.beta, rnti=_t(d.rnti), n_id=_t(d.n_id))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(_run(mod, d))), name


@pytest.mark.parametrize("name", ["straddle_1prb_64qam", "hops_12sym", "tile_plus_1prb_offset"])
def test_guard_regions_and_a_nan_filled_tx(name):
    d, mod, ref = M.inputs(name), _mod(name), M.reference(name)
    mod._plan()
    guard, n = 64, ref.size * 8
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=_dev())
    buf[guard:guard + n] = 0xFF                                             # NaN bytes where tx goes
    g, pil, rnti, n_id = _t(d.g_rows), _t(d.pilots), _t(d.rnti), _t(d.n_id)
    assert (buf.data_ptr() + guard) % 16 == 0
    mod._launch(C.c_void_p(g.data_ptr()), C.c_void_p(pil.data_ptr()), pil[0].numel(), C.c_float(d.beta), C.c_void_p(rnti.data_ptr()), C.c_void_p(n_id.data_ptr()),
                (C.c_int64 * 2)(1, 1), d.B, C.c_void_p(buf.data_ptr() + guard))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert np.all(raw[:guard] == 0xA5) and np.all(raw[guard + n:] == 0xA5)
    got = raw[guard:guard + n].view(np.complex64).reshape(ref.shape)
    assert not np.isnan(got.view(np.float32)).any()
    _same(got, ref, name)
    for t, a in ((g, d.g_rows), (pil, d.pilots), (rnti, d.rnti), (n_id, d.n_id)):
        assert np.array_equal(t.cpu().numpy(), a)                           # the inputs are read only


@pytest.mark.parametrize("name", ["straddle_1prb_64qam", "L2_data_on_dmrs_symbols", "tile_plus_1prb"])
def test_read_set(name):
    """One flipped bit of g changes exactly the element the oracle names; another slot's row changes nothing here."""
    d, mod, ref = M.inputs(name), _mod(name), M.reference(name)
    data_re = Q.data_re_ref(d.case, d.mask)
    rng = np.random.default_rng(3)
    for n in sorted({0, d.G - 1, *rng.integers(0, d.G, 3).tolist()}):
        rows = np.array(d.g_rows)
        rows[0, n // 8] ^= 0x80 >> (n % 8)
        rows[1] = rng.integers(0, 256, rows.shape[1])
        got = _np(mod(_t(rows), _t(d.pilots), d.beta, rnti=_t(d.rnti), n_id=_t(d.n_id)))
        i = n // d.qm
        sym, sc = data_re[i // d.L]
        diff = np.argwhere(got[0].view(np.uint64) != ref[0].view(np.uint64))
        assert diff.tolist() == [[i % d.L, sym, sc]], (name, n, diff[:4].tolist())
        assert not M.same(got[1], ref[1])


def test_one_full_size_slot_has_the_planned_launch():
    mod = _mod("full_size")
    v = MO.derive_host(*mod._geometry, **mod._options)
    assert (v.workgroups_per_slot, v.tiles_per_symbol, v.max_tile_blocks, mod.n_bits) == (26, 13, 33, 1257984)


def test_more_workgroups_than_the_chip_holds_at_once():
    """The 1-PRB case at 8192 slots, 2 workgroups each: every slot its own bits, pilots and (of seven) rnti / n_id."""
    name, B = "straddle_1prb_64qam", 8192
    d, mod = M.inputs(name), _mod(name)
    v = MO.derive_host(*mod._geometry, **mod._options)
    assert B * v.workgroups_per_slot > 8 * torch.cuda.get_device_properties(_dev()).multi_processor_count
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2, (B, d.G)).astype(np.uint8)
    pil = (rng.standard_normal((B,) + d.pilots.shape[1:]) + 1j * rng.standard_normal((B,) + d.pilots.shape[1:])).astype(np.complex64)
    rnti, n_id = (np.arange(B) % 7 * 9001 + 11).astype(np.int32), (np.arange(B) % 7 * 140 + 3).astype(np.int32)
    tx = mod(_t(M.pack(bits, mod.g_row_bytes, rng)), _t(pil), d.beta, rnti=_t(rnti), n_id=_t(n_id))
    _same(_np(tx), M.modulate_ref(d.case, d.mask, d.qm, bits, pil, d.beta, rnti, n_id), "8192 slots")


def test_empty_batch_out_and_argument_errors():
    name = "L2_data_on_dmrs_symbols"
    d, mod, ref = M.inputs(name), _mod(name), M.reference(name)
    dev, B, L = _dev(), d.B, d.L
    n_sc, n_sym = 12 * d.case["n_prb_grid"], d.case["n_sym"]
    g, pil, rnti, n_id = _t(d.g_rows), _t(d.pilots), _t(d.rnti), _t(d.n_id)
    empty = mod(torch.empty((0, mod.g_row_bytes), dtype=torch.uint8, device=dev), pil[0].contiguous(), d.beta, rnti=1, n_id=2)
    assert tuple(empty.shape) == (0, L, n_sc, n_sym)
    out = torch.full((B, L, n_sym, n_sc), float("nan"), dtype=torch.complex64, device=dev)
    tx = mod(g, pil, d.beta, rnti=rnti, n_id=n_id, out=out)
    assert tx.data_ptr() == out.data_ptr()
    _same(out.cpu().numpy(), ref, "out=")
    flat = torch.zeros(g.numel() + 16, dtype=torch.uint8, device=dev)
    off = flat[1:1 + g.numel()].view(g.shape)             # dense, one byte off the 16-byte grid
    assert off.is_contiguous() and off.data_ptr() % 16 == 1
    wide = torch.zeros((B, 2 * mod.g_row_bytes), dtype=torch.uint8, device=dev)[:, ::2]
    ok = dict(rnti=rnti, n_id=n_id)
    for bad in (g.to(torch.int8), g.float(), g[:, :-1], g[0], g[:, None], g.cpu(), wide, off, "x"):
        with pytest.raises(ValueError, match="g must be"):
            mod(bad, pil, d.beta, **ok)
    for bad in (pil.to(torch.complex128), pil.real.contiguous(), pil[:, :-1], pil[:1], pil[..., :1], pil.cpu(), pil.permute(0, 1, 3, 2), "x"):
        with pytest.raises(ValueError, match="pilots must be"):
            mod(g, bad, d.beta, **ok)
    for bad in (float("nan"), float("inf"), 1e39, True, "1", None):
        with pytest.raises(ValueError, match="beta_dmrs"):
            mod(g, pil, bad, **ok)
    for bad in (70000, -1, 1.0, True, torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B + 1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32)):
        with pytest.raises(ValueError, match="rnti"):
            mod(g, pil, d.beta, rnti=bad, n_id=n_id)
    with pytest.raises(ValueError, match="n_id"):
        mod(g, pil, d.beta, rnti=rnti, n_id=1024)
    with pytest.raises(ValueError, match="needs rnti and n_id"):
        mod(g, pil, d.beta, rnti=rnti)
    for bad in (out.permute(0, 1, 3, 2), out[:, :1], out.to(torch.complex128), out.cpu(), torch.view_as_real(out)):
        with pytest.raises(ValueError, match="out must be"):
            mod(g, pil, d.beta, out=bad, **ok)
    with pytest.raises(ValueError, match="PuschEqualizer"):
        MO.PuschModulator.for_equalizer(mod, "qpsk")
    lib, h = mod._lib, mod._handle
    st = (C.c_int64 * 2)(1, 1)
    args = [C.c_void_p(g.data_ptr()), C.c_void_p(pil.data_ptr()), pil[0].numel(), C.c_float(d.beta), C.c_void_p(rnti.data_ptr()), C.c_void_p(n_id.data_ptr()), st, B,
            C.c_void_p(out.data_ptr())]

    def call(i, v):
        a = list(args)
        a[i] = v
        return lib.ce_mod_modulate(h, *a, None)

    for i in (0, 8):
        assert call(i, C.c_void_p(args[i].value + 4)) == _lib.CE_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert call(1, C.c_void_p(args[1].value + 4)) == _lib.CE_ERR_INVALID and "8-byte aligned" in _lib.last_error()
    assert call(7, -1) == _lib.CE_ERR_INVALID and "n_slots" in _lib.last_error()
    assert call(2, -1) == _lib.CE_ERR_INVALID and "strides" in _lib.last_error()
    for bad in ((-1, 1), (1, -1)):
        assert call(6, (C.c_int64 * 2)(*bad)) == _lib.CE_ERR_INVALID and "strides" in _lib.last_error()
    for bad in (float("nan"), float("inf")):
        assert call(3, C.c_float(bad)) == _lib.CE_ERR_INVALID and "beta_dmrs" in _lib.last_error()
    for i in (0, 1, 8):
        assert call(i, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()
    for i in (4, 5, 6):
        assert call(i, None) == _lib.CE_ERR_INVALID and "scrambling needs" in _lib.last_error()
    assert lib.ce_mod_modulate(None, *args, None) == _lib.CE_ERR_INVALID
    assert lib.ce_mod_modulate(h, None, None, 0, C.c_float(1.0), None, None, None, 0, None, None) == 0        # n_slots == 0 launches nothing
    plain = _mod(name, scramble=False)
    plain._plan()
    buf = torch.empty_like(out)
    assert lib.ce_mod_modulate(plain._handle, args[0], args[1], args[2], args[3], None, None, None, B, C.c_void_p(buf.data_ptr()), None) == 0   # NULL rnti / n_id / strides
    torch.cuda.synchronize()
    _same(buf.cpu().numpy(), M.modulate_ref(d.case, d.mask, d.qm, d.g_bits, d.pilots, d.beta, scramble=False), "raw ABI, no scrambling")
    info = _lib.ModInfo()
    assert lib.ce_mod_plan_get_info(h, C.byref(info)) == 0
    assert (info.n_bits, info.n_symbols, info.n_data_re, info.g_row_bytes, info.n_re, info.n_dmrs_total) == (d.G, d.n_data_re * L, d.n_data_re, mod.g_row_bytes, 24, 2)
    assert info.bytes_per_slot == mod.g_row_bytes + 24 * 2 * L * 8 + L * n_sym * n_sc * 8
    assert lib.ce_mod_plan_get_info(h, None) == _lib.CE_ERR_INVALID


def test_a_non_default_stream_gives_the_same_result():
    name = "hops_13sym"
    d, mod = M.inputs(name), _mod(name)
    g, pil, rnti, n_id = _t(d.g_rows), _t(d.pilots), _t(d.rnti), _t(d.n_id)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        tx = mod(g, pil, d.beta, rnti=rnti, n_id=n_id)
    side.synchronize()
    _same(_np(tx), M.reference(name), "side stream")


def test_for_equalizer_shares_the_geometry():
    c = M.CASE_BY_NAME["L3_type2"]
    d = M.inputs("L3_type2")
    eq = EQ.PuschEqualizer(*M.hops(c), c["L"], c["case"]["n_prb_grid"], c["case"]["n_sym"], reserved_re_mask=c["mask"], device=_dev())
    mod = MO.PuschModulator.for_equalizer(eq, "64qam")
    dem = DM.PuschDemapper("64qam", eq.n_data_re * c["L"], descramble=True, device=_dev())
    assert (mod.n_data_re, mod.n_symbols, mod.n_bits) == (eq.n_data_re, dem.n_symbols, dem.n_bits) and mod.scramble
    _same(_np(_run(mod, d)), M.reference("L3_type2"), "for_equalizer")


@pytest.mark.parametrize("name", sorted(M.LOOP_GEOMETRY))
def test_the_loop_through_every_stage_returns_the_transport_block(name):
    """PuschTransportEncoder -> PuschModulator (PuschDmrs pilots) -> a frequency-selective channel on 4 ports (torch ops, no
    noise) -> estimate -> PuschEqualizer -> PuschDemapper(descramble, int8) -> PuschRateRecovery -> PuschLdpcDecoder ->
    PuschTransportBlock: the transport block sent comes back with tb_status 0; a slot whose rnti differs between modulator
    and demapper fails its CRC."""
    dev = _dev()
    ch = loop_chain.build(name, dev)
    sent = ch.sent
    assert ch.mod.n_bits == ch.dem.n_bits == ch.rm.n_bits == ch.enc.n_bits == ch.lp["G"] and ch.mod.g_row_bytes == ch.enc.g_row_bytes
    H = torch.as_tensor(M.loop_channel(ch.case, np.random.default_rng(81)), device=dev)           # [R, n_sc, L]
    rx = torch.einsum("rkl,blks->brks", H, loop_chain.modulate(ch)).contiguous()
    wrong = torch.full((ch.B,), M.LOOP_RNTI, dtype=torch.int32, device=dev)
    wrong[0] += 1
    out, tb_status = loop_chain.receive(ch, rx)
    assert np.array_equal(out, sent) and not tb_status.any(), (name, tb_status.tolist())
    out, tb_status = loop_chain.receive(ch, rx, rnti=wrong)
    assert tb_status[0, 0] != 0 and not tb_status[1:].any() and np.array_equal(out[1:], sent[1:]), (name, "wrong rnti", tb_status.tolist())
