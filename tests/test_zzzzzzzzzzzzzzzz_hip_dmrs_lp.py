"""GPU tests of the low-PAPR DM-RS generator (include/ce_dmrs.h `ce_dmrs_lp_generate`, `PuschLowPaprDmrs`): the kernel's output
against the literal oracle of tests/dmrs_lp_oracle.py.  The device only gathers from host-built tables, so every comparison
is np.array_equal on the uint32 view -- bit-exact, no tolerance.  Pinned shapes at every form and wrap, a per-slot batch, device
values out of range, the write set, an empty batch, a side stream, the refusals that need a plan, and the DFT-s-OFDM loop
"transport block -> samples -> transport block" with these pilots.

Allocations of 1 to 4 PRB use a SEEDED RANDOM phi table (dmrs_lp_oracle.random_phi): the tables of 38.211 5.2.2.2 are not in
this repository, and the generator takes them as data.

The file's name sorts it behind test_zzzzzzzzzzzzzzz_hip_tx_fuzz.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import dmrs_lp_oracle as LP
import loop_chain
import mod_oracle as MO
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, dmrs, ofdm as OF, synth as S

pytestmark = pytest.mark.gpu

T1B = S.TYPE1_CDM1                               # mask 0xAAA (the default of hop_spec is 0x555)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _case(name, n_prb_grid, hop_list, n_sym=14):
    return S.case_spec(name, n_prb_grid, hop_list, n_sym=n_sym)


def _phi(case):
    m_zc = 6 * case["hops"][0]["n_prbs"]
    return LP.random_phi(m_zc, 100 + m_zc) if m_zc <= 24 else None


def _gen(case, mode="neither", nss=14, spf=10):
    h1, h2, _ = S.numpy_hops(case)
    return dmrs.PuschLowPaprDmrs(h1, h2, case["n_prb_grid"], case["n_sym"], hopping=mode, slots_per_frame=spf, n_symb_slot=nss,
                                 phi_table=_phi(case), device=_dev())


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _ref(case, slot, n_id, mode, nss=14):
    return LP.pilots_ref(case, slot, n_id, mode, nss, _phi(case))


def _uv(case, slot, n_id, mode, nss=14):
    m_zc = 6 * case["hops"][0]["n_prbs"]
    return [LP.group_and_sequence(mode, nss, slot, l, n_id, m_zc) for h in case["hops"] for l in sorted(h["dmrs_symbols"])]


# (case, mode, n_symb_slot, slots_per_frame, slot, n_id): the smallest shapes at which each form, wrap and hopping path can go wrong
PINNED = [
    (_case("p5_len30_inside", 24, [S.hop_spec([2], 7, 5)]), "neither", 14, 10, 3, 17),             # the length-30 form; starts at PRB 7
    (_case("p5_group", 24, [S.hop_spec([2, 11], 0, 5)]), "group", 14, 10, 9, 1007),
    (_case("p6_wrap", 6, [S.hop_spec([2, 11], 0, 6)]), "group", 14, 10, 4, 29),                     # N_ZC = 31: rows 31 .. 35 wrap
    (_case("p6_inside_aaa", 52, [S.hop_spec([3], 41, 6, re_masks=[T1B])]), "neither", 14, 10, 0, 30),   # the sequence starts at the allocation
    (_case("p12_seq_4col", 24, [S.hop_spec([0, 3, 7, 11], 5, 12)]), "sequence", 14, 20, 13, 600),   # M_ZC = 72: the first size where v is live
    (_case("p11_seq", 24, [S.hop_spec([0, 3, 7, 11], 5, 11)]), "sequence", 14, 20, 13, 600),        # M_ZC = 66: v stays 0
    (_case("p2_phi", 24, [S.hop_spec([2, 11], 9, 2, re_masks=[T1B])]), "group", 14, 10, 6, 321),
    (_case("p4_phi", 24, [S.hop_spec([4], 20, 4)]), "sequence", 14, 10, 2, 77),
    (_case("p7_two_hops", 24, [S.hop_spec([2], 0, 7), S.hop_spec([9, 12], 15, 7)]), "group", 14, 40, 39, 512),
    (_case("p7_sym12", 24, [S.hop_spec([2, 9], 3, 7)], n_sym=12), "group", 12, 20, 17, 100),        # extended cyclic prefix: p = 12 slot + l
    (_case("p273", 273, [S.hop_spec([2, 11], 0, 273)]), "group", 14, 160, 159, 1000),
    (_case("p273_seq", 273, [S.hop_spec([2, 7, 11], 0, 273)]), "sequence", 14, 160, 77, 1),
    (_case("p341", 341, [S.hop_spec([5], 0, 341)]), "sequence", 14, 10, 8, 999),                   # n_re = 2046 <= CE_DMRS_MAX_RE
    (_case("p341_group", 341, [S.hop_spec([0, 13], 0, 341)]), "group", 14, 80, 79, 3),
]


@pytest.mark.parametrize("case,mode,nss,spf,slot,n_id", PINNED, ids=[p[0]["name"] for p in PINNED])
def test_pinned_shapes_one_slot(case, mode, nss, spf, slot, n_id):
    gen = _gen(case, mode, nss, spf)
    got = gen(slot, n_id)
    n_cols = sum(len(h["dmrs_symbols"]) for h in case["hops"])
    assert tuple(got.shape) == (1, 6 * case["hops"][0]["n_prbs"], n_cols, 1) and got.dtype == torch.complex64 and got.device == _dev()
    assert np.array_equal(_bits(got[0]), _bits(_ref(case, slot, n_id, mode, nss))), case["name"]


def test_the_pinned_cases_exercise_what_they_are_named_for():
    """Host only, next to the cases it vouches for: the sequence-hopping pair has c(p) = 1 on a column (so v = 1 at 12 PRB and a
    live v at 11 PRB would show), the group cases have f_gh != 0, and the 6-PRB rows 31 .. 35 repeat rows 0 .. 4."""
    by = {p[0]["name"]: p for p in PINNED}
    c, mode, nss, _, slot, n_id = by["p12_seq_4col"]
    assert sorted({v for _, v in _uv(c, slot, n_id, mode)}) == [0, 1]
    c11 = by["p11_seq"][0]
    assert {v for _, v in _uv(c11, slot, n_id, mode)} == {0} and {v for _, v in _uv(c, slot, n_id, mode)} == {0, 1}
    for name in ("p5_group", "p6_wrap", "p273", "p7_sym12", "p7_two_hops"):
        c, mode, nss, _, slot, n_id = by[name]
        assert any(u != n_id % 30 for u, _ in _uv(c, slot, n_id, mode, nss)), name
    c, mode, nss, _, slot, n_id = by["p7_sym12"]                                # 12 slot + l and 14 slot + l give other groups
    assert _uv(c, slot, n_id, mode, 12) != _uv(c, slot, n_id, mode, 14)
    r = _ref(by["p6_wrap"][0], 4, 29, "group")
    assert np.array_equal(r[31:], r[:5]) and not np.array_equal(r[30:35], r[:5])


@pytest.mark.parametrize("mode", LP.MODES)
@pytest.mark.parametrize("n_cols", [1, 2, 4])
def test_every_hopping_mode_and_column_count(mode, n_cols):
    case = _case(f"p13_{n_cols}", 24, [S.hop_spec([1, 4, 8, 12][:n_cols], 2, 13)])      # M_ZC = 78, N_ZC = 73
    got = _gen(case, mode, spf=20)(19, 859)
    assert np.array_equal(_bits(got[0]), _bits(_ref(case, 19, 859, mode)))


BATCH_CASE = _case("batch_p12", 24, [S.hop_spec([2, 7, 11], 4, 12)])


@pytest.mark.parametrize("mode", ["group", "sequence"])
def test_a_batch_with_per_slot_device_parameters(mode):
    """B = 67 slots, every slot against the oracle and against its own one-slot call; a stride-0 parameter and a strided view."""
    dev, B, spf = _dev(), 67, 40
    rng = np.random.default_rng(7)
    slots, n_ids = rng.integers(0, spf, B).astype(np.int32), rng.integers(0, 1008, B).astype(np.int32)
    slots[:2], n_ids[:2] = (0, spf - 1), (1007, 0)
    gen = _gen(BATCH_CASE, mode, spf=spf)
    d_slot, d_id = torch.as_tensor(slots, device=dev), torch.as_tensor(n_ids, device=dev)
    got = gen(d_slot, d_id)
    assert tuple(got.shape) == (B, 72, 3, 1)
    bits = _bits(got)
    for b in range(B):
        assert np.array_equal(bits[b], _bits(_ref(BATCH_CASE, int(slots[b]), int(n_ids[b]), mode))), b
        assert np.array_equal(_bits(gen(int(slots[b]), int(n_ids[b])))[0], bits[b]), b
    # host arrays are moved; a strided device view is taken as it is
    assert np.array_equal(_bits(gen(slots, n_ids)), bits)
    wide = torch.as_tensor(np.stack([slots, n_ids, slots], 1), device=dev)
    assert wide[:, 1].stride(0) == 3 and np.array_equal(_bits(gen(wide[:, 0], wide[:, 1])), bits)
    # one value for the whole batch: an int, and a one-element tensor (stride 0)
    one = gen(d_slot, torch.full((1,), 421, dtype=torch.int32, device=dev))
    assert np.array_equal(_bits(one), _bits(gen(d_slot, 421)))
    for b in (0, 33, 66):
        assert np.array_equal(_bits(one)[b], _bits(_ref(BATCH_CASE, int(slots[b]), 421, mode))), b


@pytest.mark.parametrize("mode", ["group", "sequence"])
def test_device_values_out_of_range_give_the_documented_wrapped_result(mode):
    """include/ce_dmrs.h: slot enters as slot mod slots_per_frame and n_id as an unsigned value -- u through n_id mod 30, c_init as
    floor(n_id / 30) or n_id masked to 31 bits; the oracle takes such an n_id as it is.  Nothing else is touched: `out` is a view
    between guards."""
    dev, spf = _dev(), 10
    slots = np.array([10, 13, 2 ** 31 - 1, -1, 7, 7, 7, 7], np.int64)
    n_ids = np.array([5, 5, 5, 5, 1008, 65535, 2 ** 31 - 1, -2], np.int64)
    B, gen = len(slots), _gen(BATCH_CASE, mode, spf=spf)
    n, guard = B * 72 * 3, 64
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.complex64, device=dev)
    before = _bits(buf).copy()
    out = buf[guard:guard + n].view(B, 72, 3, 1)
    got = gen(torch.as_tensor(slots.astype(np.int32), device=dev), torch.as_tensor(n_ids.astype(np.int32), device=dev), out=out)
    assert got is out
    after = _bits(buf)
    assert np.array_equal(after[:2 * guard], before[:2 * guard]) and np.array_equal(after[2 * (guard + n):], before[2 * (guard + n):])
    for b in range(B):
        s, i = int(slots[b]) % (1 << 32) % spf, int(n_ids[b]) % (1 << 32)          # the unsigned 32-bit values the kernel sees
        assert np.array_equal(_bits(got[b]), _bits(_ref(BATCH_CASE, s, i, mode))), (b, s, i)


def test_write_set_empty_batch_and_side_stream():
    case = _case("out_p6", 24, [S.hop_spec([2, 11], 3, 6)])
    gen, dev = _gen(case, "group"), _dev()
    B, per = 5, 36 * 2
    n = B * per
    ref = np.stack([_ref(case, s, 9, "group") for s in range(B)])
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    for guard in (64, 63):      # 63: the slab starts 8 bytes off a 16-byte boundary (the kernel's 8-byte store path)
        buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.complex64, device=dev)
        buf[:guard] = complex(7.0, -3.0)
        buf[guard + n:] = complex(-2.0, 5.0)
        before = _bits(buf).copy()
        out = buf[guard:guard + n].view(B, 36, 2, 1)
        assert out.data_ptr() % 16 == (0 if guard == 64 else 8)
        assert gen(slots, 9, out=out) is out
        after = _bits(buf)
        assert np.array_equal(after[:2 * guard], before[:2 * guard]) and np.array_equal(after[2 * (guard + n):], before[2 * (guard + n):])
        assert np.array_equal(after[2 * guard:2 * (guard + n)], _bits(ref).ravel())          # every element written, none left NaN
    good = torch.empty((B, 36, 2, 1), dtype=torch.complex64, device=dev)
    for bad in (good.permute(0, 2, 1, 3), torch.empty((B, 36, 2, 1), dtype=torch.complex128, device=dev),
                torch.empty((B, 36, 4, 1), dtype=torch.complex64, device=dev)[:, :, ::2], good[:4], good.cpu()):
        with pytest.raises(ValueError):
            gen(slots, 9, out=bad)
    # an empty batch launches nothing
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    assert tuple(gen(empty, 1).shape) == (0, 36, 2, 1)
    e_out = torch.empty((0, 36, 2, 1), dtype=torch.complex64, device=dev)
    assert gen(empty, 1, out=e_out) is e_out
    assert gen._lib.ce_dmrs_lp_generate(gen._plan(), None, 0, None, 0, 0, None, None) == 0
    # a non-default stream gives the same bits
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s2 = gen(slots, 9)
    side.synchronize()
    assert np.array_equal(_bits(s2), _bits(ref))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        h1, h2, _ = S.numpy_hops(case)
        dmrs.PuschLowPaprDmrs(h1, h2, 24, device="cpu")(0, 0)


def test_refusals_of_the_entry_point_that_need_a_plan():
    case = _case("ref_p6", 24, [S.hop_spec([2, 11], 3, 6)])
    gen, dev = _gen(case), _dev()
    lib, h = gen._lib, gen._plan()
    B = 3
    par = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.zeros((B * 72 + 2,), dtype=torch.complex64, device=dev)
    pp, po = par.data_ptr(), out.data_ptr()

    def call(slot=pp, ss=1, n_id=pp + 16, si=1, n=B, o=po):
        return lib.ce_dmrs_lp_generate(h, C.c_void_p(slot) if slot else None, ss, C.c_void_p(n_id) if n_id else None, si, n, C.c_void_p(o) if o else None, None)

    INV = _lib.CE_ERR_INVALID
    for kw, text in ((dict(slot=0), "null argument"), (dict(n_id=0), "null argument"), (dict(o=0), "null argument"),
                     (dict(ss=-1), "negative strides are not supported"), (dict(si=-2), "negative strides are not supported"),
                     (dict(slot=pp + 2), "slot and n_id must be 4-byte aligned"), (dict(n_id=pp + 1), "slot and n_id must be 4-byte aligned"),
                     (dict(o=po + 4), "pilots_out must be 8-byte aligned"), (dict(n=-1), "n_slots=-1")):
        assert call(**kw) == INV and text in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=1 << 31) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 slots" in _lib.last_error()
    torch.cuda.synchronize()
    assert not out.any()                                                      # none of the refused calls wrote
    assert call(o=po + 8) == 0                                                # 8-byte alignment is enough
    torch.cuda.synchronize()
    want = _bits(np.stack([_ref(case, 0, 0, "neither")] * B))
    assert np.array_equal(_bits(out[1:1 + B * 72]), want.ravel()) and not out[0].any() and not out[-1].any()


LOOP_N, LOOP_SCS, LOOP_ADVANCE, LOOP_F0 = 512, 30e3, 18, 10e3
LOOP_DELAYS, LOOP_AMPS = (0, 2, 5, 11), (1.0, 0.35, 0.2, 0.1)          # the four-port integer-tap channel of test_zzzzzzzzzzzzzz_hip_ofdm_tx.py


def test_the_dft_s_ofdm_loop_with_low_papr_pilots_returns_the_transport_block():
    """PuschTransportEncoder -> PuschModulator with PuschLowPaprDmrs pilots (group hopping) -> PuschTransformPrecoder.grid_ ->
    PuschOfdmModulator -> the four-port integer-tap channel -> PuschOfdmDemodulator -> estimate -> PuschEqualizer ->
    PuschTransformDeprecoder -> PuschDemapper -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock on the bg2_z7_rep
    geometry (4 PRB of a 24-PRB grid: M_ZC = 24, so the phi table is the seeded random one): the transport block comes back with
    tb_status 0; received with the pilots of another n_id (another group u), every slot fails."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    assert ch.L == 1 and ch.pre is not None and ch.case["hops"][0]["n_prbs"] == 4 and len(ch.case["hops"]) == 1
    gen = _gen(ch.case, "group")
    n_id, other = MO.LOOP_N_ID, MO.LOOP_N_ID + 7
    slot = MO.LOOP_SLOT % 10
    assert _uv(ch.case, slot, n_id, "group")[0][0] != _uv(ch.case, slot, other, "group")[0][0]
    pil, pil_other = gen(slot, n_id), gen(slot, other)
    assert tuple(pil.shape) == tuple(ch.pil.shape) == (1, 24, 1, 1)
    assert np.array_equal(_bits(pil[0]), _bits(_ref(ch.case, slot, n_id, "group")))
    N, a = LOOP_N, LOOP_ADVANCE
    cp = OF.nr_cp_lengths(LOOP_SCS, N)
    assert ch.n_prb_grid == 24 and max(LOOP_DELAYS) < min(cp) - a
    dem = OF.PuschOfdmDemodulator(N, ch.n_prb_grid, cp, window_advance=a, sym_phasor=OF.nr_symbol_phasors(LOOP_F0, LOOP_SCS, N, cp), device=dev)
    ofdm = OF.PuschOfdmModulator.for_demodulator(dem)
    taps = np.array(LOOP_AMPS)[None] * np.exp(2j * np.pi * np.random.default_rng(82).random((MO.LOOP_PORTS, len(LOOP_DELAYS))))

    def air(s):
        T = s.shape[-1]
        rx = torch.zeros((ch.B, MO.LOOP_PORTS, T), dtype=torch.complex64, device=dev)
        for r in range(MO.LOOP_PORTS):
            for i, dl in enumerate(LOOP_DELAYS):
                rx[:, r, dl:] += complex(taps[r, i]) * s[:, 0, :T - dl]
        return rx

    ch.pil = pil
    rx = dem(air(ofdm(ch.pre.grid_(loop_chain.modulate(ch)))))
    out, tb_status = loop_chain.receive(ch, rx, deprecode=True)
    assert np.array_equal(out, ch.sent) and not tb_status.any(), tb_status.tolist()
    ch.pil = pil_other
    out, tb_status = loop_chain.receive(ch, rx, deprecode=True)
    assert np.all(tb_status[:, 0] != 0), tb_status.tolist()
