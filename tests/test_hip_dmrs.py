"""GPU tests of the DM-RS generation extension (include/ce_dmrs.h): the kernel's output against the bit-serial oracle
(tests/dmrs_oracle.py).  The operator is integer work plus sign flips of one float32 constant, so every comparison is
np.array_equal on the int32 view -- bit-exact, no tolerance."""
import numpy as np
import pytest
import torch

from conftest import check_outputs

import ce_oracle as O
import dmrs_oracle as D
from dmrs_oracle import CASE_A, CASE_B, CASE_C, T1, T2
from srsran_ce_pytorch_amd import dmrs, estimator as E, synth as S

pytestmark = pytest.mark.gpu

TOL_CH = 2e-5   # tests/test_hip_parity.py's tolerances for oracle comparisons
TOL_SC = 2e-5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _gen(case, nss=14, crb=0):
    h1, h2, _ = S.numpy_hops(case)
    return dmrs.PuschDmrs(h1, h2, case["n_layers"], case["n_prb_grid"], case["n_sym"], grid_start_crb=crb, n_symb_slot=nss, device=_dev())


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.int32)


def _check_slots(got, case, slots, n_ids, n_scids, nss=14, crb=0):
    got = got.cpu().numpy()
    assert got.shape[0] == len(slots) and got.dtype == np.complex64
    for b, (s, i, c) in enumerate(zip(slots, n_ids, n_scids)):
        ref = D.pilots_ref(case, int(s), int(i), int(c), nss, crb)
        assert got[b].shape == ref.shape
        assert np.array_equal(_bits(got[b]), _bits(ref)), f"{case['name']}: slot {b} = ({s}, {i}, {c})"


GEOMETRIES = [
    CASE_A, CASE_B, CASE_C,
    (S.case_spec("prb0", 273, [S.hop_spec([2, 11], 0, 1)], n_layers=2), 3, 10, 0, 14, 0),                      # first table word
    (S.case_spec("prb272", 273, [S.hop_spec([2, 11], 272, 1, re_masks=T1)], n_layers=3), 11, 999, 1, 14, 0),   # last table word
    (S.case_spec("type2_L2", 52, [S.hop_spec([2, 7, 11], 4, 9, re_masks=T2)], n_layers=2), 5, 300, 1, 14, 0),
    (S.case_spec("type2_L3", 52, [S.hop_spec([3], 1, 50, re_masks=T2)], n_layers=3), 6, 301, 0, 14, 7),
    (S.case_spec("sym12", 24, [S.hop_spec([2, 9], 2, 5)], n_layers=1, n_sym=12), 39, 77, 1, 12, 0),
    (S.case_spec("scattered", 106, [S.hop_spec([2, 7], 4, 6, re_masks=T1, mask_prbs=[4, 5, 9, 40, 41, 105]),
                                    S.hop_spec([11], 0, 6, re_masks=T1, mask_prbs=[0, 1, 2, 50, 77, 78])], n_layers=4), 17, 513, 1, 14, 3),
]


@pytest.mark.parametrize("case,slot,n_id,n_scid,nss,crb", GEOMETRIES, ids=[g[0]["name"] for g in GEOMETRIES])
def test_scalar_parameters_one_slot(case, slot, n_id, n_scid, nss, crb):
    gen = _gen(case, nss, crb)
    got = gen(slot, n_id, n_scid)
    assert tuple(got.shape) == (1, gen.n_re, gen.n_dmrs_total, case["n_layers"]) and got.device == _dev()
    _check_slots(got, case, [slot], [n_id], [n_scid], nss, crb)


@pytest.mark.parametrize("n_layers", [1, 4])
def test_full_band_hop_three_slots(n_layers):
    case = S.bench_case("filter", n_layers)
    slots, n_ids, n_scids = [0, 19, 159], [65535, 0, 1007], [1, 0, 1]
    dev = _dev()
    got = _gen(case)(*(torch.tensor(v, dtype=torch.int32, device=dev) for v in (slots, n_ids, n_scids)))
    assert tuple(got.shape) == (3, 1638, 2, n_layers)
    _check_slots(got, case, slots, n_ids, n_scids)


def _popcount_search(case, want):
    """(slot, n_id, n_scid) whose c_init has `want` set bits on some DM-RS symbol of the case."""
    for slot in range(160):
        for n_id in (0, 1, 65535):
            for n_scid in (0, 1):
                for sym in case["hops"][0]["dmrs_symbols"]:
                    if bin(D.c_init(14, slot, sym, n_id, n_scid)).count("1") == want:
                        return slot, n_id, n_scid
    raise AssertionError(f"no c_init with {want} set bits")


def test_per_slot_parameter_batch_with_odd_tail():
    case = S.case_spec("batch", 24, [S.hop_spec([0, 11], 3, 5)], n_layers=2)
    B = 257
    rng = np.random.default_rng(5)
    slots, n_ids, n_scids = rng.integers(0, 160, B), rng.integers(0, 65536, B), rng.integers(0, 2, B)
    special = [(159, 65535, 1), (0, 0, 0), _popcount_search(case, 1), _popcount_search(case, 31)]
    for b, (s, i, c) in zip((0, 100, 255, 256), special):
        slots[b], n_ids[b], n_scids[b] = s, i, c
    dev = _dev()
    gen = _gen(case)
    got = gen(*(torch.as_tensor(v.astype(np.int32), device=dev) for v in (slots, n_ids, n_scids)))
    _check_slots(got, case, slots, n_ids, n_scids)
    # host arrays are moved; strided device views are taken as they are
    assert torch.equal(gen(slots, n_ids, n_scids), got)
    wide = torch.as_tensor(np.stack([slots, n_ids], 1).astype(np.int32), device=dev)
    assert torch.equal(gen(wide[:, 0], wide[:, 1], torch.as_tensor(n_scids.astype(np.int32))), got)


def test_stride_zero_mixing():
    case = S.case_spec("mix", 24, [S.hop_spec([2, 11], 3, 5)], n_layers=1)
    slots = np.arange(20, dtype=np.int32)
    got = _gen(case)(torch.as_tensor(slots, device=_dev()), 40, torch.ones(1, dtype=torch.int32, device=_dev()))
    _check_slots(got, case, slots, [40] * 20, [1] * 20)


def test_out_reuse_and_guard_region():
    case = S.case_spec("out", 24, [S.hop_spec([2, 11], 3, 5)], n_layers=1)
    gen, dev = _gen(case), _dev()
    B, n = 5, 5 * 30 * 2
    ref = np.stack([D.pilots_ref(case, s, 9, 1) for s in range(B)])
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    for guard in (64, 63):      # 63: the slab starts 8 bytes off a 16-byte boundary (the kernel's 8-byte store path)
        buf = torch.full((n + 2 * guard,), complex(7.0, -3.0), dtype=torch.complex64, device=dev)
        out = buf[guard:guard + n].view(B, 30, 2, 1)
        assert gen(slots, 9, 1, out=out) is out
        host = buf.cpu().numpy()
        assert np.all(host[:guard] == np.complex64(7 - 3j)) and np.all(host[guard + n:] == np.complex64(7 - 3j))
        assert np.array_equal(_bits(host[guard:guard + n]), _bits(ref.ravel()))
    good = torch.empty((B, 30, 2, 1), dtype=torch.complex64, device=dev)
    for bad in (good.permute(0, 2, 1, 3), torch.empty((B, 30, 2, 1), dtype=torch.complex128, device=dev),
                torch.empty((B, 30, 4, 1), dtype=torch.complex64, device=dev)[:, :, ::2], good[:4], good.cpu()):
        with pytest.raises(ValueError):
            gen(slots, 9, 1, out=bad)


def test_empty_batch_launches_nothing():
    gen, dev = _gen(CASE_A[0]), _dev()
    got = gen(torch.empty(0, dtype=torch.int32, device=dev), 1, 0)
    assert tuple(got.shape) == (0, 18, 2, 1)
    out = torch.empty((0, 18, 2, 1), dtype=torch.complex64, device=dev)
    assert gen(torch.empty(0, dtype=torch.int32, device=dev), 1, 0, out=out) is out


E2E_CASE = S.case_spec("e2e_25prb", 52, [S.hop_spec([2, 11], 10, 25)], n_layers=2, seed=77)


def _e2e_inputs(monkeypatch, slot, n_id, n_scid, n_items=2):
    pil = _gen(E2E_CASE)(slot, n_id, n_scid)
    monkeypatch.setattr(S, "qpsk_pilots", lambda rng, n_re, n_dmrs, n_layers: pil[0].cpu().numpy())   # build_case's signal model from these pilots
    return pil, S.build_case(E2E_CASE, n_items)


def test_generated_pilots_end_to_end_through_the_estimator(monkeypatch):
    pil, b = _e2e_inputs(monkeypatch, 13, 421, 1)
    assert np.array_equal(_bits(b.pilots), _bits(D.pilots_ref(E2E_CASE, 13, 421, 1)))
    rx = torch.as_tensor(b.grids, device=_dev())[None]
    out = E.estimate(rx, pil, b.beta, b.hop1, b.hop2, b.config)
    torch.cuda.synchronize()
    for it in range(b.grids.shape[0]):
        ref = O.srs_channel_estimator(b.grids[it], b.pilots, b.beta, b.hop1, b.hop2, b.config)
        got = [float(t[0, it]) for t in out[1:]]
        check_outputs(out[0][0, it].cpu().numpy(), got, ref[0], list(ref[1:]), TOL_CH, TOL_SC, f"e2e[{it}]")


def test_generator_on_a_side_stream_next_to_the_estimator(monkeypatch):
    """The generator writes the NEXT step's pilots on a side stream while estimate() runs on the current one; the step
    after consumes them behind an ordinary wait_stream.  Same bits as the serial order."""
    dev = _dev()
    pil0, b = _e2e_inputs(monkeypatch, 13, 421, 1, n_items=4)
    gen = _gen(E2E_CASE)
    B = 48
    rx = torch.as_tensor(b.grids, device=dev)[None].expand(B, -1, -1, -1).contiguous()
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    cur = pil0.expand(B, -1, -1, -1).contiguous()
    # serial order
    nxt_serial = gen(slots, 421, 1)
    step0_serial = E.estimate(rx, cur, b.beta, b.hop1, b.hop2, b.config)
    step1_serial = E.estimate(rx, nxt_serial, b.beta, b.hop1, b.hop2, b.config)
    torch.cuda.synchronize()
    # overlapped
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        nxt = gen(slots, 421, 1)
    step0 = E.estimate(rx, cur, b.beta, b.hop1, b.hop2, b.config)
    torch.cuda.current_stream(dev).wait_stream(side)
    step1 = E.estimate(rx, nxt, b.beta, b.hop1, b.hop2, b.config)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(nxt), _bits(nxt_serial))
    for a, s in zip(step0 + step1, step0_serial + step1_serial):
        assert np.array_equal(a.cpu().numpy().view(np.int32 if a.is_complex() else np.int64), s.cpu().numpy().view(np.int32 if s.is_complex() else np.int64))
