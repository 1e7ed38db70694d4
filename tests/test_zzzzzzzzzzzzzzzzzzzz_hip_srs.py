"""GPU tests of the SRS channel estimator (include/ce_tp.h `ce_srs_profile` / `ce_srs_estimate`, `SrsEstimator`) against the
float64 oracle of tests/srs_oracle.py under its rules: every case through both launches; the read set (the whole grid NaN but the
used combs' elements; strided, offset and expanded views); the write set (guard words round all five outputs); bitwise independence
of an item from its batch and of a receive port from the others; a NaN confined to its (item, port); the delay as a tensor, with
stride 0 and out of range; a side stream and an empty batch; the refusals of the launches on made-up addresses with nothing
written; and the loop srs_map -> PuschOfdmModulator -> PuschChannelEmulator -> PuschOfdmDemodulator -> SrsEstimator on the
demodulator's grid view.

The file's name sorts it behind test_zzzzzzzzzzzzzzzzzzz_hip_prach.py: every earlier GPU test keeps its place in the run."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ofdm_oracle as OO
import srs_oracle as SO
from srsran_ce_pytorch_amd import _lib, channel as CH, ofdm as OF, srs as S

pytestmark = pytest.mark.gpu

GUARD = 0x7FC54321                                            # a quiet NaN with a payload, as float32; an unlikely int32
PAD = 67


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())


def _estimator(c, **over):
    return S.SrsEstimator(**{**SO.plan_kwargs(c), **over}, device=_dev())


def _params(d, b=slice(None)):
    """(slot, n_id) as the wrapper takes them: ints where the case has one value, device int32 tensors [B] otherwise."""
    out = []
    for v in (d.slot, d.n_id):
        out.append(int(v[0]) if v.size == 1 else _t(v.astype(np.int32))[b])
    return out


def _np_est(out):
    torch.cuda.synchronize()
    return SimpleNamespace(h_sb=out.h_sb.cpu().numpy(), h_wb=out.h_wb.cpu().numpy(), noise=out.noise.cpu().numpy(), epre=out.epre.cpu().numpy())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def _same_bits(a, b, what="", names=("h_sb", "h_wb", "noise", "epre")):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"{what}: {name} differs by bits"


def _sub(a, b=slice(None), r=slice(None)):
    return SimpleNamespace(h_sb=a.h_sb[b, r], h_wb=a.h_wb[b, r], noise=a.noise[b, r], epre=a.epre[b, r])


def _both(est, y, slot, n_id, delay=None):
    """(profile [B, R, win_len], delay [B]) as numpy and the estimate at `delay` (default: the profile's own)."""
    p = est.profile(y, slot, n_id)
    e = est(y, slot, n_id, delay=p.delay if delay is None else delay)
    torch.cuda.synchronize()
    return p.profile.cpu().numpy(), p.delay.cpu().numpy(), _np_est(e)


@pytest.mark.parametrize("geometry,hopping", SO.CASES, ids=SO.CASE_IDS)
def test_cases_against_the_oracle(geometry, hopping):
    d = SO.inputs(geometry, hopping)
    c = d.c
    est = _estimator(c)
    slot, n_id = _params(d)
    p = est.profile(_t(d.y), slot, n_id)
    assert tuple(p.profile.shape) == (c.B, c.R, c.win_len) and p.profile.dtype == torch.float32
    assert tuple(p.delay.shape) == (c.B,) == tuple(p.ta_s.shape) and p.delay.dtype == torch.int32 and p.ta_s.dtype == torch.float64
    out = est(_t(d.y), slot, n_id, delay=p.delay)
    assert tuple(out.h_sb.shape) == (c.B, c.R, c.n_ap, c.n_symb, c.n_blocks) and tuple(out.h_wb.shape) == (c.B, c.R, c.n_ap) and tuple(out.noise.shape) == (c.B, c.R) == tuple(out.epre.shape)
    got = _np_est(out)
    SO.check(d, prof=p.profile.cpu().numpy(), delay=p.delay.cpu().numpy(), est=got, what=f"{geometry}-{hopping}")
    assert np.array_equal(p.delay.cpu().numpy(), d.sent)
    assert np.allclose(p.ta_s.cpu().numpy(), d.sent / (c.N * c.k_tc * 30e3), rtol=1e-12, atol=0)
    # the channel comes back: the gains, with the constant phases put back, to the noise of sigma over a block
    back = S.srs_band_response(got.h_sb, d.delay, c.k_tc, c.N, c.ports, c.start_prb)
    assert np.abs(back - d.H[:, :, :, None, None]).max() <= 6 * SO.SIGMA * np.sqrt(c.n_ap / c.Q)
    assert np.all(np.abs(got.noise / SO.SIGMA ** 2 - 1) <= 6 / np.sqrt(c.n_symb * c.n_combs * c.M - c.n_symb * c.n_ap * c.n_blocks))
    # delay = None is delay 0
    _same_bits(_np_est(est(_t(d.y), slot, n_id)), _np_est(est(_t(d.y), slot, n_id, delay=torch.zeros(c.B, dtype=torch.int32, device=_dev()))), geometry)


READ_SET = [("a_c4_4p_one_comb_m36", "group"), ("b_c4_4p_two_combs", "neither"), ("c_c2_4p_m144_4sym", "sequence"), ("e_c4_2p_m12_phi", "group")]


@pytest.mark.parametrize("geometry,hopping", READ_SET, ids=[f"{g}-{h}" for g, h in READ_SET])
def test_read_set_only_the_used_combs_elements(geometry, hopping):
    """The whole grid NaN but the used combs' elements, inside a wider NaN-filled buffer that starts at an odd element: finite,
    and the dense call's results by bits.  Stride 0 repeats an item."""
    d = SO.inputs(geometry, hopping)
    c = d.c
    est = _estimator(c)
    slot, n_id = _params(d)
    want = _both(est, _t(d.y), slot, n_id)
    used = np.zeros((c.n_sym, c.n_sc), bool)
    for comb in c.combs:
        for s in range(c.n_symb):
            used[c.l0 + s, 12 * c.start_prb[s] + comb:12 * c.start_prb[s] + comb + c.k_tc * c.M:c.k_tc] = True
    y = np.where(used[None, None], d.y, np.complex64(complex(np.nan, np.nan)))
    width, lead = c.n_sc + 7, 3
    buf = torch.full((2 * (lead + c.B * c.R * c.n_sym * width),), float("nan"), dtype=torch.float32, device=_dev()).view(torch.complex64)
    view = buf[lead:].view(c.B, c.R, c.n_sym, width)[..., :c.n_sc]
    view.copy_(_t(y))
    assert not view.is_contiguous() and view.data_ptr() % 16 == 8
    got = _both(est, view, slot, n_id)
    assert np.all(np.isfinite(got[0])) and all(np.all(np.isfinite(getattr(got[2], k).view(np.float32))) for k in ("h_sb", "h_wb", "noise", "epre"))
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    _same_bits(got[2], want[2], f"{geometry} NaN-filled view")
    # the ports outside the items, and the grid view of the demodulator's layout permuted back
    swapped = _t(d.y).permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert not swapped.is_contiguous() or 1 in (c.B, c.R)
    _same_bits(_both(est, swapped, slot, n_id)[2], want[2], f"{geometry} ports outside")
    grid = _t(d.y).permute(0, 1, 3, 2)                                # [B, R, n_sc, n_sym], as the demodulator and the decompressor return it
    _same_bits(_both(est, grid.permute(0, 1, 3, 2), slot, n_id)[2], want[2], f"{geometry} grid view")
    if isinstance(slot, int):                                        # stride 0: one item expanded equals the batch of copies
        one = _t(d.y[:1])
        a, b = _both(est, one.expand(3, -1, -1, -1), slot, n_id), _both(est, one.repeat(3, 1, 1, 1), slot, n_id)
        assert np.array_equal(_bits(a[0]), _bits(b[0]))
        _same_bits(a[2], b[2], f"{geometry} expanded")


def _raw(est, entry, y, st, B, R, slot, slot_st, n_id, id_st, *rest):
    """The library's return code of a launch entry point on the current stream with the arguments as they stand."""
    est._plan()
    ptr = lambda x: C.c_void_p(x if isinstance(x, int) else (x.data_ptr() if x is not None else None))      # noqa: E731
    pointers = (0,) if entry == "ce_srs_profile" else (0, 2, 3, 4, 5)          # profile | delay, delay_stride, h_sb, h_wb, noise, epre
    args = [ptr(a) if k in pointers else a for k, a in enumerate(rest)]
    with torch.cuda.device(est.device):
        return getattr(est._lib, entry)(est._handle, ptr(y), *st, B, R, ptr(slot), slot_st, ptr(n_id), id_st, *args,
                                        C.c_void_p(torch.cuda.current_stream(est.device).cuda_stream))


def _guarded(n_words):
    """An int32 buffer of GUARD words with `n_words` to write in the middle: (buffer, the middle)."""
    buf = torch.full((PAD + n_words + PAD + 1,), GUARD, dtype=torch.int32, device=_dev())
    off = PAD + (1 if (buf.data_ptr() + 4 * PAD) % 8 else 0)            # the middle 8-byte aligned (complex outputs)
    return buf, buf[off:off + n_words]


def _sizes(c, B, R):
    """The five outputs in 32-bit words: profile, h_sb, h_wb, noise, epre."""
    return [B * R * c.win_len, 2 * B * R * c.n_ap * c.n_symb * c.n_blocks, 2 * B * R * c.n_ap, B * R, B * R]


@pytest.mark.parametrize("geometry,hopping", [("a_c4_4p_one_comb_m36", "neither"), ("c_c2_4p_m144_4sym", "group"), ("f_c2_2p_m1632", "sequence")])
def test_write_set_guard_words_round_all_five_outputs(geometry, hopping):
    d = SO.inputs(geometry, hopping)
    c = d.c
    est = _estimator(c)
    slot, n_id = _params(d)
    prof, delay, want = _both(est, _t(d.y), slot, n_id)
    y = _t(d.y)
    st = (c.R * c.n_sym * c.n_sc, c.n_sym * c.n_sc, c.n_sc)
    sl, idt, dl = _t(np.resize(d.slot, c.B).astype(np.int32)), _t(np.resize(d.n_id, c.B).astype(np.int32)), _t(delay.astype(np.int32))
    bufs = [_guarded(n) for n in _sizes(c, c.B, c.R)]
    assert _raw(est, "ce_srs_profile", y, st, c.B, c.R, sl, 1, idt, 1, bufs[0][1]) == 0, _lib.last_error()
    assert _raw(est, "ce_srs_estimate", y, st, c.B, c.R, sl, 1, idt, 1, dl, 1, *(mid for _, mid in bufs[1:])) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for (buf, mid), ref in zip(bufs, (prof, want.h_sb, want.h_wb, want.noise, want.epre)):
        host, inner = buf.cpu().numpy(), mid.cpu().numpy()
        assert np.count_nonzero(host != GUARD) <= inner.size and np.array_equal(inner.view(np.uint32), _bits(ref).reshape(-1)), f"{geometry}: written outside an output"
        assert np.count_nonzero(host == GUARD) >= 2 * PAD


@pytest.mark.parametrize("geometry,hopping", [("a_c4_4p_one_comb_m36", "group"), ("c_c2_4p_m144_4sym", "sequence"), ("g_c2_1p_m408_r5", "neither")])
def test_an_item_does_not_depend_on_its_batch_nor_a_port_on_the_others(geometry, hopping):
    d = SO.inputs(geometry, hopping)
    c = d.c
    est = _estimator(c)
    y = _t(d.y)
    prof, delay, batch = _both(est, y, *_params(d))
    dl = _t(delay.astype(np.int32))
    for b in range(c.B):
        sl = slice(b, b + 1)
        p1, d1, e1 = _both(est, y[sl], *_params(d, sl), delay=dl[sl])
        assert np.array_equal(_bits(p1), _bits(prof[sl])), f"item {b}"
        _same_bits(e1, _sub(batch, sl), f"{geometry} item {b}")
    for r in range(c.R):
        sl = slice(r, r + 1)
        p1, _, e1 = _both(est, y[:, sl], *_params(d), delay=dl)
        assert np.array_equal(_bits(p1), _bits(prof[:, sl])), f"port {r}"
        _same_bits(e1, _sub(batch, slice(None), sl), f"{geometry} port {r}")


def test_a_nan_stays_in_its_item_and_port():
    d = SO.inputs("c_c2_4p_m144_4sym", "group")
    c = d.c
    est = _estimator(c)
    slot, n_id = _params(d)
    dl = _t(d.delay.astype(np.int32))
    prof, _, clean = _both(est, _t(d.y), slot, n_id, delay=dl)
    y = d.y.copy()
    y[1, 0, c.l0 + 2, 12 * c.start_prb[2] + c.combs[0] + c.k_tc * 40] = complex(float("nan"), 1.0)
    p2, _, got = _both(est, _t(y), slot, n_id, delay=dl)
    keep = np.ones((c.B, c.R), bool)
    keep[1, 0] = False
    assert np.array_equal(_bits(p2[keep]), _bits(prof[keep])) and np.all(np.isnan(p2[1, 0]))
    for k in ("h_sb", "h_wb", "noise", "epre"):
        assert np.array_equal(_bits(getattr(got, k)[keep]), _bits(getattr(clean, k)[keep])), k
    on_comb = [i for i, (comb, _) in enumerate(c.ports) if comb == c.combs[0]]
    assert np.isnan(got.noise[1, 0]) and np.isnan(got.epre[1, 0]) and np.all(np.isnan(got.h_wb[1, 0, on_comb])) and np.all(np.isnan(got.h_sb[1, 0, on_comb, 2, 40 // c.Q]))


def test_the_delay_as_a_tensor_with_stride_0_and_out_of_range():
    d = SO.inputs("c_c2_4p_m144_4sym", "neither")
    c = d.c
    est = _estimator(c)
    y, (slot, n_id) = _t(d.y), _params(d)
    dl = d.delay.astype(np.int64)
    want = _np_est(est(y, slot, n_id, delay=_t(dl.astype(np.int32))))
    SO.check(d, est=want, what="delay tensor")
    for shift in (5 * c.N, -3 * c.N, 2 ** 31 - c.N):                 # taken mod N
        moved = ((dl + shift + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
        _same_bits(_np_est(est(y, slot, n_id, delay=_t(moved))), want, f"delay + {shift}")
    wide = _t(np.stack([dl, dl + 1], 1).astype(np.int32))[:, 0]      # element stride 2
    assert wide.stride(0) == 2
    _same_bits(_np_est(est(y, slot, n_id, delay=wide)), want, "strided delay")
    one = _t(np.array([dl[1]], np.int32))
    same = _np_est(est(y, slot, n_id, delay=one.expand(c.B)))        # stride 0: item 1's delay for every item
    _same_bits(_sub(same, slice(1, 2)), _sub(want, slice(1, 2)), "expanded delay")
    assert not np.array_equal(_bits(same.h_sb[0]), _bits(want.h_sb[0]))
    for bad in (dl, _t(dl), _t(dl.astype(np.int32))[:2], _t(dl.astype(np.int32)).cpu(), _t(dl.astype(np.int32)).flip(0)[None]):
        with pytest.raises(ValueError):
            est(y, slot, n_id, delay=bad)


def test_a_side_stream_and_an_empty_batch():
    d = SO.inputs("a_c4_4p_one_comb_m36", "group")
    c = d.c
    est = _estimator(c)
    y, (slot, n_id) = _t(d.y), _params(d)
    want = _both(est, y, slot, n_id)
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        p = est.profile(y, slot, n_id)
        e = est(y, slot, n_id, delay=p.delay)
    side.synchronize()
    assert np.array_equal(_bits(p.profile.cpu().numpy()), _bits(want[0])) and np.array_equal(p.delay.cpu().numpy(), want[1])
    _same_bits(_np_est(e), want[2], "side stream")
    p0 = est.profile(y[:0], slot, n_id)
    e0 = est(y[:0], slot, n_id, delay=p0.delay)
    assert tuple(p0.profile.shape) == (0, c.R, c.win_len) and tuple(p0.delay.shape) == (0,) == tuple(p0.ta_s.shape)
    assert tuple(e0.h_sb.shape) == (0, c.R, c.n_ap, c.n_symb, c.n_blocks) and tuple(e0.noise.shape) == (0, c.R)
    # n_items == 0 launches nothing, whatever the pointers
    assert _raw(est, "ce_srs_profile", 0x8, (0, 0, 0), 0, 1, None, 0, None, 0, None) == 0
    assert _raw(est, "ce_srs_estimate", None, (0, 0, 0), 0, 1, 0x4, 0, 0x4, 0, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()


def test_refusals_of_the_launches_with_nothing_written():
    d = SO.inputs("a_c4_4p_one_comb_m36", "neither")
    c = d.c
    est = _estimator(c)
    B, R = c.B, c.R
    y = _t(d.y)
    st = (R * c.n_sym * c.n_sc, c.n_sym * c.n_sc, c.n_sc)
    sl, idt, dl = _t(np.full(B, 7, np.int32)), _t(np.full(B, 777, np.int32)), _t(np.zeros(B, np.int32))
    bufs = [_guarded(n) for n in _sizes(c, B, R)]
    pf, hs, hw, nz, ep = (mid for _, mid in bufs)
    a = y.data_ptr()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    P, E = "ce_srs_profile", "ce_srs_estimate"
    bad = [("n_items", INV, P, (y, st, -1, R, sl, 1, idt, 1, pf)), ("n_rx", INV, P, (y, st, B, 0, sl, 1, idt, 1, pf)), ("n_rx", INV, P, (y, st, B, 65, sl, 1, idt, 1, pf)),
           ("null", INV, P, (None, st, B, R, sl, 1, idt, 1, pf)), ("null", INV, P, (y, st, B, R, None, 1, idt, 1, pf)), ("null", INV, P, (y, st, B, R, sl, 1, None, 1, pf)),
           ("null", INV, P, (y, st, B, R, sl, 1, idt, 1, None)),
           ("must be >= 0", INV, P, (y, (-1, st[1], st[2]), B, R, sl, 1, idt, 1, pf)), ("must be >= 0", INV, P, (y, (st[0], -1, st[2]), B, R, sl, 1, idt, 1, pf)),
           ("must be >= 0", INV, P, (y, (st[0], st[1], -1), B, R, sl, 1, idt, 1, pf)), ("must be >= 0", INV, P, (y, st, B, R, sl, -1, idt, 1, pf)),
           ("must be >= 0", INV, P, (y, st, B, R, sl, 1, idt, -1, pf)),
           ("8-byte", INV, P, (a + 4, st, B, R, sl, 1, idt, 1, pf)), ("4-byte", INV, P, (y, st, B, R, sl.data_ptr() + 2, 1, idt, 1, pf)),
           ("4-byte", INV, P, (y, st, B, R, sl, 1, idt, 1, pf.data_ptr() + 2)),
           ("address space", INV, P, (y, (2 ** 62, st[1], st[2]), B, R, sl, 1, idt, 1, pf)), ("address space", INV, P, (y, (st[0], 2 ** 61, st[2]), B, R, sl, 1, idt, 1, pf)),
           ("address space", INV, P, (y, (st[0], st[1], 2 ** 61), B, R, sl, 1, idt, 1, pf)),
           ("2^31-1 workgroups", UNS, P, (y, (0, 0, st[2]), 2 ** 31 // 3 + 1, R, sl, 0, idt, 0, pf)),
           ("n_items", INV, E, (y, st, -1, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep)), ("n_rx", INV, E, (y, st, B, 65, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep)),
           ("null", INV, E, (None, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep)), ("null", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, None, hw, nz, ep)),
           ("null", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, None, nz, ep)), ("null", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, None, ep)),
           ("null", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, None)),
           ("must be >= 0", INV, E, (y, (st[0], -1, st[2]), B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep)), ("delay_stride", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, -1, hs, hw, nz, ep)),
           ("8-byte", INV, E, (a + 4, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep)), ("8-byte", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs.data_ptr() + 4, hw, nz, ep)),
           ("8-byte", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw.data_ptr() + 4, nz, ep)), ("4-byte", INV, E, (y, st, B, R, sl, 1, idt, 1, dl.data_ptr() + 1, 1, hs, hw, nz, ep)),
           ("4-byte", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz.data_ptr() + 2, ep)), ("4-byte", INV, E, (y, st, B, R, sl, 1, idt, 1, dl, 1, hs, hw, nz, ep.data_ptr() + 1))]
    before = d.y.copy()
    for text, code, entry, args in bad:
        rc = _raw(est, entry, *args)
        assert rc == code and text in _lib.last_error(), (text, entry, rc, _lib.last_error())
    torch.cuda.synchronize()
    assert all(bool((buf == GUARD).all()) for buf, _ in bufs) and np.array_equal(y.cpu().numpy().view(np.uint64), before.view(np.uint64))


def test_refusals_of_the_wrapper_before_any_launch():
    d = SO.inputs("a_c4_4p_one_comb_m36", "neither")
    c = d.c
    est = _estimator(c)
    y = _t(d.y)
    wide = torch.zeros((c.B, c.R, c.n_sym, 2 * c.n_sc), dtype=torch.complex64, device=_dev())
    bad = [d.y, y.cpu(), y.to(torch.complex128), y.real.contiguous(), y[0], y[..., :c.n_sc - 1], wide[..., ::2], y[:, :1].expand(c.B, 65, c.n_sym, c.n_sc), y[:, :0],
           y[:, :, :13]]
    for t in bad:
        with pytest.raises(ValueError):
            est.profile(t, 7, 777)
        with pytest.raises(ValueError):
            est(t, 7, 777)
    for slot, n_id in ((-1, 0), (0, -1), (0, 65536), (1.0, 0), (True, 0), (_t(np.zeros(c.B, np.int64)), 0), (0, _t(np.zeros(c.B + 1, np.int32))), (0, torch.zeros(c.B, dtype=torch.int32))):
        with pytest.raises(ValueError):
            est.profile(y, slot, n_id)
    got = est.profile(wide[..., :c.n_sc + 5], 7, 777)              # a longer last dimension is a view like any other
    torch.cuda.synchronize()
    assert not got.profile.any()                                   # an all-zero grid: exact zeros


def test_the_loop_from_srs_map_through_ofdm_and_a_delayed_channel_to_the_estimator():
    """srs_map -> PuschOfdmModulator -> PuschChannelEmulator (one tap per (rx, tx) at a common delay of D samples, no noise) ->
    PuschOfdmDemodulator -> SrsEstimator on the demodulator's grid view, n_fft_ofdm = N k_tc: delay == D, and srs_band_response
    returns the gains (referred to the grid's subcarrier 0: the grid's centre sits on DC, so exp(+j 2 pi (n_sc / 2) D / n_fft) comes
    with them).  Tolerance: ofdm_oracle's rule once per stage of the chain (modulator, emulator, demodulator) plus h_sb's own."""
    k_tc, n_ap, n_cs, k_bar, m_srs, n_prb_grid, N, R, B, D = 2, 2, 3, 1, 16, 24, 256, 3, 2, 9
    n_fft, scs, n_sym, l0, start_prb = N * k_tc, 30e3, 14, 12, (4, 7)
    slot, n_id = 5, 301
    cp = OF.nr_cp_lengths(scs, n_fft, n_sym)
    assert D < min(cp)
    seq = S.srs_sequence(k_tc, n_ap, n_cs, k_bar, m_srs, 2, l0, slot, n_id, "group", 14, 20)
    tx = S.srs_map(seq, k_tc, n_ap, n_cs, k_bar, start_prb, l0, n_prb_grid, n_sym)                     # [n_ap, n_sc, n_sym]
    dem = OF.PuschOfdmDemodulator(n_fft, n_prb_grid, cp, n_sym=n_sym, device=_dev())
    mod = OF.PuschOfdmModulator.for_demodulator(dem)
    grid = _t(np.broadcast_to(tx.astype(np.complex64).transpose(0, 2, 1)[None], (B, n_ap, n_sym, 12 * n_prb_grid)).copy()).permute(0, 1, 3, 2)
    rng = np.random.default_rng(91)
    gains = (rng.standard_normal((B, R, n_ap)) + 1j * rng.standard_normal((B, R, n_ap))).astype(np.complex64)
    taps = np.zeros((B, R, n_ap, D + 1), np.complex64)
    taps[..., D] = gains
    rx = CH.PuschChannelEmulator(n_ap, R, D + 1, device=_dev())(mod(grid), _t(taps))
    rg = dem(rx)                                                                                       # [B, R, n_sc, n_sym]
    y = rg.permute(0, 1, 3, 2)
    assert y.data_ptr() == rg.data_ptr() and tuple(y.shape) == (B, R, n_sym, 12 * n_prb_grid)
    est = S.SrsEstimator(k_tc, n_ap, n_cs, k_bar, m_srs, n_prb_grid, N, n_symb=2, l0=l0, start_prb=start_prb, n_sym=n_sym, hopping="group",
                         slots_per_frame=20, scs_hz=scs, device=_dev())
    p = est.profile(y, slot, n_id)
    out = est(y, slot, n_id, delay=p.delay)
    torch.cuda.synchronize()
    assert np.array_equal(p.delay.cpu().numpy(), np.full(B, D)) and np.allclose(p.ta_s.cpu().numpy(), D / (n_fft * scs), rtol=1e-12)
    h_sb = out.h_sb.cpu().numpy()
    back = S.srs_band_response(h_sb, p.delay.cpu().numpy(), k_tc, N, est.ports, start_prb)
    want = gains.astype(np.complex128) * np.exp(2j * np.pi * (12 * n_prb_grid // 2) * D / n_fft)
    rms = OO.window_rms(rx.cpu().numpy(), n_fft, cp)[..., 0, l0:l0 + 2].max(-1)                         # [B, R]
    e_block = SO.block_energy(SimpleNamespace(l0=l0, start_prb=start_prb, k_tc=k_tc, M=12 * m_srs // k_tc, n_symb=2, n_blocks=m_srs // 4, Q=48 // k_tc,
                                              ports=est.ports), y.cpu().numpy())
    tol = (3 * OO.T_OFDM * OO.EPS * (np.log2(n_fft) * rms[:, :, None] + np.abs(want)))[..., None, None] + SO.TOL["h_sb"] * SO.EPS * SO.c_h(48 // k_tc) * np.sqrt(e_block)
    err = np.abs(back - want[..., None, None])
    print(f"loop: max |h - gain| / tolerance = {(err / tol).max():.3f}, delay {p.delay.cpu().numpy()}")
    assert np.all(err <= tol)
    assert np.all(out.noise.cpu().numpy() <= 1e-9 * out.epre.cpu().numpy())
