"""GPU tests of the rate-recovery extension (include/ce_rm.h): the kernel's soft buffers against the literal restatement of
TS 38.212 5.4.2 / 5.5 in tests/rm_oracle.py, by value and without a tolerance (float32 additions in the defined order are
reproducible bit for bit; int8 sums are integers), in both formats, with and without a kept HARQ buffer.

The file's name sorts it behind test_zz_hip_demod.py: rate recovery consumes what the demapper's tests cover, and every
earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import demod_oracle as D
import eq_oracle as Q
import rm_oracle as R
from srsran_ce_pytorch_amd import demod as DM, dmrs, equalizer as EQ, estimator as E, ratematch as RM, synth as S

pytestmark = pytest.mark.gpu
FORMATS = [("f32", torch.float32), ("i8", torch.int8)]
FMT_IDS = [f for f, _ in FORMATS]
NAMES = [c["name"] for c in R.CASES]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _rm(x, dt):
    c = x.c
    return RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], dtype=dt, n_ref=c["n_ref"], filler_llr=R.FILLER, device=_dev())


def _llr(x, fmt):
    return x.llr_i8 if fmt == "i8" else x.llr_f32


def _harq(x, fmt):
    return x.harq_i8 if fmt == "i8" else x.harq_f32


def _run(rm, llr, rv, harq=None, out=None):
    got = rm(_t(llr) if isinstance(llr, np.ndarray) else llr, rv, harq=_t(harq) if isinstance(harq, np.ndarray) else harq, out=out)
    torch.cuda.synchronize()
    return got


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_case_under_every_rv_against_the_oracle(name, fmt, dt):
    x = R.inputs(name)
    d = x.d
    rm = _rm(x, dt)
    filler = 127 if fmt == "i8" else np.float32(R.FILLER)
    for shift in range(4):
        rv = _t(R.rvs_of(shift), torch.int32)
        for with_harq in (False, True):
            ref, hits = R.reference(name, fmt, shift, with_harq)
            got = _run(rm, _llr(x, fmt), rv, _harq(x, fmt) if with_harq else None)
            assert tuple(got.shape) == (R.N_SLOTS, d.C, d.N_cb) and got.dtype == dt and got.device == _dev()
            g = got.cpu().numpy()
            assert np.array_equal(g, ref), (name, fmt, shift, with_harq, int(np.sum(g != ref)))
            # fillers hold the filler value whatever harq holds there; a position nothing reaches keeps harq, or 0
            assert np.all(g[:, :, d.f0:d.f1] == filler)
            live = np.ones(d.N_cb, bool)
            live[d.f0:d.f1] = False
            untouched = (hits == 0) & live
            kept = _harq(x, fmt) if with_harq else np.zeros_like(ref)
            assert np.array_equal(g[untouched], kept[untouched])
            assert untouched.any() != x.c["rep"]


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", ["bg2_a24_rep", "bg1_a96_k0_in_filler", "bg2_a3848_c2"])
def test_each_slot_of_a_batch_equals_its_own_single_slot_call(name, fmt, dt):
    x = R.inputs(name)
    rm = _rm(x, dt)
    rvs = R.rvs_of(1)
    llr, harq = _llr(x, fmt), _harq(x, fmt)
    whole = _bytes(_run(rm, llr, _t(rvs, torch.int32), harq))
    for b in range(R.N_SLOTS):
        one = _bytes(_run(rm, llr[b:b + 1], _t(rvs[b:b + 1], torch.int32), harq[b:b + 1]))
        assert np.array_equal(one[0], whole[b]), b
        same = _bytes(_run(rm, llr[b:b + 1], rvs[b], harq[b:b + 1]))
        assert np.array_equal(same, one)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_stride_0_rv_equals_a_tensor_of_equal_values_and_a_strided_view(fmt, dt):
    x = R.inputs("bg1_a96_rep")
    rm = _rm(x, dt)
    llr = _llr(x, fmt)
    a = _bytes(_run(rm, llr, 2))
    b = _bytes(_run(rm, llr, _t([2] * R.N_SLOTS, torch.int32)))
    wide = _t(np.repeat([2] * R.N_SLOTS, 3), torch.int32)[::3]                    # an element stride of 3
    assert wide.stride(0) == 3
    c = _bytes(_run(rm, llr, wide))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    mixed = _t([0, 9, 9, 3, 9, 9, 1, 9, 9], torch.int32)[::3]                     # the stride is honoured per slot
    ref, _ = R.recover(x.d, llr, [0, 3, 1], None, R.FILLER)
    assert np.array_equal(_run(rm, llr, mixed).cpu().numpy(), ref)
    ref, _ = R.recover(x.d, llr, [2, 2, 2], None, R.FILLER)
    assert np.array_equal(_run(rm, llr, 2).cpu().numpy(), ref)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_device_rv_values_7_and_minus_1_behave_as_3(fmt, dt):
    x = R.inputs("bg1_a8448_lbrm")
    rm = _rm(x, dt)
    llr, harq = _llr(x, fmt), _harq(x, fmt)
    three = _bytes(_run(rm, llr, 3, harq))
    odd = _bytes(_run(rm, llr, _t([7, -1, 3], torch.int32), harq))
    assert np.array_equal(three, odd)
    ref, _ = R.recover(x.d, llr, [3, 3, 3], harq, R.FILLER)
    assert np.array_equal(_run(rm, llr, _t([-1, 7, 0x7FFFFFFF], torch.int32), harq).cpu().numpy(), ref)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", ["bg2_a24_rep", "bg1_a8448_c2"])
def test_out_is_harq_equals_the_call_with_separate_buffers(name, fmt, dt):
    x = R.inputs(name)
    rm = _rm(x, dt)
    rv = _t(R.rvs_of(2), torch.int32)
    separate = _run(rm, _llr(x, fmt), rv, _harq(x, fmt))
    buf = _t(_harq(x, fmt))
    got = _run(rm, _llr(x, fmt), rv, buf, out=buf)
    assert got is buf and np.array_equal(_bytes(buf), _bytes(separate))
    ref, _ = R.reference(name, fmt, 2, True)
    assert np.array_equal(buf.cpu().numpy(), ref)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", ["bg1_a96_rep", "bg1_a16896_c3"])
def test_two_transmissions_combine_as_the_oracle_combines_them(name, fmt, dt):
    """rv 0, then rv 2 of other LLRs into the kept buffer, in place."""
    x = R.inputs(name)
    rm = _rm(x, dt)
    first = _llr(x, fmt)
    second = np.ascontiguousarray(first[::-1, ::-1])                                  # other values of the same draw
    ref1, _ = R.recover(x.d, first, [0] * R.N_SLOTS, None, R.FILLER)
    ref2, hits2 = R.recover(x.d, second, [2] * R.N_SLOTS, ref1, R.FILLER)
    soft = _run(rm, first, 0)
    assert np.array_equal(soft.cpu().numpy(), ref1)
    again = _run(rm, second, 2, soft, out=soft)
    assert again is soft and np.array_equal(soft.cpu().numpy(), ref2)
    assert not np.array_equal(ref1, ref2) and hits2.any()


def test_guard_regions_round_out_stay_untouched_with_misaligned_rows():
    """N_cb = 350: slot rows start at elements 0, 350, 700 -- 4-byte units of the int8 output straddle slots, and the
    whole output ends inside a unit."""
    x = R.inputs("bg2_a24_rep")
    d = x.d
    assert d.N_cb == 350 and d.C == 1
    dev = _dev()
    n = R.N_SLOTS * d.N_cb
    guard = 64                                                   # keeps the view 16-byte aligned in both formats
    for (fmt, dt), fill in zip(FORMATS, (-5.0, 77)):
        rm = _rm(x, dt)
        for with_harq in (False, True):
            buf = torch.full((n + 2 * guard,), fill, dtype=dt, device=dev)
            out = buf[guard:guard + n].view(R.N_SLOTS, d.C, d.N_cb)
            got = _run(rm, _llr(x, fmt), _t(R.rvs_of(3), torch.int32), _harq(x, fmt) if with_harq else None, out=out)
            assert got is out
            h = buf.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + n:] == fill)
            ref, _ = R.reference("bg2_a24_rep", fmt, 3, with_harq)
            assert np.array_equal(h[guard:guard + n].reshape(ref.shape), ref)
        # one and two slots: the output ends 2 bytes / 0 bytes into an int8 unit
        for B in (1, 2):
            buf = torch.full((B * d.N_cb + 2 * guard,), fill, dtype=dt, device=dev)
            out = buf[guard:guard + B * d.N_cb].view(B, d.C, d.N_cb)
            hq = torch.full((B * d.N_cb + guard,), fill, dtype=dt, device=dev)
            hq[:B * d.N_cb] = _t(_harq(x, fmt)[:B]).reshape(-1)
            _run(rm, _llr(x, fmt)[:B], 1, hq[:B * d.N_cb].view(B, d.C, d.N_cb), out=out)
            h = buf.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + B * d.N_cb:] == fill)
            ref, _ = R.recover(d, _llr(x, fmt)[:B], [1] * B, _harq(x, fmt)[:B], R.FILLER)
            assert np.array_equal(h[guard:guard + B * d.N_cb].reshape(ref.shape), ref)


def test_empty_batch_launches_nothing():
    x = R.inputs("bg1_a96_k0_in_filler")
    dev = _dev()
    for _, dt in FORMATS:
        rm = _rm(x, dt)
        out = rm(torch.empty((0, x.d.G), dtype=dt, device=dev), 0)
        assert tuple(out.shape) == (0, x.d.C, x.d.N_cb) and out.dtype == dt
        out = rm(torch.empty((0, x.d.G), dtype=dt, device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
        assert tuple(out.shape) == (0, x.d.C, x.d.N_cb)


def test_argument_errors():
    x = R.inputs("bg2_a3848_c2")
    d = x.d
    dev = _dev()
    rm = _rm(x, torch.int8)
    B, shape = R.N_SLOTS, (R.N_SLOTS, d.C, d.N_cb)
    llr, harq = _t(x.llr_i8), _t(x.harq_i8)
    rv = _t(R.rvs_of(0), torch.int32)
    good = rm(llr, rv, harq=harq)
    assert tuple(good.shape) == shape
    n = B * d.C * d.N_cb
    off_l = torch.empty((B * d.G + 1,), dtype=torch.int8, device=dev)[1:].view(B, d.G).copy_(llr)            # 1 byte off
    off_h = torch.empty((n + 4,), dtype=torch.int8, device=dev)[4:].view(shape).copy_(harq)                   # 4 bytes off
    off_o = torch.empty((n + 8,), dtype=torch.int8, device=dev)[8:].view(shape)                               # 8 bytes off
    bad_calls = [
        dict(llr=llr.float()), dict(llr=llr.to(torch.int16)),                                                  # wrong dtype
        dict(llr=llr[:, :-1]), dict(llr=llr[:, :-2].contiguous()), dict(llr=llr.view(B, 2, d.G // 2)), dict(llr=llr.reshape(-1)),  # wrong shape
        dict(llr=llr.cpu()), dict(llr=x.llr_i8),                                                               # CPU tensor, not a tensor
        dict(llr=torch.zeros((B, 2 * d.G), dtype=torch.int8, device=dev)[:, ::2]),                            # not dense
        dict(llr=off_l), dict(harq=off_h), dict(out=off_o),                                                    # misaligned
        dict(rv=None), dict(rv=4), dict(rv=-1), dict(rv=1.0), dict(rv=True),
        dict(rv=rv[:2]), dict(rv=rv.long()), dict(rv=rv.cpu()), dict(rv=rv.view(B, 1)),
        dict(harq=harq.float()), dict(harq=harq[:2]), dict(harq=harq[:, :, :-1]), dict(harq=harq.cpu()), dict(harq=harq.view(B, -1)),
        dict(harq=torch.zeros((B, d.C, 2 * d.N_cb), dtype=torch.int8, device=dev)[:, :, ::2]),
        dict(out=good.float()), dict(out=good[:, :, :-1]), dict(out=good.cpu()), dict(out=good[:2]),
        dict(out=torch.empty((B, d.C, 2 * d.N_cb), dtype=torch.int8, device=dev)[:, :, ::2]),
    ]
    for kw in bad_calls:
        args = dict(llr=llr, rv=rv, harq=harq, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            rm(args["llr"], args["rv"], harq=args["harq"], out=args["out"])
    with pytest.raises(ValueError, match="16-byte"):
        rm(off_l, rv)
    # the library refuses what the Python checks would have caught
    lib, h = rm._lib, rm._plan()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.ce_rm_recover(h, p(off_l), p(rv), 1, B, None, p(good), None) == -1
    assert lib.ce_rm_recover(h, p(llr), p(rv), 1, B, p(off_h), p(good), None) == -1
    assert lib.ce_rm_recover(h, p(llr), p(rv), 1, B, None, p(off_o), None) == -1
    assert lib.ce_rm_recover(h, p(llr), p(rv), -1, B, None, p(good), None) == -1
    assert lib.ce_rm_recover(h, p(llr), None, 1, B, None, p(good), None) == -1
    assert lib.ce_rm_recover(h, p(llr), p(rv), 1, -1, None, p(good), None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(good.cpu().numpy(), R.reference("bg2_a3848_c2", "i8", 0, True)[0])


def test_end_to_end_grid_to_soft_buffers():
    """The demapper's end-to-end chain (random bits -> scrambled -> 16QAM -> channel -> PuschDmrs -> estimate ->
    PuschEqualizer -> PuschDemapper) with PuschRateRecovery appended: at every transmitted position of every code block the
    hard decision is the sent bit the oracle's map puts there, untransmitted positions are 0, fillers hold the filler."""
    dev = _dev()
    case = D.e2e_case()
    h1, h2, cfg = S.numpy_hops(case)
    pil = dmrs.PuschDmrs(h1, h2, 2, 52, device=dev)(D.E2E_SLOT, D.E2E_N_ID, D.E2E_N_SCID)
    eq = EQ.PuschEqualizer(h1, h2, 2, 52, device=dev)
    data_re = eq.data_re()
    assert np.array_equal(data_re, Q.data_re_ref(case))
    grids, bits, _ = D.e2e_slot(pil[0].cpu().numpy(), data_re, np.random.default_rng(78))
    rx = torch.as_tensor(grids, device=dev)[None]
    ch_est, noise, *_ = E.estimate(rx, pil, case["beta"], h1, h2, cfg)
    x_hat, nvar = eq(rx, ch_est, noise)
    A, bg, rv = 16896, 1, 0
    for (fmt, dt), filler in zip(FORMATS, (np.float32(55.25), 127)):
        dem = DM.PuschDemapper("16qam", eq.n_data_re * 2, out_dtype=dt, llr_scale=1.0, descramble=True, device=dev)
        llr = dem(x_hat, nvar, rnti=D.E2E_RNTI, n_id=D.E2E_SCR_ID)
        rm = RM.PuschRateRecovery(bg, A, "16qam", 2, dem.n_bits, dtype=dt, filler_llr=55.25, device=dev)
        d = R.derive(bg, A, 4, 2, dem.n_bits)
        assert dem.n_bits == len(bits) == 28800 and rm.n_code_blocks == d.C == 3 and max(rm.e) <= d.P    # every E_r <= P: no position is hit twice
        soft = rm(llr, rv)
        torch.cuda.synchronize()
        got = soft[0].cpu().numpy()
        assert got.shape == (d.C, d.N_cb)
        blk, pos, _ = R.slot_map(d, rv)
        sent = np.zeros((d.C, d.N_cb), bool)
        hit = np.zeros((d.C, d.N_cb), bool)
        sent[blk, pos] = bits.astype(bool)
        hit[blk, pos] = True
        assert hit.sum() == len(bits)
        assert np.array_equal(got[hit] < 0, sent[hit]), fmt
        assert np.all(got[:, d.f0:d.f1] == filler) and not hit[:, d.f0:d.f1].any()
        hit[:, d.f0:d.f1] = True
        assert np.all(got[~hit] == 0) and (~hit).any()
        # and the values are the demapper's own, moved
        assert np.array_equal(got[blk, pos], llr[0].cpu().numpy())
