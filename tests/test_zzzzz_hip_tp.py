"""GPU tests of the transform de-precoding extension (include/ce_tp.h): the kernel against the float64 oracle of
tests/tp_oracle.py under its two tolerance rules, on the smallest shapes at which each radix, each pass count and each
rows-per-workgroup setting occurs; bitwise independence of a row from its batch; the in-place form; special values; guard
regions; argument errors; `for_equalizer` on real equalizers; and the chain into the demapper and rate recovery.

The file's name sorts it behind test_zzzz_hip_stage_fuzz.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import demod_oracle as D
import rm_oracle as R
import tp_oracle as T
from srsran_ce_pytorch_amd import demod as DM, deprecode as DP, equalizer as EQ, ratematch as RM, synth as S

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _tp(M, S):
    return DP.PuschTransformDeprecoder(M // 12, S, device=_dev())


def _run(tp, x_hat, nvar, **kw):
    x, nv = tp(_t(x_hat) if isinstance(x_hat, np.ndarray) else x_hat, _t(nvar) if isinstance(nvar, np.ndarray) else nvar, **kw)
    torch.cuda.synchronize()
    return x, nv


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)      # one word per element: the shape stays


@pytest.mark.parametrize("M,S", T.CASES, ids=[f"m{M}_s{S}" for M, S in T.CASES])
def test_every_shape_against_the_oracle(M, S):
    d = T.inputs(M, S)
    tp = _tp(M, S)
    x, nv = _run(tp, d.x_hat, d.nvar)
    assert tuple(x.shape) == tuple(nv.shape) == (T.N_SLOTS, S * M) and x.dtype == torch.complex64 and nv.dtype == torch.float32
    assert x.device == nv.device == _dev()
    T.check(x.cpu().numpy(), nv.cpu().numpy(), d.ref_x, d.ref_nv, DP.derive_host(M // 12, S), f"M={M} S={S}")
    # the equalizer's [B, S M, 1] is the same call
    x3, nv3 = _run(tp, _t(d.x_hat)[:, :, None], _t(d.nvar)[:, :, None])
    assert tuple(x3.shape) == (T.N_SLOTS, S * M) and np.array_equal(_bits(x3), _bits(x)) and np.array_equal(_bits(nv3), _bits(nv))
    # nvar_out is one value per row
    rows = nv.cpu().numpy().reshape(T.N_SLOTS, S, M)
    assert np.all(rows == rows[:, :, :1])


@pytest.mark.parametrize("M,S", [(12, 3), (12, 14), (972, 3), (1500, 3)], ids=["rpw4_one_partial", "rpw4_last_partial", "rpw2_last_partial", "rpw1"])
def test_each_slot_of_a_batch_equals_its_own_single_slot_call(M, S):
    """Every rows-per-workgroup setting the host chooses (4, 2, 1), with a slot's last workgroup not full where rows share one."""
    view = DP.derive_host(M // 12, S)
    assert view.rows_per_workgroup == {12: 4, 972: 2, 1500: 1}[M] and (S % view.rows_per_workgroup != 0 or view.rows_per_workgroup == 1)
    d = T.inputs(M, S)
    tp = _tp(M, S)
    x, nv = _run(tp, d.x_hat, d.nvar)
    wx, wn = _bits(x), _bits(nv)
    for b in range(T.N_SLOTS):
        ox, on = _run(tp, d.x_hat[b:b + 1], d.nvar[b:b + 1])
        assert np.array_equal(_bits(ox)[0], wx[b]) and np.array_equal(_bits(on)[0], wn[b]), b
    # a row's result does not depend on its place: the slots in reverse order
    rx, rn = _run(tp, d.x_hat[::-1], d.nvar[::-1])
    assert np.array_equal(_bits(rx)[::-1], wx) and np.array_equal(_bits(rn)[::-1], wn)
    # nor on its place inside the slot: one symbol at a time through the S = 1 plan
    one = _tp(M, 1)
    for s in (0, S - 1):
        ox, on = _run(one, d.x_hat[:, s * M:(s + 1) * M], d.nvar[:, s * M:(s + 1) * M])
        assert np.array_equal(_bits(ox), wx[:, s * M:(s + 1) * M]) and np.array_equal(_bits(on), wn[:, s * M:(s + 1) * M]), s


@pytest.mark.parametrize("M,S", [(24, 3), (972, 14), (3240, 3)])
def test_in_place_equals_out_of_place(M, S):
    d = T.inputs(M, S)
    tp = _tp(M, S)
    x, nv = _run(tp, d.x_hat, d.nvar)
    xh, nh = _t(d.x_hat), _t(d.nvar)
    gx, gn = _run(tp, xh, nh, out=xh, nvar_out=nh)
    assert gx is xh and gn is nh
    assert np.array_equal(_bits(xh), _bits(x)) and np.array_equal(_bits(nh), _bits(nv))
    # the equalizer's 3-D tensors, viewed to 2-D
    xh3, nh3 = _t(d.x_hat)[:, :, None].contiguous(), _t(d.nvar)[:, :, None].contiguous()
    _run(tp, xh3, nh3, out=xh3.view(T.N_SLOTS, -1), nvar_out=nh3.view(T.N_SLOTS, -1))
    assert np.array_equal(_bits(xh3[:, :, 0]), _bits(x)) and np.array_equal(_bits(nh3[:, :, 0]), _bits(nv))
    # one of the two in place
    xh = _t(d.x_hat)
    gx, gn = _run(tp, xh, d.nvar, out=xh)
    assert np.array_equal(_bits(gx), _bits(x)) and np.array_equal(_bits(gn), _bits(nv))


@pytest.mark.parametrize("M,S", T.SPECIAL, ids=[f"m{M}_s{S}" for M, S in T.SPECIAL])
def test_special_values_are_dropped_and_a_dropped_row_is_an_erasure(M, S):
    d = T.special_inputs(M, S)
    tp = _tp(M, S)
    x, nv = _run(tp, d.x_hat, d.nvar)
    gx, gn = x.cpu().numpy(), nv.cpu().numpy()
    T.check(gx, gn, d.ref_x, d.ref_nv, DP.derive_host(M // 12, S), f"special M={M} S={S}")
    assert np.all(gx[2, :M] == 0) and np.all(np.isposinf(gn[2, :M]))
    if S > 1:
        assert np.all(np.isfinite(gn[2, M:])) and np.any(gx[2, M:] != 0)
    dem = DM.PuschDemapper("16qam", S * M, device=_dev())
    llr = dem(x, nv)
    torch.cuda.synchronize()
    llr = llr.cpu().numpy()
    assert np.all(llr[2, :M * 4] == 0) and np.all(np.isfinite(llr)) and np.all(llr[:2] != 0)
    D.check(llr, D.llr_ref(gx, gn, 4), D.unit_tolerance(gx, gn, 4), f"demapped special M={M} S={S}")


@pytest.mark.parametrize("M,S", [(12, 1), (3240, 14)])
def test_guard_regions_round_both_outputs_stay_untouched(M, S):
    d = T.inputs(M, S)
    tp = _tp(M, S)
    dev, n, guard = _dev(), T.N_SLOTS * S * M, 64
    xbuf = torch.full((n + 2 * guard,), complex(-5.0, 7.0), dtype=torch.complex64, device=dev)
    nbuf = torch.full((n + 2 * guard,), -3.0, dtype=torch.float32, device=dev)
    gx, gn = _run(tp, d.x_hat, d.nvar, out=xbuf[guard:guard + n].view(T.N_SLOTS, -1), nvar_out=nbuf[guard:guard + n].view(T.N_SLOTS, -1))
    hx, hn = xbuf.cpu().numpy(), nbuf.cpu().numpy()
    for h, fill in ((hx, np.complex64(complex(-5.0, 7.0))), (hn, np.float32(-3.0))):
        assert np.all(h[:guard] == fill) and np.all(h[guard + n:] == fill)
    T.check(hx[guard:guard + n].reshape(T.N_SLOTS, -1), hn[guard:guard + n].reshape(T.N_SLOTS, -1), d.ref_x, d.ref_nv, DP.derive_host(M // 12, S),
            f"guarded M={M} S={S}")
    # a single slot: the launch ends with the buffer
    xbuf.fill_(complex(-5.0, 7.0))
    nbuf.fill_(-3.0)
    m = S * M
    _run(tp, d.x_hat[:1], d.nvar[:1], out=xbuf[guard:guard + m].view(1, -1), nvar_out=nbuf[guard:guard + m].view(1, -1))
    hx, hn = xbuf.cpu().numpy(), nbuf.cpu().numpy()
    assert np.all(hx[guard + m:] == np.complex64(complex(-5.0, 7.0))) and np.all(hn[guard + m:] == np.float32(-3.0))
    assert np.all(hx[:guard] == np.complex64(complex(-5.0, 7.0))) and np.all(hn[:guard] == np.float32(-3.0))
    assert np.all(hn[guard:guard + m] > 0)


def test_argument_errors():
    M, S = 24, 3
    d = T.inputs(M, S)
    tp = _tp(M, S)
    dev, B, n = _dev(), T.N_SLOTS, S * M
    xh, nv = _t(d.x_hat), _t(d.nvar)
    good_x, good_n = tp(xh, nv)
    off_x = torch.empty((B * n + 1,), dtype=torch.complex64, device=dev)[1:].view(B, n).copy_(xh)          # 8 bytes off
    off_n = torch.empty((B * n + 1,), dtype=torch.float32, device=dev)[1:].view(B, n).copy_(nv)            # 4 bytes off
    big = torch.zeros((B * n + 2,), dtype=torch.complex64, device=dev)
    big[:B * n] = xh.reshape(-1)
    bign = torch.zeros((B * n + 4,), dtype=torch.float32, device=dev)
    bign[:B * n] = nv.reshape(-1)
    bad_calls = [
        dict(x_hat=xh.to(torch.complex128)), dict(x_hat=nv), dict(nvar=nv.double()), dict(nvar=xh),               # wrong dtype
        dict(x_hat=xh[:, :-1]), dict(x_hat=xh[:, :-12].contiguous()), dict(x_hat=xh.view(B, S, M)), dict(x_hat=xh.reshape(-1)),   # wrong shape
        dict(x_hat=xh.view(B, n // 2, 2)), dict(nvar=nv[:2]), dict(nvar=nv.view(B, S, M)),
        dict(x_hat=xh.cpu()), dict(nvar=nv.cpu()), dict(x_hat=d.x_hat), dict(nvar=None),                          # CPU tensor, not a tensor
        dict(x_hat=torch.zeros((B, 2 * n), dtype=torch.complex64, device=dev)[:, ::2]),                          # not dense
        dict(x_hat=off_x), dict(nvar=off_n), dict(out=off_x), dict(nvar_out=off_n),                              # misaligned
        dict(out=good_x.to(torch.complex128)), dict(out=good_x[:, :-1]), dict(out=good_x.cpu()), dict(out=good_x[:2]), dict(out=good_x[:, :, None]),
        dict(nvar_out=good_n.double()), dict(nvar_out=good_n[:2]), dict(nvar_out=good_n.cpu()),
        dict(x_hat=big[:B * n].view(B, n), out=big[2:].view(B, n)),                                               # overlapping, not identical
        dict(nvar=bign[:B * n].view(B, n), nvar_out=bign[4:].view(B, n)),
        dict(out=good_x, nvar_out=good_x.view(torch.float32)[:, :n]),                                            # (not dense: refused as such)
        dict(nvar_out=xh.view(torch.float32).reshape(-1)[:B * n].view(B, n)),                                     # nvar_out inside x_hat
    ]
    for kw in bad_calls:
        args = dict(x_hat=xh, nvar=nv, out=None, nvar_out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            tp(args["x_hat"], args["nvar"], out=args["out"], nvar_out=args["nvar_out"])
    with pytest.raises(ValueError, match="16-byte"):
        tp(off_x, nv)
    with pytest.raises(ValueError, match="overlaps"):
        tp(big[:B * n].view(B, n), nv, out=big[2:].view(B, n))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        DP.PuschTransformDeprecoder(2, 3, device="cpu")(xh, nv)
    # the library refuses what the Python checks would have caught
    lib, h = tp._lib, tp._plan()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.ce_tp_deprecode(h, p(off_x), p(nv), B, p(good_x), p(good_n), None) == -1
    assert lib.ce_tp_deprecode(h, p(xh), p(off_n), B, p(good_x), p(good_n), None) == -1
    assert lib.ce_tp_deprecode(h, p(xh), p(nv), B, p(off_x), p(good_n), None) == -1
    assert lib.ce_tp_deprecode(h, p(xh), p(nv), B, p(good_x), p(off_n), None) == -1
    assert lib.ce_tp_deprecode(h, p(xh), p(nv), -1, p(good_x), p(good_n), None) == -1
    assert lib.ce_tp_deprecode(h, None, p(nv), B, p(good_x), p(good_n), None) == -1
    info = DP._lib.TpInfo()
    assert lib.ce_tp_plan_get_info(h, C.byref(info)) == 0 and (info.m_sc, info.n_symbols, info.bytes_per_slot) == (M, S, S * M * 24)
    torch.cuda.synchronize()
    T.check(good_x.cpu().numpy(), good_n.cpu().numpy(), d.ref_x, d.ref_nv, DP.derive_host(M // 12, S), "after the refusals")


def test_empty_batch_launches_nothing():
    dev = _dev()
    tp = _tp(60, 3)
    x, nv = tp(torch.empty((0, 180), dtype=torch.complex64, device=dev), torch.empty((0, 180), dtype=torch.float32, device=dev))
    assert tuple(x.shape) == tuple(nv.shape) == (0, 180) and x.dtype == torch.complex64 and nv.dtype == torch.float32
    x, nv = tp(torch.empty((0, 180, 1), dtype=torch.complex64, device=dev), torch.empty((0, 180, 1), dtype=torch.float32, device=dev))
    assert tuple(x.shape) == (0, 180)
    assert tp._lib.ce_tp_deprecode(tp._plan(), None, None, 0, None, None, None) == 0


def _eq(hops, n_layers=1, n_prb_grid=52, mask=0xFFF):
    case = S.case_spec("tp_for_equalizer", n_prb_grid, hops, n_layers=n_layers)
    h1, h2, _ = S.numpy_hops(case)
    return EQ.PuschEqualizer(h1, h2, n_layers, n_prb_grid, reserved_re_mask=mask, device=_dev())


def test_for_equalizer_on_real_equalizers():
    dev = _dev()
    one = _eq([S.hop_spec([2, 11], 10, 6)])
    two = _eq([S.hop_spec([2], 4, 6, start_symbol=0, n_alloc=7), S.hop_spec([9], 30, 6, start_symbol=7, n_alloc=7)])
    for eq, n_sym in ((one, 12), (two, 12)):
        tp = DP.PuschTransformDeprecoder.for_equalizer(eq)
        assert (tp.n_prbs, tp.n_symbols, tp.m_sc) == (6, n_sym, 72) and eq.n_data_re == n_sym * 72
        # the rows are whole symbols, subcarrier ascending
        re = eq.data_re().reshape(n_sym, 72, 2)
        assert np.all(re[:, :, 0] == re[:, :1, 0]) and np.all(np.diff(re[:, :, 1], axis=1) == 1)
    # the equalizer's own tensors go straight in: a flat channel of gain 2 on one port, noise 0.04 -> nvar = 0.01 on every RE
    d = T.draw(72, 12, B=2, seed=5)
    y = T.precode(d.x_tx, 72)
    rx = torch.zeros((2, 1, 12 * 52, 14), dtype=torch.complex64, device=dev)
    re = one.data_re()
    rx[:, 0, re[:, 1], re[:, 0]] = _t(2.0 * y).to(torch.complex64)
    ch = torch.full((2, 1, 12 * 52, 14, 1), 2.0, dtype=torch.complex64, device=dev)
    x_hat, nvar = one(rx, ch, torch.full((2, 1), 0.04, dtype=torch.float64, device=dev))
    assert tuple(x_hat.shape) == (2, 12 * 72, 1)
    x, nv = DP.PuschTransformDeprecoder.for_equalizer(one)(x_hat, nvar)
    torch.cuda.synchronize()
    assert np.abs(x.cpu().numpy() - d.x_tx).max() <= 1e-5 and np.allclose(nv.cpu().numpy(), 0.01, rtol=1e-5)
    for bad in (_eq([S.hop_spec([2, 11], 10, 6)], n_layers=2),                                                    # two layers
                _eq([S.hop_spec([2, 11], 10, 6)], mask=0x555),                                                   # data on the DM-RS symbols
                _eq([S.hop_spec([2, 11], 10, 7)]),                                                               # 7 PRB
                _eq([S.hop_spec([2], 4, 6, start_symbol=0, n_alloc=7), S.hop_spec([9], 30, 12, start_symbol=7, n_alloc=7)])):   # unequal hops
        with pytest.raises(ValueError):
            DP.PuschTransformDeprecoder.for_equalizer(bad)


def test_chain_into_the_demapper_and_rate_recovery():
    """The CPU chain's inputs on the device: PuschTransformDeprecoder -> PuschDemapper("16qam", descramble=True) ->
    PuschRateRecovery; the hard decision at every transmitted position is the bit sent."""
    dev = _dev()
    d = T.chain_inputs()
    tp = DP.PuschTransformDeprecoder(T.CHAIN_PRBS, T.CHAIN_SYMBOLS, device=dev)
    x, nv = _run(tp, d.x_hat, d.nvar)
    T.check(x.cpu().numpy(), nv.cpu().numpy(), d.ref_x, d.ref_nv, DP.derive_host(T.CHAIN_PRBS, T.CHAIN_SYMBOLS), "chain")
    dem = DM.PuschDemapper("16qam", d.S * d.M, descramble=True, device=dev)
    llr = dem(x, nv, rnti=T.CHAIN_RNTI, n_id=T.CHAIN_N_ID)
    A, bg, rv = 8424, 1, 0
    rm = RM.PuschRateRecovery(bg, A, "16qam", 1, dem.n_bits, dtype=torch.float32, filler_llr=55.25, device=dev)
    der = R.derive(bg, A, 4, 1, dem.n_bits)
    assert dem.n_bits == len(d.bits) == 14400 and rm.n_code_blocks == der.C == 1 and max(rm.e) <= der.P
    soft = rm(llr, rv)
    torch.cuda.synchronize()
    got_llr = llr.cpu().numpy()
    assert np.array_equal((got_llr[0] < 0).astype(np.uint8), d.bits) and np.all(got_llr != 0)
    got = soft[0].cpu().numpy()
    blk, pos, _ = R.slot_map(der, rv)
    sent = np.zeros((der.C, der.N_cb), bool)
    hit = np.zeros((der.C, der.N_cb), bool)
    sent[blk, pos] = d.bits.astype(bool)
    hit[blk, pos] = True
    assert hit.sum() == len(d.bits) and np.array_equal(got[hit] < 0, sent[hit])
    assert np.array_equal(got[blk, pos], got_llr[0])
