"""GPU tests of transform precoding (include/ce_tp.h `ce_tp_precode`, `PuschTransformPrecoder`): dense rows against the
float64 oracle `tp_oracle.precode` under the rule of tests/tpre_oracle.py on every shape of tp_oracle.CASES; bitwise
independence of a slot from its batch; the in-place form; the grid form on four modulator grids with everything but the data
rows bitwise untouched, guard regions included; the chain into the de-precoder; containment of non-finite values in their
row; every refusal of the C entry point that needs a plan, the Python argument errors, an empty batch, a side stream; and the
DFT-s-OFDM loop on the device through every stage the project has:
PuschTransportEncoder -> PuschModulator -> PuschTransformPrecoder -> channel -> estimate -> PuschEqualizer ->
PuschTransformDeprecoder -> PuschDemapper -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock.  What the loop
leans on is asserted from the oracles alone in tests/test_precode.py.

The file's name sorts it behind test_zzzzzzzzzz_hip_chain_fuzz.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import loop_chain
import mod_oracle as MO
import tp_oracle as T
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, deprecode as DP, modulator as MD, precode as PR

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _pre(M, S_):
    return PR.PuschTransformPrecoder(M // 12, S_, device=_dev())


def _run(pre, x, **kw):
    y = pre(_t(x) if isinstance(x, np.ndarray) else x, **kw)
    torch.cuda.synchronize()
    return y


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint64)                                             # one word per complex64 element: the shape stays


@pytest.mark.parametrize("M,S_", T.CASES, ids=[f"m{M}_s{S_}" for M, S_ in T.CASES])
def test_dense_rows_against_the_oracle(M, S_):
    d = P.inputs(M, S_)
    pre = _pre(M, S_)
    y = _run(pre, d.x)
    assert tuple(y.shape) == (T.N_SLOTS, S_ * M) and y.dtype == torch.complex64 and y.device == _dev()
    P.check(y.cpu().numpy(), d.ref, M, f"M={M} S={S_}")
    # the modulation symbols as [B, S M, 1] are the same call
    y3 = _run(pre, _t(d.x)[:, :, None])
    assert tuple(y3.shape) == (T.N_SLOTS, S_ * M) and np.array_equal(_bits(y3), _bits(y))


@pytest.mark.parametrize("M,S_", [(12, 3), (12, 14), (972, 3), (1500, 3)], ids=["rpw4_one_partial", "rpw4_last_partial", "rpw2_last_partial", "rpw1"])
def test_each_slot_of_a_batch_equals_its_own_single_slot_call(M, S_):
    """Every rows-per-workgroup setting the host chooses (4, 2, 1), with a slot's last workgroup not full where rows share one."""
    view = DP.derive_host(M // 12, S_)
    assert view.rows_per_workgroup == {12: 4, 972: 2, 1500: 1}[M] and (S_ % view.rows_per_workgroup != 0 or view.rows_per_workgroup == 1)
    d = P.inputs(M, S_)
    pre = _pre(M, S_)
    want = _bits(_run(pre, d.x))
    for b in range(T.N_SLOTS):
        assert np.array_equal(_bits(_run(pre, d.x[b:b + 1]))[0], want[b]), b
    # a row's result does not depend on its place: the slots in reverse order, and one symbol at a time through the S = 1 plan
    assert np.array_equal(_bits(_run(pre, d.x[::-1]))[::-1], want)
    one = _pre(M, 1)
    for s in (0, S_ - 1):
        assert np.array_equal(_bits(_run(one, d.x[:, s * M:(s + 1) * M])), want[:, s * M:(s + 1) * M]), s


@pytest.mark.parametrize("M,S_", [(24, 3), (972, 14), (3240, 3)])
def test_in_place_equals_out_of_place(M, S_):
    d = P.inputs(M, S_)
    pre = _pre(M, S_)
    want = _bits(_run(pre, d.x))
    x = _t(d.x)
    got = _run(pre, x, out=x)
    assert got is x and np.array_equal(_bits(x), want)
    x3 = _t(d.x)[:, :, None].contiguous()                                   # [B, S M, 1], viewed to 2-D
    _run(pre, x3, out=x3.view(T.N_SLOTS, -1))
    assert np.array_equal(_bits(x3[:, :, 0]), want)
    out = torch.full((T.N_SLOTS, S_ * M), float("nan"), dtype=torch.complex64, device=_dev())
    assert _run(pre, d.x, out=out) is out and np.array_equal(_bits(out), want)


def _grid_mod(d):
    c = d.c
    return MD.PuschModulator(*MO.hops(c), 1, c["case"]["n_prb_grid"], d.qm, n_sym=c["case"]["n_sym"], reserved_re_mask=0xFFF, device=_dev())


@pytest.mark.parametrize("name", P.GRID_NAMES)
def test_grid_form_transforms_the_data_rows_and_nothing_else(name):
    d = P.grid_inputs(name)
    mod = _grid_mod(d)
    pre = PR.PuschTransformPrecoder.for_modulator(mod)
    assert list(pre.row_offsets) == d.offsets and pre.slot_stride == d.stride and pre.m_sc == d.M
    n_sym, n_sc = d.tx.shape[2:]
    n, guard, fill = d.tx.size, 64, complex(-5.0, 7.0)
    buf = torch.full((n + 2 * guard,), fill, dtype=torch.complex64, device=_dev())
    tx = mod(_t(d.g_rows), _t(d.pilots), d.case["beta"], rnti=P.GRID_RNTI, n_id=P.GRID_N_ID, out=buf[guard:guard + n].view(d.B, 1, n_sym, n_sc))
    torch.cuda.synchronize()
    snap = buf.cpu().numpy().copy()
    assert MO.same(snap[guard:guard + n].reshape(d.tx.shape), d.tx)         # the modulator's grid is the oracle's: d.ref is its rows' transform
    assert tuple(tx.shape) == (d.B, 1, n_sc, n_sym) and tx.data_ptr() == buf.data_ptr() + 8 * guard
    got = pre.grid_(tx)
    torch.cuda.synchronize()
    assert got is tx
    after = buf.cpu().numpy()
    P.check(P.take_rows(after[guard:guard + n].reshape(d.tx.shape), d.offsets, d.M), d.ref, d.M, f"grid {name} M={d.M} S={d.S}")
    rows = np.zeros(n + 2 * guard, bool)
    for b in range(d.B):
        for o in d.offsets:
            rows[guard + b * d.stride + o:guard + b * d.stride + o + d.M] = True
    assert rows.sum() == d.B * d.S * d.M and not rows[:guard].any() and not rows[guard + n:].any()
    # DM-RS symbols, REs outside the allocation, symbols in no hop and both guards: bitwise the snapshot's
    assert np.array_equal(_bits(after)[~rows], _bits(snap)[~rows])
    assert np.all(after[:guard] == np.complex64(fill)) and np.all(after[guard + n:] == np.complex64(fill))
    assert (_bits(after)[rows] != _bits(snap)[rows]).mean() > 0.9           # and the rows are transformed indeed
    # a single slot: the launch ends with the buffer
    m = d.stride
    one = buf[guard:guard + m].view(1, 1, n_sym, n_sc)
    one.copy_(_t(d.tx[:1]))
    buf[guard + m:] = fill
    pre.grid_(one.permute(0, 1, 3, 2))
    torch.cuda.synchronize()
    again = buf.cpu().numpy()
    assert np.array_equal(_bits(again[:guard + m]), _bits(after[:guard + m])) and np.all(again[guard + m:] == np.complex64(fill))


@pytest.mark.parametrize("M,S_", [(12, 3), (300, 14), (3240, 3)])
def test_the_de_precoder_undoes_the_precoder(M, S_):
    """x -> precoder -> de-precoder at a constant nvar = 1e-3: the de-precoder's output against `deprecode_ref` of the GPU
    precoder's actual output under the de-precoder's own rule, and within CHAIN_MARGIN of x per axis."""
    d = P.inputs(M, S_)
    y = _run(_pre(M, S_), d.x)
    nvar = torch.full(y.shape, 1e-3, dtype=torch.float32, device=_dev())
    x, nv = DP.PuschTransformDeprecoder(M // 12, S_, device=_dev())(y, nvar)
    torch.cuda.synchronize()
    ref_x, ref_nv = T.deprecode_ref(y.cpu().numpy(), nvar.cpu().numpy(), M)
    T.check(x.cpu().numpy(), nv.cpu().numpy(), ref_x, ref_nv, DP.derive_host(M // 12, S_), f"precoder -> de-precoder M={M} S={S_}")
    dev = x.cpu().numpy().astype(np.complex128) - d.x
    worst = float(max(np.abs(dev.real).max(), np.abs(dev.imag).max()))
    print(f"M={M} S={S_}: largest per-axis distance from the symbol sent {worst:.2e} (CHAIN_MARGIN = {T.CHAIN_MARGIN:.3f})")
    assert worst <= T.CHAIN_MARGIN


@pytest.mark.parametrize("M,S_", [(12, 14), (972, 3), (3240, 3)], ids=["rpw4", "rpw2", "rpw1"])
def test_non_finite_values_stay_in_their_row(M, S_):
    d = P.inputs(M, S_)
    pre = _pre(M, S_)
    clean = _bits(_run(pre, d.x))
    x = np.array(d.x)
    b, r = 1, 1
    x[b, r * M + 3] = complex(np.nan, np.nan)
    x[b, r * M + M - 2] = complex(np.inf, 1.0)
    y = _run(pre, x).cpu().numpy()
    row = y[b, r * M:(r + 1) * M]
    assert np.all(~np.isfinite(row.real) | ~np.isfinite(row.imag))          # every output of the row
    other = np.ones(y.shape, bool)
    other[b, r * M:(r + 1) * M] = False
    assert np.array_equal(_bits(y)[other], clean[other])                    # every other row of the slot and of the batch, bitwise


def test_refusals_empty_batch_and_stream():
    M, S_ = 24, 3
    d = P.inputs(M, S_)
    pre = _pre(M, S_)
    dev, B, n = _dev(), T.N_SLOTS, S_ * M
    x = _t(d.x)
    good = pre(x)
    want = _bits(good)
    # ---- the C entry point, with a plan ----
    lib, h = pre._lib, pre._plan()
    big = torch.zeros((B * n + 64,), dtype=torch.complex64, device=dev)
    big[:B * n] = x.reshape(-1)
    y = torch.zeros((B, n), dtype=torch.complex64, device=dev)
    px, py = big.data_ptr(), y.data_ptr()
    offs = lambda *v: (C.c_int32 * S_)(*v)   # noqa: E731

    def call(x_ptr=px, xs=n, xo=None, y_ptr=py, ys=n, yo=None, slots=B):
        return lib.ce_tp_precode(h, C.c_void_p(x_ptr) if x_ptr else None, xs, xo, C.c_void_p(y_ptr) if y_ptr else None, ys, yo, slots, None)

    refused = [
        (dict(xo=offs(1, 24, 48)), "x_row_offset[0]=1 must be even and >= 0"),
        (dict(yo=offs(0, 25, 48)), "y_row_offset[1]=25 must be even and >= 0"),
        (dict(xs=73), "x_slot_stride=73 must be even and >= 0"),
        (dict(ys=n + 1), "y_slot_stride=73 must be even and >= 0"),
        (dict(ys=-2), "y_slot_stride=-2 must be even and >= 0"),
        (dict(xo=offs(-2, 24, 48)), "x_row_offset[0]=-2 must be even and >= 0"),
        (dict(xo=offs(0, 12, 48)), "x rows 0 and 1 overlap"),
        (dict(yo=offs(48, 0, 26)), "y rows 0 and 2 overlap"),
        (dict(xo=offs(0, 24, 50)), "x_row_offset[2]=50 + M=24 exceeds x_slot_stride=72"),
        (dict(ys=M), "y_row_offset[1]=24 + M=24 exceeds y_slot_stride=24"),
        (dict(x_ptr=px + 8), "x and y must be 16-byte aligned"),
        (dict(y_ptr=py + 8), "x and y must be 16-byte aligned"),
        (dict(y_ptr=px + 16), "y overlaps x"),
        (dict(y_ptr=px + 8 * (B * n - 2)), "y overlaps x"),
        (dict(x_ptr=py + 8 * (B * n - 2)), "y overlaps x"),
        (dict(y_ptr=px, yo=offs(24, 0, 48)), "the in-place form needs the identical geometry"),
        (dict(y_ptr=px, ys=n + 2), "the in-place form needs the identical geometry"),
        (dict(slots=-1), "n_slots=-1"),
        (dict(x_ptr=0), "null argument"),
        (dict(y_ptr=0), "null argument"),
    ]
    for kw, text in refused:
        assert call(**kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (kw, _lib.last_error())
    assert call(slots=1 << 31) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error()
    assert lib.ce_tp_precode(h, None, 0, None, None, 0, None, 0, None) == 0                  # n_slots == 0 launches nothing
    torch.cuda.synchronize()
    assert not y.any() and np.array_equal(big[:B * n].cpu().numpy(), d.x.reshape(-1))        # nothing was launched
    # what is not refused: explicit dense offsets, and the in-place form with them on one side only
    assert call(xo=offs(0, 24, 48), yo=offs(0, 24, 48)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y), want)
    assert call(y_ptr=px, xo=offs(0, 24, 48)) == 0                                           # NULL = dense rows: the identical geometry
    torch.cuda.synchronize()
    assert np.array_equal(_bits(big[:B * n].view(B, n)), want) and not big[B * n:].any()
    info = _lib.TpInfo()
    assert lib.ce_tp_plan_get_info(h, C.byref(info)) == 0 and (info.m_sc, info.n_symbols, info.bytes_per_slot) == (M, S_, S_ * M * 24)
    # ---- the Python argument errors ----
    off = torch.empty((B * n + 1,), dtype=torch.complex64, device=dev)[1:].view(B, n).copy_(x)            # 8 bytes off
    wide = torch.zeros((B * n + 2,), dtype=torch.complex64, device=dev)
    bad_calls = [
        dict(x=x.to(torch.complex128)), dict(x=x.real.contiguous()),                                              # wrong dtype
        dict(x=x[:, :-1]), dict(x=x[:, :-12].contiguous()), dict(x=x.view(B, S_, M)), dict(x=x.reshape(-1)), dict(x=x.view(B, n // 2, 2)),   # wrong shape
        dict(x=x.cpu()), dict(x=d.x), dict(x=None),                                                               # CPU tensor, not a tensor
        dict(x=torch.zeros((B, 2 * n), dtype=torch.complex64, device=dev)[:, ::2]),                              # not dense
        dict(x=off), dict(out=off),                                                                               # misaligned
        dict(out=good.to(torch.complex128)), dict(out=good[:, :-1]), dict(out=good.cpu()), dict(out=good[:2]), dict(out=good[:, :, None]),
        dict(x=wide[:B * n].view(B, n), out=wide[2:].view(B, n)),                                                 # overlapping, not identical
    ]
    for kw in bad_calls:
        args = dict(x=x, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            pre(args["x"], out=args["out"])
    with pytest.raises(ValueError, match="16-byte"):
        pre(off)
    with pytest.raises(ValueError, match="overlaps"):
        pre(wide[:B * n].view(B, n), out=wide[2:].view(B, n))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        PR.PuschTransformPrecoder(2, 3, device="cpu")(x)
    with pytest.raises(ValueError, match="for_modulator"):
        pre.grid_(x)
    g = P.grid_inputs("start2_partial")
    gp = PR.PuschTransformPrecoder.for_modulator(_grid_mod(g))
    n_sym, n_sc = g.tx.shape[2:]
    tx = _t(g.tx).permute(0, 1, 3, 2)
    for bad in (tx.contiguous(), tx.permute(0, 1, 3, 2), tx.to(torch.complex128), tx.cpu(), tx[:, :, :-1], tx[:, :, :, :-1], tx[:, 0], g.tx,
                torch.cat([tx, tx], 1), torch.zeros((g.B, 1, n_sym, n_sc + 1), dtype=torch.complex64, device=dev)[..., 1:].permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match="tx must be"):
            gp.grid_(bad)
    # ---- an empty batch launches nothing ----
    e = pre(torch.empty((0, n), dtype=torch.complex64, device=dev))
    assert tuple(e.shape) == (0, n) and e.dtype == torch.complex64
    assert tuple(pre(torch.empty((0, n, 1), dtype=torch.complex64, device=dev)).shape) == (0, n)
    e = torch.empty((0, 1, n_sym, n_sc), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2)
    assert gp.grid_(e) is e
    # ---- a non-default stream gives the same bits, dense and grid ----
    ref_grid = _bits(gp.grid_(_t(g.tx).permute(0, 1, 3, 2)))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    x2, tx2 = _t(d.x), _t(g.tx).permute(0, 1, 3, 2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y2 = pre(x2)
        gp.grid_(tx2)
    side.synchronize()
    assert np.array_equal(_bits(y2), want) and np.array_equal(_bits(tx2), ref_grid)
    P.check(good.cpu().numpy(), d.ref, M, "after the refusals")


def test_the_dft_s_ofdm_loop_returns_the_transport_block():
    """PuschTransportEncoder -> PuschModulator (PuschDmrs pilots) -> PuschTransformPrecoder.for_modulator(mod).grid_ -> a
    frequency-selective channel on 4 ports (torch ops, no noise) -> estimate -> PuschEqualizer ->
    PuschTransformDeprecoder.for_equalizer(eq) -> PuschDemapper(descramble, int8) -> PuschRateRecovery -> PuschLdpcDecoder ->
    PuschTransportBlock on the bg2_z7_rep geometry: the transport block sent comes back with tb_status 0; a slot whose rnti
    differs between modulator and demapper fails its CRC, and so does every slot when the precoder is skipped."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    pre, tp, sent = ch.pre, ch.tp, ch.sent
    assert ch.mod.n_bits == ch.dem.n_bits == ch.rm.n_bits == ch.enc.n_bits == ch.lp["G"] and ch.mod.g_row_bytes == ch.enc.g_row_bytes
    assert (pre.n_prbs, pre.n_symbols) == (tp.n_prbs, tp.n_symbols) == (4, 5) and pre.n_symbols * pre.m_sc == ch.eq.n_data_re
    plain = loop_chain.modulate(ch)
    tx = pre.grid_(loop_chain.modulate(ch))
    assert torch.equal(tx[:, :, :, 2], plain[:, :, :, 2]) and not torch.equal(tx, plain)          # the DM-RS symbol stays, the data rows do not
    H = torch.as_tensor(MO.loop_channel(ch.case, np.random.default_rng(81)), device=dev)        # [R, n_sc, L]
    wrong = torch.full((ch.B,), MO.LOOP_RNTI, dtype=torch.int32, device=dev)
    wrong[0] += 1

    def receive(grid, rnti):
        return loop_chain.receive(ch, torch.einsum("rkl,blks->brks", H, grid).contiguous(), rnti=rnti, deprecode=True)

    out, tb_status = receive(tx, MO.LOOP_RNTI)
    assert np.array_equal(out, sent) and not tb_status.any(), tb_status.tolist()
    out, tb_status = receive(tx, wrong)
    assert tb_status[0, 0] != 0 and not tb_status[1:].any() and np.array_equal(out[1:], sent[1:]), ("wrong rnti", tb_status.tolist())
    out, tb_status = receive(plain, MO.LOOP_RNTI)
    assert np.all(tb_status[:, 0] != 0), ("precoder skipped", tb_status.tolist())
