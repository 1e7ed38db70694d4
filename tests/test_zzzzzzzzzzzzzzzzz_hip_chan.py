"""GPU tests of the time-domain channel emulator (include/ce_tp.h `ce_chan_apply`, `PuschChannelEmulator`): every case of
chan_oracle.CASES against the float64 operator under the rule of tests/chan_oracle.py, with C_CHAN re-measured; the identity;
sigma = 0 against no noise; bitwise independence of a row from its batch and of the noise from everything but (seed, slot, port,
sample); the write set (a strided `out` inside a pattern-filled stream, in both nestings); the read set (x inside a NaN-filled
stream); containment of a NaN in the K samples behind it; a side stream, an empty batch, `out=`; every refusal of the entry
point and of the wrapper with the output unchanged; and the loop that never leaves the device: PuschTransportEncoder ->
PuschModulator (-> PuschTransformPrecoder) -> PuschOfdmModulator -> PuschChannelEmulator -> PuschOfdmDemodulator -> estimate ->
PuschEqualizer (-> PuschTransformDeprecoder) -> PuschDemapper -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock.

The file's name sorts it behind test_zzzzzzzzzzzzzzzz_hip_dmrs_lp.py: every earlier GPU test keeps its place in the run."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chan_oracle as X
import loop_chain
import mod_oracle as MO
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, channel as CH, ofdm as OF

pytestmark = pytest.mark.gpu

FILL = np.complex64(complex(-5.0, 7.0))      # the pattern of a stream the emulator writes into


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)                         # one word per complex64 element: the shape stays


def _emu(d):
    c = d.c
    return CH.PuschChannelEmulator(c["P"], c["R"], c["K"], device=_dev())


def _params(d, slots=None):
    """The keyword arguments of a case: scalars stay host values, arrays become device tensors (phase0's 32 bits as int32);
    `slots`: only these slots' values."""
    kw = dict(seed=d.seed, first_slot=d.first_slot)
    pick = (lambda a: a) if slots is None else (lambda a: a[slots])
    if d.fcw is not None:
        if isinstance(d.fcw, np.ndarray):
            kw.update(cfo=_t(pick(d.fcw)), phase0=_t(pick(d.phase0).view(np.int32)))
        else:
            kw.update(cfo=d.fcw, phase0=d.phase0)
    if d.sigma is not None:
        kw["sigma"] = _t(pick(d.sigma)) if isinstance(d.sigma, np.ndarray) else d.sigma
    return kw


def _run(emu, x, h, **kw):
    y = emu(_t(x) if isinstance(x, np.ndarray) else x, _t(h) if isinstance(h, np.ndarray) else h, **kw)
    torch.cuda.synchronize()
    return y


def _case_run(name, **over):
    d = X.inputs(name)
    kw = _params(d)
    kw.update(over)
    return d, _run(_emu(d), d.x, d.h, **kw)


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_cases_against_the_float64_oracle(name):
    d, y = _case_run(name)
    c = d.c
    assert tuple(y.shape) == (c["B"], c["R"], c["T"]) and y.dtype == torch.complex64 and y.device == _dev() and y.is_contiguous()
    X.check(y.cpu().numpy(), d, name)


def test_c_chan_is_the_recorded_value():
    """C_CHAN of the rule, the device against the float64 oracle over every case, printed per case: above C_CHAN_RECORDED or
    below a quarter of it fails."""
    worst = max(X.check(_case_run(name)[1].cpu().numpy(), X.inputs(name), name) for name in X.CASE_NAMES)
    print(f"C_CHAN (device) = {worst:.2f}  (C_CHAN_RECORDED = {X.C_CHAN_RECORDED:g}, T_CH = {X.T_CH:g})")
    assert X.C_CHAN_RECORDED / 4.0 <= worst <= X.C_CHAN_RECORDED


def test_one_unit_tap_without_cfo_and_noise_is_the_identity_bitwise():
    rng = np.random.default_rng(1)
    for B, R, T in ((3, 4, 2500), (1, 1, 1), (2, 1, 1025)):
        x = (rng.standard_normal((B, 1, T)) + 1j * rng.standard_normal((B, 1, T))).astype(np.complex64)
        y = _run(CH.PuschChannelEmulator(1, R, 1, device=_dev()), x, np.ones((1, R, 1, 1), np.complex64))
        assert np.array_equal(_bits(y), np.broadcast_to(_bits(x), (B, R, T)))


def test_sigma_zero_as_a_tensor_equals_no_noise_bitwise():
    for name in ("t2500_k12_r4", "t1025_k128_p2_r4", "t1023_k2_r4"):
        d, clean = _case_run(name, sigma=None)
        _, zero = _case_run(name, sigma=torch.zeros(d.c["B"], dtype=torch.float32, device=_dev()))
        _, zero_s = _case_run(name, sigma=0.0)
        assert np.array_equal(_bits(zero), _bits(clean)) and np.array_equal(_bits(zero_s), _bits(clean))
        assert not np.array_equal(_bits(_case_run(name)[1]), _bits(clean))       # the case's own sigma does add noise


@pytest.mark.parametrize("name", ["t1025_k128_p2_r4", "t2500_k12_r4", "t1024_k3_p4"])
def test_each_row_of_a_batch_equals_its_own_call(name):
    """The noise of a row is tied to its slot number first_slot + b and its port number r, so: a slot alone with first_slot + b
    and all R ports reproduces its rows; with a one-port h it reproduces row (b, 0) as it is, and every row (b, r) without
    noise; slots and ports in reverse order reproduce the rows without noise."""
    d, want = _case_run(name)
    c = d.c
    B, R, Pn, K = c["B"], c["R"], c["P"], c["K"]
    want = _bits(want)
    clean = _bits(_case_run(name, sigma=None)[1])
    emu, one = _emu(d), CH.PuschChannelEmulator(Pn, 1, K, device=_dev())
    for b in range(B):
        hb = d.h[b:b + 1] if d.h.shape[0] > 1 else d.h
        kw = _params(d, slice(b, b + 1))
        kw["first_slot"] = d.first_slot + b
        assert np.array_equal(_bits(_run(emu, d.x[b:b + 1], hb, **kw))[0], want[b]), b
        assert np.array_equal(_bits(_run(one, d.x[b:b + 1], hb[:, :1], **kw))[0, 0], want[b, 0]), b
        kw["sigma"] = None
        for r in range(R):
            assert np.array_equal(_bits(_run(one, d.x[b:b + 1], hb[:, r:r + 1], **kw))[0, 0], clean[b, r]), (b, r)
    rev = slice(None, None, -1)
    kw = _params(d, rev)
    kw["sigma"] = None
    y = _run(emu, d.x[::-1], d.h[::-1, ::-1], **kw)
    assert np.array_equal(_bits(y)[::-1, ::-1], clean)


def test_the_noise_depends_on_seed_slot_port_and_sample_only():
    d = X.inputs("t2500_k12_r4")
    c = d.c
    B, R, T = c["B"], c["R"], c["T"]
    emu = _emu(d)
    h_same = np.ascontiguousarray(np.broadcast_to(d.h[:, :1], d.h.shape))                          # every rx port sees the same channel
    kw = _params(d)
    kw.pop("cfo"), kw.pop("phase0")
    a = _run(emu, d.x, h_same, **kw)
    assert np.array_equal(_bits(a), _bits(_run(emu, d.x, h_same, **kw)))                             # the same seed twice
    clean = _run(emu, d.x, h_same, **dict(kw, sigma=None)).cpu().numpy().astype(np.complex128)
    na = (a.cpu().numpy() - clean) / d.sigma
    for b in range(B):                                                                              # ... and it is the oracle's noise
        for r in range(R):
            assert np.abs(na[b, r] - X.noise_ref(d.seed, d.first_slot + b, r, T)).max() < 1e-4, (b, r)
    others = [dict(kw, seed=d.seed + 1), dict(kw, seed=d.seed ^ (1 << 40)), dict(kw, first_slot=d.first_slot + 1), dict(kw, first_slot=d.first_slot + (1 << 32))]
    for o in others:
        nb = (_run(emu, d.x, h_same, **o).cpu().numpy() - clean) / d.sigma
        assert np.abs(nb - na).mean() > 0.5, o                                                     # independent noise: E |n - n'| ~ 1.25
    shifted = (_run(emu, d.x, h_same, **dict(kw, first_slot=d.first_slot + 1)).cpu().numpy() - clean) / d.sigma
    assert np.abs(shifted[:-1] - na[1:]).max() < 1e-4                                               # slot b of first_slot + 1 is slot b + 1
    for r in range(1, R):                                                                           # another port, other noise
        assert np.abs(na[:, r] - na[:, 0]).mean() > 0.5
    # not on x, h or the batch: the noise added to another signal is the same
    x2, h2 = d.x[1:2] * np.complex64(0.5j), (h_same[:1] * np.complex64(2.0))
    kw1 = dict(kw, first_slot=d.first_slot + 1)
    n2 = (_run(emu, x2, h2, **kw1).cpu().numpy() - _run(emu, x2, h2, **dict(kw1, sigma=None)).cpu().numpy()) / d.sigma
    assert np.abs(n2[0] - na[1]).max() < 1e-4


@pytest.mark.parametrize("nesting", ["port_inside_slot", "slot_inside_port"])
@pytest.mark.parametrize("name", ["t1025_k128_p2_r4", "t2500_k12_r4", "t1_k128_p2"])
def test_write_set_in_a_strided_stream(name, nesting):
    """`out` as a strided view into a pattern-filled stream with a gap behind every row and guards at both ends: every sample
    of [0, T) of every row carries the dense call's bits, every other element of the stream is unchanged."""
    d, want = _case_run(name)
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], c["T"]
    want = _bits(want)
    lead, tail, gap = 5, 77, 37                                            # an odd first sample: the rows are only 8-byte aligned
    if nesting == "port_inside_slot":
        ps = T + gap
        ss = R * ps + 101
    else:
        ss = T + gap
        ps = B * ss + 101
    n = lead + (B - 1) * ss + (R - 1) * ps + T + tail
    stream = torch.full((n,), complex(FILL), dtype=torch.complex64, device=dev)
    out = stream.as_strided((B, R, T), (ss, ps, 1), lead)
    assert out.data_ptr() % 16 == 8
    y = _run(_emu(d), d.x, d.h, out=out, **_params(d))
    assert y.data_ptr() == out.data_ptr() and tuple(y.shape) == (B, R, T) and y.stride() == out.stride()
    after = stream.cpu().numpy()
    written = np.zeros(n, bool)
    for b in range(B):
        for r in range(R):
            o = lead + b * ss + r * ps
            assert not written[o:o + T].any()
            written[o:o + T] = True
            assert np.array_equal(_bits(after[o:o + T]), want[b, r]), (b, r)
    assert (~written).sum() >= lead + tail + (gap if B * R > 1 else 0)
    assert np.all(_bits(after[~written]) == _bits(np.array([FILL]))[0])    # gaps and guards
    wide = torch.full((B, R, T + 19), complex(FILL), dtype=torch.complex64, device=dev)      # a longer last dimension
    y = _run(_emu(d), d.x, d.h, out=wide, **_params(d))
    w = wide.cpu().numpy()
    assert tuple(y.shape) == (B, R, T) and np.array_equal(_bits(w[:, :, :T]), want) and np.all(_bits(w[:, :, T:]) == _bits(np.array([FILL]))[0])


@pytest.mark.parametrize("name", ["t1025_k128_p2_r4", "t2500_k12_r4", "t1_k128_p2", "t1024_k3_p4", "t1023_k127_r4"])
def test_read_set_x_inside_a_nan_filled_stream(name):
    """x as a view into a NaN-filled stream, NaN before sample 0 and behind sample T - 1 of every row: the output is finite
    everywhere and carries the dense call's bits -- a sample before the row's start is a zero, never a load."""
    d, want = _case_run(name)
    c = d.c
    dev, B, Pn, T = _dev(), c["B"], c["P"], c["T"]
    lead, gap = 131, 139                                                   # more than K - 1 NaNs in front of every row
    ps = T + gap
    ss = Pn * ps + 7
    n = lead + (B - 1) * ss + (Pn - 1) * ps + T + gap
    stream = torch.full((n,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    xv = stream.as_strided((B, Pn, T), (ss, ps, 1), lead)
    xv.copy_(_t(d.x))
    y = _run(_emu(d), xv, d.h, **_params(d)).cpu().numpy()
    assert np.all(np.isfinite(y.view(np.float32))) and np.array_equal(_bits(y), _bits(want))


@pytest.mark.parametrize("name,t0", [("t2500_k12_r4", 1020), ("t2500_k12_r4", 0), ("t1025_k128_p2_r4", 1000), ("t2500_k128_p4_r4", 2047), ("t1025_k1_plain", 1024)])
def test_a_nan_reaches_the_k_samples_behind_it_and_nothing_else(name, t0):
    d, clean = _case_run(name)
    c = d.c
    B, Pn, K, T = c["B"], c["P"], c["K"], c["T"]
    b, p = B - 1, Pn - 1
    x = np.array(d.x)
    x[b, p, t0] = complex(np.nan, 1.0)
    y = _run(_emu(d), x, d.h, **_params(d)).cpu().numpy()
    hit = np.zeros(y.shape, bool)
    hit[b, :, t0:min(t0 + K, T)] = True
    assert np.all((~np.isfinite(y.real) | ~np.isfinite(y.imag))[hit])
    assert np.array_equal(_bits(y)[~hit], _bits(clean)[~hit])


def test_stream_empty_batch_and_out():
    d, want = _case_run("t2500_k12_r4")
    c = d.c
    dev, B, R, Pn, K, T = _dev(), c["B"], c["R"], c["P"], c["K"], c["T"]
    emu, want = _emu(d), _bits(want)
    out = torch.full((B, R, T), float("nan"), dtype=torch.complex64, device=dev)
    y = _run(emu, d.x, d.h, out=out, **_params(d))
    assert y.data_ptr() == out.data_ptr() and np.array_equal(_bits(y), want) and np.array_equal(_bits(out), want)
    e = emu(torch.empty((0, Pn, T), dtype=torch.complex64, device=dev), _t(d.h), **_params(d, slice(0, 0)))      # an empty batch launches nothing
    assert tuple(e.shape) == (0, R, T) and e.dtype == torch.complex64 and e.device == dev
    e = emu(torch.empty((0, Pn, T), dtype=torch.complex64, device=dev), _t(d.h), out=torch.empty((0, R, T + 4), dtype=torch.complex64, device=dev))
    assert tuple(e.shape) == (0, R, T)
    assert emu._lib.ce_chan_apply(3, None, 0, 0, 0, Pn, R, T, None, 0, K, None, 0, None, 0, None, 0, 0, 0, None, 0, 0, None) == 0
    side = torch.cuda.Stream(device=dev)                                   # a non-default stream gives the same bits
    x2, h2, kw = _t(d.x), _t(d.h), _params(d)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y2 = emu(x2, h2, **kw)
    side.synchronize()
    assert np.array_equal(_bits(y2), want)
    assert emu.device == dev and CH.PuschChannelEmulator(Pn, R, K).device is None


def test_refusals_of_the_entry_point_and_the_wrapper():
    d, want = _case_run("t2500_k12_r4")
    c = d.c
    dev, B, R, Pn, K, T = _dev(), c["B"], c["R"], c["P"], c["K"], c["T"]
    emu, lib = _emu(d), _lib.load()
    x, h = _t(d.x), _t(d.h)
    big = torch.zeros((B * Pn * T + B * R * T + 64,), dtype=torch.complex64, device=dev)          # x, then room for y
    big[:B * Pn * T] = x.reshape(-1)
    y = torch.zeros((B * R * T + 8,), dtype=torch.complex64, device=dev)
    fcw, ph0, sg = _t(d.fcw), _t(d.phase0.view(np.int32)), _t(np.full(B, d.sigma, np.float32))
    px, ph, py = big.data_ptr(), h.data_ptr(), y.data_ptr()
    assert B == 3 and R == 4 and Pn == 1 and h.shape[0] == 1

    def call(abi=3, x_ptr=px, xss=Pn * T, xps=T, slots=B, tx=Pn, rx=R, n=T, h_ptr=ph, tss=0, k=K, f=fcw.data_ptr(), p0=ph0.data_ptr(), s=sg.data_ptr(),
             y_ptr=py, yss=R * T, yps=T):
        vp = lambda a: C.c_void_p(a) if a else None
        return lib.ce_chan_apply(abi, vp(x_ptr), xss, xps, slots, tx, rx, n, vp(h_ptr), tss, k, vp(f), 1, vp(p0), 1, vp(s), 1, d.seed, d.first_slot,
                                 vp(y_ptr), yss, yps, None)

    refused = [
        (dict(abi=2), "ABI version 2 != 3"), (dict(slots=-1), "n_slots=-1"), (dict(tx=5), "n_tx=5 outside 1..4"), (dict(k=129), "n_taps=129 outside 1..128"),
        (dict(rx=0), "n_rx=0 must be >= 1"), (dict(n=0), "n_samples=0 must be >= 1"), (dict(x_ptr=0), "null argument"), (dict(y_ptr=0), "null argument"),
        (dict(h_ptr=0), "null argument"), (dict(p0=0), "null argument"), (dict(xss=-1), "strides must be >= 0"), (dict(yps=-T), "strides must be >= 0"),
        (dict(x_ptr=px + 4), "x must be 8-byte aligned"), (dict(y_ptr=py + 4), "y must be 8-byte aligned"), (dict(yss=1 << 60), "exceeds the address space"),
        (dict(tss=R * Pn * K - 1), "is neither 0 nor >="), (dict(yps=T - 1), f"the rows of {T} samples of {B} slots x {R} ports overlap"),
        (dict(yss=0), "overlap"), (dict(yss=T, yps=T), "overlap"), (dict(yss=T, yps=B * T - 1), "overlap"),
        (dict(y_ptr=px), "y overlaps x"), (dict(y_ptr=px + 8 * (B * Pn * T - 1)), "y overlaps x"), (dict(y_ptr=ph), "y overlaps taps"),
        (dict(y_ptr=ph + 8 * (R * Pn * K - 1)), "y overlaps taps"),
    ]
    for kw, text in refused:
        assert call(**kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (kw, _lib.last_error())
    for kw in (dict(slots=1 << 31), dict(slots=1 << 20, rx=1 << 10)):
        assert call(yss=0, yps=0, xss=0, **kw) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error(), kw
    assert call(slots=0) == 0 and call(slots=0, x_ptr=0, y_ptr=0, h_ptr=0) == 0
    torch.cuda.synchronize()
    assert not y.any() and not big[B * Pn * T:].any()                      # nothing was launched
    # what is not refused: y right behind x, and the slots of a port one behind the other
    assert call(y_ptr=px + 8 * B * Pn * T) == 0 and call(yss=T, yps=B * T) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(big[B * Pn * T:B * (Pn + R) * T].view(B, R, T)), _bits(want)) and not big[B * (Pn + R) * T:].any()
    assert np.array_equal(_bits(y[:B * R * T].view(R, B, T).permute(1, 0, 2)), _bits(want)) and not y[B * R * T:].any()
    assert np.array_equal(_bits(big[:B * Pn * T].view(B, Pn, T)), _bits(d.x))                     # x is unchanged
    # ---- the wrapper's argument errors ----
    good_out = torch.zeros((B, R, T), dtype=torch.complex64, device=dev)
    short = torch.zeros((B, R, T), dtype=torch.complex64, device=dev)
    short.untyped_storage().resize_(8 * (B * R * T - 10))
    kw0 = dict(samples=x, taps=h, cfo=fcw, phase0=ph0, sigma=d.sigma, seed=d.seed, first_slot=d.first_slot, out=good_out)
    xy = big[:B * Pn * T].view(B, Pn, T)
    bad_calls = [
        (dict(samples=x.to(torch.complex128)), "samples must be a torch.complex64 tensor"), (dict(samples=x[0]), "samples must be"),
        (dict(samples=x.expand(B, 2, T)), f"samples must be a torch.complex64 tensor \\[slots, {Pn}, >= 1\\]"), (dict(samples=x.cpu()), "samples must be a tensor on"),
        (dict(samples=d.x), "samples must be a tensor on"), (dict(samples=torch.zeros((B, Pn, 2 * T), dtype=torch.complex64, device=dev)[:, :, ::2]), "contiguous last dimension"),
        (dict(taps=h[:, :, :, :-1]), f"taps must be a dense torch.complex64 tensor \\[{B} or 1, {R}, {Pn}, {K}\\]"), (dict(taps=h.expand(2, R, Pn, K)), "taps must be"),
        (dict(taps=h.cpu()), "taps must be"), (dict(taps=h.to(torch.complex128)), "taps must be"), (dict(taps=d.h), "taps must be"),
        (dict(taps=torch.zeros((1, R, Pn, 2 * K), dtype=torch.complex64, device=dev)[..., ::2]), "taps must be a dense"),
        (dict(cfo=1.5), "cfo: expected an int"), (dict(cfo=1 << 31), f"cfo={1 << 31} outside"), (dict(cfo=fcw[:2]), "cfo: a tensor must be int32"),
        (dict(cfo=fcw.to(torch.int64)), "cfo: a tensor must be int32"), (dict(cfo=fcw.cpu()), "cfo: a tensor must be int32"),
        (dict(cfo=5, phase0=-1), "phase0=-1 outside 0..2\\^32-1"), (dict(cfo=5, phase0=1 << 32), "phase0=4294967296 outside"), (dict(phase0=ph0.to(torch.int64)), "phase0: a tensor must be int32"),
        (dict(sigma=-0.5), "sigma=-0.5 must be finite and >= 0"), (dict(sigma=float("nan")), "sigma=nan must be finite"), (dict(sigma=float("inf")), "sigma=inf must be finite"),
        (dict(sigma="1"), "sigma: expected a float"), (dict(sigma=sg[:2]), "sigma: a tensor must be float32"), (dict(sigma=sg.double()), "sigma: a tensor must be float32"),
        (dict(seed=-1), "seed=-1 outside"), (dict(seed=1 << 64), "outside 0..2\\^64-1"), (dict(seed=1.0), "seed=1.0 outside"), (dict(first_slot=1 << 63), "outside the int64 range"),
        (dict(out=good_out.to(torch.complex128)), "out must be a torch.complex64 tensor"), (dict(out=good_out[:, :, :-1]), f"out must be a torch.complex64 tensor \\[{B}, {R}, >= {T}\\]"),
        (dict(out=good_out[:1]), "out must be"), (dict(out=good_out[:, :2]), "out must be"), (dict(out=good_out.cpu()), "out must be"),
        (dict(out=np.zeros((B, R, T), np.complex64)), "out must be"), (dict(out=short), "behind the"),
        (dict(out=good_out[:1, :1].expand(B, R, T)), "overlap"),
        (dict(out=torch.zeros((B * R * T,), dtype=torch.complex64, device=dev).as_strided((B, R, T), (R * (T - 1), T - 1, 1))), "overlap"),
        (dict(samples=xy, out=big[B * Pn * T - 2:B * Pn * T - 2 + B * R * T].view(B, R, T)), "y overlaps x"),
    ]
    for kw, text in bad_calls:
        args = dict(kw0)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            emu(args.pop("samples"), args.pop("taps"), **args)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        CH.PuschChannelEmulator(Pn, R, K, device="cpu")(x, h)
    torch.cuda.synchronize()
    assert not good_out.any()                                               # none of the refused calls wrote
    X.check(_run(emu, x, h, **_params(d)).cpu().numpy(), d, "after the refusals")


LOOP_N, LOOP_SCS, LOOP_ADVANCE, LOOP_F0 = 512, 30e3, 18, 10e3
# the geometry of the samples loop of test_zzzzzzzzzzzz_hip_ofdm.py: four ports, four integer delays each inside min cp_len - a = 36 - 18 samples
LOOP_DELAYS, LOOP_AMPS = (0, 2, 5, 11), (1.0, 0.35, 0.2, 0.1)


def test_the_loop_through_the_emulator_returns_the_transport_block():
    """loop_chain.build -> loop_chain.modulate (as it is, and through PuschTransformPrecoder.grid_) -> PuschOfdmModulator ->
    PuschChannelEmulator (one tx port, four rx ports, 12 taps) -> PuschOfdmDemodulator -> loop_chain.receive on the bg2_z7_rep
    geometry (24-PRB grid, N = 512, 30 kHz, 7680 samples per slot), no host copy between modulator and demodulator.  Without
    noise and at 40 dB the transport block sent comes back with tb_status 0, both ways; at -40 dB every slot fails (far beyond
    what four ports and a rate-1/12 code recover; the CRC16 passes a wrong block once in 65536).  Without noise the
    emulator's output is np.convolve of the downloaded samples under the rule."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    B, N, a = ch.B, LOOP_N, LOOP_ADVANCE
    cp = OF.nr_cp_lengths(LOOP_SCS, N)
    assert ch.case["scs"] == LOOP_SCS and ch.n_prb_grid == 24 and OF.min_fft_size(ch.n_prb_grid) == N and max(LOOP_DELAYS) < min(cp) - a and ch.L == 1
    dem = OF.PuschOfdmDemodulator(N, ch.n_prb_grid, cp, window_advance=a, sym_phasor=OF.nr_symbol_phasors(LOOP_F0, LOOP_SCS, N, cp), device=dev)
    ofdm = OF.PuschOfdmModulator.for_demodulator(dem)
    K = max(LOOP_DELAYS) + 1
    emu = CH.PuschChannelEmulator(1, MO.LOOP_PORTS, K, device=dev)
    rng = np.random.default_rng(82)
    gains = np.array(LOOP_AMPS)[None] * np.exp(2j * np.pi * rng.random((MO.LOOP_PORTS, len(LOOP_DELAYS))))
    h = np.zeros((1, MO.LOOP_PORTS, 1, K), np.complex64)
    for r in range(MO.LOOP_PORTS):
        h[0, r, 0] = CH.taps_from_delays(LOOP_DELAYS, gains[r], 1.0, K)         # delays in samples: integers, so unit taps
    assert np.count_nonzero(h) == MO.LOOP_PORTS * len(LOOP_DELAYS)
    taps = _t(h)
    for precode in (False, True):
        tx = loop_chain.modulate(ch)
        if precode:
            tx = ch.pre.grid_(tx)
        samples = ofdm(tx)
        assert tuple(samples.shape) == (B, 1, 7680) and samples.device == dev
        rms = float(samples.abs().pow(2).mean().sqrt())
        rx = emu(samples, taps)
        out, tb_status = loop_chain.receive(ch, dem(rx), deprecode=precode)
        assert np.array_equal(out, ch.sent) and not tb_status.any(), ("no noise", precode, tb_status.tolist())
        x_host = samples.cpu().numpy()
        ref, A, n = X.apply_ref(x_host, h)
        X.check(rx.cpu().numpy(), SimpleNamespace(ref=ref, A=A, n=n, sigma=None, c=dict(P=1, K=K)), f"loop, precode={precode}")
        out, tb_status = loop_chain.receive(ch, dem(emu(samples, taps, sigma=0.01 * rms, seed=11, first_slot=MO.LOOP_SLOT)), deprecode=precode)
        assert np.array_equal(out, ch.sent) and not tb_status.any(), ("40 dB", precode, tb_status.tolist())
        out, tb_status = loop_chain.receive(ch, dem(emu(samples, taps, sigma=100.0 * rms, seed=11, first_slot=MO.LOOP_SLOT)), deprecode=precode)
        assert np.all(tb_status[:, 0] != 0), ("-40 dB", precode, tb_status.tolist())
