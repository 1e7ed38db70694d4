"""GPU tests of the OFDM demodulator (include/ce_tp.h `ce_ofdm_demodulate`, `PuschOfdmDemodulator`): every case of
ofdm_oracle.CASES against the float64 oracle `demodulate_ref` under the rule of tests/ofdm_oracle.py; bitwise independence
of a (slot, port) from its batch; the window advance on an oracle-modulated signal behind a channel; the read set (NaN
everywhere outside the windows) and the write set (a NaN-prefilled output between guards); a view into a longer capture,
`out=`, an empty batch, a side stream; containment of a NaN in its window's row; every refusal of the C entry point that
needs a plan and of the wrapper; and the loop from SAMPLES on the device through every stage the project has:
PuschTransportEncoder -> PuschModulator (-> PuschTransformPrecoder) -> ofdm_oracle.modulate and a time-domain channel on the
CPU -> PuschOfdmDemodulator -> estimate -> PuschEqualizer (-> PuschTransformDeprecoder) -> PuschDemapper -> PuschRateRecovery
-> PuschLdpcDecoder -> PuschTransportBlock.

The file's name sorts it behind test_zzzzzzzzzzz_hip_precode.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import loop_chain
import mod_oracle as MO
import ofdm_oracle as O
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, ofdm as OF

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype, device=_dev())      # a dense copy: the shared inputs are read-only


def _dem(d, **kw):
    c = d.c
    args = dict(n_sym=c["n_sym"], window_advance=c["advance"], sym_phasor=d.phi, device=_dev())
    args.update(kw)
    return OF.PuschOfdmDemodulator(c["n_fft"], c["n_prb_grid"], d.cp, **args)


def _run(dem, s, **kw):
    y = dem(_t(s) if isinstance(s, np.ndarray) else s, **kw)
    torch.cuda.synchronize()
    return y


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)                         # one word per complex64 element: the shape stays


# one case per launch geometry: 4 rows per workgroup (the last workgroup half empty), 2 (one row inactive; 7 full ones), 1
GEOMETRIES = ["n128_p10_15k_a4", "n512_p24_s1", "n512_p24_120k_slot1", "n2048_p106_15k"]


@pytest.mark.parametrize("name", O.CASE_NAMES)
def test_shapes_against_the_oracle(name):
    d = O.inputs(name)
    c = d.c
    dem = _dem(d)
    y = _run(dem, d.samples)
    assert tuple(y.shape) == (c["B"], c["R"], d.n_sc, c["n_sym"]) and y.dtype == torch.complex64 and y.device == _dev()
    assert y.permute(0, 1, 3, 2).is_contiguous()                            # the estimator's fast layout
    assert dem.n_samples == d.T and (dem.n_fft, dem.n_sc) == (c["n_fft"], d.n_sc)
    O.check(y.cpu().numpy(), d.ref, d.rms, c["n_fft"], name)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_each_slot_and_port_of_a_batch_equals_its_own_call(name):
    d = O.inputs(name)
    c = d.c
    dem = _dem(d)
    want = _bits(_run(dem, d.samples))
    for b in range(c["B"]):
        for r in range(c["R"]):
            assert np.array_equal(_bits(_run(dem, d.samples[b:b + 1, r:r + 1]))[0, 0], want[b, r]), (b, r)
    # a row's result does not depend on its place: slots and ports in reverse order
    assert np.array_equal(_bits(_run(dem, d.samples[::-1, ::-1]))[::-1, ::-1], want)


def test_window_advance_on_a_modulated_signal_behind_a_channel():
    d = O.advance_inputs()
    assert d.a == 9 and len(d.taps) - 1 < min(d.cp) - d.a
    got = {}
    for a in (0, d.a):
        dem = OF.PuschOfdmDemodulator(d.N, d.n_prb, d.cp, window_advance=a, sym_phasor=d.phi, device=_dev())
        y = _run(dem, d.samples).cpu().numpy()
        rms = O.window_rms(d.samples, d.N, d.cp, a)
        O.check(y, O.demodulate_ref(d.samples, d.N, d.n_prb, d.cp, a, d.phi), rms, d.N, f"advance a={a}")
        O.check(y, d.hx, rms, d.N, f"advance a={a} against H X")          # the transmitted grid through the channel, from either window
        got[a] = y
    assert not np.array_equal(_bits(got[0]), _bits(got[d.a]))               # two different windows indeed


@pytest.mark.parametrize("name", GEOMETRIES)
def test_read_set_and_write_set(name):
    d = O.inputs(name)
    c = d.c
    dev, B, R, T, N = _dev(), c["B"], c["R"], d.T, c["n_fft"]
    dem = _dem(d)
    want = _bits(_run(dem, d.samples))
    # ---- read set: a strided capture whose every sample outside the windows is NaN, against the same with zeros there ----
    ps, ss, lead = T + 37, R * (T + 37) + 101, 5
    w, _ = O.geometry(N, d.cp, c["advance"])
    inside = np.zeros(T, bool)
    for w_l in w:
        inside[w_l:w_l + N] = True
    assert 0 < (~inside).sum() == T - c["n_sym"] * N
    runs = {}
    for fill in (np.nan, 0.0):
        host = np.full(lead + B * ss, complex(fill, fill), np.complex64)
        for b in range(B):
            for r in range(R):
                o = lead + b * ss + r * ps
                host[o:o + T][inside] = d.samples[b, r][inside]
        cap = torch.as_tensor(host, device=dev)
        s = cap.as_strided((B, R, T), (ss, ps, 1), lead)
        assert s.data_ptr() % 16 == 8                                       # the rows are only 8-byte aligned
        runs[fill != 0.0] = _run(dem, s).cpu().numpy()
    assert np.all(np.isfinite(runs[True])) and np.array_equal(_bits(runs[True]), _bits(runs[False]))
    assert np.array_equal(_bits(runs[True]), want)
    # ---- write set: a NaN-prefilled output between guards; every element is written, the guards are untouched ----
    n, guard, fill = B * R * c["n_sym"] * d.n_sc, 64, complex(-5.0, 7.0)
    buf = torch.full((n + 2 * guard,), complex(np.nan, np.nan), dtype=torch.complex64, device=dev)
    buf[:guard] = fill
    buf[guard + n:] = fill
    out = buf[guard:guard + n].view(B, R, c["n_sym"], d.n_sc)
    y = _run(dem, d.samples, out=out)
    assert y.data_ptr() == out.data_ptr() and tuple(y.shape) == (B, R, d.n_sc, c["n_sym"])
    after = buf.cpu().numpy()
    assert np.all(after[:guard] == np.complex64(fill)) and np.all(after[guard + n:] == np.complex64(fill))
    assert np.all(np.isfinite(after[guard:guard + n])) and np.array_equal(_bits(y), want)


def test_strided_input_out_empty_batch_and_stream():
    d = O.inputs("n128_p10_15k_a4")
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], d.T
    dem = _dem(d)
    want = _bits(_run(dem, d.samples))
    # a view into a longer capture: port stride != T, an odd first sample
    cap = torch.zeros((B, R, T + 500), dtype=torch.complex64, device=dev)
    cap[:, :, 123:123 + T] = _t(d.samples)
    view = cap[:, :, 123:123 + T]
    assert view.stride() == (R * (T + 500), T + 500, 1) and not view.is_contiguous()
    assert np.array_equal(_bits(_run(dem, view)), want)
    assert np.array_equal(_bits(_run(dem, cap[:, :, 123:])), want)          # more samples than a slot: the tail is not read
    # stride 0 repeats a row
    rep = _run(dem, _t(d.samples)[1:2, 2:3].expand(B, R, T))
    assert all(np.array_equal(_bits(rep)[b, r], want[1, 2]) for b in range(B) for r in range(R))
    # out=
    out = torch.full((B, R, c["n_sym"], d.n_sc), float("nan"), dtype=torch.complex64, device=dev)
    y = _run(dem, d.samples, out=out)
    assert y.data_ptr() == out.data_ptr() and np.array_equal(_bits(y), want) and np.array_equal(_bits(out.permute(0, 1, 3, 2)), want)
    # an empty batch launches nothing
    for shape in ((0, R, T), (B, 0, T), (0, 0, T + 3)):
        e = dem(torch.empty(shape, dtype=torch.complex64, device=dev))
        assert tuple(e.shape) == (shape[0], shape[1], d.n_sc, c["n_sym"]) and e.dtype == torch.complex64
    assert dem._lib.ce_ofdm_demodulate(dem._plan(), None, 0, 0, 0, 0, None, None) == 0
    # a non-default stream gives the same bits
    side = torch.cuda.Stream(device=dev)
    s2 = _t(d.samples)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y2 = dem(s2)
    side.synchronize()
    assert np.array_equal(_bits(y2), want)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_a_nan_stays_in_its_windows_row(name):
    d = O.inputs(name)
    c = d.c
    dem = _dem(d)
    clean = _bits(_run(dem, d.samples))
    b, r, l = c["B"] - 1, 1, c["n_sym"] // 2
    w, _ = O.geometry(c["n_fft"], d.cp, c["advance"])
    s = np.array(d.samples)
    s[b, r, w[l] + 3] = complex(np.nan, 1.0)
    y = _run(dem, s).cpu().numpy()
    row = y[b, r, :, l]
    assert np.all(~np.isfinite(row.real) | ~np.isfinite(row.imag))          # every subcarrier of the symbol
    other = np.ones(y.shape, bool)
    other[b, r, :, l] = False
    assert np.array_equal(_bits(y)[other], clean[other])                    # every other symbol, port and slot, bitwise


def test_refusals_of_the_entry_point_and_the_wrapper():
    d = O.inputs("n128_p10_15k_a4")
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], d.T
    dem = _dem(d)
    s = _t(d.samples)
    good = dem(s)
    want = _bits(good)
    n_out = B * R * c["n_sym"] * d.n_sc
    # ---- the C entry point, with a plan ----
    lib, h = dem._lib, dem._plan()
    big = torch.zeros((B * R * T + n_out + 64,), dtype=torch.complex64, device=dev)
    big[:B * R * T] = s.reshape(-1)
    y = torch.zeros((n_out,), dtype=torch.complex64, device=dev)
    ps_, py = big.data_ptr(), y.data_ptr()

    def call(s_ptr=ps_, ss=R * T, ps=T, slots=B, ports=R, y_ptr=py):
        return lib.ce_ofdm_demodulate(h, C.c_void_p(s_ptr) if s_ptr else None, ss, ps, slots, ports, C.c_void_p(y_ptr) if y_ptr else None, None)

    refused = [
        (dict(ss=-1), f"slot_stride=-1 and port_stride={T} must be >= 0"),
        (dict(ps=-T), f"slot_stride={R * T} and port_stride=-{T} must be >= 0"),
        (dict(y_ptr=py + 8), "out must be 16-byte aligned"),
        (dict(s_ptr=ps_ + 4), "samples must be 8-byte aligned"),
        (dict(y_ptr=ps_), "out overlaps samples"),
        (dict(y_ptr=ps_ + 8 * (B * R * T - 2)), "out overlaps samples"),                       # the last two samples
        (dict(s_ptr=ps_ + 8 * (B * R * T - 1), ss=0, ps=0, y_ptr=ps_ + 8 * (B * R * T - 2 + T)), "out overlaps samples"),   # out starts inside the one row read
        (dict(ss=1 << 60), "exceeds the address space"),
        (dict(ps=1 << 60), "exceeds the address space"),
        (dict(slots=-1), "n_slots=-1"),
        (dict(ports=-2), "n_ports=-2"),
        (dict(s_ptr=0), "null argument"),
        (dict(y_ptr=0), "null argument"),
    ]
    for kw, text in refused:
        assert call(**kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (kw, _lib.last_error())
    for kw in (dict(slots=1 << 31), dict(ports=1 << 31), dict(slots=1 << 16, ports=1 << 14), dict(slots=(1 << 29) + 1, ports=1)):
        assert call(ss=0, ps=0, **kw) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error(), kw
    assert call(slots=0) == 0 and call(ports=0) == 0 and call(slots=0, s_ptr=0, y_ptr=0) == 0   # nothing to launch
    torch.cuda.synchronize()
    assert not y.any() and not big[B * R * T:].any()                        # nothing was launched
    # what is not refused: out right behind the samples read
    assert call(y_ptr=ps_ + 8 * (B * R * T)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(big[B * R * T:B * R * T + n_out].view(B, R, c["n_sym"], d.n_sc).permute(0, 1, 3, 2)), want)
    assert np.array_equal(big[:B * R * T].cpu().numpy(), d.samples.reshape(-1)) and not big[B * R * T + n_out:].any()
    # ---- the wrapper's argument errors ----
    dense = good.permute(0, 1, 3, 2)                                        # the dense [B, R, n_sym, n_sc] buffer
    off = torch.empty((n_out + 1,), dtype=torch.complex64, device=dev)[1:].view(dense.shape)    # 8 bytes off
    short = torch.zeros((B, R, T), dtype=torch.complex64, device=dev)
    short.untyped_storage().resize_(8 * (B * R * T - 10))                   # strides that need more than the tensor holds
    bad_calls = [
        dict(samples=s.to(torch.complex128)), dict(samples=s.real.contiguous()),                                   # wrong dtype
        dict(samples=s[:, :, :-1]), dict(samples=s[0]), dict(samples=s[None]), dict(samples=s.reshape(-1)),         # too short, wrong rank
        dict(samples=torch.zeros((B, R, 2 * T), dtype=torch.complex64, device=dev)[:, :, ::2]),                    # last dimension not contiguous
        dict(samples=s.cpu()), dict(samples=d.samples), dict(samples=None),                                       # CPU tensor, not a tensor
        dict(samples=short),
        dict(out=off), dict(out=good), dict(out=dense.to(torch.complex128)), dict(out=dense[:1]), dict(out=dense.cpu()),
        dict(out=dense[:, :, :, :-1]), dict(out=torch.zeros((B, R, c["n_sym"], 2 * d.n_sc), dtype=torch.complex64, device=dev)[..., ::2]),
        dict(samples=big[:B * R * T].view(B, R, T), out=big[B * R * T - 2:B * R * T - 2 + n_out].view(dense.shape)),   # overlapping
    ]
    for kw in bad_calls:
        args = dict(samples=s, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            dem(args["samples"], out=args["out"])
    with pytest.raises(ValueError, match="16-byte"):
        dem(s, out=off)
    with pytest.raises(ValueError, match="behind the"):
        dem(short)
    with pytest.raises(ValueError, match="out overlaps samples"):
        dem(big[:B * R * T].view(B, R, T), out=big[B * R * T - 2:B * R * T - 2 + n_out].view(dense.shape))
    with pytest.raises(ValueError, match=f"samples must be a torch.complex64 tensor \\[slots, ports, >= {T}\\]"):
        dem(s[:, :, :-1])
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        OF.PuschOfdmDemodulator(c["n_fft"], c["n_prb_grid"], d.cp, device="cpu")(s)
    O.check(_run(dem, s).cpu().numpy(), d.ref, d.rms, c["n_fft"], "after the refusals")


LOOP_N, LOOP_SCS, LOOP_ADVANCE, LOOP_F0 = 512, 30e3, 18, 10e3
# four ports, four integer delays each inside min cp_len - a = 36 - 18 samples (the three-tap profile of mod_oracle.loop_channel
# -- 0, 100 and 300 ns are 0, 1.5 and 4.6 samples at 15.36 MHz -- and a late echo)
LOOP_DELAYS, LOOP_AMPS = (0, 2, 5, 11), (1.0, 0.35, 0.2, 0.1)


def test_the_loop_from_samples_returns_the_transport_block():
    """PuschTransportEncoder -> PuschModulator (PuschDmrs pilots), once as it is and once through PuschTransformPrecoder.grid_
    -> ofdm_oracle.modulate on the CPU with the conjugates of nr_symbol_phasors -> a four-port integer-tap channel by linear
    convolution -> upload -> PuschOfdmDemodulator -> estimate -> PuschEqualizer -> (PuschTransformDeprecoder) -> PuschDemapper
    (descramble, int8) -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock on the bg2_z7_rep geometry (24-PRB grid,
    N = 512, 30 kHz, 7680 samples per slot): the transport block sent comes back with tb_status 0 both ways; a slot whose
    samples are rotated by N / 2 fails alone; a demodulator built without the phasors fails every slot (at f0 = 10 kHz the
    DM-RS symbol 2 and the data symbols 0, 1, 3, 4, 5 differ by 103, 128, 128, 103 and 25 degrees)."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    case, L, n_prb_grid, mod, sent, B = ch.case, ch.L, ch.n_prb_grid, ch.mod, ch.sent, ch.B
    N, a = LOOP_N, LOOP_ADVANCE
    cp = OF.nr_cp_lengths(LOOP_SCS, N)
    assert case["scs"] == LOOP_SCS and n_prb_grid == 24 and OF.min_fft_size(n_prb_grid) == N and max(LOOP_DELAYS) < min(cp) - a
    phi = OF.nr_symbol_phasors(LOOP_F0, LOOP_SCS, N, cp)
    turn = np.angle(phi / phi[2]) / (2 * np.pi)
    assert all(abs(turn[l]) > 0.06 for l in (0, 1, 3, 4, 5)) and sum(abs(turn[l]) > 0.25 for l in (0, 1, 3, 4, 5)) == 4
    ofdm = OF.PuschOfdmDemodulator(N, n_prb_grid, cp, window_advance=a, sym_phasor=phi, device=dev)
    bare = OF.PuschOfdmDemodulator(N, n_prb_grid, cp, window_advance=a, device=dev)
    assert ofdm.n_samples == 7680 and (ofdm.n_sc, ofdm.n_sym) == (mod.n_sc, mod.n_sym) and L == 1
    plain = loop_chain.modulate(ch)
    precoded = ch.pre.grid_(loop_chain.modulate(ch))
    torch.cuda.synchronize()
    rng = np.random.default_rng(82)
    taps = np.zeros((MO.LOOP_PORTS, max(LOOP_DELAYS) + 1), complex)
    taps[:, list(LOOP_DELAYS)] = np.array(LOOP_AMPS)[None] * np.exp(2j * np.pi * rng.random((MO.LOOP_PORTS, len(LOOP_DELAYS))))

    def air(tx):
        """[B, 4, 7680] complex64 on the device: the grid tx [B, 1, n_sc, n_sym] through the oracle's modulator and the channel."""
        s = O.modulate(tx.cpu().numpy()[:, 0], N, cp, phi)                                       # [B, T], float64
        assert s.shape == (B, ofdm.n_samples)
        return _t(np.stack([[np.convolve(s[b], taps[r])[:s.shape[1]] for r in range(MO.LOOP_PORTS)] for b in range(B)]).astype(np.complex64))

    def receive(samples, demodulator, deprecode):
        return loop_chain.receive(ch, demodulator(samples), deprecode=deprecode)

    for tx, deprecode in ((plain, False), (precoded, True)):
        samples = air(tx)
        out, tb_status = receive(samples, ofdm, deprecode)
        assert np.array_equal(out, sent) and not tb_status.any(), (deprecode, tb_status.tolist())
        rotated = samples.clone()
        rotated[0] = torch.roll(samples[0], N // 2, dims=-1)
        out, tb_status = receive(rotated, ofdm, deprecode)
        assert tb_status[0, 0] != 0 and not tb_status[1:].any() and np.array_equal(out[1:], sent[1:]), ("rotated", deprecode, tb_status.tolist())
        out, tb_status = receive(samples, bare, deprecode)
        assert np.all(tb_status[:, 0] != 0), ("no phasors", deprecode, tb_status.tolist())
