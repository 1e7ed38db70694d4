"""GPU tests of the OFDM modulator (include/ce_tp.h `ce_ofdmtx_modulate`, `PuschOfdmModulator`): every case of
ofdm_tx_oracle.CASES against the float64 operator `ofdm_oracle.modulate` under the rule of tests/ofdm_tx_oracle.py; every cyclic
prefix bitwise its symbol's tail; bitwise independence of a (slot, port) from its batch; the write set (a strided `out` inside a
pattern-filled stream, in both nestings); containment of a NaN in its symbol's samples; a side stream, an empty batch, `out=`;
every refusal of the C entry point that needs a plan and of the wrapper; and the loop that never leaves the device:
PuschTransportEncoder -> PuschModulator (-> PuschTransformPrecoder) -> PuschOfdmModulator -> a four-port integer-tap channel of
shifted device tensors -> PuschOfdmDemodulator -> estimate -> PuschEqualizer (-> PuschTransformDeprecoder) -> PuschDemapper ->
PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock.

The file's name sorts it behind test_zzzzzzzzzzzzz_hip_front_fuzz.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import loop_chain
import mod_oracle as MO
import ofdm_oracle as O
import ofdm_tx_oracle as X
import tpre_oracle as P
from srsran_ce_pytorch_amd import _lib, ofdm as OF

pytestmark = pytest.mark.gpu

FILL = np.complex64(complex(-5.0, 7.0))      # the pattern of a stream the modulator writes into


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _grid(a):
    """The device tensor PuschModulator would return for the host grid a [B, R, n_sc, n_sym]: the permuted view of a dense
    [B, R, n_sym, n_sc] buffer (a copy: the shared inputs are read-only)."""
    dense = np.array(np.swapaxes(np.asarray(a), -1, -2), order="C")
    return torch.as_tensor(dense, device=_dev()).permute(0, 1, 3, 2)


def _mod(d, **kw):
    c = d.c
    args = dict(n_sym=c["n_sym"], sym_phasor=d.phi, device=_dev())
    args.update(kw)
    return OF.PuschOfdmModulator(c["n_fft"], c["n_prb_grid"], d.cp, **args)


def _run(mod, g, **kw):
    s = mod(_grid(g) if isinstance(g, np.ndarray) else g, **kw)
    torch.cuda.synchronize()
    return s


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)                         # one word per complex64 element: the shape stays


# one case per launch geometry: 4 rows per workgroup (the last workgroup half empty), 2 (one row inactive; 7 full ones), 1
GEOMETRIES = ["n128_p10_15k_a4", "n512_p24_s1", "n512_p24_120k_slot1", "n2048_p106_15k"]


@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_shapes_against_the_oracle_and_the_prefix_is_the_tail(name):
    d = X.inputs(name)
    c = d.c
    mod = _mod(d)
    s = _run(mod, d.grid)
    assert tuple(s.shape) == (c["B"], c["R"], d.T) and s.dtype == torch.complex64 and s.device == _dev() and s.is_contiguous()
    assert mod.n_samples == d.T and (mod.n_fft, mod.n_sc) == (c["n_fft"], d.n_sc)
    got = s.cpu().numpy()
    X.check(got, d.ref, d.rms, c["n_fft"], name)
    bits, N = _bits(got), c["n_fft"]
    for l, (t, cp) in enumerate(zip(d.starts, d.cp)):                     # the cyclic prefix: the same values stored a second time
        assert np.array_equal(bits[..., t:t + cp], bits[..., t + N:t + N + cp]), (name, l)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_each_slot_and_port_of_a_batch_equals_its_own_call(name):
    d = X.inputs(name)
    c = d.c
    mod = _mod(d)
    want = _bits(_run(mod, d.grid))
    for b in range(c["B"]):
        for r in range(c["R"]):
            assert np.array_equal(_bits(_run(mod, d.grid[b:b + 1, r:r + 1]))[0, 0], want[b, r]), (b, r)
    # a row's result does not depend on its place: slots and ports in reverse order
    assert np.array_equal(_bits(_run(mod, d.grid[::-1, ::-1]))[::-1, ::-1], want)


@pytest.mark.parametrize("nesting", ["port_inside_slot", "slot_inside_port"])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_write_set_in_a_strided_stream(name, nesting):
    """`out` as a strided view into a pattern-filled stream with guards at both ends: every sample of [0, T) of every row
    carries the dense call's bits, every other element of the stream is unchanged."""
    d = X.inputs(name)
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], d.T
    mod = _mod(d)
    want = _bits(_run(mod, d.grid))
    lead, tail = 5, 77                                                     # an odd first sample: the rows are only 8-byte aligned
    if nesting == "port_inside_slot":
        ps = T + 37
        ss = R * ps + 101
    else:                                                                  # one continuous stream per port: slot b right behind slot b - 1
        ss = T
        ps = B * T + 37
    n = lead + (B - 1) * ss + (R - 1) * ps + T + tail
    stream = torch.full((n,), complex(FILL), dtype=torch.complex64, device=dev)
    out = stream.as_strided((B, R, T), (ss, ps, 1), lead)
    assert out.data_ptr() % 16 == 8
    s = _run(mod, d.grid, out=out)
    assert s.data_ptr() == out.data_ptr() and tuple(s.shape) == (B, R, T) and s.stride() == out.stride()
    after = stream.cpu().numpy()
    written = np.zeros(n, bool)
    for b in range(B):
        for r in range(R):
            o = lead + b * ss + r * ps
            assert not written[o:o + T].any()
            written[o:o + T] = True
            assert np.all(np.isfinite(after[o:o + T].view(np.float32))) and np.array_equal(_bits(after[o:o + T]), want[b, r]), (b, r)
    assert (~written).sum() >= lead + tail + (37 if B * R > 1 else 0)
    assert np.all(_bits(after[~written]) == _bits(np.array([FILL]))[0])    # gaps and guards
    # a longer last dimension: only the first T samples of each row are written
    wide = torch.full((B, R, T + 19), complex(FILL), dtype=torch.complex64, device=dev)
    s = _run(mod, d.grid, out=wide)
    assert tuple(s.shape) == (B, R, T) and s.data_ptr() == wide.data_ptr()
    w = wide.cpu().numpy()
    assert np.array_equal(_bits(w[:, :, :T]), want) and np.all(_bits(w[:, :, T:]) == _bits(np.array([FILL]))[0])


@pytest.mark.parametrize("name", GEOMETRIES)
def test_a_nan_stays_in_its_symbols_samples(name):
    d = X.inputs(name)
    c = d.c
    mod = _mod(d)
    clean = _bits(_run(mod, d.grid))
    b, r, l = c["B"] - 1, 1, c["n_sym"] // 2
    g = np.array(d.grid)
    g[b, r, d.n_sc // 3, l] = complex(np.nan, 1.0)
    s = _run(mod, g).cpu().numpy()
    t, n = d.starts[l], d.cp[l] + c["n_fft"]
    hit = s[b, r, t:t + n]
    assert np.all(~np.isfinite(hit.real) | ~np.isfinite(hit.imag))          # exactly the cp_l + N samples of the symbol
    other = np.ones(s.shape, bool)
    other[b, r, t:t + n] = False
    assert np.array_equal(_bits(s)[other], clean[other])                    # every other sample, bitwise


def test_stream_empty_batch_and_out():
    d = X.inputs("n128_p10_15k_a4")
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], d.T
    mod = _mod(d)
    want = _bits(_run(mod, d.grid))
    # out= returns the same storage
    out = torch.full((B, R, T), float("nan"), dtype=torch.complex64, device=dev)
    s = _run(mod, d.grid, out=out)
    assert s.data_ptr() == out.data_ptr() and np.array_equal(_bits(s), want) and np.array_equal(_bits(out), want)
    # an empty batch launches nothing
    for shape in ((0, R), (B, 0), (0, 0)):
        e = mod(torch.empty(shape + (c["n_sym"], d.n_sc), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2))
        assert tuple(e.shape) == shape + (T,) and e.dtype == torch.complex64 and e.device == dev
        e = mod(torch.empty(shape + (c["n_sym"], d.n_sc), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2),
                out=torch.empty(shape + (T + 4,), dtype=torch.complex64, device=dev))
        assert tuple(e.shape) == shape + (T,)
    assert mod._lib.ce_ofdmtx_modulate(mod._plan(), None, 0, 0, None, 0, 0, None) == 0
    # a non-default stream gives the same bits
    side = torch.cuda.Stream(device=dev)
    g2 = _grid(d.grid)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s2 = mod(g2)
    side.synchronize()
    assert np.array_equal(_bits(s2), want)
    # the modulator of a demodulator, and the demodulator returns the grid for any advance inside the prefix
    for a in (0, c["advance"], min(d.cp)):
        dem = OF.PuschOfdmDemodulator(c["n_fft"], c["n_prb_grid"], d.cp, n_sym=c["n_sym"], window_advance=a, sym_phasor=d.phi, device=dev)
        s3 = OF.PuschOfdmModulator.for_demodulator(dem)(g2)
        assert np.array_equal(_bits(s3), want)
        back = dem(s3).cpu().numpy()
        assert np.abs(back - d.grid).max() < 1e-4


def test_refusals_of_the_entry_point_and_the_wrapper():
    d = X.inputs("n128_p10_15k_a4")
    c = d.c
    dev, B, R, T = _dev(), c["B"], c["R"], d.T
    mod = _mod(d)
    g = _grid(d.grid)
    n_grid = B * R * c["n_sym"] * d.n_sc
    # ---- the C entry point, with a plan ----
    lib, h = mod._lib, mod._plan()
    big = torch.zeros((n_grid + B * R * T + 64,), dtype=torch.complex64, device=dev)     # the grid, then room for the samples
    big[:n_grid] = g.permute(0, 1, 3, 2).reshape(-1)
    y = torch.zeros((B * R * T + 8,), dtype=torch.complex64, device=dev)
    pg, py = big.data_ptr(), y.data_ptr()
    assert pg % 16 == 0 and py % 16 == 0 and B == 2 and R == 3

    def call(g_ptr=pg, slots=B, ports=R, s_ptr=py, ss=R * T, ps=T):
        return lib.ce_ofdmtx_modulate(h, C.c_void_p(g_ptr) if g_ptr else None, slots, ports, C.c_void_p(s_ptr) if s_ptr else None, ss, ps, None)

    refused = [
        (dict(ss=-1), f"slot_stride=-1 and port_stride={T} must be >= 0"),
        (dict(ps=-T), f"slot_stride={R * T} and port_stride=-{T} must be >= 0"),
        (dict(g_ptr=pg + 8), "grid must be 16-byte aligned"),
        (dict(s_ptr=py + 4), "samples must be 8-byte aligned"),
        (dict(ss=1 << 60), "exceeds the address space"),
        (dict(ps=1 << 60), "exceeds the address space"),
        # rows that share samples, in either nesting
        (dict(ps=T - 1), f"slot_stride={R * T} and port_stride={T - 1}: the rows of {T} samples of {B} slots x {R} ports overlap"),
        (dict(ss=R * T - 1), "overlap"),
        (dict(ss=0), "overlap"),
        (dict(ps=0), "overlap"),
        (dict(ss=T - 1, ps=B * T), "overlap"),
        (dict(ss=T, ps=B * T - 1), "overlap"),
        (dict(ss=T, ps=T), "overlap"),
        (dict(ss=0, ps=0), "overlap"),
        (dict(slots=1, ss=0, ps=T - 1), "overlap"),
        (dict(ports=1, ss=T - 1, ps=0), "overlap"),
        # samples inside the grid's memory
        (dict(s_ptr=pg), "samples overlaps grid"),
        (dict(s_ptr=pg + 8 * (n_grid - 1)), "samples overlaps grid"),                          # the grid's last element
        (dict(g_ptr=py + 8 * (B * R * T - 2)), "samples overlaps grid"),                       # the grid starts in the last two samples
        (dict(slots=-1), "n_slots=-1"),
        (dict(ports=-2), "n_ports=-2"),
        (dict(g_ptr=0), "null argument"),
        (dict(s_ptr=0), "null argument"),
    ]
    for kw, text in refused:
        assert call(**kw) == _lib.CE_ERR_INVALID and text in _lib.last_error(), (kw, _lib.last_error())
    for kw in (dict(slots=1 << 31), dict(ports=1 << 31), dict(slots=1 << 16, ports=1 << 14), dict(slots=(1 << 29) + 1, ports=1)):
        assert call(ss=0, ps=0, **kw) == _lib.CE_ERR_UNSUPPORTED and "more than 2^31-1 workgroups in one launch" in _lib.last_error(), kw
    assert call(slots=0) == 0 and call(ports=0) == 0 and call(slots=0, g_ptr=0, s_ptr=0) == 0   # nothing to launch
    torch.cuda.synchronize()
    assert not y.any() and not big[n_grid:].any()                          # nothing was launched
    # what is not refused: the samples right behind the grid, and the slots of a port one behind the other
    want = _bits(_run(mod, g))
    assert call(s_ptr=pg + 8 * n_grid) == 0 and call(ss=T, ps=B * T) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(big[n_grid:n_grid + B * R * T].view(B, R, T)), want) and not big[n_grid + B * R * T:].any()
    assert np.array_equal(_bits(y[:B * R * T].view(R, B, T).permute(1, 0, 2)), want) and not y[B * R * T:].any()
    assert np.array_equal(_bits(big[:n_grid].view(B, R, c["n_sym"], d.n_sc).permute(0, 1, 3, 2)), _bits(d.grid))      # the grid is unchanged
    # ---- the wrapper's argument errors ----
    dense = g.permute(0, 1, 3, 2)                                           # the dense [B, R, n_sym, n_sc] buffer
    off = torch.empty((n_grid + 1,), dtype=torch.complex64, device=dev)[1:].view(dense.shape).permute(0, 1, 3, 2)    # 8 bytes off
    short = torch.zeros((B, R, T), dtype=torch.complex64, device=dev)
    short.untyped_storage().resize_(8 * (B * R * T - 10))                   # strides that need more than the tensor holds
    good_out = torch.zeros((B, R, T), dtype=torch.complex64, device=dev)
    bad_calls = [
        dict(grid=g.to(torch.complex128)), dict(grid=g.real.contiguous()),                                          # wrong dtype
        dict(grid=dense), dict(grid=g.contiguous()), dict(grid=g[0]), dict(grid=g[None]), dict(grid=g[:, :, :-12]),    # not the permuted view, wrong rank, wrong n_sc
        dict(grid=g[:, :, :, :-1]), dict(grid=g.cpu()), dict(grid=d.grid), dict(grid=None),                           # wrong n_sym, CPU tensor, not a tensor
        dict(grid=off),
        dict(out=good_out.to(torch.complex128)), dict(out=good_out[:, :, :-1]), dict(out=good_out[:1]), dict(out=good_out[:, :2]),
        dict(out=good_out[0]), dict(out=good_out.cpu()), dict(out=torch.zeros((B, R, 2 * T), dtype=torch.complex64, device=dev)[:, :, ::2]),
        dict(out=np.zeros((B, R, T), np.complex64)), dict(out=short),
        dict(out=good_out[:1, :1].expand(B, R, T)),                                                                 # every row the same memory
        dict(out=torch.zeros((B * R * T,), dtype=torch.complex64, device=dev).as_strided((B, R, T), (R * (T - 1), T - 1, 1))),   # rows that share a sample
        dict(grid=big[:n_grid].view(dense.shape).permute(0, 1, 3, 2), out=big[n_grid - 2:n_grid - 2 + B * R * T].view(B, R, T)),   # overlapping
    ]
    for kw in bad_calls:
        args = dict(grid=g, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            mod(args["grid"], out=args["out"])
    with pytest.raises(ValueError, match="grid must be 16-byte aligned"):
        mod(off)
    with pytest.raises(ValueError, match="behind the"):
        mod(g, out=short)
    with pytest.raises(ValueError, match="overlap"):
        mod(g, out=good_out[:1, :1].expand(B, R, T))
    with pytest.raises(ValueError, match="samples overlaps grid"):
        mod(big[:n_grid].view(dense.shape).permute(0, 1, 3, 2), out=big[n_grid - 2:n_grid - 2 + B * R * T].view(B, R, T))
    with pytest.raises(ValueError, match=f"grid must be a torch.complex64 tensor \\[slots, ports, {d.n_sc}, {c['n_sym']}\\]"):
        mod(dense)
    with pytest.raises(ValueError, match=f"out must be a torch.complex64 tensor \\[{B}, {R}, >= {T}\\]"):
        mod(g, out=good_out[:, :, :-1])
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        OF.PuschOfdmModulator(c["n_fft"], c["n_prb_grid"], d.cp, device="cpu")(g)
    torch.cuda.synchronize()
    assert not good_out.any()                                               # none of the refused calls wrote
    X.check(_run(mod, g).cpu().numpy(), d.ref, d.rms, c["n_fft"], "after the refusals")


LOOP_N, LOOP_SCS, LOOP_ADVANCE, LOOP_F0 = 512, 30e3, 18, 10e3
# the samples loop of test_zzzzzzzzzzzz_hip_ofdm.py: four ports, four integer delays each inside min cp_len - a = 36 - 18 samples
LOOP_DELAYS, LOOP_AMPS = (0, 2, 5, 11), (1.0, 0.35, 0.2, 0.1)


def test_the_loop_without_a_host_round_trip_returns_the_transport_block():
    """PuschTransportEncoder -> PuschModulator (PuschDmrs pilots), once as it is and once through PuschTransformPrecoder.grid_
    -> PuschOfdmModulator (the conjugates of nr_symbol_phasors) -> a four-port integer-tap channel as sums of shifted, scaled
    device tensors -> PuschOfdmDemodulator -> estimate -> PuschEqualizer -> (PuschTransformDeprecoder) -> PuschDemapper
    (descramble, int8) -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock on the bg2_z7_rep geometry (24-PRB grid,
    N = 512, 30 kHz, 7680 samples per slot): the transport block sent comes back with tb_status 0 both ways; a modulator built
    without the phasors, against the demodulator built with them, fails every slot."""
    dev = _dev()
    ch = loop_chain.build(P.LOOP_NAME, dev)
    n_prb_grid, mod, sent, B = ch.n_prb_grid, ch.mod, ch.sent, ch.B
    N, a = LOOP_N, LOOP_ADVANCE
    cp = OF.nr_cp_lengths(LOOP_SCS, N)
    assert ch.case["scs"] == LOOP_SCS and n_prb_grid == 24 and OF.min_fft_size(n_prb_grid) == N and max(LOOP_DELAYS) < min(cp) - a
    phi = OF.nr_symbol_phasors(LOOP_F0, LOOP_SCS, N, cp)
    dem = OF.PuschOfdmDemodulator(N, n_prb_grid, cp, window_advance=a, sym_phasor=phi, device=dev)
    ofdm = OF.PuschOfdmModulator.for_demodulator(dem)
    bare = OF.PuschOfdmModulator(N, n_prb_grid, cp, device=dev)
    assert ofdm.n_samples == dem.n_samples == 7680 and (ofdm.n_sc, ofdm.n_sym) == (mod.n_sc, mod.n_sym) and ch.L == 1
    rng = np.random.default_rng(82)
    taps = np.array(LOOP_AMPS)[None] * np.exp(2j * np.pi * rng.random((MO.LOOP_PORTS, len(LOOP_DELAYS))))

    def air(s):
        """[B, 4, 7680] on the device of the samples s [B, 1, 7680]: port r receives sum_i taps[r, i] s delayed by LOOP_DELAYS[i]."""
        T = s.shape[-1]
        rx = torch.zeros((B, MO.LOOP_PORTS, T), dtype=torch.complex64, device=dev)
        for r in range(MO.LOOP_PORTS):
            for i, dl in enumerate(LOOP_DELAYS):
                rx[:, r, dl:] += complex(taps[r, i]) * s[:, 0, :T - dl]
        return rx

    for precode in (False, True):
        tx = loop_chain.modulate(ch)
        if precode:
            tx = ch.pre.grid_(tx)
        samples = ofdm(tx)
        assert tuple(samples.shape) == (B, 1, 7680) and samples.device == dev
        out, tb_status = loop_chain.receive(ch, dem(air(samples)), deprecode=precode)
        assert np.array_equal(out, sent) and not tb_status.any(), (precode, tb_status.tolist())
        out, tb_status = loop_chain.receive(ch, dem(air(bare(tx))), deprecode=precode)
        assert np.all(tb_status[:, 0] != 0), ("no phasors", precode, tb_status.tolist())
