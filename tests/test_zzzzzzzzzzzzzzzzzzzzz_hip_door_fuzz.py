"""A bounded, deterministic differential fuzz on the GPU of the four front-door stages the earlier fuzzes leave at pinned cases:
the seeded draws of tests/door_fuzz_cases.py through the channel emulator (`ce_chan_kernel`), the fronthaul codec
(`ce_fh_decompress_kernel`, `ce_fh_compress_kernel`), the PRACH detector (`ce_prach_kernel`) and the SRS estimator
(`ce_srs_profile_kernel`, `ce_srs_estimate_kernel`) against the float64 (the codec: bit-serial) oracles under the oracles' own rules
with T = 4 C, the constants tests/test_door_fuzz.py calibrates on these same cases with the float32 restatements; the codec is
compared bit for bit.  Around the values, in every stage: the inputs lie in NaN-filled (bytes: 0xEE-filled) buffers and are bitwise
unchanged afterwards, and no NaN reaches an output; the outputs lie in sentinel-filled buffers between guards, and every element
outside the written rows is bitwise the sentinel afterwards; one item of the batch, drawn in the dict, equals its own call bit for
bit.  Per stage: the emulator's noise on the rows whose FIR sum is exactly 0 is chan_oracle.noise_ref; the codec's round trip
compress(decompress(compress(x))) returns the oracle's bytes and no byte behind row_bytes is written; a PRACH plan holding one root
of the draw gives that root's bits; the SRS estimate at a delay shifted by a multiple of N and one receive port alone give the
batch's bits.  Nothing is skipped, and no assertion depends on what a kernel returned.

Every assertion message carries the case's dict: `realize_*` of that dict replays the case on the CPU.  Every input is one the
oracles and include/ce_tp.h define.

The 496 cases take 8.4 s on an MI355X, 17 ms each on average.  The file's name sorts it behind
test_zzzzzzzzzzzzzzzzzzzz_hip_srs.py: every earlier GPU test keeps its place in the run."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chan_oracle as CO
import door_fuzz_cases as F
import srs_oracle as SO
from srsran_ce_pytorch_amd import _lib, channel as CH, fronthaul as FH, prach as PR, srs as S

pytestmark = pytest.mark.gpu

# Cases a run flagged, kept exactly as they were drawn (the dicts of door_fuzz_cases.draw_*); they run after the seeded ones.
LOGGED_CHAN_CASES = []
LOGGED_FH_CASES = []
LOGGED_PRACH_CASES = []
LOGGED_SRS_CASES = []

GUARD = 64                                   # complex64 elements (or 32-bit words, or 4-byte groups) either side of a guarded buffer: keeps 16-byte alignment
FILL = np.complex64(complex(-5.0, 7.0))      # the sentinel of a complex stream
NAN_FILL = np.array([0x7FC12345_7FC54321], np.uint64)       # two quiet NaNs with payloads: the sentinel of a grid written into
WORD = 0x7FC54321                            # a quiet NaN with a payload, as float32; an unlikely int32: the sentinel of 32-bit outputs
BYTE_FILL, BYTE_PAD = 0xA5, 0xEE             # the sentinel of a payload written into; what surrounds a payload that is read


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)      # one word per complex64 element: the shape stays


def _w32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


FILL_BITS = _bits(np.array([FILL]))[0]


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _words(n_words):
    """(buffer, middle): an int32 buffer of WORD with `n_words` to write in its middle, the middle on 8 bytes (complex outputs)."""
    buf = torch.full((GUARD + n_words + GUARD,), WORD, dtype=torch.int32, device=_dev())
    assert (buf.data_ptr() + 4 * GUARD) % 8 == 0
    return buf, buf[GUARD:GUARD + n_words]


def _only_the_middle(buf, n_words, what):
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == WORD) and np.all(host[GUARD + n_words:] == WORD), f"{what}: written outside an output"
    return host[GUARD:GUARD + n_words]


# ================================================================ channel emulator ====

def _chan_params(d, b=None):
    """The keyword arguments of a case (of its slot b alone): scalars stay host values, arrays become device tensors."""
    pick = (lambda a: a) if b is None else (lambda a: a[b:b + 1])
    kw = dict(seed=d.seed, first_slot=d.first_slot + (0 if b is None else b))
    if d.fcw is not None:
        if isinstance(d.fcw, np.ndarray):
            kw.update(cfo=_t(pick(d.fcw)), phase0=_t(pick(d.phase0).view(np.int32)))
        else:
            kw.update(cfo=d.fcw, phase0=d.phase0)
    if d.sigma is not None:
        kw["sigma"] = _t(pick(d.sigma)) if isinstance(d.sigma, np.ndarray) else d.sigma
    return kw


@pytest.mark.parametrize("idx", range(F.N_CHAN + len(LOGGED_CHAN_CASES)))
def test_channel_fuzz_case(idx):
    c = F.draw_chan(idx) if idx < F.N_CHAN else LOGGED_CHAN_CASES[idx - F.N_CHAN]
    what = f"chan {c}"
    d = F.realize_chan(c)
    dev, B, P, R, K, T = _dev(), c["B"], c["P"], c["R"], c["K"], c["T"]
    emu = CH.PuschChannelEmulator(P, R, K, device=dev)
    x_host = np.full(F.chan_x_total(c), F.NAN, np.complex64)                # x inside a buffer of NaN: before, between and behind the rows
    F.place(x_host, d.x, c["x_lead"], (c["x_ss"], c["x_ps"]))
    x_buf = torch.as_tensor(x_host, device=dev)
    x = x_buf.as_strided((B, P, T), (c["x_ss"], c["x_ps"], 1), c["x_lead"])
    h = _t(d.h)
    stream = out = None
    if c["y_layout"] != "dense":
        stream = torch.full((2 * GUARD + F.chan_y_total(c),), complex(FILL), dtype=torch.complex64, device=dev)
        out = stream.as_strided((B, R, T), (c["y_ss"], c["y_ps"], 1), GUARD + c["y_lead"])
    y = emu(x, h, out=out, **_chan_params(d))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, R, T) and y.dtype == torch.complex64 and y.device == dev and (out is None or y.data_ptr() == out.data_ptr()), what
    got = y.cpu().numpy()
    # ---- values: finite (a read outside a row reaches NaN), the rule, an exact 0 where the unit is 0 ----
    CO.check(got, d, what, t=F.T_CHAN_FUZZ)
    bits = _bits(got)
    # ---- the write set ----
    if stream is not None:
        after = stream.cpu().numpy()
        body, rows = after[GUARD:len(after) - GUARD], F.chan_rows(c)
        assert len(body) == len(rows) and np.all(_bits(after[:GUARD]) == FILL_BITS) and np.all(_bits(after[len(after) - GUARD:]) == FILL_BITS), f"{what}: a guard was written"
        hit = ~rows & (_bits(body) != FILL_BITS)
        assert not hit.any(), f"{what}: written outside the rows, first at stream elements {np.flatnonzero(hit)[:4].tolist()}"
        for b in range(B):
            for r in range(R):
                o = c["y_lead"] + b * c["y_ss"] + r * c["y_ps"]
                assert np.array_equal(_bits(body[o:o + T]), bits[b, r]), f"{what}: row ({b}, {r}) of the stream is not what was returned"
    # ---- the inputs ----
    assert np.array_equal(_bits(x_buf), _bits(x_host)) and np.array_equal(_bits(h), _bits(d.h)), f"{what}: an input was written"
    # ---- one slot alone, under its own slot number ----
    if B > 1:
        b = c["slot"]
        one = emu(x[b:b + 1], h if c["shared"] else h[b:b + 1], **_chan_params(d, b))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(one)[0], bits[b]), f"{what}: slot {b} alone differs"
    # ---- the noise by itself, on the rows whose FIR sum is exactly 0: the difference against the same call without sigma ----
    zero = F.chan_zero_rows(c)
    if d.sigma is not None and zero.any():
        kw = _chan_params(d)
        kw["sigma"] = None
        clean = emu(x, h, **kw).cpu().numpy()
        sg = [float(s) for s in CO._per_slot(d.sigma, B)]
        for b, r in np.argwhere(zero):
            assert not clean[b, r].any(), f"{what}: row ({b}, {r}) has only zero taps and is not 0 without noise"
            n = CO.noise_ref(d.seed, d.first_slot + int(b), int(r), T)
            err = np.abs((got[b, r].astype(np.complex128) - clean[b, r]) - sg[b] * n)
            assert np.all(err <= F.T_CHAN_FUZZ * CO.EPS * sg[b] * (1.0 + np.abs(n))), f"{what}: the noise of row ({b}, {r}) is not noise_ref of (seed, first_slot + b, r, t)"


# ================================================================ fronthaul codec ====

def _fh_launch(entry, c, payload, p_off, ps, grid, g_off, gs, factor):
    """The library's return code of one launch of `entry` with the strides as they stand (a dimension of one entry keeps its
    drawn stride): payload at byte p_off of `payload`, the section's first RE at element g_off of `grid`."""
    with torch.cuda.device(_dev()):
        return getattr(_lib.load(), entry)(_lib.CE_ABI_VERSION, C.c_void_p(payload.data_ptr() + p_off), *ps, C.c_void_p(grid.data_ptr() + 8 * g_off), *gs,
                                           c["B"], c["R"], c["S"], c["n_prb"], FH.METHODS[c["method"]], c["W"], float(factor), _stream())


def _pay(a):
    """Host payload rows -> a device tensor whose rows start on 4 bytes: the last dimension padded to a multiple of 4."""
    a = np.asarray(a)
    nb = a.shape[-1]
    wide = np.full(a.shape[:-1] + (nb + (-nb) % 4,), BYTE_PAD, np.uint8)
    wide[..., :nb] = a
    return _t(wide)


def _fast(rows):
    """Host rows [B, R, S, n_sc] -> the device grid [B, R, n_sc, S] in the fast layout."""
    return _t(rows).permute(0, 1, 3, 2)


def _rows(grid):
    return grid.permute(0, 1, 3, 2).cpu().numpy()


@pytest.mark.parametrize("idx", range(F.N_FH + len(LOGGED_FH_CASES)))
def test_fronthaul_fuzz_case(idx):
    c = F.draw_fh(idx) if idx < F.N_FH else LOGGED_FH_CASES[idx - F.N_FH]
    what = f"fh {c}"
    d = F.realize_fh(c)
    dev, n, n_prb, nb = _dev(), (c["B"], c["R"], c["S"]), c["n_prb"], d.row_bytes
    n_sc, first = 12 * c["n_prb_grid"], 12 * c["start_prb"]
    scale, inv = np.float32(c["scale"]), FH.inv_scale(c["scale"])
    # ---- the decompressor: random payloads at the read side's strides -> the section of a strided grid inside a NaN-filled buffer ----
    p_host = np.full(c["pr_lead"] + F.extent(n, c["pr_strides"], nb) + c["pr_tail"], BYTE_PAD, np.uint8)
    F.place(p_host, d.payload, c["pr_lead"], c["pr_strides"])
    p_buf = torch.as_tensor(p_host, device=dev)
    total = c["gw_lead"] + F.extent(n, c["gw_strides"], n_sc) + c["gw_tail"]
    g_buf = torch.as_tensor(np.repeat(NAN_FILL, 2 * GUARD + total), device=dev).view(torch.complex64)
    assert p_buf.data_ptr() % 16 == 0 and g_buf.data_ptr() % 16 == 0, what
    rc = _fh_launch("ce_fh_decompress", c, p_buf, c["pr_lead"], c["pr_strides"], g_buf, GUARD + c["gw_lead"] + first, c["gw_strides"], scale)
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: {_lib.last_error()}"
    after = _bits(g_buf)
    body = after[GUARD:GUARD + total]
    mask = F.rows_mask(total, n, 12 * n_prb, c["gw_lead"] + first, c["gw_strides"], what)
    assert np.all(after[:GUARD] == NAN_FILL[0]) and np.all(after[GUARD + total:] == NAN_FILL[0]), f"{what}: a guard of the grid was written"
    assert np.all(body[~mask] == NAN_FILL[0]), f"{what}: the decompressor wrote outside the section's REs, first at {np.flatnonzero(~mask & (body != NAN_FILL[0]))[:4].tolist()}"
    got = F.gather(body, n, 12 * n_prb, c["gw_lead"] + first, c["gw_strides"])
    assert np.array_equal(got, _bits(d.unpacked)), f"{what}: the decompressed section differs from the oracle's"
    assert np.all(np.isfinite(got.view(np.float32))), f"{what}: a non-finite RE"
    assert np.array_equal(p_buf.cpu().numpy(), p_host), f"{what}: the payload was written"
    # ---- the decompressor on the oracle's own packed payloads, through the wrapper ----
    fh = FH.PuschFronthaulDecompressor(n_prb, c["S"], c["method"], c["W"], c["scale"], device=dev)
    comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
    assert np.array_equal(_bits(_rows(fh(_pay(d.packed)))), _bits(d.restored)), f"{what}: the oracle's packed payload decompresses differently"
    # ---- the compressor: the section of a strided grid inside a NaN-filled buffer -> rows with padding inside a sentinel-filled buffer ----
    g_host = np.full(c["gr_lead"] + F.extent(n, c["gr_strides"], n_sc) + c["gr_tail"], F.NAN, np.complex64)
    F.place(g_host, d.grid, c["gr_lead"] + first, c["gr_strides"])
    g_in = torch.as_tensor(g_host, device=dev)
    total = c["pw_lead"] + F.extent(n, c["pw_strides"], nb) + c["pw_tail"]
    out = torch.full((8 * GUARD + total,), BYTE_FILL, dtype=torch.uint8, device=dev)
    assert g_in.data_ptr() % 16 == 0 and out.data_ptr() % 4 == 0, what
    rc = _fh_launch("ce_fh_compress", c, out, 4 * GUARD + c["pw_lead"], c["pw_strides"], g_in, c["gr_lead"] + first, c["gr_strides"], inv)
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: {_lib.last_error()}"
    after = out.cpu().numpy()
    body = after[4 * GUARD:4 * GUARD + total]
    mask = F.rows_mask(total, n, nb, c["pw_lead"], c["pw_strides"], what)
    assert np.all(after[:4 * GUARD] == BYTE_FILL) and np.all(after[4 * GUARD + total:] == BYTE_FILL), f"{what}: a guard of the payload was written"
    assert np.all(body[~mask] == BYTE_FILL), f"{what}: the compressor wrote outside [0, row_bytes) of its rows, first at byte {np.flatnonzero(~mask & (body != BYTE_FILL))[:4].tolist()}"
    assert np.array_equal(F.gather(body, n, nb, c["pw_lead"], c["pw_strides"]), d.packed), f"{what}: the compressed rows differ from the oracle's"
    assert np.array_equal(_bits(g_in), _bits(g_host)), f"{what}: the grid was written"
    # ---- compress(decompress(compress(x))): the oracle's bytes (the first's own, but for a one-bit PRB without a negative value) ----
    once = comp(_fast(d.grid))
    again = comp(fh(once))
    torch.cuda.synchronize()
    assert np.array_equal(once.cpu().numpy(), d.packed) and np.array_equal(again.cpu().numpy(), d.repacked), f"{what}: the round trip's bytes differ from the oracle's"
    # ---- one row alone ----
    if n[0] * n[1] * n[2] > 1:
        b, r, s = c["row"]
        fh1 = FH.PuschFronthaulDecompressor(n_prb, 1, c["method"], c["W"], c["scale"], device=dev)
        one = fh1(_pay(d.payload[b:b + 1, r:r + 1, s:s + 1]))
        assert np.array_equal(_bits(_rows(one))[0, 0, 0], _bits(d.unpacked[b, r, s])), f"{what}: row {(b, r, s)} alone decompresses differently"
        one = FH.PuschFronthaulCompressor.for_decompressor(fh1)(_fast(d.grid[b:b + 1, r:r + 1, s:s + 1]))
        assert np.array_equal(one.cpu().numpy()[0, 0, 0], d.packed[b, r, s]), f"{what}: row {(b, r, s)} alone compresses differently"


# ================================================================ PRACH detector ====

def _np_prach(out):
    torch.cuda.synchronize()
    return SimpleNamespace(peak=out.peak.cpu().numpy(), delay=out.delay.cpu().numpy(), mean=out.mean.cpu().numpy(), profile=None if out.profile is None else out.profile.cpu().numpy())


def _same_prach(a, b, what, names=("peak", "delay", "mean", "profile")):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_w32(x), _w32(y)), f"{what}: {name} differs by bits"


def _sub_prach(a, b=slice(None), i=slice(None)):
    return SimpleNamespace(peak=a.peak[b, i], delay=a.delay[b, i], mean=a.mean[b, i], profile=None if a.profile is None else a.profile[b, i])


@pytest.mark.parametrize("idx", range(F.N_PRACH + len(LOGGED_PRACH_CASES)))
def test_prach_fuzz_case(idx):
    c = F.draw_prach(idx) if idx < F.N_PRACH else LOGGED_PRACH_CASES[idx - F.N_PRACH]
    what = f"prach {c}"
    d = F.realize_prach(c)
    dev, L, N, R, S, B = _dev(), c["L"], c["N"], c["R"], c["S"], len(c["occasions"])
    n_roots, n_shifts, combine = len(c["roots"]), c["n_shifts"], "coherent" if c["combine"] else "noncoherent"
    det = PR.PrachDetector(L, N, c["roots"], c["n_cs"], n_shifts, combine=combine, device=dev)
    assert np.array_equal(det.win_start, d.ref.win_start) and det.win_len == d.ref.win_len, what
    y_buf = torch.as_tensor(d.host, device=dev)
    y = y_buf.as_strided((B, R, S, L), tuple(c["strides"]) + (1,), c["lead"])
    # ---- the launch itself, the strides as drawn, every output between guards ----
    sizes = [B * n_roots * n_shifts, B * n_roots * n_shifts, B * n_roots] + ([B * n_roots * N] if c["return_profile"] else [])
    bufs = [_words(k) for k in sizes]
    det._plan()
    with torch.cuda.device(dev):
        rc = det._lib.ce_prach_detect(det._handle, C.c_void_p(y.data_ptr()), *c["strides"], B, R, S, *(C.c_void_p(mid.data_ptr()) for _, mid in bufs),
                                      *([] if c["return_profile"] else [None]), _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: {_lib.last_error()}"
    mids = [_only_the_middle(buf, k, what) for (buf, _), k in zip(bufs, sizes)]
    got = SimpleNamespace(peak=mids[0].view(np.float32).reshape(B, n_roots, n_shifts), delay=mids[1].reshape(B, n_roots, n_shifts), mean=mids[2].view(np.float32).reshape(B, n_roots),
                          profile=mids[3].view(np.float32).reshape(B, n_roots, N) if c["return_profile"] else None)
    # ---- peak, delay, mean and the profile against the oracle; the delay of every transmitted preamble is the oracle's ----
    assert got.profile is None or np.all(np.isfinite(got.profile)), f"{what}: a non-finite profile (a read outside a row reaches NaN)"
    F.prach_check(got, d, what, F.T_PRACH_FUZZ)
    if got.profile is not None:
        at = np.take_along_axis(got.profile, (d.ref.win_start[None, None, :] + got.delay) % N, -1)
        assert np.array_equal(_w32(at), _w32(got.peak)), f"{what}: a peak is no element of the profile"
    assert np.array_equal(_bits(y_buf), _bits(d.host)), f"{what}: y was written"
    # ---- the wrapper on the same view ----
    wrapped = _np_prach(det(y, return_profile=c["return_profile"]))
    _same_prach(wrapped, got, f"{what}: the wrapper")
    # ---- one occasion alone; a plan that holds one root of the draw ----
    if B > 1:
        b = c["occasion"]
        _same_prach(_np_prach(det(y[b:b + 1], return_profile=c["return_profile"])), _sub_prach(got, slice(b, b + 1)), f"{what}: occasion {b} alone")
    if n_roots > 1:
        i = c["root"]
        one = PR.PrachDetector(L, N, [c["roots"][i]], c["n_cs"], n_shifts, combine=combine, device=dev)
        _same_prach(_np_prach(one(y, return_profile=c["return_profile"])), _sub_prach(got, slice(None), slice(i, i + 1)), f"{what}: root {c['roots'][i]} alone")


# ================================================================ SRS estimator ====

def _np_est(out):
    torch.cuda.synchronize()
    return SimpleNamespace(h_sb=out.h_sb.cpu().numpy(), h_wb=out.h_wb.cpu().numpy(), noise=out.noise.cpu().numpy(), epre=out.epre.cpu().numpy())


def _same_est(a, b, what):
    for name in ("h_sb", "h_wb", "noise", "epre"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_w32(x), _w32(y)), f"{what}: {name} differs by bits"


def _sub_est(a, b=slice(None), r=slice(None)):
    return SimpleNamespace(h_sb=a.h_sb[b, r], h_wb=a.h_wb[b, r], noise=a.noise[b, r], epre=a.epre[b, r])


@pytest.mark.parametrize("idx", range(F.N_SRS + len(LOGGED_SRS_CASES)))
def test_srs_fuzz_case(idx):
    c = F.draw_srs(idx) if idx < F.N_SRS else LOGGED_SRS_CASES[idx - F.N_SRS]
    what = f"srs {c}"
    d = F.realize_srs(c)
    k, dev = d.c, _dev()
    B, R, N = k.B, k.R, k.N
    est = S.SrsEstimator(**SO.plan_kwargs(k), device=dev)
    assert (est.win_len, est.guard, est.m) == (k.win_len, k.g, k.M), what
    y_buf = torch.as_tensor(d.host, device=dev)
    st = tuple(c["strides"])
    if c["layout"] == "grid view":            # [B, R, n_sc, n_sym] as the demodulator and the decompressor return it, permuted back
        y = y_buf.as_strided((B, R, k.n_sc, k.n_sym), (st[0], st[1], 1, st[2]), c["lead"]).permute(0, 1, 3, 2)
    else:
        y = y_buf.as_strided((B, R, k.n_sym, k.n_sc), st + (1,), c["lead"])
    assert y.data_ptr() % 16 == (8 if c["lead"] % 2 else 0), what
    sl_t, id_t = _t(np.resize(d.slot, B).astype(np.int32)), _t(np.resize(d.n_id, B).astype(np.int32))
    slot, n_id = (sl_t, id_t) if c["per_item"] else (int(d.slot[0]), int(d.n_id[0]))
    # ---- launch 1 and the wrapper's delay ----
    p = est.profile(y, slot, n_id)
    torch.cuda.synchronize()
    prof, delay = p.profile.cpu().numpy(), p.delay.cpu().numpy()
    F.srs_check(d, F.T_SRS_FUZZ, prof=prof, delay=delay, what=what)            # the delay rule; on a signal item the oracle's delay
    if k.win_len == 1:
        assert np.all(delay == -k.g), f"{what}: a window of one index has the delay -g"
    # ---- launch 2 at that delay ----
    e = est(y, slot, n_id, delay=p.delay)
    got = _np_est(e)
    F.srs_check(d, F.T_SRS_FUZZ, est=got, what=what)
    for b, kind in enumerate(c["items"]):
        if kind == "zero":
            assert not prof[b].any() and not got.h_sb[b].any() and not got.h_wb[b].any() and not got.noise[b].any() and not got.epre[b].any(), f"{what}: item {b} is all zero, its outputs are not"
    assert np.array_equal(_bits(y_buf), _bits(d.host)), f"{what}: y was written"
    # ---- a delay shifted by a multiple of N ----
    _same_est(_np_est(est(y, slot, n_id, delay=p.delay + c["shift"] * N)), got, f"{what}: the delay shifted by {c['shift']} N")
    # ---- both launches themselves, every output between guards ----
    sizes = [B * R * k.win_len, 2 * B * R * k.n_ap * k.n_symb * k.n_blocks, 2 * B * R * k.n_ap, B * R, B * R]
    bufs = [_words(n) for n in sizes]
    est._plan()
    lead = (est._handle, C.c_void_p(y.data_ptr()), *st, B, R, C.c_void_p(sl_t.data_ptr()), 1, C.c_void_p(id_t.data_ptr()), 1)
    with torch.cuda.device(dev):
        rc1 = est._lib.ce_srs_profile(*lead, C.c_void_p(bufs[0][1].data_ptr()), _stream())
        rc2 = est._lib.ce_srs_estimate(*lead, C.c_void_p(p.delay.data_ptr()), 1, *(C.c_void_p(mid.data_ptr()) for _, mid in bufs[1:]), _stream())
    torch.cuda.synchronize()
    assert rc1 == 0 and rc2 == 0, f"{what}: {_lib.last_error()}"
    for (buf, _), n, ref in zip(bufs, sizes, (prof, got.h_sb, got.h_wb, got.noise, got.epre)):
        assert np.array_equal(_only_the_middle(buf, n, what).view(np.uint32), _w32(ref).reshape(-1)), f"{what}: the launch and the wrapper differ"
    # ---- one receive port alone; one item alone ----
    if R > 1:
        r = slice(c["port"], c["port"] + 1)
        assert np.array_equal(_w32(est.profile(y[:, r], slot, n_id).profile), _w32(prof[:, r])), f"{what}: the profile of port {c['port']} alone differs"
        _same_est(_np_est(est(y[:, r], slot, n_id, delay=p.delay)), _sub_est(got, slice(None), r), f"{what}: port {c['port']} alone")
    if B > 1:
        b = slice(c["item"], c["item"] + 1)
        s1, i1 = (sl_t[b], id_t[b]) if c["per_item"] else (slot, n_id)
        assert np.array_equal(_w32(est.profile(y[b], s1, i1).profile), _w32(prof[b])), f"{what}: the profile of item {c['item']} alone differs"
        _same_est(_np_est(est(y[b], s1, i1, delay=p.delay[b])), _sub_est(got, b), f"{what}: item {c['item']} alone")
