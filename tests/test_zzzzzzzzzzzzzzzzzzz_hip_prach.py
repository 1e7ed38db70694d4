"""GPU tests of the PRACH preamble detector (include/ce_tp.h `ce_prach_detect`, `PrachDetector`) against the float64 oracle of
tests/prach_oracle.py under its rules: every case with and without the profile; detection and arrival times; the read set (a
strided view inside a NaN-filled buffer, ports and repetitions in both nestings); the write set (outputs inside guard-filled
buffers); bitwise independence of an occasion from its batch and of a root from its plan; a NaN confined to its occasion; a side
stream, an empty batch; every refusal of the launch and of the wrapper with nothing written; and the loop prach_preamble_freq ->
PuschFronthaulCompressor -> PuschFronthaulDecompressor -> PrachDetector on the decompressor's grid, without a copy.

The file's name sorts it behind test_zzzzzzzzzzzzzzzzzz_hip_fh.py: every earlier GPU test keeps its place in the run."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import prach_oracle as PO
from srsran_ce_pytorch_amd import _lib, fronthaul as FH, prach as PR

pytestmark = pytest.mark.gpu

COMBINE = {0: "noncoherent", 1: "coherent"}
GUARD = 0x7FC54321                                            # a quiet NaN with a payload, as float32; an unlikely int32


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())


def _detector(d, roots=None, **kw):
    c = d.c
    return PR.PrachDetector(c["L"], c["N"], d.roots if roots is None else roots, c["n_cs"], c["n_shifts"], combine=COMBINE[c["combine"]], device=_dev(), **kw)


def _np(out):
    torch.cuda.synchronize()
    return SimpleNamespace(peak=out.peak.cpu().numpy(), delay=out.delay.cpu().numpy(), mean=out.mean.cpu().numpy(),
                           profile=None if out.profile is None else out.profile.cpu().numpy())


def _same_bits(a, b, what=""):
    for name in ("peak", "delay", "mean", "profile"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: {name} differs by bits"


def _sub(a, b=slice(None), i=slice(None)):
    """The occasions `b` and roots `i` of a result."""
    return SimpleNamespace(peak=a.peak[b, i], delay=a.delay[b, i], mean=a.mean[b, i], profile=None if a.profile is None else a.profile[b, i])


@pytest.mark.parametrize("with_profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("name", PO.CASE_NAMES)
def test_cases_against_the_oracle(name, with_profile):
    d = PO.inputs(name)
    det = _detector(d)
    out = det(_t(d.y), return_profile=with_profile)
    B, c = len(d.c["occasions"]), d.c
    assert tuple(out.peak.shape) == (B, 3, c["n_shifts"]) == tuple(out.delay.shape) and tuple(out.mean.shape) == (B, 3)
    assert out.peak.dtype == torch.float32 and out.delay.dtype == torch.int32 and out.mean.dtype == torch.float32 and out.detected is None and out.arrival_s is None
    assert (out.profile is None) != with_profile
    got = _np(out)
    PO.check(got, d, f"{name} ({'with' if with_profile else 'without'} profile)")
    for b, kind in enumerate(c["occasions"]):
        if kind == "zero":                                       # an all-zero occasion: exact zeros
            assert not got.peak[b].any() and not got.delay[b].any() and not got.mean[b].any() and (got.profile is None or not got.profile[b].any())
    if with_profile:
        assert tuple(out.profile.shape) == (B, 3, c["N"]) and out.profile.dtype == torch.float32
        idx = (d.ref.win_start[None, None, :] + got.delay) % c["N"]
        assert np.array_equal(np.take_along_axis(got.profile, idx, -1).view(np.uint32), got.peak.view(np.uint32))      # the peak is an element of the profile
        w, first = PO.window_search(got.profile, d.ref.win_start, d.ref.win_len)
        assert np.array_equal(first, got.delay) and np.array_equal(w, got.peak)                                      # .. its window's largest, at the first index
        _same_bits(_sub(got), SimpleNamespace(**{**vars(_np(det(_t(d.y)))), "profile": got.profile}), name)           # the profile changes nothing else


@pytest.mark.parametrize("name", PO.CASE_NAMES)
def test_detection_returns_the_transmitted_set_and_the_arrival_times(name):
    d = PO.inputs(name)
    c = d.c
    scs = 30e3
    out = _detector(d, scs_ra_hz=scs)(_t(d.y), threshold=PO.threshold(d))
    torch.cuda.synchronize()
    assert out.detected.dtype == torch.bool and out.arrival_s.dtype == torch.float64 and tuple(out.detected.shape) == tuple(out.peak.shape) == tuple(out.arrival_s.shape)
    found = {tuple(int(x) for x in t) for t in np.argwhere(out.detected.cpu().numpy())}
    assert found == set(d.sent), (sorted(found), d.sent)
    arrival = out.arrival_s.cpu().numpy()
    pre = PO.case_preambles(c)
    for k, (b, i, v) in enumerate(d.sent):
        delay = pre[k % 3][2]
        assert abs(arrival[b, i, v] - delay / (c["L"] * scs)) <= 0.5 / (c["N"] * scs), (name, b, i, v)                # the index nearest to the peak: half a sample
    want = PR.prach_arrival_seconds(c["L"], c["N"], c["n_cs"], np.arange(c["n_shifts"])[None, None, :], out.delay.cpu().numpy(), scs)
    assert np.allclose(arrival, want, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("nesting", ["port_outside", "repetition_outside"])
@pytest.mark.parametrize("name", ["a_139_256_b3", "i_839_2048_b3_coh", "g_139_512_1x12"])
def test_read_set_a_strided_view_inside_a_nan_filled_buffer(name, nesting):
    """139 of 144 (839 of 844) subcarriers of a wider grid that starts at an odd element, ports and repetitions in both nestings:
    finite, and the dense call's results by bits."""
    d = PO.inputs(name)
    B, R, S, L = d.y.shape
    width, lead = L + 5, 3
    shape, perm = ((B, R, S, width), (0, 1, 2, 3)) if nesting == "port_outside" else ((B, S, R, width), (0, 2, 1, 3))
    buf = torch.full((2 * (lead + int(np.prod(shape))),), float("nan"), dtype=torch.float32, device=_dev()).view(torch.complex64)
    view = buf[lead:].view(shape).permute(*perm)[..., :L]
    view.copy_(_t(d.y))
    assert not view.is_contiguous() and view.shape == (B, R, S, L)
    det = _detector(d)
    got = _np(det(view, return_profile=True))
    assert all(np.all(np.isfinite(getattr(got, k))) for k in ("peak", "mean", "profile"))
    _same_bits(got, _np(det(_t(d.y), return_profile=True)), f"{name} {nesting}")
    # stride 0 repeats a row: one port expanded to R ports equals the batch of R copies
    one = _t(d.y[:, :1])
    _same_bits(_np(det(one.expand(B, R, S, L))), _np(det(one.repeat(1, R, 1, 1))), f"{name} expanded")


def _raw(det, y, st, B, R, S, peak, delay, mean, profile):
    """The library's return code of ce_prach_detect on the current stream with the arguments as they stand."""
    det._plan()
    ptr = lambda x: C.c_void_p(x if isinstance(x, int) else (x.data_ptr() if x is not None else None))      # noqa: E731
    with torch.cuda.device(det.device):
        return det._lib.ce_prach_detect(det._handle, ptr(y), *st, B, R, S, ptr(peak), ptr(delay), ptr(mean), ptr(profile),
                                        C.c_void_p(torch.cuda.current_stream(det.device).cuda_stream))


def _guarded(n, pad=67):
    """An int32 buffer of GUARD words with `n` elements to write in the middle: (buffer, the middle)."""
    buf = torch.full((pad + n + pad,), GUARD, dtype=torch.int32, device=_dev())
    return buf, buf[pad:pad + n]


@pytest.mark.parametrize("name", ["a_139_256_b3", "h_839_1024_64win", "k_1151_4096"])
def test_write_set_outputs_inside_guard_filled_buffers(name):
    d = PO.inputs(name)
    det = _detector(d)
    want = _np(det(_t(d.y), return_profile=True))
    B, R, S, L = d.y.shape
    nw, nm, npf = want.peak.size, want.mean.size, want.profile.size
    bufs = [_guarded(nw), _guarded(nw), _guarded(nm), _guarded(npf)]
    y = _t(d.y)
    assert _raw(det, y, (R * S * L, S * L, L), B, R, S, *(mid for _, mid in bufs)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for (buf, mid), n, ref in zip(bufs, (nw, nw, nm, npf), (want.peak, want.delay, want.mean, want.profile)):
        host = buf.cpu().numpy()
        assert np.all(host[:67] == GUARD) and np.all(host[67 + n:] == GUARD), f"{name}: written outside the output"
        assert np.array_equal(host[67:67 + n].view(np.uint32), ref.reshape(-1).view(np.uint32))
    # without a profile the other three are the same and nothing else is written
    bufs = [_guarded(nw), _guarded(nw), _guarded(nm)]
    assert _raw(det, y, (R * S * L, S * L, L), B, R, S, *(mid for _, mid in bufs), None) == 0
    torch.cuda.synchronize()
    for (buf, mid), n, ref in zip(bufs, (nw, nw, nm), (want.peak, want.delay, want.mean)):
        host = buf.cpu().numpy()
        assert np.all(host[:67] == GUARD) and np.all(host[67 + n:] == GUARD) and np.array_equal(host[67:67 + n].view(np.uint32), ref.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("name", ["a_139_256_b3", "e_139_512_circle_b3", "i_839_2048_b3_coh"])
def test_an_occasion_does_not_depend_on_its_batch_nor_a_root_on_its_plan(name):
    d = PO.inputs(name)
    det = _detector(d)
    y = _t(d.y)
    batch = _np(det(y, return_profile=True))
    for b in range(d.y.shape[0]):
        _same_bits(_sub(batch, slice(b, b + 1)), _np(det(y[b:b + 1], return_profile=True)), f"{name} occasion {b}")
    for i, u in enumerate(d.roots):
        _same_bits(_sub(batch, slice(None), slice(i, i + 1)), _np(_detector(d, roots=[u])(y, return_profile=True)), f"{name} root {u}")
    swapped = _np(_detector(d, roots=d.roots[::-1])(y, return_profile=True))
    _same_bits(_sub(batch, slice(None), slice(None, None, -1)), swapped, f"{name} roots reversed")


def test_a_nan_stays_in_its_occasion():
    d = PO.inputs("a_139_256_b3")
    det = _detector(d)
    clean = _np(det(_t(d.y), return_profile=True))
    y = d.y.copy()
    y[1, 2, 1, 77] = complex(float("nan"), 1.0)
    got = _np(det(_t(y), return_profile=True))
    for b in (0, 2):
        _same_bits(_sub(got, slice(b, b + 1)), _sub(clean, slice(b, b + 1)), f"occasion {b}")
    assert np.all(np.isnan(got.peak[1])) and not got.delay[1].any() and np.all(np.isnan(got.mean[1])) and np.all(np.isnan(got.profile[1]))


def test_a_side_stream_and_an_empty_batch():
    d = PO.inputs("b_139_256_3x1")
    det = _detector(d)
    y = _t(d.y)
    want = _np(det(y, return_profile=True))
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        out = det(y, return_profile=True)
    side.synchronize()
    _same_bits(_np(out), want, "side stream")
    empty = det(y[:0], threshold=3.0, return_profile=True)
    assert tuple(empty.peak.shape) == (0, 3, 10) == tuple(empty.delay.shape) == tuple(empty.detected.shape) == tuple(empty.arrival_s.shape)
    assert tuple(empty.mean.shape) == (0, 3) and tuple(empty.profile.shape) == (0, 3, 256)
    # n_occasions == 0 launches nothing, whatever the pointers
    assert _raw(det, 0x8, (0, 0, 0), 0, 1, 1, 0x4, 0x4, 0x4, None) == 0
    assert _raw(det, None, (0, 0, 0), 0, 1, 1, None, None, None, None) == 0
    torch.cuda.synchronize()


def test_refusals_of_the_launch_with_nothing_written():
    d = PO.inputs("a_139_256_b3")
    det = _detector(d)
    B, R, S, L = d.y.shape
    y = _t(d.y)
    dense = (R * S * L, S * L, L)
    bufs = [_guarded(B * 3 * 10), _guarded(B * 3 * 10), _guarded(B * 3), _guarded(B * 3 * 256)]
    p, dl, m, pf = (mid for _, mid in bufs)
    a = y.data_ptr()
    INV, UNS = _lib.CE_ERR_INVALID, _lib.CE_ERR_UNSUPPORTED
    bad = [("n_occasions", INV, (y, dense, -1, R, S, p, dl, m, pf)), ("n_ports", INV, (y, dense, B, 0, S, p, dl, m, pf)), ("n_ports", INV, (y, dense, B, 65, S, p, dl, m, pf)),
           ("n_reps", INV, (y, dense, B, R, 0, p, dl, m, pf)), ("n_reps", INV, (y, dense, B, R, 13, p, dl, m, pf)),
           ("null", INV, (None, dense, B, R, S, p, dl, m, pf)), ("null", INV, (y, dense, B, R, S, None, dl, m, pf)), ("null", INV, (y, dense, B, R, S, p, None, m, pf)),
           ("null", INV, (y, dense, B, R, S, p, dl, None, pf)),
           ("must be >= 0", INV, (y, (-1, S * L, L), B, R, S, p, dl, m, pf)), ("must be >= 0", INV, (y, (R * S * L, -1, L), B, R, S, p, dl, m, pf)),
           ("must be >= 0", INV, (y, (R * S * L, S * L, -1), B, R, S, p, dl, m, pf)),
           ("8-byte", INV, (a + 4, dense, B, R, S, p, dl, m, pf)), ("4-byte", INV, (y, dense, B, R, S, p.data_ptr() + 2, dl, m, pf)),
           ("4-byte", INV, (y, dense, B, R, S, p, dl.data_ptr() + 1, m, pf)), ("4-byte", INV, (y, dense, B, R, S, p, dl, m.data_ptr() + 2, pf)),
           ("4-byte", INV, (y, dense, B, R, S, p, dl, m, pf.data_ptr() + 3)),
           ("address space", INV, (y, (2 ** 62, S * L, L), B, R, S, p, dl, m, pf)), ("address space", INV, (y, (R * S * L, 2 ** 61, L), B, R, S, p, dl, m, pf)),
           ("address space", INV, (y, (R * S * L, S * L, 2 ** 61), B, R, S, p, dl, m, pf)),
           ("peak overlaps y", INV, (y, dense, B, R, S, a + 8, dl, m, pf)), ("delay overlaps y", INV, (y, dense, B, R, S, p, a, m, pf)),
           ("mean overlaps y", INV, (y, dense, B, R, S, p, dl, a + 8 * (B * R * S * L - 1), pf)), ("profile overlaps y", INV, (y, dense, B, R, S, p, dl, m, a - 4 * B * 3 * 256 + 4)),
           ("2^31-1 workgroups", UNS, (y, (0, 0, 0), 2 ** 31 // 3 + 1, R, S, p, dl, m, pf))]
    before = d.y.copy()
    for text, code, (yy, st, b, r, s, *outs) in bad:
        rc = _raw(det, yy, st, b, r, s, *outs)
        assert rc == code and text in _lib.last_error(), (text, rc, _lib.last_error())
    null_plan = det._lib.ce_prach_detect(None, C.c_void_p(a), *dense, B, R, S, C.c_void_p(p.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(m.data_ptr()), None, None)
    assert null_plan == INV
    torch.cuda.synchronize()
    assert all(bool((buf == GUARD).all()) for buf, _ in bufs) and np.array_equal(y.cpu().numpy().view(np.uint64), before.view(np.uint64))


def test_refusals_of_the_wrapper_before_any_launch():
    d = PO.inputs("a_139_256_b3")
    det = _detector(d)
    y = _t(d.y)
    B, R, S, L = d.y.shape
    wide = torch.zeros((B, R, S, 2 * L), dtype=torch.complex64, device=_dev())
    bad = [d.y, y.cpu(), y.to(torch.complex128), y.real.contiguous(), y[0], y[..., :L - 1], wide[..., ::2], y[:, :1].expand(B, 65, S, L), y[:, :, :1].expand(B, R, 13, L),
           y[:, :0], y[:, :, :0]]
    for t in bad:
        with pytest.raises(ValueError):
            det(t)
    for thr in (-1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError):
            det(y, threshold=thr)
    with pytest.raises(RuntimeError):
        PR.PrachDetector(139, 256, [1], 13, 10, device="cpu")(y)
    got = det(wide[..., :L])                                  # a longer last dimension is a view like any other
    torch.cuda.synchronize()
    assert not got.peak.any() and not got.mean.any()


@pytest.mark.parametrize("iq_width", [9, 14])
def test_the_loop_from_preambles_through_the_fronthaul_to_the_detector(iq_width):
    """prach_preamble_freq -> rows of a 12-PRB section (139 of 144 subcarriers) -> PuschFronthaulCompressor ->
    PuschFronthaulDecompressor -> PrachDetector on the decompressor's grid view, without a copy: the transmitted (root, shift)
    set and the delays come back."""
    L, N, n_cs, n_shifts, roots = 139, 256, 13, 10, (1, 138, 70)
    B, R, S, n_prb = 2, 2, 3, 12
    rng = np.random.default_rng(77)
    sent = {(0, 0, 0): 0.0, (0, 1, 9): PO.off_half_sample(L, N, 9 * n_cs, 0.6 * n_cs), (1, 2, 4): PO.off_half_sample(L, N, 4 * n_cs, 0.3 * n_cs), (1, 0, 7): 0.0}
    rows = np.zeros((B, R, S, 12 * n_prb), np.complex128)
    rows[..., :L] = np.sqrt(0.05 / 2.0) * (rng.standard_normal((B, R, S, L)) + 1j * rng.standard_normal((B, R, S, L)))
    for (b, i, v), delay in sent.items():
        rows[b, :, :, :L] += np.exp(2j * np.pi * rng.random(R))[:, None, None] * PR.prach_preamble_freq(roots[i], v * n_cs, L, delay)[None, None, :]
    fh = FH.PuschFronthaulDecompressor(n_prb, n_sym=S, method="bfp", iq_width=iq_width, scale=2.0 ** -12, device=_dev())
    comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
    grid = fh(comp(_t(rows.astype(np.complex64)).permute(0, 1, 3, 2)))                       # [B, R, 144, S], the fast layout
    y = grid.permute(0, 1, 3, 2)[..., :L]
    assert y.data_ptr() == grid.data_ptr() and tuple(y.shape) == (B, R, S, L) and not y.is_contiguous()
    det = PR.PrachDetector(L, N, roots, n_cs, n_shifts, device=_dev())
    ref = PO.detect_ref(y.cpu().numpy(), L, N, roots, n_cs, n_shifts, 0)                   # the oracle on what the decompressor delivered
    d = SimpleNamespace(c=dict(occasions=("signal",) * B), ref=ref, N=N, L=L, sent=tuple(sent))
    hit, miss = PO.hit_miss(d)
    assert hit / miss >= PO.MIN_HIT_OVER_MISS
    out = det(y, threshold=float(np.sqrt(hit * miss)))
    PO.check(_np(out), d, f"loop, BFP {iq_width}")
    assert {tuple(int(x) for x in t) for t in np.argwhere(out.detected.cpu().numpy())} == set(sent)
    clean = PO.detect_ref(rows[..., :L], L, N, roots, n_cs, n_shifts, 0)                   # the delays of what was sent, before quantisation
    arrival = out.arrival_s.cpu().numpy()
    for (b, i, v), delay in sent.items():
        assert int(out.delay[b, i, v]) == int(clean.delay[b, i, v])
        assert abs(arrival[b, i, v] - delay / (L * det.scs_ra_hz)) <= 0.5 / (N * det.scs_ra_hz)
