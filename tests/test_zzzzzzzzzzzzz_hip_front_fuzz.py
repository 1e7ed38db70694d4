"""A bounded, deterministic differential fuzz on the GPU of the three PUSCH kernels the first two fuzzes leave at pinned cases:
the seeded draws of tests/front_fuzz_cases.py through `ce_tp_precode` (a sweep over every valid allocation size plus general
row geometries: x and y with their own offsets, order, gaps and strides), PuschOfdmDemodulator and PuschDmrs, each against
its oracle under the oracle's own rule -- the precoder under tpre_oracle.check and the demodulator under ofdm_oracle.check
with T = 4 C, the constants tests/test_front_fuzz.py calibrates on these same cases; the generator bit for bit on the int32
view.  Around the values: every element of an output buffer the kernel must not write is bitwise the sentinel it was
prefilled with, guards included; an input is bitwise unchanged; one slot, or one (slot, port), of a batch equals its own
call bit for bit.  A descriptor the header refuses must be refused with the class of its error code; nothing is skipped.

Every assertion message carries the case's dict: `realize_*` of that dict replays the case on the CPU.  Every input is one
the oracle and the header define.

The file's name sorts it behind test_zzzzzzzzzzzz_hip_ofdm.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import front_fuzz_cases as F
import ofdm_oracle as OO
import tpre_oracle as P
from srsran_ce_pytorch_amd import dmrs as DG, ofdm as OF, precode as PR, synth as S

pytestmark = pytest.mark.gpu

# Cases a run flagged, kept exactly as they were drawn (the dicts of front_fuzz_cases.draw_*); they run after the seeded ones.
LOGGED_PRE_CASES = []
LOGGED_OFDM_CASES = []
LOGGED_DMRS_CASES = []

GUARD = 64                                   # complex64 elements either side of a guarded buffer: keeps 16-byte alignment
FILL = np.complex64(complex(-5.0, 7.0))      # the sentinel
NAN = np.complex64(complex(np.nan, np.nan))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype, device=_dev())


def _case(draw, n, logged, idx):
    return draw(idx) if idx < n else logged[idx - n]


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)      # one word per complex64 element: the shape stays


def _is_fill(a):
    return bool(np.all(_bits(a) == _bits(np.array([FILL]))[0]))


# ---------------------------------------------------------------- transform precoding ----

def _pre_layout(c, side, n_slots):
    """(offsets, stride, extent, rows): `rows` marks, in a tensor of `extent` elements, those of its n_slots x S rows."""
    M, off, stride = 12 * c["n_prb"], F.pre_offsets(c, side), c[side + "_stride"]
    extent = (n_slots - 1) * stride + max(off) + M
    rows = np.zeros(extent, bool)
    for b in range(n_slots):
        for o in off:
            assert not rows[b * stride + o:b * stride + o + M].any()
            rows[b * stride + o:b * stride + o + M] = True
    assert rows.sum() == n_slots * c["S"] * M
    return off, stride, extent, rows


def _pre_run(pre, c, x, what):
    """x [n, S M] through ce_tp_precode in the case's form and geometry -> y's rows [n, S M].  x lies in a buffer whose other
    elements are NaN (the sentinel for an in-place form), y in one prefilled with the sentinel, both between guards and
    exactly as long as the header's extent.  Asserts what the call must leave alone."""
    n, M, S_ = x.shape[0], 12 * c["n_prb"], c["S"]
    in_place = c["form"].endswith("in place")
    x_off, x_stride, x_ext, _ = _pre_layout(c, "x", n)
    y_off, y_stride, y_ext, y_rows = _pre_layout(c, "y", n)
    host = np.full(x_ext + 2 * GUARD, FILL if in_place else NAN, np.complex64)
    host[:GUARD] = host[GUARD + x_ext:] = FILL
    for b in range(n):
        for r, o in enumerate(x_off):
            host[GUARD + b * x_stride + o:GUARD + b * x_stride + o + M] = x[b, r * M:(r + 1) * M]
    x_buf = _t(host)
    y_buf = x_buf if in_place else torch.full((y_ext + 2 * GUARD,), complex(FILL), dtype=torch.complex64, device=_dev())
    xp, yp = x_buf.data_ptr() + 8 * GUARD, y_buf.data_ptr() + 8 * GUARD
    assert xp % 16 == 0 and yp % 16 == 0
    offs = lambda v: None if v is None else (C.c_int32 * S_)(*v)   # noqa: E731  (NULL = dense rows)
    pre._plan()
    pre._launch(C.c_void_p(xp), x_stride, offs(c["x_off"]), C.c_void_p(yp), y_stride, offs(c["y_off"]), n)
    torch.cuda.synchronize()
    after = y_buf.cpu().numpy()
    body = after[GUARD:GUARD + y_ext]
    assert _is_fill(after[:GUARD]) and _is_fill(after[GUARD + y_ext:]), f"{what}: a guard of y was written"
    assert _is_fill(body[~y_rows]), f"{what}: y was written outside its rows, first at element {np.flatnonzero(~y_rows & (_bits(body) != _bits(np.array([FILL]))[0]))[:4].tolist()}"
    if not in_place:
        assert np.array_equal(_bits(x_buf), _bits(host)), f"{what}: x was written"
    return np.stack([np.concatenate([body[b * y_stride + o:b * y_stride + o + M] for o in y_off]) for b in range(n)])


@pytest.mark.parametrize("idx", range(F.N_PRE + len(LOGGED_PRE_CASES)))
def test_precoder_fuzz_case(idx):
    c = _case(F.draw_pre, F.N_PRE, LOGGED_PRE_CASES, idx)
    what = f"pre {c}"
    d = F.realize_pre(c)
    pre = PR.PuschTransformPrecoder(c["n_prb"], c["S"], device=_dev())
    got = _pre_run(pre, c, d.x, what)
    assert got.shape == (c["B"], c["S"] * d.M), what
    P.check(got, d.ref, d.M, what, t=F.T_PRE_FUZZ)
    if c["form"] == "dense":                         # the wrapper's call is the same launch
        y = pre(_t(d.x))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(y), _bits(got)), f"{what}: the wrapper's dense call differs"
    if c["B"] > 1:                                   # a slot of the batch against its own single-slot call, bit for bit
        b = c["slot"]
        one = _pre_run(pre, c, d.x[b:b + 1], what + f" slot {b} alone")
        assert np.array_equal(_bits(one)[0], _bits(got)[b]), f"{what}: slot {b} alone differs"


# ---------------------------------------------------------------- OFDM demodulator ----

def _ofdm_samples(c, s):
    """The device tensor [B, R, T] of samples s in the case's memory layout."""
    B, R, T = s.shape
    if c["layout"] == "odd view":                    # a view at an odd first sample of a longer capture: 8-byte aligned only
        cap = np.full((B, R, c["lead"] + T + c["tail"]), NAN if c["nan_outside"] else 0, np.complex64)
        cap[:, :, c["lead"]:c["lead"] + T] = s
        view = _t(cap)[:, :, c["lead"]:c["lead"] + T]
        assert view.data_ptr() % 16 == 8 and (B * R == 1 or not view.is_contiguous())
        return view
    if c["layout"] == "permuted":                    # [R, B, T] storage viewed as [B, R, T]: port_stride > slot_stride
        view = _t(s.transpose(1, 0, 2)).permute(1, 0, 2)
        assert view.stride() == (T, B * T, 1)
        return view
    if c["layout"] == "port stride 0":
        assert all(np.array_equal(_bits(s[:, r]), _bits(s[:, 0])) for r in range(R))
        return _t(s[:, :1]).expand(B, R, T)
    if c["layout"] == "slot stride 0":
        assert all(np.array_equal(_bits(s[b]), _bits(s[0])) for b in range(B))
        return _t(s[:1]).expand(B, R, T)
    return _t(s)


@pytest.mark.parametrize("idx", range(F.N_OFDM + len(LOGGED_OFDM_CASES)))
def test_demodulator_fuzz_case(idx):
    c = _case(F.draw_ofdm, F.N_OFDM, LOGGED_OFDM_CASES, idx)
    what = f"ofdm {c}"
    d = F.realize_ofdm(c)
    N, B, R, n_sym = c["n_fft"], c["B"], c["R"], c["n_sym"]
    dem = OF.PuschOfdmDemodulator(N, c["n_prb_grid"], c["cp_len"], n_sym=n_sym, window_advance=c["advance"], sym_phasor=d.phi, device=_dev())
    assert dem.n_samples == d.T, what
    samples = _ofdm_samples(c, d.samples)
    assert tuple(samples.shape) == (B, R, d.T), what
    out = buf = None
    n = B * R * n_sym * d.n_sc
    if c["out"]:                                     # NaN-prefilled between guards: every element is written, no guard is
        buf = torch.full((n + 2 * GUARD,), complex(NAN), dtype=torch.complex64, device=_dev())
        buf[:GUARD] = complex(FILL)
        buf[GUARD + n:] = complex(FILL)
        out = buf[GUARD:GUARD + n].view(B, R, n_sym, d.n_sc)
    y = dem(samples, out=out)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, R, d.n_sc, n_sym) and y.dtype == torch.complex64 and (out is None or y.data_ptr() == out.data_ptr()), what
    got = y.cpu().numpy()
    # the unit: rms_window |phi_l| where phasors are given -- the transform's error passes through that product at the store
    OO.check(got, d.ref, d.rms, N, what, t=F.T_OFDM_FUZZ)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    if buf is not None:
        after = buf.cpu().numpy()
        assert _is_fill(after[:GUARD]) and _is_fill(after[GUARD + n:]), f"{what}: a guard of out was written"
    if B * R > 1:                                    # a (slot, port) of the batch against its own call, bit for bit
        b, r = c["slot"], c["port"]
        one = dem(_t(d.samples[b:b + 1, r:r + 1]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(one)[0, 0], _bits(got)[b, r]), f"{what}: (slot, port) = ({b}, {r}) alone differs"


# ---------------------------------------------------------------- DM-RS generator ----

def _dmrs_param(p):
    """A parameter in its drawn form; the elements a strided view skips hold other values."""
    v = np.array(p["values"], np.int64)
    if p["form"] == "int":
        return int(v[0])
    if p["form"] == "host array":
        return v
    if p["form"] == "length-1 tensor":
        return _t(v[:1], torch.int32)
    if p["form"] == "stride-2 view":
        t = _t(np.stack([v, v[::-1] + 1], 1).reshape(-1).astype(np.int32))[::2]
        assert t.shape[0] == len(v) and (len(v) == 1 or t.stride(0) == 2)
        return t
    return _t(v.astype(np.int32))


@pytest.mark.parametrize("idx", range(F.N_DMRS + len(LOGGED_DMRS_CASES)))
def test_generator_fuzz_case(idx):
    c = _case(F.draw_dmrs, F.N_DMRS, LOGGED_DMRS_CASES, idx)
    what = f"dmrs {c}"
    h1, h2, _ = S.numpy_hops(F.dmrs_case_spec(c))
    make = lambda: DG.PuschDmrs(h1, h2, c["L"], c["n_prb_grid"], c["n_sym"], grid_start_crb=c["grid_start_crb"], n_symb_slot=c["n_symb_slot"], device=_dev())   # noqa: E731
    if c["refuse"]:                                  # a descriptor the header refuses: the class of its error code
        with pytest.raises(F.DMRS_REFUSAL_CLASS[c["refuse"]]):
            make()
        return
    d = F.realize_dmrs(c)
    gen = make()
    B = c["B"]
    shape = (B, gen.n_re, gen.n_dmrs_total, c["L"])
    assert d.ref.shape == shape, (what, d.ref.shape, shape)
    out = buf = None
    n = int(np.prod(shape))
    if c["out"]:                                     # between guards; first element 16-byte aligned, or 8 bytes off (the 8-byte store path)
        lead = GUARD - 1 if c["out_off8"] else GUARD
        buf = torch.full((lead + n + GUARD,), complex(FILL), dtype=torch.complex64, device=_dev())
        out = buf[lead:lead + n].view(shape)
        assert out.data_ptr() % 16 == (8 if c["out_off8"] else 0)
    got = gen(*(_dmrs_param(c["params"][k]) for k in ("slot", "n_id", "n_scid")), out=out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == shape and got.dtype == torch.complex64 and (out is None or got is out), what
    a, ref = got.cpu().numpy().view(np.int32), d.ref.view(np.int32)
    assert np.array_equal(a, ref), f"{what}: pilots differ, first at (slot, row, column, 2 layer + re/im) {np.argwhere(a != ref)[:4].tolist()}; slots {d.slots[:4]}"
    if buf is not None:
        after = buf.cpu().numpy()
        assert _is_fill(after[:lead]) and _is_fill(after[lead + n:]), f"{what}: a guard of out was written"
