"""GPU tests of the soft-demapper extension (include/ce_demod.h): the kernel's LLRs against the float64 brute-force oracle
of tests/demod_oracle.py under the tolerance rule stated there (T = 4 C, C measured by tests/test_demod.py on these same
inputs), in both output formats, with and without descrambling.  Where two launches must agree (a slot alone and inside a
batch, one parameter for the batch and a tensor of equal values, descrambling as sign flips) the comparison is exact.

The file's name sorts it behind test_z_hip_eq.py: the demapper consumes what the equalizer's tests cover, and every
earlier GPU test keeps its place in the run."""
import math

import numpy as np
import pytest
import torch

import demod_oracle as D
import eq_oracle as Q
from srsran_ce_pytorch_amd import demod as DM, dmrs, equalizer as EQ, estimator as E, synth as S

pytestmark = pytest.mark.gpu
FORMATS = [torch.float32, torch.int8]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())      # a copy: the shared inputs are read-only


def _dem(d, fmt, descramble):
    return DM.PuschDemapper(d.qm, d.M, out_dtype=fmt, llr_scale=d.scale, descramble=descramble, device=_dev())


def _run(d, fmt, descramble, x=None, nvar=None, rnti=None, n_id=None, out=None, dem=None):
    dem = _dem(d, fmt, descramble) if dem is None else dem
    x = _t(d.x if x is None else x)
    nvar = _t(d.nvar if nvar is None else nvar)
    if descramble:
        rnti = _t(d.rnti, torch.int32) if rnti is None else rnti
        n_id = _t(d.n_id, torch.int32) if n_id is None else n_id
    llr = dem(x, nvar, rnti=rnti, n_id=n_id, out=out)
    torch.cuda.synchronize()
    return llr


def _check(llr, d, ref, tol, what):
    got = llr.cpu().numpy()
    return D.check(got, ref, tol, what, scale=d.scale if got.dtype == np.int8 else None)


@pytest.mark.parametrize("fmt", FORMATS, ids=["f32", "i8"])
@pytest.mark.parametrize("name", [c["name"] for c in D.CASES])
def test_llrs_against_the_oracle_and_descrambling_as_sign_flips(name, fmt):
    d = D.inputs(name)
    plain = _run(d, fmt, False)
    assert tuple(plain.shape) == (d.B, d.G) and plain.dtype == fmt and plain.device == _dev()
    _check(plain, d, d.ref, d.tol, f"{name} {fmt}")
    flip = D.flips(d.c)
    desc = _run(d, fmt, True)
    _check(desc, d, np.where(flip, -d.ref, d.ref), d.tol, f"{name} {fmt} descrambled")
    p, q = plain.cpu().numpy(), desc.cpu().numpy()
    assert np.array_equal(q, np.where(flip, -p, p))            # values: -0.0 == 0.0; int8 never holds -128
    assert flip.any() and not flip.all()


@pytest.mark.parametrize("fmt", FORMATS, ids=["f32", "i8"])
@pytest.mark.parametrize("name", ["16qam_37", "64qam_1003", "256qam_4099"])
def test_each_slot_of_a_batch_equals_its_own_single_slot_call(name, fmt):
    d = D.inputs(name)
    dem = _dem(d, fmt, True)
    whole = _run(d, fmt, True, dem=dem).cpu().numpy()
    for b in range(d.B):
        one = _run(d, fmt, True, x=d.x[b:b + 1], nvar=d.nvar[b:b + 1], rnti=_t(d.rnti[b:b + 1], torch.int32),
                   n_id=_t(d.n_id[b:b + 1], torch.int32), dem=dem).cpu().numpy()
        assert np.array_equal(one[0].view(np.uint8), whole[b].view(np.uint8)), b


@pytest.mark.parametrize("fmt", FORMATS, ids=["f32", "i8"])
def test_stride_0_parameters_equal_a_tensor_of_equal_values(fmt):
    d = D.inputs("64qam_1003")
    dem = _dem(d, fmt, True)
    rnti, n_id = d.rnti[2], d.n_id[2]
    a = _run(d, fmt, True, rnti=rnti, n_id=n_id, dem=dem).cpu().numpy()
    b = _run(d, fmt, True, rnti=_t([rnti] * d.B, torch.int32), n_id=_t([n_id] * d.B, torch.int32), dem=dem).cpu().numpy()
    wide = _t(np.repeat([rnti] * d.B, 3), torch.int32)[::3]                     # an element stride of 3
    c = _run(d, fmt, True, rnti=wide, n_id=n_id, dem=dem).cpu().numpy()
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    flip = np.broadcast_to(D.scrambling(D.c_init(rnti, n_id), d.G).astype(bool), (d.B, d.G))
    _check(torch.as_tensor(a), d, np.where(flip, -d.ref, d.ref), d.tol, f"one (rnti, n_id) for the batch {fmt}")


@pytest.mark.parametrize("fmt", FORMATS, ids=["f32", "i8"])
@pytest.mark.parametrize("name", ["16qam_37", "256qam_4099"])
def test_special_values_are_erasures(name, fmt):
    d = D.inputs(name)
    x, nv = d.x.copy(), d.nvar.copy()
    fx, fn = x.reshape(-1), nv.reshape(-1)
    bad_nv = [math.inf, 0.0, -1.0, math.nan, -math.inf]
    bad_x = [complex(math.inf, 0.1), complex(0.1, -math.inf), complex(math.nan, 0.2), complex(0.3, math.nan)]
    rows = np.arange(0, len(fx), 7)
    for i, r in enumerate(rows):
        k = i % (len(bad_nv) + len(bad_x))
        if k < len(bad_nv):
            fn[r] = bad_nv[k]
        else:
            fx[r] = bad_x[k - len(bad_nv)]
    ref, tol = D.llr_ref(x, nv, d.qm), D.unit_tolerance(x, nv, d.qm)
    erased = np.zeros(len(fx), bool)
    erased[rows] = True
    erased = np.repeat(erased, d.qm).reshape(d.B, d.G)
    assert np.all(ref[erased] == 0) and np.all(tol[erased] == 0) and np.all(tol[~erased] > 0)
    for descramble in (False, True):
        got = _run(d, fmt, descramble, x=x, nvar=nv)
        flip = D.flips(d.c) if descramble else np.zeros((d.B, d.G), bool)
        _check(got, d, np.where(flip, -ref, ref), tol, f"{name} {fmt} special values")
        assert np.all(got.cpu().numpy()[erased] == 0)
    # the equalizer's "no usable channel" convention
    got = _run(d, fmt, True, x=np.zeros_like(d.x), nvar=np.full_like(d.nvar, np.inf))
    assert not np.any(got.cpu().numpy())


def test_out_buffer_guards_on_a_misaligned_slot_row():
    d = D.inputs("16qam_37")
    assert d.G % 16 != 0 and d.G % 4 == 0
    dev = _dev()
    guard = 64                                                   # keeps the view 16-byte aligned; slot rows 1 and 2 are not
    for fmt, fill in ((torch.int8, 77), (torch.float32, -5.0)):
        buf = torch.full((d.B * d.G + 2 * guard,), fill, dtype=fmt, device=dev)
        out = buf[guard:guard + d.B * d.G].view(d.B, d.G)
        got = _run(d, fmt, True, out=out)
        assert got is out
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + d.B * d.G:] == fill)
        flip = D.flips(d.c)
        _check(out, d, np.where(flip, -d.ref, d.ref), d.tol, f"out= {fmt}")
    # float32 rows of an odd number of elements: G = 2 (one QPSK symbol)
    d = D.inputs("qpsk_1")
    buf = torch.full((d.B * d.G + 8,), -5.0, dtype=torch.float32, device=dev)
    out = buf[4:4 + d.B * d.G].view(d.B, d.G)
    _run(d, torch.float32, False, out=out)
    h = buf.cpu().numpy()
    assert np.all(h[:4] == -5.0) and np.all(h[4 + d.B * d.G:] == -5.0)
    D.check(h[4:4 + d.B * d.G].reshape(d.B, d.G), d.ref, d.tol, "out= qpsk_1")


def test_equalizer_shaped_inputs_are_accepted():
    d = D.inputs("qpsk_156")
    dem = _dem(d, torch.float32, False)
    flat = _run(d, torch.float32, False, dem=dem)
    x3, n3 = _t(d.x).view(d.B, 78, 2), _t(d.nvar).view(d.B, 78, 2)             # [B, n_data_re, L]
    got = dem(x3, n3)
    torch.cuda.synchronize()
    assert torch.equal(got, flat) and tuple(got.shape) == (d.B, d.G)


def test_argument_errors():
    d = D.inputs("16qam_37")
    dev = _dev()
    dem = _dem(d, torch.int8, True)
    x, nv = _t(d.x), _t(d.nvar)
    rnti, n_id = _t(d.rnti, torch.int32), _t(d.n_id, torch.int32)
    good = dem(x, nv, rnti=rnti, n_id=n_id)
    assert tuple(good.shape) == (d.B, d.G)
    x_wide = torch.zeros((d.B, 2 * d.M), dtype=torch.complex64, device=dev)
    off_x = torch.empty((d.B * d.M + 1,), dtype=torch.complex64, device=dev)[1:].view(d.B, d.M).copy_(x)     # 8 bytes off
    off_n = torch.empty((d.B * d.M + 1,), dtype=torch.float32, device=dev)[1:].view(d.B, d.M).copy_(nv)      # 4 bytes off
    off_o = torch.empty((d.B * d.G + 1,), dtype=torch.int8, device=dev)[1:].view(d.B, d.G)
    bad_calls = [
        dict(x_hat=x.to(torch.complex128)), dict(nvar=nv.double()), dict(x_hat=x.real.contiguous()),          # wrong dtype
        dict(x_hat=x[:, :-1]), dict(nvar=nv[:, :-1].contiguous()), dict(nvar=nv[:1]), dict(x_hat=x[:, :-1].contiguous(), nvar=nv[:, :-1].contiguous()),  # wrong shape
        dict(x_hat=x.cpu()), dict(nvar=nv.cpu()),                                                              # CPU tensor
        dict(x_hat=x_wide[:, ::2]),                                                                            # not dense
        dict(x_hat=off_x), dict(nvar=off_n),                                                                   # misaligned
        dict(rnti=None), dict(n_id=None), dict(rnti=None, n_id=None),                                          # missing with descramble=True
        dict(rnti=rnti[:2]), dict(n_id=n_id.long()), dict(rnti=rnti.cpu()), dict(rnti=70000), dict(n_id=-1), dict(n_id=1.5),
        dict(out=good.float()), dict(out=good[:, :-1]), dict(out=good.cpu()), dict(out=good[:2]), dict(out=off_o),
        dict(out=torch.empty((d.B, 2 * d.G), dtype=torch.int8, device=dev)[:, ::2]),
    ]
    for kw in bad_calls:
        args = dict(x_hat=x, nvar=nv, rnti=rnti, n_id=n_id, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            dem(args["x_hat"], args["nvar"], rnti=args["rnti"], n_id=args["n_id"], out=args["out"])
    with pytest.raises(ValueError, match="16-byte"):
        dem(off_x, nv, rnti=rnti, n_id=n_id)
    # a plan without descrambling needs neither parameter
    plain = DM.PuschDemapper(d.qm, d.M, out_dtype=torch.int8, llr_scale=d.scale, device=dev)
    assert tuple(plain(x, nv).shape) == (d.B, d.G)


def test_empty_batch_launches_nothing():
    d = D.inputs("16qam_37")
    dev = _dev()
    for fmt in FORMATS:
        dem = _dem(d, fmt, True)
        out = dem(torch.empty((0, d.M), dtype=torch.complex64, device=dev), torch.empty((0, d.M), dtype=torch.float32, device=dev),
                  rnti=1, n_id=2)
        assert tuple(out.shape) == (0, d.G) and out.dtype == fmt


def test_end_to_end_grid_to_descrambled_bits():
    """random bits -> scrambled -> 16QAM -> channel -> PuschDmrs -> estimate -> PuschEqualizer -> PuschDemapper:
    the hard decisions are the bits that were sent.  (tests/test_demod.py runs the same chain through the CPU oracles
    and checks the equalized symbols' margin to the 16QAM decision boundaries.)"""
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
    for fmt in FORMATS:
        dem = DM.PuschDemapper("16qam", eq.n_data_re * 2, out_dtype=fmt, llr_scale=1.0, descramble=True, device=dev)
        llr = dem(x_hat, nvar, rnti=D.E2E_RNTI, n_id=D.E2E_SCR_ID)
        torch.cuda.synchronize()
        got = llr[0].cpu().numpy()
        assert got.shape == bits.shape
        assert np.array_equal(got < 0, bits.astype(bool)), fmt
        if fmt == torch.float32:
            flip = D.scrambling(D.c_init(D.E2E_RNTI, D.E2E_SCR_ID), len(bits)).astype(bool)[None]
            xh, nv = x_hat.cpu().numpy(), nvar.cpu().numpy()
            ref = D.llr_ref(xh, nv, 4)
            D.check(llr.cpu().numpy(), np.where(flip, -ref, ref), D.unit_tolerance(xh, nv, 4), "end to end")
