"""GPU tests of the equalizer extension (include/ce_eq.h): the kernel's two outputs against the float64 oracle of
tests/eq_oracle.py under the tolerance rule stated there (T = 4 C, C measured by tests/test_eq.py on these same inputs).
Where two launches must agree (rx layouts, a slot alone and inside a batch) the comparison is bit for bit.

The file's name sorts it behind the rest of the suite: the equalizer consumes what the estimator's tests cover, and every
earlier GPU test keeps its place in the run."""
import math

import numpy as np
import pytest
import torch

import eq_oracle as Q
from srsran_ce_pytorch_amd import dmrs, equalizer as EQ, estimator as E, synth as S

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _eq(d):
    h1, h2, _ = S.numpy_hops(d.case)
    return EQ.PuschEqualizer(h1, h2, d.L, d.case["n_prb_grid"], d.case["n_sym"], reserved_re_mask=d.mask, device=_dev())


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())      # a copy: the shared inputs are read-only


def _rx_sc_fastest(rx):
    """[B, R, n_sc, n_sym] view of a [B, R, n_sym, n_sc] buffer: the layout the estimator's pilot loads coalesce on."""
    return _t(np.asarray(rx).transpose(0, 1, 3, 2)).contiguous().permute(0, 1, 3, 2)


def _run(d, eq=None, rx=None, ch_est=None, noise=None, out=None):
    eq = _eq(d) if eq is None else eq
    rx = _rx_sc_fastest(d.rx) if rx is None else rx
    ch = _t(d.ch_est if ch_est is None else ch_est)
    nz = _t(d.noise if noise is None else noise)
    x, nv = eq(rx, ch, nz, out=out)
    torch.cuda.synchronize()
    return x, nv


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("name", [c["name"] for c in Q.CASES])
def test_both_outputs_against_the_oracle(name):
    d = Q.inputs(name)
    eq = _eq(d)
    assert eq.n_data_re == len(d.data_re) and np.array_equal(eq.data_re(), d.data_re)
    x, nv = _run(d, eq)
    shape = (d.B, len(d.data_re), d.L)
    assert tuple(x.shape) == shape and tuple(nv.shape) == shape and x.dtype == torch.complex64 and nv.dtype == torch.float32
    assert x.device == _dev() and nv.device == _dev()
    Q.check(x.cpu().numpy(), nv.cpu().numpy(), d.ref, name)


@pytest.mark.parametrize("name", ["offset", "hopping", "short_alloc", "L4_R8"])
def test_rx_layouts_give_identical_bits(name):
    d = Q.inputs(name)
    eq = _eq(d)
    x0, n0 = _run(d, eq, rx=_rx_sc_fastest(d.rx))                          # permuted view of a [B, R, n_sym, n_sc] buffer
    x1, n1 = _run(d, eq, rx=_t(d.rx))                                     # contiguous [B, R, n_sc, n_sym]
    wide = torch.zeros((d.B, d.R, d.rx.shape[2], 2 * d.rx.shape[3] + 1), dtype=torch.complex64, device=_dev())
    wide[..., ::2][..., : d.rx.shape[3]] = _t(d.rx)
    x2, n2 = _run(d, eq, rx=wide[..., ::2][..., : d.rx.shape[3]])         # neither axis has unit stride
    Q.check(x0.cpu().numpy(), n0.cpu().numpy(), d.ref, name)
    for x, n in ((x1, n1), (x2, n2)):
        assert np.array_equal(_bits(x), _bits(x0)) and np.array_equal(_bits(n), _bits(n0))


def test_each_slot_of_a_batch_equals_its_own_single_slot_call():
    d = Q.inputs("batch5")
    assert d.B == 5 and len({tuple(r) for r in d.noise}) == 5            # per-slot noise differs
    eq = _eq(d)
    x, nv = _run(d, eq)
    Q.check(x.cpu().numpy(), nv.cpu().numpy(), d.ref, "batch5")
    for b in range(d.B):
        xb, nb = _run(d, eq, rx=_rx_sc_fastest(d.rx[b:b + 1]), ch_est=d.ch_est[b:b + 1], noise=d.noise[b:b + 1])
        assert np.array_equal(_bits(xb[0]), _bits(x[b])) and np.array_equal(_bits(nb[0]), _bits(nv[b])), b


@pytest.mark.parametrize("name", ["dmrs_data_type1", "hopping"])
def test_noise_special_values_drop_the_port(name):
    d = Q.inputs(name)
    eq = _eq(d)
    keep = [r for r in range(d.R) if r != 1]
    ref = Q.equalize_ref(d.rx[:, keep], d.ch_est[:, keep], d.noise[:, keep], d.data_re)
    for bad in (math.inf, 0.0, -1.0, math.nan):
        noise = d.noise.copy()
        noise[:, 1] = bad
        x, nv = _run(d, eq, noise=noise)
        Q.check(x.cpu().numpy(), nv.cpu().numpy(), ref, f"{name}: port 1 noise {bad}")
    # every port bad: no usable channel
    noise = np.array([[math.inf, 0.0, -1.0, math.nan]] * d.B)[:, : d.R]
    x, nv = _run(d, eq, noise=noise)
    assert not np.any(_bits(x)) and np.all(nv.cpu().numpy() == np.inf)
    # zero h at some data REs gives the same there, and the oracle's answer everywhere else
    ch = d.ch_est.copy()
    rows = np.arange(0, len(d.data_re), 7)
    ch[:, :, d.data_re[rows, 1], d.data_re[rows, 0], :] = 0
    x, nv = _run(d, eq, ch_est=ch)
    x, nv = x.cpu().numpy(), nv.cpu().numpy()
    assert np.all(x[:, rows] == 0) and np.all(nv[:, rows] == np.inf)
    ref0 = Q.equalize_ref(d.rx, ch, d.noise, d.data_re)
    assert np.all(ref0.b[:, rows] == 0)
    Q.check(x, nv, ref0, f"{name}: zero h")


def test_out_buffers_guards_and_argument_errors():
    d = Q.inputs("offset")
    eq, dev = _eq(d), _dev()
    n = d.B * len(d.data_re) * d.L
    guard = 64
    bx = torch.full((n + 2 * guard,), complex(7.0, -3.0), dtype=torch.complex64, device=dev)
    bn = torch.full((n + 2 * guard,), -5.0, dtype=torch.float32, device=dev)
    shape = (d.B, len(d.data_re), d.L)
    out = (bx[guard:guard + n].view(shape), bn[guard:guard + n].view(shape))
    x, nv = _run(d, eq, out=out)
    assert x is out[0] and nv is out[1]
    hx, hn = bx.cpu().numpy(), bn.cpu().numpy()
    assert np.all(hx[:guard] == np.complex64(7 - 3j)) and np.all(hx[guard + n:] == np.complex64(7 - 3j))
    assert np.all(hn[:guard] == -5.0) and np.all(hn[guard + n:] == -5.0)
    Q.check(hx[guard:guard + n].reshape(shape), hn[guard:guard + n].reshape(shape), d.ref, "out=")

    rx, ch, nz = _rx_sc_fastest(d.rx), _t(d.ch_est), _t(d.noise)
    good = (torch.empty(shape, dtype=torch.complex64, device=dev), torch.empty(shape, dtype=torch.float32, device=dev))
    eq(rx, ch, nz, out=good)
    ch_wide = torch.zeros(tuple(ch.shape[:-1]) + (2 * d.L,), dtype=torch.complex64, device=dev)
    off_x = torch.empty((n + 1,), dtype=torch.complex64, device=dev)[1:].view(shape)          # 8 bytes off 16-byte alignment
    off_n = torch.empty((n + 2,), dtype=torch.float32, device=dev)[2:].view(shape)
    off_ch = torch.empty((ch.numel() + 1,), dtype=torch.complex64, device=dev)[1:].view(ch.shape).copy_(ch)
    bad_calls = [
        dict(ch_est=ch_wide[..., ::2]),                                                        # not dense
        dict(ch_est=ch.to(torch.complex128)), dict(rx=rx.to(torch.complex128)), dict(noise=nz.float()),   # wrong dtype
        dict(ch_est=ch[:, :1]), dict(noise=nz[:, :1]), dict(rx=rx[:, :, :-12]),               # wrong shape
        dict(rx=rx.cpu()), dict(ch_est=ch.cpu()), dict(noise=nz.cpu()),                       # CPU tensor
        dict(ch_est=off_ch),                                                                   # misaligned
        dict(out=(good[0].cpu(), good[1])), dict(out=(good[0], good[1].double())), dict(out=(good[0][:, :-1], good[1][:, :-1])),
        dict(out=(torch.empty((d.B, len(d.data_re), 2 * d.L), dtype=torch.complex64, device=dev)[..., ::2], good[1])),
        dict(out=(off_x, good[1])), dict(out=(good[0], off_n)),
    ]
    for kw in bad_calls:
        args = dict(rx=rx, ch_est=ch, noise=nz, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            eq(args["rx"], args["ch_est"], args["noise"], out=args["out"])


def test_empty_batch_launches_nothing():
    d = Q.inputs("offset")
    eq, dev = _eq(d), _dev()
    n_sc, n_sym = d.rx.shape[2:]
    x, nv = eq(torch.empty((0, d.R, n_sc, n_sym), dtype=torch.complex64, device=dev),
               torch.empty((0, d.R, n_sc, n_sym, d.L), dtype=torch.complex64, device=dev),
               torch.empty((0, d.R), dtype=torch.float64, device=dev))
    assert tuple(x.shape) == (0, len(d.data_re), d.L) == tuple(nv.shape)
    assert x.dtype == torch.complex64 and nv.dtype == torch.float32


E2E_CASE = S.case_spec("eq_e2e_25prb", 52, [S.hop_spec([2, 11], 10, 25)], n_layers=2, seed=78)
E2E_PORTS = 4


def e2e_slot(pilots, data_re, rng):
    """One noiseless slot: `pilots` [n_re, n_dmrs, L] on the DM-RS REs and QPSK data on `data_re`, through the three-tap
    channel model of synth.build_case (no CFO).  Returns (grids [R, n_sc, n_sym] complex64, x_tx [n_data_re, L])."""
    case = E2E_CASE
    n_sc, n_sym, L = 12 * case["n_prb_grid"], case["n_sym"], case["n_layers"]
    hop = S.numpy_hops(case)[0]
    f_sc = np.arange(n_sc) * case["scs"]
    tap_delay = np.array([0.0, 100e-9, 300e-9]) + case["delay_ns"] * 1e-9
    tap_amp = np.array([1.0, 0.35, 0.2])
    x_tx = ((2 * rng.integers(0, 2, (len(data_re), L)) - 1) + 1j * (2 * rng.integers(0, 2, (len(data_re), L)) - 1)) / np.sqrt(2.0)
    grids = np.zeros((E2E_PORTS, n_sc, n_sym), np.complex64)
    res = np.flatnonzero(np.kron(hop.maskPRBs, hop.DMRSREmask[:, 0]))
    for r in range(E2E_PORTS):
        H = np.stack([(tap_amp * np.exp(2j * math.pi * rng.random(3)))[None, :] @ np.exp(-2j * math.pi * tap_delay[:, None] * f_sc[None, :])
                      for _ in range(L)], -1)[0]                                           # [n_sc, L]
        g = np.zeros((n_sc, n_sym), complex)
        for col, sym in enumerate(case["hops"][0]["dmrs_symbols"]):
            g[res, sym] = case["beta"] * np.sum(H[res] * pilots[:, col, :], -1)
        g[data_re[:, 1], data_re[:, 0]] = np.sum(H[data_re[:, 1]] * x_tx, -1)
        grids[r] = g.astype(np.complex64)
    return grids, x_tx


def test_end_to_end_estimate_then_equalize():
    dev = _dev()
    h1, h2, cfg = S.numpy_hops(E2E_CASE)
    pil = dmrs.PuschDmrs(h1, h2, 2, 52, device=dev)(13, 421, 1)
    eq = EQ.PuschEqualizer(h1, h2, 2, 52, device=dev)
    data_re = eq.data_re()
    assert np.array_equal(data_re, Q.data_re_ref(E2E_CASE))
    grids, x_tx = e2e_slot(pil[0].cpu().numpy(), data_re, np.random.default_rng(78))
    rx = torch.as_tensor(grids, device=dev)[None]
    ch_est, noise, *_ = E.estimate(rx, pil, E2E_CASE["beta"], h1, h2, cfg)
    x, nv = eq(rx, ch_est, noise)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (1, len(data_re), 2) == tuple(nv.shape)
    ref = Q.equalize_ref(grids[None], ch_est.cpu().numpy(), noise.cpu().numpy(), data_re)
    Q.check(x.cpu().numpy(), nv.cpu().numpy(), ref, "end to end")
    got = x[0].cpu().numpy()
    assert np.array_equal(np.sign(got.real), np.sign(x_tx.real)) and np.array_equal(np.sign(got.imag), np.sign(x_tx.imag))
