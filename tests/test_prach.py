"""CPU tests of the PRACH preamble detector (include/ce_tp.h `ce_prach_*`, srsran_ce_pytorch_amd/prach.py): the float64 oracle
of tests/prach_oracle.py on hand-made inputs, the library's host entry points (windows, tables, refusals) against it, the host
helpers, the wrapper's refusals, the calibration of the tolerance and the two conditions on the GPU tests' inputs.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import prach_oracle as PO
from srsran_ce_pytorch_amd import _lib, prach as PR

CSRC = _lib.CSRC
GEOMETRIES = [(139, 256), (139, 512), (571, 1024), (839, 1024), (839, 2048), (1151, 2048), (1151, 4096)]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _i32(values):
    return (C.c_int32 * max(len(values), 1))(*values)


def _derive(lib, L, N, roots, n_cs, n_shifts, combine=0):
    view, ws, wl = _lib.TpHostView(), (C.c_int32 * 64)(*([-7] * 64)), C.c_int32(-7)
    rc = lib.ce_prach_derive_host(L, N, len(roots), _i32(roots), n_cs, n_shifts, combine, C.byref(view), ws, C.byref(wl))
    return rc, view, list(ws), wl.value


# ---- the oracle on hand-made inputs ----

@pytest.mark.parametrize("L,N,n_cs,n_shifts", [(139, 256, 13, 10), (839, 1024, 13, 64), (139, 512, 0, 1)])
def test_one_aligned_preamble_gives_its_amplitude_squared_and_nothing_elsewhere(L, N, n_cs, n_shifts):
    """A noiseless preamble of amplitude a whose peak falls on an index of the N grid: peak = a^2 at that index, delay as
    expected, and in the other windows of the root only the side lobes of the Dirichlet kernel."""
    a, u, v = 0.7, 5, n_shifts // 2
    c_v = v * n_cs
    ws, wl = PO.windows(L, N, n_cs, n_shifts)
    d_want = 7
    # the delay that puts the peak on the index win_start[v] + d_want
    delay = ((int(ws[v]) + d_want) % N) * L / N - ((L - c_v) % L)
    y = (a * PO.preamble_freq(u, c_v, L, delay))[None, None, None, :]
    ref = PO.detect_ref(y, L, N, (u, 1), n_cs, n_shifts, 0)
    assert abs(ref.peak[0, 0, v] - a * a) < 1e-12 and ref.delay[0, 0, v] == d_want
    assert abs(PO.peak_position(L, N, c_v, delay) - (int(ws[v]) + d_want) % N) < 1e-9
    others = np.delete(ref.peak[0, 0], v)
    assert others.size == 0 or others.max() < 0.05 * a * a                      # side lobes: at most (L sin(pi x / L))^-2, x >= g - 1 samples of the L grid away
    assert abs(ref.mean[0, 0] - a * a / L) < 1e-12                              # Parseval: sum_n |z|^2 = (N / L^2) sum_k |Z|^2
    # a different root correlates at the 1 / L level everywhere
    assert ref.peak[0, 1].max() < 4.0 * a * a / L and abs(ref.mean[0, 1] - a * a / L) < 1e-12


def test_combining_and_term_order_of_the_oracle():
    rng = np.random.default_rng(1)
    y = rng.standard_normal((2, 3, 4, 139)) + 1j * rng.standard_normal((2, 3, 4, 139))
    non = PO.profile_ref(y, 139, 256, (1, 70), 0)
    each = sum(PO.profile_ref(y[:, r:r + 1, s:s + 1], 139, 256, (1, 70), 0) for r in range(3) for s in range(4))
    assert np.allclose(non, each, rtol=1e-12, atol=0)
    coh = PO.profile_ref(y, 139, 256, (1, 70), 1)
    assert np.allclose(coh, PO.profile_ref(y.sum(2, keepdims=True), 139, 256, (1, 70), 0), rtol=1e-12, atol=0)
    # the literal matrix and the library transform agree where both apply
    big = PO.profile_ref(y[:1, :1, :1], 139, 1024, (1,), 0)
    assert np.allclose(big[..., ::4], PO.profile_ref(y[:1, :1, :1], 139, 256, (1,), 0), rtol=1e-9, atol=1e-15)


# ---- the library's host entry points ----

@pytest.mark.parametrize("L,N", GEOMETRIES)
def test_windows_of_the_library_follow_the_formula_and_are_disjoint(lib, L, N):
    """Every n_cs that admits n_shifts >= 2, with the most windows it admits (up to 64): the formula, and pairwise disjoint."""
    g = -(-N // L)
    for n_cs in range(1, L // 2 + 1):
        n_shifts = min(L // n_cs, 64)
        rc, view, ws, wl = _derive(lib, L, N, [1], n_cs, n_shifts)
        assert rc == 0, (n_cs, _lib.last_error())
        want_ws, want_wl = PO.windows(L, N, n_cs, n_shifts)
        assert ws[:n_shifts] == [int(x) for x in want_ws] and wl == want_wl == (n_cs * N) // L and ws[n_shifts:] == [-7] * (64 - n_shifts)
        assert ws[0] == N - g                                                   # window 0 wraps round N
        seen = np.zeros(N, np.int32)
        for s in ws[:n_shifts]:
            seen[(s + np.arange(wl)) % N] += 1
        assert seen.max() == 1, (L, N, n_cs)
    rc, view, ws, wl = _derive(lib, L, N, [1], 0, 1)
    assert rc == 0 and ws[0] == 0 and wl == N and ws[1] == -7
    assert view.m_sc == N and view.threads == 256 and view.n_workgroups_per_slot == 1
    assert view.rows_per_workgroup == {256: 4, 512: 2, 1024: 2, 2048: 1, 4096: 1}[N] and view.lds_bytes == view.rows_per_workgroup * 16 * N
    assert int(np.prod(view.radix[:view.n_passes])) == N


@pytest.mark.parametrize("L", PO.L_RA)
def test_tables_of_the_library_against_the_oracle(lib, L):
    roots = [1, L - 1, L // 2 + 1, 2, 7, L - 3]
    N = 2048 if L > 1024 else 1024
    tw, tab = PR.tables(L, N, roots)
    want = PO.root_table(roots, L)
    assert tab.shape == (len(roots), L) and np.abs(tab - want).max() <= 1e-7
    assert np.abs(np.abs(tab.astype(np.complex128)) - 1.0).max() <= 1e-7
    assert np.abs(tw - np.exp(2j * np.pi * np.arange(N) / N)).max() <= 1e-7
    # a root's row does not depend on the other roots of the plan; either table may be left out
    _, one = PR.tables(L, N, [roots[3]])
    assert np.array_equal(one[0].view(np.uint64), tab[3].view(np.uint64))
    only = np.full((1, L), 7, np.complex64)
    assert lib.ce_prach_copy_tables(L, N, 1, _i32([roots[3]]), None, C.c_void_p(only.ctypes.data)) == 0 and np.array_equal(only, one)
    assert lib.ce_prach_copy_tables(L, N, 1, _i32([roots[3]]), None, None) == 0


def test_host_helpers():
    L, N = 139, 256
    x = PR.prach_root_freq(5, L)
    assert x.dtype == np.complex128 and np.abs(x - PO.root_freq(5, L)).max() < 1e-9 and np.abs(np.abs(x) - np.sqrt(L)).max() < 1e-9
    p = PR.prach_preamble_freq(5, 26, L, delay=3.25)
    assert np.abs(p - PO.preamble_freq(5, 26, L, 3.25)).max() < 1e-9 and np.abs(np.abs(p) - 1.0).max() < 1e-12
    # the preamble is the DFT of the cyclically shifted sequence: x_{u,v}(n) = x_u((n + C_v) mod L)
    shifted = np.roll(PO.zc(5, L), -26)
    assert np.abs(PR.prach_preamble_freq(5, 26, L) - PO.dft_matrix(L) @ shifted / np.sqrt(L)).max() < 1e-9
    ws, wl = PR.prach_windows(L, N, 13, 10)
    want = PO.windows(L, N, 13, 10)
    assert ws.dtype == np.int32 and np.array_equal(ws, want[0]) and wl == want[1]
    # arrival time: a preamble `delay` sequence samples late, found at the index nearest to its peak
    for v, delay in ((0, 0.0), (3, 4.4), (9, 7.8)):
        pos = PO.peak_position(L, N, v * 13, delay)
        d = (int(round(pos)) - int(ws[v])) % N
        assert 0 <= d < wl
        got = float(PR.prach_arrival_seconds(L, N, 13, v, d, 15e3))
        assert abs(got - delay / (L * 15e3)) <= 0.5 / (N * 15e3) + 1e-15
    assert float(PR.prach_arrival_seconds(L, 512, 0, 0, 37, 15e3)) == 37 / (512 * 15e3)     # n_cs = 0: the window starts at 0, no guard
    arr = PR.prach_arrival_seconds(L, N, 13, np.arange(10), np.zeros(10, np.int64), 15e3)
    assert arr.shape == (10,) and np.all(arr < 0) and np.all(arr >= -3.0 / (N * 15e3))      # the guard: ceil(N / L) = 2 samples and the fraction
    for bad in (lambda: PR.prach_root_freq(0, L), lambda: PR.prach_root_freq(L, L), lambda: PR.prach_root_freq(1, 140), lambda: PR.prach_preamble_freq(1, L, L),
                lambda: PR.prach_preamble_freq(1, -1, L), lambda: PR.prach_root_freq(1.0, L), lambda: PR.prach_windows(L, N, 13, 11)):
        with pytest.raises(ValueError):
            bad()


def test_exports_and_registration(lib):
    names = ["ce_prach_derive_host", "ce_prach_copy_tables", "ce_prach_plan_create", "ce_prach_plan_destroy", "ce_prach_detect"]
    assert [n for n in _lib.REGISTRY["ce_tp.h"].signatures if n.startswith("ce_prach_")] == names
    assert [len(getattr(lib, n).argtypes) for n in names] == [10, 6, 10, 1, 13]
    assert "ce_prach.hip" in _lib.SOURCES and (CSRC / "ce_prach.hip").is_file()
    from srsran_ce_pytorch_amd import PrachDetector, prach_preamble_freq     # noqa: F401


GOOD = dict(L=139, N=256, roots=[1, 138, 70], n_cs=13, n_shifts=10, combine=0)
BAD_PLANS = [("l_ra", dict(L=140)), ("l_ra", dict(L=0)), ("n_fft", dict(N=128)), ("n_fft", dict(N=300)), ("n_fft", dict(N=8192)), ("must exceed", dict(L=839, N=512)),
             ("must exceed", dict(L=1151, N=1024)), ("roots[1]", dict(roots=[1, 0])), ("roots[0]", dict(roots=[139])), ("roots[0]", dict(roots=[-1])),
             ("repeats", dict(roots=[5, 70, 5])), ("n_roots", dict(roots=[])), ("n_roots", dict(roots=list(range(1, 66)))),
             ("exceeds", dict(n_cs=14, n_shifts=10)), ("exceeds", dict(n_cs=70, n_shifts=2)), ("n_cs=0", dict(n_cs=0, n_shifts=2)), ("n_cs", dict(n_cs=-1)),
             ("n_cs", dict(n_cs=139, n_shifts=1)), ("n_shifts", dict(n_shifts=0)), ("n_shifts", dict(n_cs=1, n_shifts=65)), ("combine", dict(combine=2)),
             ("combine", dict(combine=-1))]


@pytest.mark.parametrize("text,change", BAD_PLANS, ids=[f"{i}_{t.split('[')[0].replace(' ', '_')}" for i, (t, _) in enumerate(BAD_PLANS)])
def test_host_entry_points_refuse(lib, text, change):
    """ce_prach_derive_host, ce_prach_copy_tables (where the value is one of its own) and ce_prach_plan_create -- which validates
    before it touches a device -- refuse with CE_ERR_INVALID and leave their outputs alone."""
    p = {**GOOD, **change}
    rc, view, ws, wl = _derive(lib, p["L"], p["N"], p["roots"], p["n_cs"], p["n_shifts"], p["combine"])
    assert rc == _lib.CE_ERR_INVALID and text in _lib.last_error(), _lib.last_error()
    assert ws == [-7] * 64 and wl == -7
    handle = C.c_void_p()
    rc = lib.ce_prach_plan_create(_lib.CE_ABI_VERSION, 0, p["L"], p["N"], len(p["roots"]), _i32(p["roots"]), p["n_cs"], p["n_shifts"], p["combine"], C.byref(handle))
    assert rc == _lib.CE_ERR_INVALID and text in _lib.last_error() and not handle.value
    if set(change) <= {"L", "N", "roots"}:
        buf = np.full(16, 7, np.float32)
        assert lib.ce_prach_copy_tables(p["L"], p["N"], len(p["roots"]), _i32(p["roots"]), C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data)) == _lib.CE_ERR_INVALID
        assert np.all(buf == 7)
    with pytest.raises(ValueError):
        PR.PrachDetector(p["L"], p["N"], p["roots"], p["n_cs"], p["n_shifts"], combine={0: "noncoherent", 1: "coherent"}.get(p["combine"], "both"))


def test_null_arguments_and_the_abi_version(lib):
    view, ws, wl, roots = _lib.TpHostView(), (C.c_int32 * 64)(), C.c_int32(), _i32([1])
    assert lib.ce_prach_derive_host(139, 256, 1, roots, 13, 10, 0, None, ws, C.byref(wl)) == _lib.CE_ERR_INVALID
    assert lib.ce_prach_derive_host(139, 256, 1, roots, 13, 10, 0, C.byref(view), None, C.byref(wl)) == _lib.CE_ERR_INVALID
    assert lib.ce_prach_derive_host(139, 256, 1, roots, 13, 10, 0, C.byref(view), ws, None) == _lib.CE_ERR_INVALID
    assert lib.ce_prach_derive_host(139, 256, 1, None, 13, 10, 0, C.byref(view), ws, C.byref(wl)) == _lib.CE_ERR_INVALID
    assert lib.ce_prach_copy_tables(139, 256, 1, None, None, None) == _lib.CE_ERR_INVALID
    handle = C.c_void_p()
    assert lib.ce_prach_plan_create(_lib.CE_ABI_VERSION, 0, 139, 256, 1, roots, 13, 10, 0, None) == _lib.CE_ERR_INVALID
    assert lib.ce_prach_plan_create(_lib.CE_ABI_VERSION + 1, 0, 139, 256, 1, roots, 13, 10, 0, C.byref(handle)) == _lib.CE_ERR_INVALID and "ABI" in _lib.last_error()
    lib.ce_prach_plan_destroy(None)


def test_detect_refuses_before_it_looks_at_the_plan_or_a_device(lib):
    """A null plan is refused first; the checks behind it run on made-up addresses in tests of the GPU file, where a plan exists."""
    a = C.c_void_p(0x1000)
    assert lib.ce_prach_detect(None, a, 0, 0, 0, 1, 1, 1, a, a, a, None, None) == _lib.CE_ERR_INVALID and "null" in _lib.last_error()


def test_wrapper_refuses_what_is_no_int_or_no_name():
    for kw in (dict(l_ra=139.0), dict(n_fft="256"), dict(roots=5), dict(roots=[1.5]), dict(roots="12"), dict(n_cs=True), dict(n_shifts=None), dict(combine="both"),
               dict(combine=0), dict(scs_ra_hz=0.0), dict(scs_ra_hz=float("nan")), dict(roots=[2 ** 40])):
        args = {**dict(l_ra=139, n_fft=256, roots=[1, 138], n_cs=13, n_shifts=10), **kw}
        with pytest.raises(ValueError):
            PR.PrachDetector(**args)
    det = PR.PrachDetector(139, 256, [1, 138, 70], 13, 10, combine="coherent")       # no GPU needed
    assert (det.l_ra, det.n_fft, det.roots, det.n_roots, det.n_cs, det.n_shifts, det.combine, det.scs_ra_hz) == (139, 256, (1, 138, 70), 3, 13, 10, "coherent", 15e3)
    assert (det.rows_per_workgroup, det.threads_per_row, det.win_len) == (4, 64, 23) and np.array_equal(det.win_start, PO.windows(139, 256, 13, 10)[0])
    assert PR.PrachDetector(839, 1024, [1], 0, 1).scs_ra_hz == 1.25e3


# ---- the tolerance and the conditions on the GPU tests' inputs ----

def _f32(d):
    c = d.c
    view, ws, wl = PR.derive_host(c["L"], c["N"], d.roots, c["n_cs"], c["n_shifts"])
    tw, tab = PR.tables(c["L"], c["N"], d.roots)
    return PO.detect_f32(d.y, c["L"], view, tw, tab, ws, wl, c["combine"])


def test_float32_restatement_calibrates_the_tolerance():
    """C_PRACH: the largest error ratio of the float32 restatement of the kernel's arithmetic over the GPU tests' inputs."""
    worst = 0.0
    for name in PO.CASE_NAMES:
        d = PO.inputs(name)
        f = _f32(d)
        r = [x for x in PO.ratios(f, d.ref, d.N)]
        print(f"{name}: profile {r[0]:.2f}, peak {r[1]:.2f}, mean {r[2]:.2f}")
        worst = max(worst, *r)
        PO.check(_AsKernel(f), d, name)                                 # the restatement itself passes the GPU tests' check
    print(f"C_PRACH = {worst:.2f} (recorded {PO.C_PRACH_RECORDED})")
    assert worst <= PO.C_PRACH_RECORDED and PO.T_PRACH == 4.0 * PO.C_PRACH_RECORDED
    assert worst >= 0.25 * PO.C_PRACH_RECORDED                                   # the recorded constant is a measurement, not a cushion


class _AsKernel:
    """The restatement's results in the dtypes the kernel writes."""

    def __init__(self, f):
        self.peak, self.mean, self.profile, self.delay = f.peak.astype(np.float32), f.mean.astype(np.float32), f.profile.astype(np.float32), f.delay.astype(np.int32)


def test_the_cases_reach_every_path():
    c = PO.CASES.values()
    assert {x["N"] for x in c} == set(PO.FFT_SIZES) and {x["L"] for x in c} == set(PO.L_RA) and {x["combine"] for x in c} == {0, 1}
    assert {len(x["occasions"]) for x in c} == {1, 3}
    terms = {(x["N"], x["R"] if x["combine"] else x["R"] * x["S"]) for x in c}
    assert {(256, 3), (256, 5), (512, 3), (256, 1)} <= terms and any(x["S"] == 12 for x in c) and any(x["n_cs"] == 0 for x in c) and any(x["n_shifts"] == 64 for x in c)
    assert any("noise" in x["occasions"] for x in c) and any("zero" in x["occasions"] for x in c)
    for name in PO.CASE_NAMES:
        d = PO.inputs(name)
        assert d.roots == (1, d.L - 1, d.L // 2 + 1)
        windows = {v for (_, _, v) in d.sent}
        assert 0 in windows and d.c["n_shifts"] - 1 in windows
        for b, kind in enumerate(d.c["occasions"]):
            if kind == "zero":
                assert not d.y[b].any() and not d.ref.peak[b].any() and not d.ref.delay[b].any() and not d.ref.mean[b].any()


@pytest.mark.parametrize("name", PO.CASE_NAMES)
def test_signal_windows_have_unambiguous_peaks_and_detection_has_room(name):
    """The two conditions on the inputs: in EVERY window with a transmitted preamble the oracle's gap between the largest and the
    second-largest value exceeds 100 times the two tolerances involved, and min hit ratio / max miss ratio >= 4."""
    d = PO.inputs(name)
    assert len(d.sent) == 3 * sum(k == "signal" for k in d.c["occasions"])
    for (gap, tol), s in zip(PO.signal_gaps(d), d.sent):
        assert gap > PO.GAP_TOLERANCES * tol, (name, s, gap, tol)
    hit, miss = PO.hit_miss(d)
    print(f"{name}: min hit ratio {hit:.1f}, max miss ratio {miss:.1f}")
    assert hit / miss >= PO.MIN_HIT_OVER_MISS
    # the zero-delay preamble of window 0 sits ceil(N / L) indices into its window; the late ones where their delay puts them
    ws = d.ref.win_start
    for (b, i, v), (_, _, delay) in zip(d.sent, PO.case_preambles(d.c) * len(d.c["occasions"])):
        pos = PO.peak_position(d.L, d.N, v * d.c["n_cs"], delay)
        assert (int(ws[v]) + int(d.ref.delay[b, i, v])) % d.N == int(round(pos)) % d.N, (name, b, i, v)
        assert abs(pos - round(pos)) <= 0.2 + 1e-9                               # away from the half-sample positions
