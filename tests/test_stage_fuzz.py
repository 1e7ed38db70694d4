"""What the draws of tests/stage_fuzz_cases.py must satisfy by themselves, before tests/test_zzzz_hip_stage_fuzz.py runs the
kernels on them: every kernel path the hand-picked cases leave out is reached by at least MIN_PER_CLASS cases of its
stage; the library derives and refuses the rate-recovery descriptors as the oracle does, and the kernel's gather
arithmetic restated in numpy (test_rm.check_gather_arithmetic) agrees with the oracle's literal walk on them, so a GPU
mismatch there points at the kernel around the closed form; the two tolerance constants are at least what the float32
restatements need; and the equalizer's rule stays tight on every element.  No GPU."""
import collections

import numpy as np
import pytest
import torch

import demod_oracle as D
import eq_oracle as Q
import rm_oracle as R
import stage_fuzz_cases as F
from srsran_ce_pytorch_amd import equalizer as EQ, ratematch as RM, synth as S
from test_rm import _same, check_gather_arithmetic

MIN_PER_CLASS = 8
RM_CLASSES = ["B > 8", "B > 8, B % 8 != 0", "odd N_cb, C > 1", "lead 1 or 3", "lead != 0, C > 1", "extra tile", "N_cb == K - 2 Zc", "max E > 2 P",
              "repetition, C > 1, e_lo != e_hi", "k0[rv] in the fillers", "rv tensor", "rv strided", "rv scalar", "harq none", "harq separate",
              "harq in_place", "guarded"]
EQ_CLASSES = ([f"n_sym {n}" for n in F.EQ_N_SYM] + [f"R {r}" for r in (3, 5, 6, 7)] + [f"mask 0x{m:03x}" for m in F.EQ_MASKS]
              + [f"scale {a:g}" for a in F.EQ_SCALES] + [f"layout {k}" for k in range(3)]
              + ["B > 5", "another PRB start", "first hop starts after symbol 0", "two hops of unequal width", "two hops overlapping partly inside a chunk"])
DM_CLASSES = ([f"Qm {q}" for q in (2, 4, 6, 8)] + ["M at a tile boundary", "B > 3", "odd M, B > 1", "scale no power of two", "rnti 0", "rnti 65535", "n_id 0",
                                                   "n_id 1023", "params scalar", "params tensor", "params stride0", "descramble", "plain", "erasures",
                                                   "nvar spread above x16", "beyond the outer level"])


def _report(stage, counts, classes):
    print(f"{stage}: cases per class over {F.N_CASES} draws")
    for k in classes:
        print(f"  {k:>45}: {counts[k]}")
    short = {k: counts[k] for k in classes if counts[k] < MIN_PER_CLASS}
    assert not short, f"{stage}: classes below {MIN_PER_CLASS} cases: {short}"


@pytest.fixture(scope="module")
def rm_cases():
    return [F.draw_rm(i) for i in range(F.N_CASES)]


def test_draws_are_reproducible_and_plain():
    for draw in (F.draw_rm, F.draw_eq, F.draw_dm):
        a, b = draw(7), draw(7)
        assert a == b and a != draw(8) and eval(repr(a)) == a     # a case replays from its printed dict


def test_rate_recovery_draw_reaches_every_path(rm_cases):
    counts = collections.Counter(k for c in rm_cases for k in F.rm_classes(c))
    _report("rate recovery", counts, RM_CLASSES)
    assert 1 <= counts["refused"] <= F.N_CASES // 10, counts["refused"]
    assert sum(c["B"] > 8 for c in rm_cases) * 3 >= F.N_CASES
    assert {c["B"] for c in rm_cases} == set(range(1, 21)) and {rv for c in rm_cases for rv in c["rvs"]} == {0, 1, 2, 3}
    assert {c["qm"] for c in rm_cases} == {2, 4, 6, 8} and {c["L"] for c in rm_cases} == {1, 2, 3, 4} and {c["bg"] for c in rm_cases} == {1, 2}
    assert max(c["G"] for c in rm_cases) <= F.RM_MAX_G + 1


def test_library_derives_and_refuses_the_rate_recovery_draws_as_the_oracle(rm_cases):
    n_refused = 0
    for c in rm_cases:
        d = F.rm_derive(c)
        args = (c["bg"], c["A"], c["qm"], c["L"], c["G"])
        for dtype in (torch.int8, torch.float32):
            if isinstance(d, Exception):
                with pytest.raises(type(d)):
                    RM.derive_host(*args, dtype, c["n_ref"])
                with pytest.raises(type(d)):
                    RM.PuschRateRecovery(*args, dtype=dtype, n_ref=c["n_ref"], filler_llr=F.RM_FILLER)
            else:
                _same(RM.derive_host(*args, dtype, c["n_ref"]), d)
        n_refused += isinstance(d, Exception)
    print(f"{n_refused} descriptors refused alike")


def test_kernel_gather_arithmetic_on_the_rate_recovery_draws(rm_cases):
    """Slots 0..3, 8, 9 and the batch's last, under every rv, both formats."""
    for c in rm_cases:
        d = F.rm_derive(c)
        if isinstance(d, Exception):
            continue
        slots = sorted({0, 1, 2, 3, 8, 9, c["B"] - 1})
        for unit, dtype in ((1, torch.float32), (4, torch.int8)):
            try:
                check_gather_arithmetic(d, RM.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], dtype, c["n_ref"]), unit, slots)
            except AssertionError as e:
                raise AssertionError(f"{c}: unit {unit}: {e}") from e


def test_rate_recovery_values_saturate_where_the_draw_says(rm_cases):
    """int8 sums leave [-127, 127] in (nearly) every repetition case and nowhere else: both branches of the clamp run."""
    n_rep = n_sat = 0
    for c in rm_cases[::5]:
        d = F.rm_derive(c)
        if isinstance(d, Exception):
            continue
        x = F.realize_rm(c)
        wide, _ = R.recover(d, x.llr_i8.astype(np.float32), c["rvs"], x.harq_i8.astype(np.float32), F.RM_FILLER)
        wide[:, :, d.f0:d.f1] = 0
        saturated = bool(np.any(np.abs(wide) > 127))
        rep = max(d.E) > d.P
        assert rep or not saturated, c
        n_rep, n_sat = n_rep + rep, n_sat + saturated
    print(f"{n_rep} repetition cases of {len(rm_cases[::5])} sampled, {n_sat} saturate")
    assert n_sat >= 3


def test_equalizer_draw_reaches_every_path_and_keeps_the_rule_tight():
    """Coverage counts; the library's data-RE enumeration against the plain loops; C_EQ_FUZZ re-measured with equalize_f32;
    and, from the oracle alone: b > 0 everywhere and no element's relative tolerance above 5e-2 (the bound of
    test_eq.py::test_the_draw_keeps_the_rule_tight), so an O(1) indexing error cannot hide under the rule."""
    counts, worst, worst_tol = collections.Counter(), 0.0, 0.0
    for i in range(F.N_CASES):
        c = F.draw_eq(i)
        counts.update(F.eq_classes(c))
        assert 1 <= c["L"] <= c["R"] <= 8 and 1 <= c["B"] <= 12 and 1 <= c["n_prb_grid"] <= 24, c
        d = F.realize_eq(c)
        case = F.eq_case_spec(c)
        h1, h2, _ = S.numpy_hops(case)
        eq = EQ.PuschEqualizer(h1, h2, c["L"], c["n_prb_grid"], c["n_sym"], reserved_re_mask=c["mask"])
        assert eq.n_data_re == len(d.data_re) > 0 and np.array_equal(eq.data_re(), d.data_re), c
        assert np.all(d.ref.b > 0), c
        tol = float(Q.rel_tolerance(d.ref, F.T_EQ_FUZZ).max())
        assert tol <= 5e-2, (c, tol)
        x, nvar = Q.equalize_f32(d.rx, d.ch_est, d.noise, d.data_re)
        rx_, rn_ = Q.error_ratios(x, nvar, d.ref)
        worst, worst_tol = max(worst, float(rx_.max()), float(rn_.max())), max(worst_tol, tol)
    _report("equalizer", counts, EQ_CLASSES)
    print(f"C_EQ_FUZZ = {worst:.2f} (recorded {F.C_EQ_FUZZ:g}, T = {F.T_EQ_FUZZ:g}); largest relative tolerance {worst_tol:.2e}")
    assert worst <= F.C_EQ_FUZZ and F.T_EQ_FUZZ == 4.0 * F.C_EQ_FUZZ and round(F.C_EQ_FUZZ, 1) == F.C_EQ_FUZZ


def test_demapper_draw_reaches_every_path_and_calibrates_the_tolerance():
    counts, worst = collections.Counter(), 0.0
    for i in range(F.N_CASES):
        c = F.draw_dm(i)
        d = F.realize_dm(c)
        counts.update(F.dm_classes(c, d))
        assert d.x.dtype == np.complex64 and d.nvar.dtype == np.float32 and d.scale > 0 and np.isfinite(d.scale), c
        assert np.all(d.ref[np.repeat(d.erased, d.qm, axis=1)] == 0) and np.all((d.tol == 0) == np.repeat(~D.usable(d.x, d.nvar), d.qm, axis=1)), c
        assert len(c["rnti"]) == len(c["n_id"]) == c["B"] and (c["param_kind"] == "tensor" or len(set(zip(c["rnti"], c["n_id"]))) == 1), c
        live = d.tol > 0
        if live.any():
            with np.errstate(invalid="ignore"):
                f32 = D.llr_f32(d.x, d.nvar, d.qm).astype(np.float64)
            worst = max(worst, float((np.abs(f32 - d.ref)[live] / d.tol[live]).max()))
    _report("demapper", counts, DM_CLASSES)
    assert all(counts[f"M {m}"] >= 1 for m in F.DM_EDGE_M), counts
    print(f"C_DEMOD_FUZZ = {worst:.2f} (recorded {F.C_DEMOD_FUZZ:g}, T = {F.T_DEMOD_FUZZ:g})")
    assert worst <= F.C_DEMOD_FUZZ and F.T_DEMOD_FUZZ == 4.0 * F.C_DEMOD_FUZZ and round(F.C_DEMOD_FUZZ, 1) == F.C_DEMOD_FUZZ
