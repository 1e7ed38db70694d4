"""What the draws of tests/front_fuzz_cases.py must satisfy by themselves, before tests/test_zzzzzzzzzzzzz_hip_front_fuzz.py
runs the kernels on them: every kernel path the pinned cases of the precoder, the OFDM demodulator and the DM-RS generator
leave out is reached by at least the stated number of cases (the three tables are printed); the row geometries are ones the
header accepts; the two tolerance constants are at least what the float32 restatements need; the library's host views agree
with the oracles on every draw and refuse the refused descriptors with the class of the header's error code.  No GPU."""
import collections

import numpy as np
import pytest

import dmrs_oracle as DM
import front_fuzz_cases as F
import ofdm_oracle as OO
import tp_oracle as TP
import tpre_oracle as P
from srsran_ce_pytorch_amd import deprecode as DP, ofdm as OF, synth as S
from test_chain_fuzz import ALL_RADIX, _report
from test_dmrs import kernel_combination

PRE_CLASSES_1 = ALL_RADIX + [f"threads_per_row {t}" for t in (64, 128, 256)] + ["S % rows_per_workgroup != 0"]
PRE_CLASSES_8 = ["form " + f for f in F.PRE_FORMS] + ["x dense, y rows", "x rows, y dense", "offsets not ascending", "a gap", "stride = extent"]
PRE_ALSO = [f"n_prb {n}" for n in F.TP_EDGE_PRBS] + ["x rows, y rows", "x and y geometries differ", "stride > extent", "B > 1"] + [f"rows_per_workgroup {n}" for n in (4, 2, 1)]
OFDM_CLASSES = ([f"n_fft {n}" for n in OF.FFT_SIZES] + ["cp " + k for k in F.OFDM_CP_KINDS] + ["cp_len 0 present", "cp_len N present", "advance = min cp > 0",
                "an odd window start", "a partial last workgroup at 4 rows", "a partial last workgroup at 2 rows"] + ["phasor " + k for k in F.OFDM_PHASORS]
                + ["layout " + k for k in F.OFDM_LAYOUTS] + ["n_prb_grid 1", "n_prb_grid = n_fft // 12"])
OFDM_ALSO = ["0 < advance < min cp", "out=", "NaN outside the windows", "more than one (slot, port)", "rows_per_workgroup 1"]
DMRS_ORDERS = ["masks 0x%03X 0x%03X" % (a, b) for t in (1, 2) for a in F.DMRS_MASKS[t] for b in F.DMRS_MASKS[t] if a != b]
DMRS_CLASSES = ([f"type {t}, L {n}" for t in (1, 2) for n in (1, 2, 3, 4)] + DMRS_ORDERS + ["two hops", "scattered", "crb 0", "crb 1..274", "crb 275..2199",
                "n_words >= 128", "n_symb_slot 12"] + [f"{n} as {f}" for n in ("slot", "n_id", "n_scid") for f in F.DMRS_PARAM_FORMS]
                + ["out-of-range device values", "store 16 bytes", "store 8 bytes"])
DMRS_ALSO = (["crb limit", "B = 257", "B > 1", "crb odd", "one hop", "n_sym < n_symb_slot", "out= aligned", "out= 8 bytes off", "grid <= 24"]
             + [f"grid {n}" for n in F.DMRS_WIDE_GRIDS] + ["refused: " + k for k in F.DMRS_REFUSALS])      # (counts the draw fixes)


def test_draws_are_reproducible_and_plain():
    for draw in (F.draw_pre, F.draw_ofdm, F.draw_dmrs):
        a, b = draw(7), draw(7)
        assert a == b and a != draw(8) and eval(repr(a)) == a     # a case replays from its printed dict
    for draw, n in ((F.draw_pre, F.N_PRE), (F.draw_ofdm, F.N_OFDM), (F.draw_dmrs, F.N_DMRS)):
        assert all(eval(repr(draw(i))) == draw(i) for i in range(n))
    assert (F.STAGE_PRE, F.STAGE_OFDM, F.STAGE_DMRS) == (9, 10, 11)      # behind the first two fuzzes' 1 .. 8
    assert F.BASE_SEED == 20261020


def _accepted_rows(M, S_, stride, offsets):
    """The header's conditions on one tensor's rows, from its text: even and >= 0, inside the stride, pairwise disjoint."""
    assert stride % 2 == 0 and len(offsets) == S_ and all(o >= 0 and o % 2 == 0 and o + M <= stride for o in offsets)
    s = sorted(offsets)
    assert all(b - a >= M for a, b in zip(s, s[1:]))


def test_precoder_draw_reaches_every_path_and_calibrates_the_tolerance():
    """A sweep over every valid size plus 32 row-geometry cases; C_PRE_FUZZ re-measured with tpre_oracle.precode_f32, the
    float32 restatement of the kernel's arithmetic, never with the kernel."""
    counts, worst = collections.Counter(), 0.0
    assert [F.draw_pre(i)["n_prb"] for i in range(F.N_PRE_SWEEP)] == TP.VALID_PRBS
    for i in range(F.N_PRE):
        c = F.draw_pre(i)
        counts.update(F.pre_classes(c))
        M = 12 * c["n_prb"]
        assert 1 <= c["S"] <= 14 and 1 <= c["B"] <= 5 and 0 <= c["slot"] < c["B"] and c["form"] in F.PRE_FORMS, c
        assert i < F.N_PRE_SWEEP or c["n_prb"] in F.TP_EDGE_PRBS or M <= 72, c
        for side in "xy":
            _accepted_rows(M, c["S"], c[side + "_stride"], F.pre_offsets(c, side))
        if c["form"].startswith("dense"):
            assert c["x_off"] is None and c["y_off"] is None and c["x_stride"] == c["y_stride"] == c["S"] * M, c
        elif c["form"] == "rows in place":
            assert c["x_off"] is not None and c["x_off"] == c["y_off"] and c["x_stride"] == c["y_stride"], c
        else:
            assert c["x_off"] is not None or c["y_off"] is not None, c
        d = F.realize_pre(c)
        assert d.x.dtype == np.complex64 and d.x.shape == d.ref.shape == (c["B"], c["S"] * M), c
        assert np.abs(d.x).reshape(c["B"], c["S"], M).max(-1).min() > 0, c                                    # no all-zero row
        view = DP.derive_host(c["n_prb"], c["S"])
        got = P.precode_f32(d.x, view, DP.twiddles(c["n_prb"], c["S"]))
        worst = max(worst, P.check(got, d.ref, M, f"float32 restatement {c}", t=F.C_PRE_FUZZ))
    _report("precoder", F.N_PRE, counts, PRE_CLASSES_1, 1)
    _report("precoder", F.N_PRE, counts, PRE_CLASSES_8, 8, PRE_ALSO)
    print(f"C_PRE_FUZZ = {worst:.3f} (recorded {F.C_PRE_FUZZ:g}, T = {F.T_PRE_FUZZ:g})")
    assert worst <= F.C_PRE_FUZZ and F.T_PRE_FUZZ == 4.0 * F.C_PRE_FUZZ and round(F.C_PRE_FUZZ, 1) == F.C_PRE_FUZZ
    assert worst >= 0.25                                          # the restatement is float32 indeed


def test_demodulator_draw_reaches_every_path_is_accepted_and_calibrates_the_tolerance():
    """ofdm.derive_host accepts every draw; its window starts (through the slot length the wrapper derives) and T are
    ofdm_oracle.geometry's; C_OFDM_FUZZ re-measured with ofdm_oracle.demodulate_f32 under the unit the GPU test uses."""
    counts, worst, worst_by = collections.Counter(), 0.0, collections.defaultdict(float)
    for i in range(F.N_OFDM):
        c = F.draw_ofdm(i)
        counts.update(F.ofdm_classes(c))
        N, cp = c["n_fft"], c["cp_len"]
        assert N in OF.FFT_SIZES and 1 <= c["n_prb_grid"] <= N // 12 and 1 <= c["n_sym"] == len(cp) <= 14 and all(0 <= v <= N for v in cp), c
        assert 0 <= c["advance"] <= min(cp) and 1 <= c["B"] <= 3 and 1 <= c["R"] <= 4 and c["lead"] % 2 == 1, c
        assert c["cp_kind"] != "extended" or (cp == [N // 4] * c["n_sym"] and c["n_sym"] <= 12), c
        assert c["cp_kind"] != "normal" or cp == OF.nr_cp_lengths(c["scs"], N, c["n_sym"], c["cp_slot"]), c
        view = OF.derive_host(N, c["n_prb_grid"], cp, c["n_sym"], c["advance"])            # raises where the library refuses the draw
        w, T = OO.geometry(N, cp, c["advance"])
        dem = OF.PuschOfdmDemodulator(N, c["n_prb_grid"], cp, n_sym=c["n_sym"], window_advance=c["advance"])
        assert dem.n_samples == T == sum(cp) + c["n_sym"] * N and view.m_sc == N and view.n_workgroups_per_slot == -(-c["n_sym"] // view.rows_per_workgroup), c
        assert w == [sum(cp[:l]) + l * N + cp[l] - c["advance"] for l in range(c["n_sym"])] and w[0] >= 0 and w[-1] + N <= T, c
        d = F.realize_ofdm(c)
        assert d.samples.shape == (c["B"], c["R"], T) and d.samples.dtype == np.complex64 and np.all(np.isfinite(d.ref)) and np.all(d.rms > 0), c
        inside = F.ofdm_inside(c)
        assert np.all(np.isfinite(d.samples[:, :, inside])) and (not c["nan_outside"] or np.all(np.isnan(d.samples[:, :, ~inside]))), c
        assert (d.phi is None) == (c["phasor"] == "none"), c
        if c["phasor"] == "unit":
            assert np.abs(np.abs(d.phi) - 1).max() < 1e-6, c
        if c["phasor"] == "scaled":
            assert 0.25 <= np.abs(d.phi).min() and np.abs(d.phi).max() <= 4.0 + 1e-6, c
        got = OO.demodulate_f32(d.samples, view, OF.twiddles(N), c["n_prb_grid"], cp, c["advance"], d.phi)
        r = OO.check(got, d.ref, d.rms, N, f"float32 restatement {c}", t=F.C_OFDM_FUZZ)
        worst, worst_by[c["phasor"]] = max(worst, r), max(worst_by[c["phasor"]], r)
    _report("OFDM demodulator", F.N_OFDM, counts, OFDM_CLASSES, 5, OFDM_ALSO)
    print("largest ratio per phasor kind: " + ", ".join(f"{k} {worst_by[k]:.3f}" for k in F.OFDM_PHASORS))
    print(f"C_OFDM_FUZZ = {worst:.3f} (recorded {F.C_OFDM_FUZZ:g}, T = {F.T_OFDM_FUZZ:g})")
    assert worst <= F.C_OFDM_FUZZ and F.T_OFDM_FUZZ == 4.0 * F.C_OFDM_FUZZ and round(F.C_OFDM_FUZZ, 1) == F.C_OFDM_FUZZ
    assert worst >= 0.25


def test_generator_draw_reaches_every_path_and_the_host_view_reproduces_the_oracle():
    """Coverage counts; a refused draw is refused with the class of the header's error code; the limit-crb draws against the
    integers; every other draw whose kept window ends below word DMRS_HOST_WORDS through test_dmrs.kernel_combination -- the
    kernel's arithmetic on the library's host view -- against dmrs_oracle.pilots_ref of the draw's first slot, bit for bit."""
    counts = collections.Counter()
    n_oracle = 0
    for i in range(F.N_DMRS):
        c = F.draw_dmrs(i)
        counts.update(F.dmrs_classes(c))
        grid, crb = c["n_prb_grid"], c["grid_start_crb"]
        assert (1 <= grid <= 24 or grid in F.DMRS_WIDE_GRIDS) and c["type"] in (1, 2) and 1 <= c["L"] <= 4 and len(c["masks"]) == 2, c
        assert set(c["params"]) == {"slot", "n_id", "n_scid"} and all(len(p["values"]) in (1, c["B"]) for p in c["params"].values()), c
        assert all((p["form"] in F.DMRS_BATCH_FORMS) or len(p["values"]) == 1 for p in c["params"].values()), c
        assert all(-(1 << 31) <= v < (1 << 31) for p in c["params"].values() for v in p["values"]), c
        wild = [name for name, p in c["params"].items() if any(not 0 <= v <= ((1 << 31) - 1 if name == "slot" else F.DMRS_PARAM_RANGE[name]) for v in p["values"])]
        assert bool(wild) == c["out_of_range"] and (not wild or all(p["form"] in F.DMRS_DEVICE_FORMS for p in c["params"].values())), c
        if c["refuse"]:
            assert c["refuse"] == F._dmrs_refusal(i), c
            with pytest.raises(F.DMRS_REFUSAL_CLASS[c["refuse"]]):
                F.dmrs_view(c)
            continue
        assert c["masks"][0] != c["masks"][1] and set(c["masks"]) <= set(F.DMRS_MASKS[c["type"]]) and 6 * (crb + grid) <= 1 << 20, c
        syms = [s for h in c["hops"] for s in h["dmrs_symbols"]]
        assert len(set(syms)) == len(syms) and all(0 <= s < c["n_sym"] for s in syms) and all(1 <= len(h["dmrs_symbols"]) <= 4 for h in c["hops"]), c
        assert c["n_sym"] <= c["n_symb_slot"] and len({len(h["mask_prbs"]) if h["mask_prbs"] is not None else h["n_prbs"] for h in c["hops"]}) == 1, c
        n_cols = len(syms)
        assert c["B"] in (1, 257) or c["B"] * n_cols * (1602 + 12 * (crb + grid)) <= F.DMRS_MAX_BITS, c
        view = F.dmrs_view(c)
        lo, hi = F.dmrs_span(c)
        ppp = 6 if c["type"] == 1 else 4
        assert (view.ppp, view.n_re, view.n_dmrs_total) == (ppp, ppp * c["hops"][0]["n_prbs"], n_cols), c
        assert [view.word0[h] for h in range(len(c["hops"]))] == lo and [view.n_words[h] for h in range(len(c["hops"]))] == [b - a + 1 for a, b in zip(lo, hi)], c
        assert [view.col_sym[k] for k in range(n_cols)] == syms and [view.col_hop[k] for k in range(n_cols)] == [h for h, hop in enumerate(c["hops"]) for _ in hop["dmrs_symbols"]], c
        if i in F.DMRS_LIMIT_CASES:
            assert crb == F.DMRS_CRB_LIMIT - grid - F.DMRS_LIMIT_CASES[i] and c["B"] == 1 and n_cols == 1 and c["crb_band"] == "limit", c
            assert view.m[0][view.n_re - 1] == ppp * (crb + max(c["hops"][0]["mask_prbs"] or [c["hops"][0]["prb_start"] + c["hops"][0]["n_prbs"] - 1])) + ppp - 1, c
            continue
        assert max(hi) < F.DMRS_HOST_WORDS, c
        slot, n_id, n_scid = F.dmrs_slot_params(c)[0]
        ref = DM.pilots_ref(F.dmrs_case_spec(c), slot, n_id, n_scid, c["n_symb_slot"], crb)
        got = kernel_combination(view, c["L"], slot % (1 << 32), n_id % (1 << 32), n_scid % (1 << 32), c["n_symb_slot"])
        assert got.shape == ref.shape and np.array_equal(got.view(np.int32), ref.view(np.int32)), c
        n_oracle += 1
    _report("DM-RS generator", F.N_DMRS, counts, DMRS_CLASSES, 5, DMRS_ALSO)
    print(f"{counts['refused']} refused descriptors; {n_oracle} host views against the oracle; limit cases " + ", ".join(
        f"{i}: crb {F.draw_dmrs(i)['grid_start_crb']} word0 {F.dmrs_span(F.draw_dmrs(i))[0][0]}" for i in F.DMRS_LIMIT_CASES))
    assert counts["refused"] == 8 and counts["crb limit"] == 4 and counts["B = 257"] == 2 and n_oracle == F.N_DMRS - 12
    assert all(F.dmrs_span(F.draw_dmrs(i))[0][0] > 40000 for i in F.DMRS_LIMIT_CASES)     # the kept window far into the sequence


def test_generator_realization_matches_its_draw():
    """Every tenth accepted draw realized: the shape, and slots of different parameters differ."""
    for i in range(0, F.N_DMRS, 10):
        c = F.draw_dmrs(i)
        if c["refuse"] or i in F.DMRS_LIMIT_CASES:
            continue
        d = F.realize_dmrs(c)
        view = F.dmrs_view(c)
        assert d.ref.shape == (c["B"], view.n_re, view.n_dmrs_total, c["L"]) and d.ref.dtype == np.complex64, c
        assert np.all(np.abs(np.abs(d.ref.real) - float(DM.A)) == 0) and np.all(np.abs(np.abs(d.ref.imag) - float(DM.A)) == 0), c
        h1, h2, _ = S.numpy_hops(d.case)
        assert int(h1.DMRSsymbols.sum()) == len(c["hops"][0]["dmrs_symbols"]), c
