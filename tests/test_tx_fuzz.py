"""What the draws of tests/tx_fuzz_cases.py must satisfy by themselves, before tests/test_zzzzzzzzzzzzzzz_hip_tx_fuzz.py runs the
OFDM modulator on them: every kernel path the pinned cases of ofdm_oracle.CASES leave out is reached by at least the stated
number of cases (the table is printed); `ofdm.derive_host` accepts every draw and the output geometry is one the header accepts;
the two tolerance constants are at least what the float32 restatements need; an all-zero symbol is exactly 0 in both the
reference and the restatement; and the float64 oracles agree on the pairing the GPU round trip relies on.  No GPU."""
import collections

import numpy as np

import ofdm_oracle as OO
import ofdm_tx_oracle as X
import tx_fuzz_cases as F
from srsran_ce_pytorch_amd import ofdm as OF
from test_chain_fuzz import _report

TX_CLASSES = ([f"n_fft {n}" for n in OF.FFT_SIZES] + ["n_prb_grid 1", "n_prb_grid = n_fft // 12"] + [f"rows_per_workgroup {n}" for n in (4, 2, 1)]
              + ["a partial last workgroup at 4 rows", "a partial last workgroup at 2 rows"] + ["cp " + k for k in F.TX_CP_KINDS]
              + ["cp_len 0 present", "cp_len N present", "an odd symbol start"] + ["phasor " + k for k in F.TX_PHASORS]
              + ["layout " + k for k in F.TX_LAYOUTS] + ["an odd first sample", "more than one (slot, port)", "zero PRBs", "a zero symbol",
                                                         "built through for_demodulator"])
TX_ALSO = ([f"n_prb_grid = n_fft // 12 at n_fft {n}" for n in OF.FFT_SIZES] + ["more than one workgroup per (slot, port)", "B R >= 64", "an odd row stride",
           "grid behind the buffer's start", "advance = min cp > 0", "0 < advance < min cp"])


def _draws():
    return [F.draw_tx(i) for i in range(F.N_TX)]


def _view(c):
    return OF.derive_host(c["n_fft"], c["n_prb_grid"], c["cp_len"], c["n_sym"], 0)


def test_draws_are_reproducible_and_plain():
    a, b = F.draw_tx(7), F.draw_tx(7)
    assert a == b and a != F.draw_tx(8) and eval(repr(a)) == a            # a case replays from its printed dict
    assert all(eval(repr(c)) == F.draw_tx(c["idx"]) for c in _draws())
    assert F.STAGE_TX == 12 and F.N_TX == 120 and F.BASE_SEED == 20261020  # behind the earlier fuzzes' 1 .. 11
    d, e = F.realize_tx(a), F.realize_tx(b)
    assert np.array_equal(d.grid.view(np.uint64), e.grid.view(np.uint64)) and np.array_equal(d.ref, e.ref)


def test_every_class_is_reached():
    counts = collections.Counter()
    for c in _draws():
        counts.update(F.tx_classes(c))
    _report("OFDM modulator", F.N_TX, counts, TX_CLASSES, 3, TX_ALSO)
    assert counts["B R >= 64"] == len(F.TX_BIG_BATCH_CASES) == 2


def test_every_draw_is_accepted_by_the_library_and_the_rows_do_not_overlap():
    """ofdm.derive_host accepts every draw and the wrapper's T is the oracle's; the output geometry by the header's own rule,
    computed from the strides: the rows marked in a boolean array, no element twice (inside tx_rows), and in one of the two
    nestings the header names."""
    for c in _draws():
        N, cp, B, R = c["n_fft"], c["cp_len"], c["B"], c["R"]
        assert N in OF.FFT_SIZES and 1 <= c["n_prb_grid"] <= N // 12 and 1 <= c["n_sym"] == len(cp) <= 14 and all(0 <= v <= N for v in cp), c
        assert c["cp_kind"] != "extended" or (cp == [N // 4] * c["n_sym"] and c["n_sym"] <= 12), c
        assert c["cp_kind"] != "normal" or cp == OF.nr_cp_lengths(c["scs"], N, c["n_sym"], c["cp_slot"]), c
        view = _view(c)                                                    # raises where the library refuses the draw
        starts, T = X.symbol_starts(N, cp)
        assert OF.PuschOfdmModulator(N, c["n_prb_grid"], cp, n_sym=c["n_sym"]).n_samples == T == OO.geometry(N, cp)[1] == sum(cp) + c["n_sym"] * N, c
        assert view.m_sc == N and view.n_workgroups_per_slot == -(-c["n_sym"] // view.rows_per_workgroup), c
        if c["idx"] in F.TX_BIG_BATCH_CASES:
            assert N == 128 and B * R >= 64 and view.n_workgroups_per_slot >= 3 and B * R * T <= 2 * F.TX_MAX_SAMPLES, c
        else:
            assert 1 <= B <= 3 and 1 <= R <= 4 and B * R * T <= F.TX_MAX_SAMPLES and (N < 4096 or B * R <= F.TX_MAX_ITEMS_4096), c
        assert 0 <= c["slot"] < B and 0 <= c["port"] < R and c["grid_lead"] % 2 == 0 and c["layout"] in F.TX_LAYOUTS, c
        assert 0 <= c["advance"] <= min(cp) and (c["via_dem"] or c["advance"] == 0), c
        # the output
        ss, ps, L = c["slot_stride"], c["port_stride"], c["row_len"]
        rows = F.tx_rows(c)
        assert rows.sum() == B * R * T and L >= T and (L == T) == (c["layout"] != "longer rows"), c
        port_inner = (R == 1 or ps >= T) and (B == 1 or ss >= (R - 1) * ps + T)
        slot_inner = (B == 1 or ss >= T) and (R == 1 or ps >= (B - 1) * ss + T)
        assert port_inner or slot_inner, c
        assert c["layout"].endswith("odd sample") == bool(c["lead"] % 2), c
        if c["layout"] in ("dense", "out= dense", "longer rows"):
            assert (c["lead"], ss, ps) == (0, R * L, L), c
        elif c["layout"].startswith("ports in slots"):
            assert port_inner and ps >= T and ss >= (R - 1) * ps + T, c
        else:
            assert slot_inner and ss >= T and ps >= B * ss, c
        # the content
        assert all(0 <= l < c["n_sym"] for l in c["zero_syms"]) and len(set(c["zero_syms"])) == len(c["zero_syms"]) < c["n_sym"], c
        assert c["prb_run"] is None or (0 <= c["prb_run"][0] and 1 <= c["prb_run"][1] < c["n_prb_grid"] and sum(c["prb_run"]) <= c["n_prb_grid"]), c


def test_restatement_calibrates_the_tolerance_and_zero_symbols_are_exact_zeros():
    """C_TX_FUZZ re-measured with ofdm_tx_oracle.modulate_f32, the float32 restatement of the kernel's arithmetic, never with
    the kernel, under the comparison the GPU test uses (tx_check: ofdm_tx_oracle.check where the unit is not 0, `== 0` where it
    is).  Per draw also what the realization promises: the zeros where the dict puts them and nowhere else, at least one
    symbol that carries values, the phasors' moduli, the prefix as the tail."""
    worst, by = 0.0, collections.defaultdict(float)
    for c in _draws():
        d = F.realize_tx(c)
        N, B, R, n_sym = c["n_fft"], c["B"], c["R"], c["n_sym"]
        assert d.grid.shape == (B, R, d.n_sc, n_sym) and d.grid.dtype == np.complex64 and d.ref.shape == d.rms.shape == (B, R, d.T), c
        assert np.all(np.isfinite(d.ref)) and (d.phi is None) == (c["phasor"] == "none"), c
        if c["phasor"] == "unit":
            assert np.abs(np.abs(d.phi) - 1).max() < 1e-6, c
        if c["phasor"] == "scaled":
            assert 0.25 <= np.abs(d.phi).min() and np.abs(d.phi).max() <= 4.0 + 1e-6, c
        # exact zeros where the dict puts them, values everywhere else
        live = np.ones((d.n_sc, n_sym), bool)
        live[:, c["zero_syms"]] = False
        if c["prb_run"] is not None:
            p0, n_run = c["prb_run"]
            live[:12 * p0] = live[12 * (p0 + n_run):] = False
        assert not d.grid[:, :, ~live].any() and np.all(d.grid[:, :, live] != 0), c
        assert live.any(0).sum() == n_sym - len(c["zero_syms"]) >= 1, c                      # a symbol that is not all zero: the case tests values
        sym = X.symbol_of_sample(N, c["cp_len"])
        zero = np.isin(sym, c["zero_syms"])
        assert np.all(d.rms[..., zero] == 0) and np.all(d.rms[..., ~zero] > 0) and not d.ref[..., zero].any(), c
        got = X.modulate_f32(d.grid, _view(c), OF.twiddles(N), c["cp_len"], d.phi)
        assert not got[..., zero].any(), c                                                   # the restatement: exactly 0 too
        r = F.tx_check(got, d.ref, d.rms, N, f"float32 restatement {c}", F.C_TX_FUZZ)
        worst = max(worst, r)
        for k in (f"n_fft {N}", "cp " + c["cp_kind"], "phasor " + c["phasor"]):
            by[k] = max(by[k], r)
        bits = np.ascontiguousarray(got).view(np.uint64)
        for t, cp in zip(d.starts, c["cp_len"]):
            assert np.array_equal(bits[..., t:t + cp], bits[..., t + N:t + N + cp]), c
    print("largest ratio: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by.items())))
    print(f"C_TX_FUZZ = {worst:.3f} (recorded {F.C_TX_FUZZ:g}, T = {F.T_TX_FUZZ:g})")
    assert worst <= F.C_TX_FUZZ and F.T_TX_FUZZ == 4.0 * F.C_TX_FUZZ and round(F.C_TX_FUZZ, 1) == F.C_TX_FUZZ
    assert worst >= 0.25                                          # the restatement is float32 indeed


def test_round_trip_pairing_in_float64_and_its_constant():
    """For the draws built through `for_demodulator`: ofdm_oracle.demodulate_ref of the float64 modulation returns
    |phi_l|^2 X[k, l] at the drawn advance (and at 0 and min cp) to 1e-10 of the (slot, port)'s largest |phi_l|^2 |X| -- the
    modulator applies conj(phi_l), the demodulator phi_l, and the advance is compensated at the demodulator's store.  C_PAIR
    re-measured with demodulate_f32 of modulate_f32 under the unit eps |phi_l|^2 (log2(N) rms_l(X) + |X|), rms_l(X) the rms of
    the symbol's N bins."""
    worst, n = 0.0, 0
    for c in _draws():
        if not c["via_dem"]:
            continue
        n += 1
        d = F.realize_tx(c)
        N, cp = c["n_fft"], c["cp_len"]
        scale = np.abs(d.pair_ref).max((-1, -2), keepdims=True)
        assert np.all(scale > 0), c
        for a in sorted({0, c["advance"], min(cp)}):
            back = OO.demodulate_ref(d.ref, N, c["n_prb_grid"], cp, a, d.phi)
            assert back.shape == d.pair_ref.shape and np.all(np.abs(back - d.pair_ref) <= 1e-10 * scale), (a, c)
        view = _view(c)
        s = X.modulate_f32(d.grid, view, OF.twiddles(N), cp, d.phi)
        dview = OF.derive_host(N, c["n_prb_grid"], cp, c["n_sym"], c["advance"])
        back = OO.demodulate_f32(s, dview, OF.twiddles(N), c["n_prb_grid"], cp, c["advance"], d.phi)
        worst = max(worst, F.tx_check(back, d.pair_ref, d.pair_rms, N, f"float32 round trip {c}", F.C_PAIR, rule=OO.check))
    print(f"C_PAIR = {worst:.3f} over {n} draws (recorded {F.C_PAIR:g}, T = {F.T_PAIR:g})")
    assert n >= 30 and worst <= F.C_PAIR and F.T_PAIR == 4.0 * F.C_PAIR and round(F.C_PAIR, 1) == F.C_PAIR
    assert worst >= 0.25
