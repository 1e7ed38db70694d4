"""What the draws of tests/door_fuzz_cases.py must satisfy by themselves, before tests/test_zzzzzzzzzzzzzzzzzzzzz_hip_door_fuzz.py
runs the channel emulator, the fronthaul codec, the PRACH detector and the SRS estimator on them: a case replays from its printed
dict; every kernel path the pinned cases of chan_oracle.CASES, fh_oracle.CASES, prach_oracle.CASES and srs_oracle.GEOMETRIES leave
out is reached by at least three cases (the tables are printed); the library's host entry points accept every draw and derive the
oracles' integers; the rows of every written layout are pairwise disjoint; the tolerance constants are what the float32
restatements need, no more and not much less; the delay rules' conditions hold on the oracle for every transmitted preamble and
every sounding item; every case has an output whose unit is not 0, and its zeros are where the dict puts them.  No GPU."""
import collections

import numpy as np

import chan_oracle as CO
import door_fuzz_cases as F
import fh_oracle as FO
import prach_oracle as PO
import srs_oracle as SO
from srsran_ce_pytorch_amd import _lib, channel as CH, fronthaul as FH, prach as PR, srs as S
from test_chain_fuzz import _report

CHAN_CLASSES = ([f"n_tx {p}" for p in (1, 2, 3, 4)] + [f"K {k}" for k in (1, 2, 3, 4, 5, "6..126 even", "6..126 odd", 127, 128)] + ["K never pinned (4..11, 13..126)", "K > T"]
                + [f"halo {h}" for h in (0, 2, 4, "6..126")] + ["T 1", "T 2", "T 3", "T a multiple of the tile", "an even T just behind a tile edge", "an odd T in the first tile"]
                + [f"tiles {t}" for t in (1, 2, 3, "4+")] + ["taps shared", "taps per slot", "a zero tap row", "a zero tap row for every tx port", "noise checked by itself",
                                                       "noise checked by itself under a sigma tensor", "noise checked by itself over more than one tile"]
                + ["cfo " + k for k in ("none", "scalar", "tensor")] + ["fcw 0", "fcw -2^31", "fcw 2^31 - 1", "fcw 1", "fcw -1"] + ["sigma " + k for k in ("none", "scalar", "tensor")]
                + ["sigma 0 beside non-zero values", "an amplitude beyond a decade from 1"] + ["first_slot " + k for k in ("0", "negative", "above 2^32")]
                + ["x " + k for k in F.CHAN_X_LAYOUTS] + ["y " + k for k in F.CHAN_Y_LAYOUTS] + ["x at an odd element", "y at an odd element", "x strided at an odd element with CFO and noise"])
CHAN_ALSO = ["an odd T", "more than one slot"]
FH_CLASSES = ([f"W {w}" for w in range(1, 17)] + ["method none"] + [f"prb_bytes {b}" for b in (7, 10, 13, 16, 19, 22, 31, 34, 40, 46)] + [f"n_prb {n}" for n in F.FH_N_PRB]
              + ["tiles of 64 PRBs: " + t for t in ("1", "2", "3", "4 or more")] + [f"row_bytes mod 4 = {k}" for k in range(4)] + ["scale " + k for k in F.FH_SCALES]
              + [f"{side}: {w} accesses" for side in ("decompressor", "compressor") for w in ("16-byte", "8-byte")] + ["grid written: " + k for k in list(F.FH_NESTINGS) + F.FH_PARITIES]
              + ["grid read: " + k for k in F.FH_PARITIES] + ["payload written: " + k for k in F.FH_NESTINGS]
              + ["a section of a wider grid", "grid written at an odd element", "grid read with a repeated row (stride 0)", "payload read with a repeated row (stride 0)",
                 "payload written with bytes behind row_bytes"])
FH_ALSO = ["more than one row"]
PRACH_CLASSES = ([f"(L, N) = ({L}, {N})" for L, N in F.PRACH_PAIRS] + [f"rows_per_workgroup {r}" for r in (4, 2, 1)] + [f"outputs per thread {k}" for k in (4, 8, 16)]
                 + ["L 139 at 8 or 16 outputs per thread"] + ["n_roots " + k for k in ("1", "2", "3", "4..12", "64")] + ["roots other than 1, L - 1, L // 2 + 1", "root 1 present", "root L - 1 present"]
                 + ["n_cs " + k for k in ("0", "small", "typical", "large")] + ["n_shifts 1", "n_shifts 64", "n_shifts no multiple of 4 with more than three roots"]
                 + ["combine coherent", "combine noncoherent"] + ["R " + k for k in ("1", "2", "3", "4", "5", "6..16", "64")]
                 + ["fewer terms than rows_per_workgroup", "as many terms as rows_per_workgroup", "terms no multiple of rows_per_workgroup", "more than 12 terms", "more than 5 ports"]
                 + ["layout " + k for k in F.PRACH_LAYOUTS] + ["y at an odd element", "rows longer than L", "profile returned", "profile not returned"]
                 + ["an occasion of " + k for k in ("signal", "noise", "zero")] + ["more than one preamble in an occasion", "an amplitude beyond a decade from 1"])
PRACH_ALSO = [f"L {L}" for L in PO.L_RA] + [f"N {N}" for N in PO.FFT_SIZES] + ["more than one occasion"]
SRS_SHAPES = {128: (64, 4, 2), 256: (64, 4, 4), 512: (128, 2, 4), 1024: (128, 2, 8), 2048: (256, 1, 8), 4096: (256, 1, 16)}       # N: threads per row, rows per workgroup, outputs per thread
SRS_CLASSES = ([f"N {n}: {t} threads per row, {r} rows per workgroup, {o} outputs per thread" for n, (t, r, o) in SRS_SHAPES.items()] + ["N the smallest size above M"]
               + ["k_tc 2", "k_tc 4", "n_ap 1", "n_ap 2", "n_ap 4", "n_combs 1", "n_combs 2", "four ports on one comb at k_tc 2", "n_ap 1 at k_tc 4"]
               + ["M " + k for k in ("12", "24", "36", "48", "60", "72", "above 72")] + ["M 72: sequence hopping live", "a phi-table sequence", "m_srs 272"]
               + [f"n_symb {k}" for k in (1, 2, 4)] + ["n_symb_slot 12", "n_symb_slot 14", "n_sym < 14"] + [f"slots_per_frame {k}" for k in F.SRS_SLOTS_PER_FRAME]
               + ["n_id above 1023", "bit 12 of c_init set with hopping", "slot above 2^30", "slot and n_id per item", "slot and n_id as ints"]
               + ["hopping " + k for k in ("neither", "group", "sequence")] + ["sequence hopping live"] + ["win_len " + k for k in F.SRS_WIN_KINDS]
               + ["win_len above the default", "win_len above N - g"] + ["R " + k for k in ("1", "2", "3", "4", "5", "64")] + ["layout " + k for k in F.SRS_LAYOUTS]
               + ["start_prb differs between symbols", "a zero item", "an amplitude beyond a decade from 1"])
SRS_ALSO = [f"N {n}" for n in SRS_SHAPES] + ["more than one item"]
# The re-measured constants may not fall below this share of their recorded values either.  The measurement is deterministic (seeded
# draws, numpy float32): measured / recorded is 0.73 .. 0.99 for the eight constants as recorded (the rounding up to 0.1 costs h_wb
# 0.146 -> 0.2 the most), so 0.7 holds them all and a restatement that lost a third of its error fails.
FLOOR = 0.7


def _chan():
    return [F.draw_chan(i) for i in range(F.N_CHAN)]


def _fh():
    return [F.draw_fh(i) for i in range(F.N_FH)]


def _prach():
    return [F.draw_prach(i) for i in range(F.N_PRACH)]


def _srs():
    return [F.draw_srs(i) for i in range(F.N_SRS)]


def _prach_view(c):
    return PR.derive_host(c["L"], c["N"], c["roots"], c["n_cs"], c["n_shifts"], "coherent" if c["combine"] else "noncoherent")


def test_draws_are_reproducible_and_plain():
    for draw, n in ((F.draw_chan, F.N_CHAN), (F.draw_fh, F.N_FH), (F.draw_prach, F.N_PRACH), (F.draw_srs, F.N_SRS)):
        a, b = draw(7), draw(7)
        assert a == b and a != draw(8) and eval(repr(a)) == a             # a case replays from its printed dict
        assert all(eval(repr(c)) == draw(c["idx"]) for c in (draw(i) for i in range(n)))
    assert (F.STAGE_CHAN, F.STAGE_FH, F.STAGE_PRACH, F.STAGE_SRS) == (13, 14, 15, 16) and F.BASE_SEED == 20261020     # behind the earlier fuzzes' 1 .. 12
    a, b = F.realize_chan(F.draw_chan(7)), F.realize_chan(F.draw_chan(7))
    assert np.array_equal(a.x.view(np.uint64), b.x.view(np.uint64)) and np.array_equal(a.ref, b.ref)
    a, b = F.realize_fh(F.draw_fh(7)), F.realize_fh(F.draw_fh(7))
    assert np.array_equal(a.grid.view(np.uint64), b.grid.view(np.uint64)) and np.array_equal(a.payload, b.payload) and np.array_equal(a.packed, b.packed)
    a, b = F.realize_prach(F.draw_prach(7)), F.realize_prach(F.draw_prach(7))
    assert np.array_equal(a.host.view(np.uint64), b.host.view(np.uint64)) and np.array_equal(a.ref.profile, b.ref.profile)
    a, b = F.realize_srs(F.draw_srs(7)), F.realize_srs(F.draw_srs(7))
    assert np.array_equal(a.host.view(np.uint64), b.host.view(np.uint64)) and np.array_equal(a.prof, b.prof)


def test_every_class_is_reached():
    counts = collections.Counter()
    for c in _chan():
        counts.update(F.chan_classes(c))
    _report("channel emulator", F.N_CHAN, counts, CHAN_CLASSES, 3, CHAN_ALSO)
    counts = collections.Counter()
    for c in _fh():
        counts.update(F.fh_classes(c))
    _report("fronthaul codec", F.N_FH, counts, FH_CLASSES, 3, FH_ALSO)
    assert counts["n_prb 341"] == len(F.FH_BIG_CASES) and all(counts[f"W {w}"] == F.N_FH // 17 for w in range(1, 17))
    # every width (17: "none") meets both instantiations of both kernels.  The parity kinds cycle nominally: a kind the shape cannot
    # hold (no dimension of one entry, or none of several) is drawn as "all even" and recorded as that, so the table counts what is realised
    for w in range(1, 18):
        mine = [c for c in _fh() if c["idx"] % 17 == w - 1]
        assert {F.fh_wide(c, "gw") for c in mine} == {F.fh_wide(c, "gr") for c in mine} == {True, False}, w
    counts = collections.Counter()
    for c in _prach():
        counts.update(F.prach_classes(c, _prach_view(c)[0]))
    _report("PRACH detector", F.N_PRACH, counts, PRACH_CLASSES, 3, PRACH_ALSO)
    assert counts["n_roots 64"] == len(F.PRACH_64_ROOT_CASES) and counts["R 64"] == len(F.PRACH_64_PORT_CASES)
    counts = collections.Counter()
    for c in _srs():
        counts.update(F.srs_classes(c, S.derive_host(**SO.plan_kwargs(F.srs_case(c)))))
    _report("SRS estimator", F.N_SRS, counts, SRS_CLASSES, 3, SRS_ALSO)
    assert counts["m_srs 272"] == len(F.SRS_272_CASES) and counts["R 64"] == len(F.SRS_64_PORT_CASES)


def _nesting_ok(n, strides, row):
    """The header's rule for a written side: by ascending stride, each stride of a dimension with more than one entry at least
    the extent of everything inside it."""
    ext = row
    for k, s in sorted(((k, s) for k, s in zip(n, strides) if k > 1), key=lambda ks: ks[1]):
        if s < ext:
            return False
        ext += (k - 1) * s
    return True


def test_channel_draws_are_accepted_and_the_rows_do_not_overlap():
    for c in _chan():
        P, K, T, R, B = c["P"], c["K"], c["T"], c["R"], c["B"]
        emu = CH.PuschChannelEmulator(P, R, K)                              # raises where the library's wrapper refuses the draw
        assert (emu.n_tx, emu.n_rx, emu.n_taps) == (P, R, K) and 1 <= P <= CH.MAX_TX and 1 <= K <= CH.MAX_TAPS and 1 <= T <= 4500 and 1 <= R <= 4 and 1 <= B <= 3, c
        assert B * R * P * K * T <= F.CHAN_MAX_WORK and 0 <= c["slot"] < B and len(c["amp"]) == B, c
        assert 0 < c["noise_seed"] >> 32 < 1 << 32 and c["noise_seed"] & 0xFFFFFFFF and -2 ** 63 <= c["first_slot"] < 2 ** 63, c
        words = [] if c["cfo"] == "none" else ([c["fcw"]] if c["cfo"] == "scalar" else c["fcw"])
        phases = [] if c["cfo"] == "none" else ([c["phase0"]] if c["cfo"] == "scalar" else c["phase0"])
        assert all(-2 ** 31 <= w < 2 ** 31 for w in words) and all(0 <= p < 2 ** 32 for p in phases) and len(words) == len(phases) == {"none": 0, "scalar": 1, "tensor": B}[c["cfo"]], c
        sig = [] if c["noise"] == "none" else ([c["sigma"]] if c["noise"] == "scalar" else c["sigma"])
        assert all(s >= 0 and float(np.float32(s)) == s for s in sig) and (c["noise"] != "tensor" or (len(sig) == B and 0.0 in sig)), c
        rows = F.chan_rows(c)                                               # asserts: no element twice
        assert rows.sum() == B * R * T and _nesting_ok((B, R), (c["y_ss"], c["y_ps"]), T), c
        assert min(c["x_ss"], c["x_ps"]) >= 0 and F.chan_x_total(c) >= c["x_lead"] + T, c
        x_rows = F.rows_mask(F.chan_x_total(c), (B, P), T, c["x_lead"], (c["x_ss"], c["x_ps"]), c)
        assert x_rows.sum() == B * P * T, c                                 # x need not be disjoint; these draws keep NaN between the rows
        if c["zero_tap"] is not None:
            assert 0 <= c["zero_tap"][0] < R and -1 <= c["zero_tap"][1] < P, c


def test_channel_restatement_calibrates_the_tolerance_and_zero_rows_are_exact_zeros():
    """C_CHAN_FUZZ re-measured with chan_oracle.apply_f32 under chan_oracle.ratio (which demands the reference's 0 where the unit
    is 0).  Per draw: the unit is 0 exactly on the rows whose every tap is 0 and whose slot has no noise, and nowhere else; never
    on every output."""
    worst, by = 0.0, collections.defaultdict(float)
    for c in _chan():
        d = F.realize_chan(c)
        B = c["B"]
        assert d.x.shape == (B, c["P"], c["T"]) and d.h.shape == (1 if c["shared"] else B, c["R"], c["P"], c["K"]) and np.all(np.isfinite(d.ref)), c
        u = CO.unit(d.A, d.n, d.sigma, c["P"], c["K"])
        quiet = np.ones(B, bool) if d.sigma is None else np.array([float(s) == 0.0 for s in CO._per_slot(d.sigma, B)])
        want = F.chan_zero_rows(c) & quiet[:, None]
        assert np.array_equal((u == 0).all(-1), want) and np.array_equal((u == 0).any(-1), want) and not want.all(), c
        assert not d.ref[want].any(), c
        got = CO.apply_f32(d.x, d.h, d.fcw, d.phase0, d.sigma, d.seed, d.first_slot)
        assert not got[want].any(), c                                       # the restatement: exactly 0 too
        r = CO.ratio(got, d)
        worst = max(worst, r)
        for k in (f"n_tx {c['P']}", "cfo " + c["cfo"], "sigma " + c["noise"], "K " + ("1..5" if c["K"] <= 5 else "6..128")):
            by[k] = max(by[k], r)
    print("largest ratio: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by.items())))
    print(f"C_CHAN_FUZZ = {worst:.3f} (recorded {F.C_CHAN_FUZZ:g}, T = {F.T_CHAN_FUZZ:g})")
    assert worst <= F.C_CHAN_FUZZ and F.T_CHAN_FUZZ == 4.0 * F.C_CHAN_FUZZ and round(F.C_CHAN_FUZZ, 1) == F.C_CHAN_FUZZ
    assert worst >= FLOOR * F.C_CHAN_FUZZ                                   # ... and no less: a restatement that lost part of its arithmetic falls below


def test_fronthaul_draws_are_accepted_and_the_rows_do_not_overlap():
    """ce_fh_row_bytes is the oracle's; both written sides are pairwise disjoint in a nesting the header accepts; the payload's base
    and strides are multiples of 4; `fh_wide` is the header's rule spelled out on the byte address."""
    for c in _fh():
        n, n_prb, W = (c["B"], c["R"], c["S"]), c["n_prb"], c["W"]
        nb = FO.row_bytes(c["method"], W, n_prb)
        assert FH.row_bytes(c["method"], W, n_prb) == nb == n_prb * FO.prb_bytes(c["method"], W) and 1 <= W <= 16 and 1 <= n_prb <= FH.MAX_PRBS, c
        assert FH.SCALE_MIN <= c["scale"] <= FH.SCALE_MAX and float(np.float32(c["scale"])) == c["scale"], c
        FH.PuschFronthaulDecompressor(c["n_prb_grid"], c["S"], c["method"], W, c["scale"])       # raises where the wrapper refuses the draw
        assert 0 <= c["start_prb"] and c["start_prb"] + n_prb <= c["n_prb_grid"] <= FH.MAX_PRBS and n[0] * n[1] * n[2] * n_prb <= max(F.FH_MAX_PRB_ROWS, n_prb), c
        n_sc = 12 * c["n_prb_grid"]
        total = c["gw_lead"] + F.extent(n, c["gw_strides"], n_sc) + c["gw_tail"]
        assert F.rows_mask(total, n, n_sc, c["gw_lead"], c["gw_strides"], c).sum() == n[0] * n[1] * n[2] * n_sc and _nesting_ok(n, c["gw_strides"], n_sc), c
        total = c["pw_lead"] + F.extent(n, c["pw_strides"], nb) + c["pw_tail"]
        assert F.rows_mask(total, n, nb, c["pw_lead"], c["pw_strides"], c).sum() == n[0] * n[1] * n[2] * nb and _nesting_ok(n, c["pw_strides"], nb), c
        for side in ("pw", "pr"):
            assert c[side + "_lead"] % 4 == 0 and all(s % 4 == 0 and s >= 0 for s in c[side + "_strides"]), c
        for side in ("gr", "pr"):
            assert all((s == 0) == (dim in c[side + "_repeat"]) for dim, (k, s) in enumerate(zip(n, c[side + "_strides"])) if k > 1), c
        for side in ("gw", "gr"):
            base = 8 * c[side + "_lead"] + 96 * c["start_prb"]
            assert F.fh_wide(c, side) == (base % 16 == 0 and all(k == 1 or (8 * s) % 16 == 0 for k, s in zip(n, c[side + "_strides"]))), c
        assert all(0 <= r < k for r, k in zip(c["row"], n)) and all(0 <= p < n_prb for p in c["edge_prb"]), c


def test_fronthaul_round_trip_on_the_oracle_and_the_edges_of_the_exponent():
    """On the oracle: compress(decompress(compress(x))) returns the bytes of compress(x) for every draw -- but at W = 1 for a PRB
    that holds a positive and no negative value: its one-bit mantissas are all 0, it decompresses to zeros and compresses again
    with e = 0 (the header states the round trip without that exception; the kernels follow the definition, as the oracle does).
    Every case holds all 16 exponents among its random parameter bytes or its compressed ones where it has PRBs enough, and the
    edge PRBs quantise to the peaks the dict asks for."""
    seen_e = collections.Counter()
    for c in _fh():
        d = F.realize_fh(c)
        n_prb, pb = c["n_prb"], FO.prb_bytes(c["method"], c["W"])
        assert d.grid.shape == (c["B"], c["R"], c["S"], 12 * n_prb) and d.payload.shape[-1] == d.row_bytes == n_prb * pb, c
        v = np.array([FO.quantise(r, c["scale"]) for r in d.grid.reshape(-1, 12 * n_prb).view(np.float32)]).reshape(-1, n_prb, 24)
        differs = (d.repacked != d.packed).reshape(-1, n_prb, pb).any(-1)
        one_bit = c["method"] == "bfp" and c["W"] == 1
        assert np.array_equal(differs, (v.min(-1) >= 0) & (v.max(-1) > 0) if one_bit else np.zeros(differs.shape, bool)), c
        L, edges = F.fh_edge_values(c)
        last = {p: e for p, e in zip(c["edge_prb"], edges)}                 # a PRB drawn twice holds the later edge
        for p, e in last.items():
            mag = np.where(v[:, p] >= 0, v[:, p], ~v[:, p]).max(-1)
            assert np.all(mag == (e if e >= 0 else ~e)) and np.all((v[:, p] == e).any(-1)), (c, p, e)
        if c["method"] == "bfp":
            seen_e.update((d.packed.reshape(-1, n_prb, pb)[..., 0] & 15).reshape(-1).tolist())
            assert np.all(d.packed.reshape(-1, n_prb, pb)[..., 0] < 16), c                          # the compressor's reserved nibble is 0
            if d.payload.size // pb >= 256:
                assert set((d.payload.reshape(-1, n_prb, pb)[..., 0] & 15).reshape(-1).tolist()) == set(range(16)), c
                assert (d.payload.reshape(-1, n_prb, pb)[..., 0] >> 4).any(), c
    assert set(seen_e) == set(range(16)), sorted(seen_e)


def test_prach_draws_are_accepted_and_derive_the_oracles_windows():
    for c in _prach():
        L, N, R, S, B = c["L"], c["N"], c["R"], c["S"], len(c["occasions"])
        view, ws, wl = _prach_view(c)                                       # raises where the library refuses the draw
        ows, owl = PO.windows(L, N, c["n_cs"], c["n_shifts"])
        assert np.array_equal(ws, ows) and wl == owl and int(view.m_sc) == N and (L, N) in F.PRACH_PAIRS, c
        assert int(view.rows_per_workgroup) == F.PRACH_ROWS_PER_WORKGROUP.get(N, 1), c
        assert 1 <= len(c["roots"]) == len(set(c["roots"])) <= PR.MAX_ROOTS and all(1 <= u < L for u in c["roots"]) and 1 <= R <= PR.MAX_PORTS and 1 <= S <= PR.MAX_REPS, c
        assert 1 <= B <= 3 and "signal" in c["occasions"] and B * len(c["roots"]) * (R if c["combine"] else R * S) * N <= F.PRACH_MAX_POINTS, c
        assert c["n_cs"] == 0 or c["n_cs"] >= F.prach_min_ncs(L, N), c
        seen = set()
        for b, i, v, j in c["preambles"]:
            assert c["occasions"][b] == "signal" and 0 <= i < len(c["roots"]) and 0 <= v < c["n_shifts"] and (b, i, v) not in seen, c
            assert 0 <= j and -(-N // L) + j + 1 < wl or c["n_cs"] == 0, c   # the peak and its neighbour lie inside the window, behind the guard
            seen.add((b, i, v))
        assert {b for b, *_ in c["preambles"]} == {b for b, k in enumerate(c["occasions"]) if k == "signal"}, c
        assert all(1 <= sum(1 for p in c["preambles"] if p[0] == b) <= 3 for b, k in enumerate(c["occasions"]) if k == "signal"), c
        assert min(c["strides"]) >= 0 and c["row_len"] >= L and 0 <= c["occasion"] < B and 0 <= c["root"] < len(c["roots"]), c
        if c["layout"] in ("port outside", "repetition outside"):
            assert F.rows_mask(F.prach_total(c), (B, R, S), c["row_len"], c["lead"], c["strides"], c).sum() == B * R * S * c["row_len"], c
        if c["layout"].startswith("stride 0"):
            assert c["strides"][1 if c["layout"].endswith("ports") else 2] == 0, c


def test_prach_restatement_calibrates_the_tolerance_and_the_delay_rule_holds_on_the_oracle():
    """C_PRACH_FUZZ re-measured with prach_oracle.detect_f32 on the library's own view and tables.  Per draw: an all-zero occasion
    is exactly 0 in the reference and in the restatement and nothing else is; in every window that carries a transmitted preamble
    the oracle's gap between the largest and the second-largest value exceeds GAP_TOLERANCES pairs of fuzz tolerances, and the
    oracle finds the preamble at the index it was sent at."""
    worst, by, least = 0.0, collections.defaultdict(float), np.inf
    for c in _prach():
        d = F.realize_prach(c)
        L, N = c["L"], c["N"]
        view, ws, wl = _prach_view(c)
        for b, kind in enumerate(c["occasions"]):
            assert (kind == "zero") == (not d.y[b].any()) == (not d.ref.profile[b].any()) and np.all(d.ref.mean[b] > 0) == (kind != "zero"), c
        assert np.all(np.isfinite(d.y.view(np.float32))) and d.sent, c
        tw, table = PR.tables(L, N, c["roots"])
        got = PO.detect_f32(d.y, L, view, tw, table, ws, wl, c["combine"])
        got.peak, got.delay, got.mean = got.peak.astype(np.float32), got.delay.astype(np.int32), got.mean.astype(np.float32)
        r = max(F.prach_check(got, d, f"float32 restatement {c}", F.C_PRACH_FUZZ))
        worst = max(worst, r)
        terms = c["R"] if c["combine"] else c["R"] * c["S"]
        for k in (f"N {N}", "terms " + ("1..12" if terms <= 12 else "13..64" if terms <= 64 else "65..768"), "layout " + c["layout"]):
            by[k] = max(by[k], r)
        g = -(-N // L)
        for (b, i, v), (gap, tol) in zip(d.sent, F.prach_gaps(d, F.T_PRACH_FUZZ)):
            assert gap > PO.GAP_TOLERANCES * tol, (c, (b, i, v), gap, tol)
            least = min(least, gap / tol)
            j = [p[3] for p in c["preambles"] if tuple(p[:3]) == (b, i, v)][0]
            assert abs(int(d.ref.delay[b, i, v]) - ((g if c["n_cs"] else 0) + j)) <= 1, (c, (b, i, v))     # (off_half_sample may step one index back)
    print("largest ratio: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by.items())))
    print(f"C_PRACH_FUZZ = {worst:.3f} (recorded {F.C_PRACH_FUZZ:g}, T = {F.T_PRACH_FUZZ:g}); the smallest gap is {least:.0f} tolerance pairs")
    assert worst <= F.C_PRACH_FUZZ and F.T_PRACH_FUZZ == 4.0 * F.C_PRACH_FUZZ and round(F.C_PRACH_FUZZ, 1) == F.C_PRACH_FUZZ
    assert worst >= FLOOR * F.C_PRACH_FUZZ


def test_srs_draws_are_accepted_and_derive_the_oracles_integers():
    for c in _srs():
        k = F.srs_case(c)
        hv = S.derive_host(**SO.plan_kwargs(k))                             # raises where the library refuses the draw
        default = SO.case("a_c4_4p_one_comb_m36", **{**{n: getattr(k, n) for n in ("k_tc", "n_ap", "n_cs", "k_bar", "m_srs", "N")}}).win_len
        assert (hv.m, hv.q_len, hv.n_blocks, hv.n_combs, hv.guard, hv.default_win_len) == (k.M, k.Q, k.n_blocks, k.n_combs, k.g, default), c
        assert list(zip(hv.port_comb, hv.port_cs)) == k.ports == S.srs_ports(k.k_tc, k.n_ap, k.n_cs, k.k_bar) and int(hv.view.m_sc) == k.N, c
        assert hv.v_live == (k.M >= 72 and c["hopping"] == "sequence") and k.win_len == (default if c["win_len"] is None else c["win_len"]) and 1 <= k.win_len <= k.N, c
        assert k.N in S.FFT_SIZES and k.M < k.N <= F.SRS_MAX_RATIO * k.M and 1 <= k.R <= S.MAX_RX and k.B * k.R * k.n_sym * k.n_sc <= F.SRS_MAX_RES, c
        assert k.n_symb <= k.n_sym <= k.n_symb_slot and 0 <= k.l0 <= k.n_sym - k.n_symb and all(0 <= p <= k.n_prb_grid - k.m_srs for p in k.start_prb) and k.n_prb_grid <= 341, c
        assert len(c["slot"]) == len(c["n_id"]) == (k.B if c["per_item"] else 1) and all(0 <= v < 2 ** 31 for v in c["slot"]) and all(0 <= v <= S.N_ID_MAX for v in c["n_id"]), c
        assert c["win_len"] is None or k.n_ap == 1 or c["win_len"] <= default, c
        assert all(0 <= j < k.win_len for j in c["window_index"]) and "signal" in c["items"] and 0 <= c["item"] < k.B and 0 <= c["port"] < k.R, c
        assert abs(c["shift"]) >= 1 and abs(c["shift"]) * k.N + k.N < 2 ** 31 and min(c["strides"]) >= 0, c
        n = (k.B, k.R, k.n_sym)
        assert F.rows_mask(F.srs_total(c), n, c["row_len"], c["lead"], c["strides"], c).sum() == k.B * k.R * k.n_sym * c["row_len"] and c["row_len"] >= k.n_sc, c
        assert (c["lead"] % 2 == 1) == c["layout"].startswith("odd element"), c


def test_srs_restatements_calibrate_the_tolerances_and_the_delay_rule_holds_on_the_oracle():
    """C_SRS_FUZZ[quantity] re-measured with srs_oracle.profile_f32 / estimate_f32 on the library's own view and tables.  Per draw:
    a zero item is exactly 0 in the reference and in the restatement, and nothing else is; every signal item's delay is the one
    sent (at win_len = 1 that is -g), and where its window has two indices or more the oracle's gap between the largest and the
    second-largest value of sum_r profile exceeds GAP_TOLERANCES pairs of fuzz tolerances; NaN outside the used combs never
    reaches the oracle."""
    from types import SimpleNamespace
    worst, least = collections.defaultdict(float), np.inf
    where = {}
    for c in _srs():
        d = F.realize_srs(c)
        k = d.c
        hv = S.derive_host(**SO.plan_kwargs(k))
        tw, w, rho = S.tables(k.k_tc, k.n_ap, k.n_cs, k.k_bar, k.m_srs, k.N)
        lib = SimpleNamespace(hv=hv, tw=tw, w=w, rho=rho)
        prof = SO.profile_f32(k, lib, d.y, d.slot, d.n_id)
        est = SO.estimate_f32(k, lib, d.y, d.slot, d.n_id, d.delay)
        assert np.all(np.isfinite(d.full)) and np.all(np.isfinite(d.est.h_sb)) and np.all(np.isfinite(d.y[:, :, d.used])), c
        assert c["layout"].endswith("NaN outside the combs") == bool(np.isnan(d.y[:, :, ~d.used].real).all() and (~d.used).any()) or not (~d.used).any(), c
        for b, kind in enumerate(c["items"]):
            zero = kind == "zero"
            assert zero == (not d.prof[b].any()) == (not d.est.epre[b].any()) == (not prof[b].any()) == (not est.epre[b].any()) == (not est.h_sb[b].any()), c
            assert zero or (np.all(d.est.epre[b] > 0) and np.all(d.full[b].mean(-1) > 0)), c
            assert zero or d.delay[b] == d.sent[b] == c["window_index"][b] - k.g, (c, b, d.delay[b])
        r = F.srs_check(d, F.C_SRS_FUZZ, prof=prof, delay=SO.delay_of(k, prof).astype(np.int32), est=est, what=f"float32 restatement {c}")
        for q, v in r.items():
            if v > worst[q]:
                worst[q], where[q] = v, c["idx"]
        for b, (gap, tol) in enumerate(F.srs_gaps(d, F.T_SRS_FUZZ["profile"])):
            if c["items"][b] == "signal" and k.win_len >= 2:
                assert gap > SO.GAP_TOLERANCES * tol, (c, b, gap, tol)
                least = min(least, gap / tol)
            assert k.win_len >= 2 or d.delay[b] == -k.g, c
    print("C_SRS_FUZZ = " + ", ".join(f"{q} {worst[q]:.3f} (draw {where[q]}; recorded {F.C_SRS_FUZZ[q]:g})" for q in F.C_SRS_FUZZ) + f"; the smallest gap is {least:.0f} tolerance pairs")
    for q, rec in F.C_SRS_FUZZ.items():
        assert worst[q] <= rec and F.T_SRS_FUZZ[q] == 4.0 * rec and round(rec, 1) == rec, q
        assert worst[q] >= FLOOR * rec, q
    assert set(F.C_SRS_FUZZ) == set(SO.C_RECORDED) == {"profile", "h_sb", "h_wb", "noise", "epre"}


def test_abi_constants_the_draws_rely_on():
    assert (_lib.CE_FH_MAX_PRBS, PR.MAX_ROOTS, PR.MAX_SHIFTS, PR.MAX_PORTS, PR.MAX_REPS, S.MAX_RX) == (341, 64, 64, 64, 12, 64)
    assert tuple(PR.L_RA) == PO.L_RA and tuple(PR.FFT_SIZES) == PO.FFT_SIZES and len(F.PRACH_PAIRS) == 13
