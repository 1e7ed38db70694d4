"""What the draws of tests/chain_fuzz_cases.py must satisfy by themselves, before tests/test_zzzzzzzzzz_hip_chain_fuzz.py runs
the kernels on them: every kernel path the pinned cases of the five stages leave out is reached by at least the stated
number of cases; the library's host views agree with the oracles' integers on every draw and refuse what the oracles refuse;
the de-precoder's tolerance constant is at least what the float32 restatement needs; and -- from the oracle alone -- the
decoder's batches hold, inside one workgroup, blocks that stop at different iterations and blocks that pass and fail.
No GPU."""
import collections

import numpy as np
import pytest
import torch

import chain_fuzz_cases as F
import enc_oracle as E
import eq_oracle as Q
import tb_oracle as T
import tp_oracle as TP
from srsran_ce_pytorch_amd import deprecode as DP, encoder as EN, ldpc as LD, modulator as MO, synth as S, transportblock as TB

ALL_RADIX = sorted({"radix " + "x".join(str(int(r)) for r in DP.derive_host(n, 1).radix[:DP.derive_host(n, 1).n_passes]) for n in TP.VALID_PRBS})
TP_CLASSES = (ALL_RADIX + [f"threads_per_row {t}" for t in (64, 128, 256)] + [f"n_prb {n}" for n in F.TP_EDGE_PRBS]
              + ["S % rows_per_workgroup != 0", "in place", "erasures", "a dropped row"])
LDPC_CLASSES = ([f"degree {d}" for d in range(2, 20)] + ["bpw capped by threads", "bpw capped by LDS", "bpw = 1", "threads % 64 != 0", "a partial last workgroup",
                                                         "more than one workgroup", "f32 input", "scale 1.3", "early_stop off", "n_punct 0"])
LDPC_ALSO = ["a block straddles a wave", "scale 1", "scale 4", "n_punct 1", "n_punct 2", "n_punct > 2", "n_in below full", "k_out % 32 != 0", "k_out % 128 != 0",
             "k_out % 128 == 0", "nb below", "nb multiple", "nb partial", "dtype i8"] + [f"max_iters {n}" for n in F.LDPC_ITERS]
TB_CLASSES = ([f"C {'> 1' if multi else '= 1'}, piece {piece}" for multi, piece in F.TB_PIECES]
              + ["CRC16", "CRC24A", "P % 32 != 0", "P % 8 != 0", "S C % 4 != 0", "C % 4 != 0"])
TB_ALSO = F.TB_CORRUPTIONS[:2] + F.TB_CORRUPTIONS[3:] + ["C > 4", "bg 1", "bg 2"]      # (a CRC24B flip needs C > 1: counted, not bounded)
ENC_CLASSES = ([f"col_dwords {k}" for k in range(1, 13)] + ["Zc % 32 == 0", "cw_required, C > 1", "C > 1, no cw_required", "rows_needed < n_rows", "repetition",
                                                            "k0[rv] in the fillers", "unequal E_r", "CRC16", "CRC24A", "core nr", "core triangular"]
               + [f"form {f}" for f in F.ENC_FORMS])
ENC_ALSO = ["truncated graph", "cw requested", "rv tensor", "rv strided", "rv scalar", "bg 1", "bg 2"]
MOD_CLASSES = ([f"Qm {q}" for q in (2, 4, 6, 8)] + [f"L {n}" for n in (1, 2, 3, 4)]
               + ["two hops", "first hop starts after symbol 0", "symbols in no hop", "tiles_per_symbol > 1", "an allocation crossing a tile edge",
                  "data on DM-RS symbols", "bits per symbol % 32 != 0", "params scalar", "params tensor", "params stride0", "scrambling off"])
MOD_ALSO = ["a tile beyond the first", "wide grid", "out= prefilled with NaN", "pilots shared", "pilots per slot", "beta 1", "beta 1.4125", "beta drawn", "B > 1",
            "dmrs T1", "dmrs T2", "dmrs T1_CDM0", "dmrs T1_CDM1", "rnti 0", "rnti 65535", "n_id 0", "n_id 1023"]


def _report(stage, n, counts, classes, least, also=()):
    print(f"{stage}: cases per class over {n} draws (at least {least} each)")
    for k in classes:
        print(f"  {k:>45}: {counts[k]}")
    for k in also:
        print(f"  {k:>45}: {counts[k]}  (counted only)")
    short = {k: counts[k] for k in classes if counts[k] < least}
    assert not short, f"{stage}: classes below {least} cases: {short}"
    none = [k for k in also if counts[k] == 0]
    assert not none, f"{stage}: never reached: {none}"


def test_draws_are_reproducible_and_plain():
    for draw in (F.draw_tp, F.draw_ldpc, F.draw_tb, F.draw_enc, F.draw_mod):
        a, b = draw(7), draw(7)
        assert a == b and a != draw(8) and eval(repr(a)) == a     # a case replays from its printed dict
    assert (F.STAGE_TP, F.STAGE_LDPC, F.STAGE_TB, F.STAGE_ENC, F.STAGE_MOD) == (4, 5, 6, 7, 8)      # behind the first fuzz's 1, 2, 3


def test_deprecoder_sweep_reaches_every_path_and_calibrates_the_tolerance():
    """One case per valid allocation size; C_TP_FUZZ re-measured with tp_oracle.deprecode_f32, the float32 restatement of
    the kernel's arithmetic, never with the kernel."""
    counts, worst = collections.Counter(), 0.0
    assert [F.draw_tp(i)["n_prb"] for i in range(F.N_TP)] == TP.VALID_PRBS
    for i in range(F.N_TP):
        c = F.draw_tp(i)
        d = F.realize_tp(c)
        counts.update(F.tp_classes(c, d))
        assert 1 <= c["S"] <= 14 and 1 <= c["B"] <= 5 and d.x_hat.dtype == np.complex64 and d.nvar.dtype == np.float32, c
        assert np.isposinf(d.ref_nv).any() == c["dropped_row"], c
        if d.row is not None:
            b, s = d.row
            assert np.all(np.isposinf(d.ref_nv[b, s * d.M:(s + 1) * d.M])) and np.all(d.ref_x[b, s * d.M:(s + 1) * d.M] == 0), c
        view = DP.derive_host(c["n_prb"], c["S"])
        x, nv = TP.deprecode_f32(d.x_hat, d.nvar, view, DP.twiddles(c["n_prb"], c["S"]))
        TP.check(x, nv, d.ref_x, d.ref_nv, view, f"float32 restatement {c}", t=F.C_TP_FUZZ)
        worst = max(worst, TP.x_ratio(x, d.ref_x, d.M))
    _report("de-precoder", F.N_TP, counts, TP_CLASSES, 1)
    print(f"C_TP_FUZZ = {worst:.3f} (recorded {F.C_TP_FUZZ:g}, T = {F.T_TP_FUZZ:g})")
    assert worst <= F.C_TP_FUZZ and F.T_TP_FUZZ == 4.0 * F.C_TP_FUZZ and round(F.C_TP_FUZZ, 1) == F.C_TP_FUZZ


def test_decoder_draw_reaches_every_path_and_mixes_its_workgroups():
    """Coverage counts; the host view's geometry against its two stated caps; and, from the oracle alone: in at least a third
    of the cases one workgroup holds blocks that stop at different iterations, in at least ten one holds ok = 1 and ok = 0."""
    counts = collections.Counter()
    n_mixed_stop = n_mixed_ok = 0
    zcs = []
    for i in range(F.N_LDPC):
        c = F.draw_ldpc(i)
        counts.update(F.ldpc_classes(c))
        zcs.append(c["zc"])
        n_rows, n_sys = len(c["degrees"]), c["n_sys"]
        assert 2 <= c["zc"] <= 384 and 2 <= n_sys <= 22 and 1 <= n_rows <= 46 and n_sys + n_rows <= 68 and 2 + i % 18 in c["degrees"], c
        rows = F.ldpc_graph(c)
        assert [len(r) for r in rows] == c["degrees"] and all(r[-1] == (n_sys + k, 0) and len({col for col, _ in r}) == len(r)
                                                               and all(col < n_sys + k for col, _ in r[:-1]) for k, r in enumerate(rows)), c
        v = F.ldpc_view(c)
        by_threads, by_lds = F.ldpc_caps(c, v)
        bpw = int(v.blocks_per_workgroup)
        assert bpw == max(1, min(by_threads, by_lds)) and v.threads == bpw * c["zc"] and v.max_row_degree == max(c["degrees"]), c
        assert 1 <= c["n_in"] <= (n_sys + n_rows - c["n_punct"]) * c["zc"] and 1 <= c["k_out"] <= n_sys * c["zc"] and 0 <= c["n_punct"] <= n_sys, c
        d = F.realize_ldpc(c)
        assert d.llr.shape == (c["nb"], c["n_in"]) and d.llr.dtype == (np.int8 if c["dtype"] == "i8" else np.float32), c
        if c["dtype"] == "i8":
            assert "random" not in d.kinds or d.llr.min() == -128 or c["n_in"] < 64, c
        groups = [d.status[g:g + bpw] for g in range(0, c["nb"], bpw)]
        n_mixed_stop += any(len(set(g[:, 0].tolist())) > 1 for g in groups)
        n_mixed_ok += any(set(g[:, 1].tolist()) == {0, 1} for g in groups)
    _report("LDPC decoder", F.N_LDPC, counts, LDPC_CLASSES, 3, LDPC_ALSO)
    assert zcs[:51] == F.NR_ZC and counts["an NR lifting size"] >= 51
    print(f"{n_mixed_stop} cases with a workgroup whose blocks stop at different iterations, {n_mixed_ok} with one holding ok = 1 and ok = 0")
    assert 3 * n_mixed_stop >= F.N_LDPC and n_mixed_ok >= 10


def test_degree_ladder_holds_every_degree():
    g = F.ladder_graph()
    assert sorted(len(r) for r in g.rows) == list(range(2, 20)) and g.zc == 7
    v = LD.derive_host(LD.LdpcGraph(g.rows, g.n_cols), g.zc, (g.n_cols - 1) * g.zc, g.n_sys * g.zc, n_punctured_cols=1)
    assert v.max_row_degree == 19 and v.blocks_per_workgroup >= 6


def test_assembly_draw_reaches_every_instance():
    """Coverage counts, all ten tb_residues<MULTI, PIECE> instances among them; the library's host view against the oracle's
    integers on every draw; a refused size is refused alike."""
    counts = collections.Counter()
    for i in range(F.N_TB):
        c = F.draw_tb(i)
        counts.update(F.tb_classes(c))
        assert 1 <= c["A"] <= F.TB_MAX_A and 1 <= c["S"] <= 12 and c["tries"] < 200000, c
        d = F.tb_derive(c)
        if isinstance(d, Exception):
            assert c["source"] == "edge", c
            with pytest.raises(type(d)):
                TB.derive_host(c["bg"], c["A"])
            continue
        v = TB.derive_host(c["bg"], c["A"])
        assert (v.c, v.k_prime, v.p, v.in_row_bytes, v.tb_row_bytes, v.l_tb, v.piece_dwords) == (d.C, d.Kp, d.P, d.in_row_bytes, d.tb_row_bytes, d.L_tb, F.tb_piece(d)), c
    _report("TB assembly", F.N_TB, counts, TB_CLASSES, 8, TB_ALSO)
    assert 1 <= counts["refused"] <= F.N_TB // 10, counts["refused"]
    assert [(F.draw_tb(i)["bg"], F.draw_tb(i)["A"]) for i in (4, 9, 14, 19)] == F.TB_NAMED_EDGES and isinstance(F.tb_derive(F.draw_tb(19)), ValueError)
    edges = {(c["bg"], c["A"]) for c in map(F.draw_tb, range(F.N_TB)) if c["source"] == "edge"}
    print(f"{counts['refused']} refused sizes; {len(edges)} distinct edges of {len(F.TB_EDGES)} drawn")
    assert {(1, 3824), (1, 3825), (1, 8424), (1, 8425)} <= set(F.TB_EDGES) and max(T.derive(bg, A).C for bg, A in F.TB_EDGES if F._tb_valid(bg, A)) == 11


def test_assembly_corruptions_do_what_they_say():
    """From the oracle alone, on every fifth draw: untouched rows pass everywhere, a refreshed CRC24B passes its block and
    fails the transport block, a CRC24B flip fails a block only, random rows fail."""
    seen = collections.Counter()
    for i in range(0, F.N_TB, 3):
        c = F.draw_tb(i)
        if isinstance(F.tb_derive(c), Exception):
            continue
        x = F.realize_tb(c)
        d = x.d
        assert x.rows.shape == (c["S"], d.C, d.in_row_bytes) and x.rows.dtype == np.uint8, c
        seen[x.kind] += 1
        if x.kind == "untouched":
            assert not x.tb_status.any() and not x.cb_status[..., 0].any() and np.array_equal(np.unpackbits(x.tb, axis=-1)[:, :d.A], x.tb_bits), c
        elif x.kind == "random rows":
            assert x.tb_status[:, 0].all(), c
        elif x.kind == "crc24b flips":
            assert x.cb_status[..., 0].any() and not x.tb_status[:, 0].any(), c
        elif x.kind == "refreshed crc24b":
            assert not x.cb_status[..., 0].any() and x.tb_status[:, 0].any(), c
        else:
            assert x.tb_status[:, 0].any(), c
    print(dict(seen))
    assert len(seen) == len(F.TB_CORRUPTIONS)


def test_three_pinned_assembly_cases_reach_the_missing_instances():
    for name, want in (("c1_piece3", (False, 3)), ("c1_piece4", (False, 4)), ("c2_piece4", (True, 4))):
        d = T.case_derive(name)
        assert (d.C > 1, F.tb_piece(d)) == want and [c["name"] for c in T.CASES[-3:]] == ["c1_piece3", "c1_piece4", "c2_piece4"]
        assert TB.derive_host(d.bg, d.A).piece_dwords == want[1]


def test_encoder_draw_reaches_every_path_and_refuses_alike():
    """Coverage counts; the rejection loop that pins a lifting size ends and all 51 sizes are present; the library derives
    the oracle's integers on every accepted draw and refuses the refused descriptors with the oracle's exception class, the
    malformed graphs with ValueError."""
    counts, zcs = collections.Counter(), set()
    for i in range(F.N_ENC):
        c = F.draw_enc(i)
        counts.update(F.enc_classes(c))
        assert c["tries"] < F.ENC_MAX_TRIES and 1 <= c["S"] <= 6 and len(c["rvs"]) == c["S"] and c["G"] <= F.RM_MAX_G + 1, c
        d = F.enc_derive(c)
        sh = E.SHAPE[c["bg"]]
        args = (c["bg"], c["A"], c["qm"], c["L"], c["G"])
        if isinstance(d, Exception):
            g = F.enc_graph(c, 2)
            with pytest.raises(type(d)):
                EN.PuschTransportEncoder(*args, LD.LdpcGraph(g.rows, g.n_cols), n_ref=c["n_ref"])
            continue
        g = F.enc_graph(c, d.Zc)
        if c["bad_graph"]:
            with pytest.raises(ValueError):
                EN.PuschTransportEncoder(*args, LD.LdpcGraph(g.rows, g.n_cols), n_ref=c["n_ref"])
            continue
        zcs.add(d.Zc)
        assert not c["want_zc"] or d.Zc == c["want_zc"], c
        v = F.enc_view(c, g)
        assert (v.c, v.zc, v.k_prime, v.n_cb, v.f0, v.f1, v.e_lo, v.e_hi, tuple(v.k0)) == (d.C, d.Zc, d.Kp, d.N_cb, d.f0, d.f1, min(d.E), max(d.E), d.k0), c
        assert v.col_dwords == -(-d.Zc // 32) and 4 <= len(g.rows) <= sh["n_rows"] and (g.n_cols - 2) * d.Zc >= d.N_cb, c
        assert (len(g.rows) == sh["n_rows"]) or c["n_ref"], c                  # truncated only where n_ref makes N_cb fit
        assert (v.core_form == 0) == E.is_triangular(g.rows, g.n_sys) == (c["form"] == "tri"), c
    _report("encoder", F.N_ENC, counts, ENC_CLASSES, 3, ENC_ALSO)
    print(f"{counts['refused descriptor']} refused descriptors, {counts['refused graph']} refused graphs: "
          + ", ".join(f"{k} {counts['refused graph: ' + k]}" for k in F.ENC_BAD_GRAPHS))
    assert set(F.NR_ZC) <= zcs and [F.draw_enc(i)["want_zc"] for i in range(51)] == F.NR_ZC
    assert 3 <= counts["refused descriptor"] <= 12 and 2 <= counts["refused graph"] <= 10 and all(counts["refused graph: " + k] for k in F.ENC_BAD_GRAPHS)


def test_modulator_draw_reaches_every_path_and_is_accepted():
    """MO.derive_host accepts every draw -- none refused, none skipped -- and its n_bits is the oracle's G."""
    counts = collections.Counter()
    for i in range(F.N_MOD):
        c = F.draw_mod(i)
        counts.update(F.mod_classes(c))
        v = F.mod_view(c)                                         # raises where the library refuses the draw
        case = F.mod_case_spec(c)
        n_data_re = len(Q.data_re_ref(case, c["mask"]))
        assert v.n_bits == n_data_re * c["L"] * c["qm"] > 0 and v.n_data_re == n_data_re, c
        assert 1 <= c["B"] <= 6 and c["B"] * v.n_bits <= max(F.MOD_MAX_BITS, v.n_bits) and max(h["n_prbs"] for h in c["hops"]) <= 24, c
        assert len(c["rnti"]) == len(c["n_id"]) == c["B"] and (c["param_kind"] == "tensor" or len(set(zip(c["rnti"], c["n_id"]))) == 1), c
        assert c["wide"] == (c["n_prb_grid"] in F.MOD_WIDE_GRIDS) and (c["beta"] == 1.4125 or float(np.float32(c["beta"])) == c["beta"]), c
        h1, h2, _ = S.numpy_hops(case)
        mod = MO.PuschModulator(h1, h2, c["L"], c["n_prb_grid"], c["qm"], n_sym=c["n_sym"], reserved_re_mask=c["mask"], scramble=c["scramble"])
        assert mod.n_bits == v.n_bits and mod.g_row_bytes == 16 * -(-v.n_bits // 128), c
    _report("modulator", F.N_MOD, counts, MOD_CLASSES, 8, MOD_ALSO)


def test_modulator_realization_matches_its_draw():
    """Every tenth draw realized: shapes, the garbage behind G, and the reference differs between two slots."""
    for i in range(0, F.N_MOD, 10):
        c = F.draw_mod(i)
        d = F.realize_mod(c)
        v = F.mod_view(c)
        assert d.G == v.n_bits and d.g_rows.shape == (c["B"], v.g_row_bytes) and d.n_re == v.n_re and d.n_cols == v.n_dmrs_total, c
        assert d.ref.shape == (c["B"], c["L"], c["n_sym"], 12 * c["n_prb_grid"]) and d.ref.dtype == np.complex64, c
        assert np.count_nonzero(d.ref[0, 0]) >= d.n_data_re, c
        assert torch.from_numpy(d.g_rows).is_contiguous()
