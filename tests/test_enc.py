"""CPU-side checks of the transport-block encoder extension (include/ce_enc.h): the ABI, the host derivation against the
oracles of rate recovery and transport-block assembly, every graph refusal by message before any device call, the oracle
against itself (zero syndromes, encode_nr against the forward-substitution encoder, and the whole loop segment -> encode ->
slot map -> LLRs -> recover -> decode_ref -> assemble_ref from the oracles alone), and the Python wrapper's argument errors.
No GPU."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import enc_oracle as E
import ldpc_oracle as O
import rm_oracle as R
import tb_oracle as T
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, encoder as EN, ldpc as LD, ratematch as RM

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _graph(name):
    g = E.graph(name)
    return LD.LdpcGraph(g.rows, g.n_cols)


def _view(name, graph=None):
    c = E.CASE_BY_NAME[name]
    return EN.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], graph or _graph(name), c["n_ref"])


def test_library_exports_every_declared_enc_symbol(lib):
    header = (ROOT / "include" / "ce_enc.h").read_text()
    # the header against the binding: tests/test_abi_conformance.py; here the sizes this stage's header implies, the
    # package's re-export and what the header says of the NR-core form
    # LP64 sizes implied by the header: desc 10 * 4 + 3 pointers; info 6 * 4 + 8; view 44 * 4
    assert (C.sizeof(_lib.EncDesc), C.sizeof(_lib.EncInfo), C.sizeof(_lib.EncHostView)) == (64, 32, 176)
    assert "ce_enc.hip" in _lib.SOURCES and "ce_enc.h" in _lib.REGISTRY
    assert PKG.PuschTransportEncoder is EN.PuschTransportEncoder
    assert "THIS PROJECT'S READING" in header and "nothing is tested against them" in header      # the NR-core form is stated as this project's reading


@pytest.mark.parametrize("name", E.NAMES)
def test_host_view_equals_the_oracles(lib, name):
    c, d, g = E.CASE_BY_NAME[name], E.case_derive(name), E.graph(name)
    t = T.derive(c["bg"], c["A"])
    v = _view(name)
    assert (v.b, v.k_cb, v.c, v.b_prime, v.k_prime, v.k_b, v.zc, v.k, v.n, v.n_cb, v.f0, v.f1, v.p_rm) == \
        (d.B, d.K_cb, d.C, d.Bp, d.Kp, d.K_b, d.Zc, d.K, d.N, d.N_cb, d.f0, d.f1, d.P)
    assert [v.e_lo] * v.n_lo + [v.e_hi] * (v.c - v.n_lo) == d.E and tuple(v.k0) == d.k0
    rm = RM.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], n_ref=c["n_ref"])
    assert tuple(v.s) == tuple(rm.s) and (v.n_lo, v.e_lo, v.e_hi) == (rm.n_lo, rm.e_lo, rm.e_hi)
    assert (v.l_tb, v.l_cb, v.p, v.g_tb, v.g_cb, v.tb_row_bytes) == (t.L_tb, t.L_cb, t.P, t.g_tb, t.g_cb, t.tb_row_bytes)
    assert v.g_row_bytes == 16 * -(-d.G // 128) and v.cw_row_bytes == 16 * -(-g.n_cols * d.Zc // 128)
    assert v.n_sys == g.n_sys and v.n_edges == sum(len(r) for r in g.rows)
    tri = c["form"] == "tri"
    assert v.core_form == (_lib.CE_ENC_CORE_TRIANGULAR if tri else _lib.CE_ENC_CORE_NR)
    if not tri:
        shifts = {i: s for i in range(4) for col, s in g.rows[i] if col == g.n_sys}
        assert v.core_rows == sum(1 << i for i in shifts) == sum(1 << i for i in E.HOLDERS[c["form"]])
        odd = [s for s in shifts.values() if list(shifts.values()).count(s) % 2]
        assert v.core_shift == odd[0]
    assert v.rows_needed == min(len(g.rows), max(4, -(-(2 * d.Zc + d.N_cb) // d.Zc) - g.n_sys))
    assert v.col_dwords == -(-d.Zc // 32) and 32 * (v.ext_dwords - 1) >= 2 * d.Zc + 32
    starts = np.cumsum([0] + d.E)[1:-1]
    assert v.cw_required == int(any(s % 32 for s in starts)) and v.threads == _lib.CE_ENC_THREADS and 0 < v.lds_bytes <= 65536
    enc = EN.PuschTransportEncoder(c["bg"], c["A"], c["qm"], c["L"], c["G"], _graph(name), n_ref=c["n_ref"])
    assert (enc.n_code_blocks, enc.zc, enc.n_cb, enc.needs_codeword, enc.core_form, enc.device) == \
        (d.C, d.Zc, d.N_cb, bool(v.cw_required), "triangular" if tri else "nr", None)


@functools.lru_cache(maxsize=None)
def _sweep_graph(bg, zc):
    sh = E.SHAPE[bg]
    return LD.LdpcGraph(E.nr_core_graph(np.random.default_rng(zc), sh["n_sys"], sh["n_rows"], zc, sh["core_degree"], sh["ext"], zc & 1), sh["n_sys"] + sh["n_rows"])


def test_integers_are_rate_recoverys_and_assemblys_over_a_sweep(lib):
    """The (base graph, size) sweep of test_tb.py: the same integers as rm_oracle / tb_oracle where they derive, and what
    ce_rm_derive_host refuses is refused here in its words."""
    rng = np.random.default_rng(1)
    sizes = sorted({1, 2, 8, 3824, 3825, 8424, 8425, 1277992, 2 ** 31 - 25} | set(rng.integers(1, 1300000, 300).tolist())
                   | set(rng.integers(1, 8000, 150).tolist()))                      # mostly C <= 2: sizes that do derive
    refused = accepted = 0
    for bg in (1, 2):
        for A in sizes:
            try:
                d = R.derive(bg, A, 2, 1, 1 << 21)
            except ValueError:
                d = None
            graph = _sweep_graph(bg, d.Zc if d else 2)
            desc, keep = EN.build_desc(bg, A, "qpsk", 1, 1 << 21, graph)
            view = _lib.EncHostView()
            rc = lib.ce_enc_derive_host(C.byref(desc), C.byref(view))
            text = _lib.last_error()
            rdesc = RM.build_desc(bg, A, "qpsk", 1, 1 << 21)
            rrc = lib.ce_rm_derive_host(C.byref(rdesc), C.byref(_lib.RmHostView()))
            rtext = _lib.last_error()
            if d is None:
                refused += 1
                assert rc == rrc == _lib.CE_ERR_INVALID and text == rtext, (bg, A, text, rtext)
                continue
            accepted += 1
            t = T.derive(bg, A)
            assert rc == 0, (bg, A, text)
            assert (view.b, view.c, view.k_prime, view.zc, view.n_cb, view.f0, view.f1, view.p_rm, view.p, view.l_tb, view.l_cb) == \
                (d.B, d.C, d.Kp, d.Zc, d.N_cb, d.f0, d.f1, d.P, t.P, t.L_tb, t.L_cb), (bg, A)
            assert tuple(view.k0) == d.k0 and [view.e_lo] * view.n_lo + [view.e_hi] * (view.c - view.n_lo) == d.E
            del keep
    assert refused > 50 and accepted > 100


def _refusal(lib, name, rows=None, n_cols=None, **fields):
    c, g = E.CASE_BY_NAME[name], E.graph(name)
    graph = LD.LdpcGraph(g.rows if rows is None else rows, g.n_cols if n_cols is None else n_cols)
    desc, keep = EN.build_desc(c["bg"], c["A"], c["qm"], c["L"], c["G"], graph, c["n_ref"])
    for k, v in fields.items():
        setattr(desc, k, v)
    view, handle = _lib.EncHostView(), C.c_void_p()
    rc = lib.ce_enc_derive_host(C.byref(desc), C.byref(view))
    text = _lib.last_error() if rc else ""
    if rc:
        assert lib.ce_enc_plan_create(C.byref(desc), C.byref(handle)) == rc and not handle.value      # before any device call
    del keep
    return rc, text


def _edit(name, r, fn):
    rows = [list(row) for row in E.graph(name).rows]
    rows[r] = fn(rows[r])
    return rows


def test_every_graph_refusal_names_the_row_or_column(lib):
    nr, tri = "bg2_z7_rep", "bg2_z7_tri"
    n_sys = 10
    assert _refusal(lib, nr) == (0, "") and _refusal(lib, tri) == (0, "")
    own = lambda r: n_sys + r                                                            # noqa: E731
    broken = [
        # an extension row
        (_edit(nr, 9, lambda row: [(c, 3 if c == own(9) else s) for c, s in row]), r"row 9: its own parity column 19 must appear exactly once, at shift 0"),
        (_edit(nr, 9, lambda row: [e for e in row if e[0] != own(9)]), r"row 9: its own parity column 19 must appear exactly once"),
        (_edit(nr, 9, lambda row: row + [(own(9), 0)]), r"row 9: its own parity column 19 must appear exactly once"),
        (_edit(nr, 9, lambda row: row + [(own(7), 0)]), r"row 9: column 17 is neither below n_sys \+ 4 = 14 nor the row's own column 19"),
        (_edit(nr, 2, lambda row: row + [(own(7), 0)]), r"row 2: column 17 lies beyond the core columns"),
        # the core
        (_edit(nr, 0, lambda row: row + [(n_sys, 2)]), r"row 0 holds core column 10 more than once"),
        (_edit(nr, 2, lambda row: [(c, 1 if c == n_sys + 2 else s) for c, s in row]), r"column 12 must appear in exactly rows 1 and 2, both at shift 0 \(row 2"),
        (_edit(nr, 3, lambda row: row + [(n_sys + 1, 0)]), r"column 11 must appear in exactly rows 0 and 1, both at shift 0 \(row 3"),
        (_edit(nr, 2, lambda row: [e for e in row if e[0] != n_sys + 3]), r"column 13 must appear in exactly rows 2 and 3, both at shift 0 \(row 2"),
        (_edit(nr, 3, lambda row: [e for e in row if e[0] != n_sys]), r"column 10 appears in 2 of the four core rows, not in three"),
        (_edit(nr, 1, lambda row: row + [(n_sys, 0)]), r"column 10 appears in 4 of the four core rows, not in three"),
        (_edit(tri, 2, lambda row: [(c, 1 if c == n_sys + 2 else s) for c, s in row]), r"neither triangular nor an NR core: column 1\d"),
        # ranges
        (_edit(nr, 5, lambda row: [(c, 7 if i == 0 else s) for i, (c, s) in enumerate(row)]), r"row 5, column \d+: shift 7 outside 0..6"),
        (_edit(nr, 5, lambda row: [(52, 0)] + row), r"row 5: column 52 outside 0..51"),
        (_edit(nr, 5, lambda row: row + [(0, 0)] * 20), r"row 5 has \d+ edges: 1..19 are supported"),
    ]
    for rows, pattern in broken:
        rc, text = _refusal(lib, nr, rows=rows)                                          # both graphs serve the same (A, G)
        assert rc == _lib.CE_ERR_INVALID and re.search(pattern, text), (pattern, text)
    # three different shifts of the first parity column
    rows = [list(r) for r in E.graph(nr).rows]
    k = 0
    for i in range(4):
        rows[i] = [(c, (k := k + 1) if c == n_sys else s) for c, s in rows[i]]
    rc, text = _refusal(lib, nr, rows=rows)
    assert rc == _lib.CE_ERR_INVALID and re.search(r"column 10 has three different shifts 1, 2, 3: two must be equal", text), text
    # the shape of the base graph, and a graph too short for the buffer
    g = E.graph(nr)
    rc, text = _refusal(lib, nr, rows=g.rows[:41], n_cols=52)
    assert rc == _lib.CE_ERR_INVALID and "base graph 2 has n_sys = 10 and at most 52 columns; the graph given has n_sys = 11 and 52 columns" in text, text
    rc, text = _refusal(lib, "bg1_z15", n_cols=69)
    assert rc == _lib.CE_ERR_INVALID and "n_sys = 23" in text, text
    rc, text = _refusal(lib, nr, rows=g.rows[:3], n_cols=13)
    assert rc == _lib.CE_ERR_INVALID and "n_rows=3 outside 4..46" in text, text
    rc, text = _refusal(lib, nr, rows=g.rows[:20], n_cols=30)                            # N_cb = 350 > 28 * 7
    assert rc == _lib.CE_ERR_INVALID and "too short for the circular buffer: (n_cols - 2) Zc = 196 < N_cb = 350" in text, text
    assert _refusal(lib, "bg1_z15_rows12")[0] == 0                                       # a prefix is accepted where n_ref makes N_cb fit
    c = E.CASE_BY_NAME["bg1_z15_rows12"]
    with pytest.raises(ValueError, match="too short"):
        EN.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], _graph("bg1_z15_rows12"), 0)
    # the descriptor's own fields, and what rate recovery refuses, in its words
    for fields, word in ((dict(abi_version=4), "ABI"), (dict(base_graph=3), "base_graph"), (dict(tbs=0), "tbs"), (dict(qm=3), "qm"), (dict(n_layers=5), "n_layers"),
                         (dict(g_bits=481), "g_bits"), (dict(n_ref=5), "n_ref"), (dict(row_start=None), "null graph")):
        rc, text = _refusal(lib, nr, **fields)
        assert rc == _lib.CE_ERR_INVALID and word in text, (fields, text)
    rdesc = RM.build_desc(2, 24, "qpsk", 1, 481)
    assert lib.ce_rm_derive_host(C.byref(rdesc), C.byref(_lib.RmHostView())) == _lib.CE_ERR_INVALID
    assert _lib.last_error() == _refusal(lib, nr, g_bits=481)[1]


def test_null_arguments_are_refused(lib):
    assert lib.ce_enc_derive_host(None, None) == _lib.CE_ERR_INVALID and lib.ce_enc_plan_create(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_enc_plan_get_info(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_enc_encode(None, None, None, 0, 0, None, None, None) == _lib.CE_ERR_INVALID
    lib.ce_enc_plan_destroy(None)


# ---- the oracle against itself ----

@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("zc", [2, 7, 15, 36, 208])
def test_encode_nr_gives_zero_syndromes_and_equals_forward_substitution(bg, zc):
    sh = E.SHAPE[bg]
    rng = np.random.default_rng(100 * bg + zc)
    info = rng.integers(0, 2, (2, sh["n_sys"] * zc))
    for variant in (0, 1, 2):
        rows = E.nr_core_graph(rng, sh["n_sys"], sh["n_rows"], zc, sh["core_degree"], sh["ext"], variant)
        assert max(len(r) for r in rows) <= O.MAX_ROW_DEGREE and not E.is_triangular(rows, sh["n_sys"])
        held = [i for i in range(4) if any(c == sh["n_sys"] for c, _ in rows[i])]
        assert tuple(held) == E.HOLDERS[variant]
        cw = E.encode_nr(rows, sh["n_sys"], zc, info)
        assert np.array_equal(cw[:, :sh["n_sys"] * zc], info) and not O.syndrome(rows, zc, cw).any(), (bg, zc, variant)
    rows = O.random_graph(rng, sh["n_sys"], sh["n_rows"], zc, sh["core_degree"], sh["ext"])
    assert E.is_triangular(rows, sh["n_sys"])
    assert np.array_equal(E.encode_nr(rows, sh["n_sys"], zc, info), O.encode(rows, sh["n_sys"], zc, info))


@pytest.mark.parametrize("name", E.NAMES)
def test_pinned_cases_are_codewords_and_place_their_bits(name):
    d, g = E.case_derive(name), E.graph(name)
    tb_bits, tb_rows = E.inputs(name)
    bits, cw = E.transmit(d, g, tb_bits, E.rvs_of(name, 0))
    assert bits.shape == (len(tb_bits), d.G) and cw.shape == (len(tb_bits), d.C, g.n_cols * d.Zc)
    assert not O.syndrome(g.rows, d.Zc, cw).any() and not cw[..., d.Kp:d.K].any()          # fillers are 0
    assert np.array_equal(cw[..., :d.Kp], T.segment(tb_bits, d.bg).reshape(cw.shape[0], d.C, d.Kp))
    assert np.array_equal(LD.unpack_bits(tb_rows, d.A), tb_bits)
    g_rows, cw_rows = E.reference(name, 0)
    assert np.array_equal(LD.unpack_bits(g_rows, d.G), bits) and np.array_equal(LD.unpack_bits(cw_rows, cw.shape[-1]), cw)


LOOPS = E.LOOPS


def loop_reference(name, rvs_list, flip_slot=None, negate_slot=None):
    """The oracle-only loop: segment -> encode -> slot map -> +-64 int8 LLRs -> recover (combining the transmissions of
    rvs_list) -> decode_ref -> assemble_ref.  Returns (tb bits sent, tb rows out, tb_status)."""
    d, g = E.case_derive(name), E.graph(name)
    tb_bits = np.array(E.inputs(name)[0])
    if flip_slot is not None:
        tb_bits[flip_slot, d.A // 2] ^= 1
    soft = None
    for rv in rvs_list:
        bits, _ = E.transmit(d, g, tb_bits, [rv] * len(tb_bits))
        llr = (64 - 128 * bits.astype(np.int64)).astype(np.int8)
        if negate_slot is not None:
            llr[negate_slot] = -llr[negate_slot]
        soft, _ = R.recover(d, llr, [rv] * len(tb_bits), harq=soft)
    L, status, _ = O.decode_ref(g.rows, g.n_cols, d.Zc, O.channel(O.quantise(soft.reshape(-1, d.N_cb)), g.n_cols, d.Zc, 2), 8, True)
    t = T.derive(d.bg, d.A)
    tb, tb_status, _ = T.assemble_ref(O.pack(L, d.Kp).reshape(len(tb_bits), d.C, -1), t)
    return tb_bits, tb, tb_status


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_the_oracle_loop_returns_the_transport_block(name):
    c = E.CASE_BY_NAME[name]
    assert {k: c[k] for k in ("bg", "A", "qm", "L", "G")} == {k: v for k, v in LOOPS[name].items() if k != "pinned"}
    d = E.case_derive(name)
    assert all(getattr(d, k) == v for k, v in LOOPS[name]["pinned"].items())
    sent, tb, status = loop_reference(name, [0])
    assert np.array_equal(LD.unpack_bits(tb, d.A), sent) and not status.any()
    sent, tb, status = loop_reference(name, [0, 2], flip_slot=1)                      # a flipped payload bit is a valid block too
    assert np.array_equal(LD.unpack_bits(tb, d.A), sent) and not status.any() and not np.array_equal(sent, E.inputs(name)[0])
    _, _, status = loop_reference(name, [0], negate_slot=0)                           # every LLR negated: the CRC fails
    assert status[0, 0] != 0 and not status[1:].any()


def test_noisy_codewords_decode_at_the_existing_es_n0():
    for name in ("bg2_z7_rep", "bg1_z15", "bg2_z36_kb8"):
        d, g = E.case_derive(name), E.graph(name)
        rng = np.random.default_rng(77)
        info = rng.integers(0, 2, (3, d.K))
        cw = E.encode_nr(g.rows, g.n_sys, d.Zc, info)
        llr = O.noisy_llr(rng, cw[:, 2 * d.Zc:], O.ESN0_DB, O.SCALE)
        L, status, _ = O.decode_ref(g.rows, g.n_cols, d.Zc, O.channel(O.quantise(llr), g.n_cols, d.Zc, 2), 8, True)
        assert np.all(status[:, 1] == 1) and np.array_equal(L[:, :d.K] < 0, info == 1), name


# ---- the Python wrapper ----

def test_python_wrapper_without_a_device():
    g = _graph("bg2_z7_rep")
    with pytest.raises(ValueError, match="base_graph"):
        EN.PuschTransportEncoder(3, 24, "qpsk", 1, 480, g)
    with pytest.raises(ValueError, match="tbs"):
        EN.PuschTransportEncoder(2, 0, "qpsk", 1, 480, g)
    with pytest.raises(ValueError, match="g_bits"):
        EN.PuschTransportEncoder(2, 24, "16qam", 1, 482, g)
    with pytest.raises(ValueError, match="n_sys = 22"):
        EN.PuschTransportEncoder(1, 24, "qpsk", 1, 480, g)
    with pytest.raises(ValueError, match="LdpcGraph"):
        EN.PuschTransportEncoder(2, 24, "qpsk", 1, 480, E.graph("bg2_z7_rep").rows)
    enc = EN.PuschTransportEncoder(2, 24, "qpsk", 1, 480, g)
    assert (enc.n_code_blocks, enc.zc, enc.n_cb, enc.k_prime, enc.payload_bits, enc.tb_row_bytes, enc.g_row_bytes, enc.cw_row_bytes, enc.codeword_bits) == \
        (1, 7, 350, 40, 40, 16, 64, 48, 364)
    assert enc.core_form == "nr" and not enc.needs_codeword and enc.device is None
    rm = RM.PuschRateRecovery(1, 8448, "16qam", 3, 16812, n_ref=9000)
    two = EN.PuschTransportEncoder.for_rate_recovery(rm, _graph("bg1_z208_lbrm"))
    assert (two.base_graph, two.tbs, two.qm, two.n_layers, two.n_bits, two.n_ref, two.n_code_blocks, two.n_cb, two.needs_codeword) == \
        (1, 8448, 4, 3, 16812, 9000, 2, 9000, True)
    with pytest.raises(ValueError, match="PuschRateRecovery"):
        EN.PuschTransportEncoder.for_rate_recovery(None, g)
    for bad in (torch.zeros((3, 16), dtype=torch.int8), torch.zeros((3, 15), dtype=torch.uint8), torch.zeros((16,), dtype=torch.uint8),
                torch.zeros((3, 1, 16), dtype=torch.uint8), torch.zeros((3, 32), dtype=torch.uint8)[:, ::2], np.zeros((3, 16), np.uint8)):
        with pytest.raises(ValueError, match=r"\[slots, 16\]"):
            enc(bad)
