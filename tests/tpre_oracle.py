"""Oracle of the transform precoding entry point (include/ce_tp.h `ce_tp_precode`), the seeded inputs its GPU tests run
on, and the tolerance rule they follow.

The float64 reference is `tp_oracle.precode` (TS 38.211 6.3.1.4 literally; an explicit M x M matrix up to M = 512).
`precode_f32` restates the kernel's float32 arithmetic -- conjugate, `tp_oracle.passes_f32` (the de-precoder
restatement's passes) over the radix sequence and the twiddle table of the library's host entry points, the scale
float32(1 / sqrt(M)) in the last pass, conjugate -- only to calibrate the tolerance.

Tolerance rule, per output i of a row (eps = 2^-24, rms_row = the rms of the row's reference outputs), the shape of
`tp_oracle.x_unit`:
    |got_i - ref_i| <= T_PRE eps (log2(M) rms_row + |ref_i|)
A float32 FFT of length M errs in proportion to log2(M) times the rms of its outputs, the final scaling in proportion to
the output itself.  T_PRE = 4 C_PRE, where C_PRE is the largest ratio of `precode_f32`'s own error to that unit over the
inputs of the GPU tests (`inputs` over tp_oracle.CASES, `grid_inputs` over GRID_NAMES); the factor 4 is tp_oracle's, for
FMA contraction and pass-internal ordering on the GPU that the restatement cannot mirror.  tests/test_precode.py
re-measures C_PRE and fails if it exceeds C_PRE_RECORDED."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import dmrs_oracle
import enc_oracle as E
import eq_oracle as Q
import mod_oracle as MO
import tp_oracle as T
from srsran_ce_pytorch_amd import synth as S

F = T.F
C_PRE_RECORDED = 1.0     # measured 0.93 (test_precode.py::test_float32_restatement_calibrates_the_tolerance prints it per case), rounded up
T_PRE = 4.0 * C_PRE_RECORDED


def precode_f32(x, view, tw) -> np.ndarray:
    """complex64 [B, S M] of x [B, S M].  `view`: the library's host view of the shape; `tw`: its twiddle table (complex64 [M])."""
    M = int(view.m_sc)
    radix = [int(r) for r in view.radix[:view.n_passes]]
    x = np.asarray(x).astype(np.complex64)
    B = x.shape[0]
    x = x.reshape(-1, M)
    re, im = x.real.astype(F), (-x.imag).astype(F)                   # conjugate on load: exact
    scale = F(1.0 / np.sqrt(float(M)))                               # in double, rounded once
    re, im = T.passes_f32(re, im, radix, tw, scale)
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, -im                                     # conjugate on store: exact
    return out.reshape(B, -1)


def check(got, ref, M: int, what="", t=None) -> float:
    """The comparison every GPU test uses.  Prints the largest error ratio first and returns it."""
    t = T_PRE if t is None else t
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), f"{what}: non-finite output"
    r = T.x_ratio(got, ref, M)
    print(f"{what}: max |y - ref| / (2^-24 (log2(M) rms_row + |ref|)) = {r:.2f}  (bound {t:g})")
    assert r <= t, f"{what}: error ratio {r:.2f} > {t:g}"
    return r


# ---- dense rows: tp_oracle.CASES filled with seeded 16QAM symbols ----

@functools.lru_cache(maxsize=None)
def inputs(M: int, S_: int):
    """x [B, S M] complex64 (`tp_oracle.draw(...).x_tx`) and ref = precode(x) in float64; shared and read-only."""
    x = T.draw(M, S_).x_tx.astype(np.complex64)
    d = SimpleNamespace(M=M, S=S_, B=x.shape[0], x=x, ref=T.precode(x, M))
    for a in (d.x, d.ref):
        a.setflags(write=False)
    return d


# ---- grid cases: one layer, no data on DM-RS symbols ----
GRID_CASES = [
    # the geometry of the loop through every stage (mod_oracle.LOOP_GEOMETRY["bg2_z7_rep"]): 4 PRB at PRB 3 of 24, 5 data rows
    MO.mod_case("bg2_z7_rep", 24, [S.hop_spec([2], 3, 4, 0, 6)], 1, 2, B=3, seed=31),
    # two hops of 6 PRB at different prb_start, one DM-RS symbol each: 12 rows with two different offsets inside a symbol
    MO.mod_case("two_hops", 52, [S.hop_spec([2], 4, 6, 0, 7), S.hop_spec([9], 30, 6, 7, 7)], 1, 4, B=2, seed=32),
    # symbols 2 .. 9, DM-RS on 3: 7 rows of M = 24 at 4 rows per workgroup, the slot's last workgroup holds 3
    MO.mod_case("start2_partial", 24, [S.hop_spec([3], 5, 2, 2, 8)], 1, 4, B=2, seed=33),
    # M = 3240: one row per workgroup, 7 passes
    MO.mod_case("270_of_273", 273, [S.hop_spec([2, 11], 3, 270)], 1, 4, B=2, seed=34),
]
GRID_BY_NAME = {c["name"]: c for c in GRID_CASES}
GRID_NAMES = [c["name"] for c in GRID_CASES]
GRID_RNTI, GRID_N_ID = 0x4601, 333


def grid_rows(case):
    """(offsets, M, slot stride) by a brute-force walk of eq_oracle.data_re_ref: per symbol with data the offset
    sym n_sc + its lowest data subcarrier, in complex elements of a dense [n_sym, n_sc] slot."""
    n_sc = 12 * case["n_prb_grid"]
    re = Q.data_re_ref(case, 0xFFF)
    offsets, widths = [], set()
    for sym in sorted(set(re[:, 0].tolist())):
        sc = re[re[:, 0] == sym, 1]
        assert np.array_equal(sc, np.arange(sc[0], sc[0] + len(sc)))           # one contiguous run per symbol
        offsets.append(int(sym * n_sc + sc[0]))
        widths.add(len(sc))
    assert len(widths) == 1
    return offsets, widths.pop(), case["n_sym"] * n_sc


def take_rows(tx, offsets, M):
    """[B, S M] of a dense grid tx [B, 1, n_sym, n_sc]: the rows at `offsets`."""
    flat = np.asarray(tx).reshape(tx.shape[0], -1)
    return np.concatenate([flat[:, o:o + M] for o in offsets], axis=1)


@functools.lru_cache(maxsize=None)
def grid_inputs(name):
    """A grid case's seeded inputs (g_bits, packed g_rows, pilots), the modulator oracle's tx [B, 1, n_sym, n_sc], its data
    rows x [B, S M] and ref = precode(x); shared and read-only."""
    c = GRID_BY_NAME[name]
    case, qm, B = c["case"], c["qm"], c["B"]
    rng = np.random.default_rng(15000 + case["seed"])
    offsets, M, stride = grid_rows(case)
    G = len(offsets) * M * qm
    g_bits = rng.integers(0, 2, (B, G)).astype(np.uint8)
    hs = dmrs_oracle.hops_of(case)
    n_re, n_cols = int(hs[0][1].sum() * hs[0][2][:, 0].sum()), sum(len(sy) for sy, _, _ in hs)
    pilots = (rng.standard_normal((B, n_re, n_cols, 1)) + 1j * rng.standard_normal((B, n_re, n_cols, 1))).astype(np.complex64)
    tx = MO.modulate_ref(case, 0xFFF, qm, g_bits, pilots, case["beta"], GRID_RNTI, GRID_N_ID)
    x = take_rows(tx, offsets, M)
    d = SimpleNamespace(c=c, name=name, case=case, qm=qm, B=B, M=M, S=len(offsets), offsets=offsets, stride=stride, g_bits=g_bits,
                        g_rows=MO.pack(g_bits, 16 * -(-G // 128), rng), pilots=pilots, tx=tx, x=x, ref=T.precode(x, M))
    for a in (d.g_bits, d.g_rows, d.pilots, d.tx, d.x, d.ref):
        a.setflags(write=False)
    return d


# ---- the DFT-s-OFDM loop on the bg2_z7_rep geometry ----
LOOP_NAME, LOOP_NVAR = "bg2_z7_rep", 1e-3


def loop_tx(precoded=True):
    """(tx [B, 1, n_sym, n_sc] complex128, offsets, M): enc_oracle's g of the loop case through mod_oracle.modulate_ref with
    dmrs_oracle's pilots, the data rows precoded by tp_oracle.precode."""
    lp, case = E.LOOPS[LOOP_NAME], MO.loop_case(LOOP_NAME)
    tb_bits = E.inputs(LOOP_NAME)[0]
    bits, _ = E.transmit(E.case_derive(LOOP_NAME), E.graph(LOOP_NAME), tb_bits, [0] * len(tb_bits))          # rv 0 in every slot
    pil = dmrs_oracle.pilots_ref(case, MO.LOOP_SLOT, MO.LOOP_N_ID, MO.LOOP_N_SCID)
    tx = MO.modulate_ref(case, 0xFFF, lp["qm"], bits, pil, case["beta"], MO.LOOP_RNTI, MO.LOOP_SCR_ID).astype(np.complex128)
    offsets, M, _ = grid_rows(case)
    if precoded:
        flat = tx.reshape(tx.shape[0], -1)
        for o in offsets:
            flat[:, o:o + M] = T.precode(flat[:, o:o + M], M)
    return tx, offsets, M
