"""Seeded random cases for the OFDM modulator (csrc/ce_ofdm.hip `ce_ofdmtx_kernel`, entry point `ce_ofdmtx_modulate`, wrapper
`PuschOfdmModulator`), the one PUSCH kernel the three earlier fuzzes leave at the pinned cases of ofdm_oracle.CASES, for
tests/test_tx_fuzz.py (CPU: what the draws must satisfy by themselves) and tests/test_zzzzzzzzzzzzzzz_hip_tx_fuzz.py (GPU: the
kernel against the oracle on them).

The structure is tests/front_fuzz_cases.py's: `draw_tx(idx)` derives a case from np.random.default_rng([BASE_SEED, STAGE_TX,
idx]) as a plain dict of Python values (stage id 12, behind the earlier fuzzes' 1 .. 11, so none of their draws changes);
`realize_tx(case)` turns it into arrays, seeded by the dict's own "seed"; `tx_classes(case)` names the kernel paths it reaches,
from `ofdm.derive_host` and the dict alone.  The reference is ofdm_oracle.modulate in float64 and the rule ofdm_tx_oracle.check:
neither is restated here.  `tx_check` adds the one clause the rule cannot express: a sample of an all-zero symbol, whose unit
is 0, must be exactly 0."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import ofdm_oracle as OO
import ofdm_tx_oracle as X
from front_fuzz_cases import OFDM_CP_KINDS, OFDM_PHASORS, OFDM_SCS
from srsran_ce_pytorch_amd import ofdm as OF
from stage_fuzz_cases import BASE_SEED, _pick, _rng   # noqa: F401  (BASE_SEED: the seed all four fuzzes share)

STAGE_TX = 12
N_TX = 120

# T = 4 C as in ofdm_tx_oracle.py; C = the float32 numpy restatements' largest error ratio over the realized draws
# (tests/test_tx_fuzz.py re-measures both and fails if one exceeds its recorded value); never measured on a kernel
C_TX_FUZZ = 0.9          # measured 0.846 (ofdm_tx_oracle.modulate_f32 over the 120 draws), rounded up
T_TX_FUZZ = 4.0 * C_TX_FUZZ
C_PAIR = 3.3             # measured 3.216 (ofdm_oracle.demodulate_f32 of modulate_f32 over the draws built through for_demodulator), rounded up
T_PAIR = 4.0 * C_PAIR

TX_CP_KINDS, TX_PHASORS, TX_SCS = OFDM_CP_KINDS, OFDM_PHASORS, OFDM_SCS      # the demodulator fuzz's: normal / extended / free; none / unit / scaled
TX_LAYOUTS = ["dense", "out= dense", "longer rows", "ports in slots", "slots in ports", "ports in slots at an odd sample", "slots in ports at an odd sample"]
TX_BIG_BATCH_CASES = [31, 91]      # N = 128, B R >= 64, 9 .. 14 symbols: three or four workgroups per (slot, port), hundreds in flight
TX_MAX_SAMPLES = 1 << 18           # B R T of a case (the two big batches: at most twice that): the float64 reference stays far under a second
TX_MAX_ITEMS_4096 = 2              # B R at N = 4096


def draw_tx(idx):
    """One modulator case.  Everything in it is defined by include/ce_tp.h: n_fft one of the six sizes, 12 n_prb_grid <= n_fft,
    1 .. 14 symbols, 0 <= cp_len[l] <= n_fft, finite phasors of any modulus, a 16-byte aligned dense grid, 8-byte aligned
    samples whose rows of T are pairwise disjoint with the ports inside a slot or the slots inside a port.

    The transform length; the grid width (1 PRB, all that fit, or between); 1 .. 14 symbols whose cyclic prefixes are NR
    normal ones at a drawn numerology and slot, NR extended ones (N / 4; at most the 12 symbols of such a slot) or free per
    symbol from {0, 1, N, U(0, N), U(0, 40)}; the phasors; B in 1 .. 3 and R in 1 .. 4, lowered until B R T <= TX_MAX_SAMPLES
    (and B R <= 2 at N = 4096), except in the two big-batch cases; the grid's content (a run of non-zero PRBs in a third of
    the cases, one to three all-zero symbols in a quarter, never all of them) and its place in a longer buffer; the output
    layout with its lead, strides and tail in elements; the (slot, port) of the single-row comparison; whether the modulator
    is built through `for_demodulator`, and then the demodulator's window advance from {0, min cp, U(0, min cp)}."""
    rng = _rng(STAGE_TX, idx)
    big = idx in TX_BIG_BATCH_CASES
    N = 128 if big else int(_pick(rng, list(OF.FFT_SIZES)))
    n_prb = int(_pick(rng, [1, N // 12, int(rng.integers(1, N // 12 + 1))]))
    n_sym = int(rng.integers(9, 15)) if big else int(rng.integers(1, 15))
    kind = str(_pick(rng, TX_CP_KINDS))
    scs, cp_slot = float(_pick(rng, TX_SCS)), 0
    if kind == "normal":
        cp_slot = int(rng.integers(0, int(scs / 15e3)))
        cp = [int(v) for v in OO.cp_lengths_ref(scs, N, n_sym, cp_slot)]
    elif kind == "extended":
        n_sym = min(n_sym, 12)
        cp = [N // 4] * n_sym
    else:
        cp = [int(_pick(rng, [0, 1, N, int(rng.integers(0, N + 1)), int(rng.integers(0, 41))])) for _ in range(n_sym)]
    T = sum(cp) + n_sym * N
    B, R = (int(rng.integers(8, 11)), int(rng.integers(8, 11))) if big else (int(rng.integers(1, 4)), int(rng.integers(1, 5)))
    while not big and (B * R * T > TX_MAX_SAMPLES or (N == 4096 and B * R > TX_MAX_ITEMS_4096)):
        B, R = (B, R - 1) if R >= B else (B - 1, R)
    # ---- the grid: content and placement ----
    prb_run = None
    if n_prb > 1 and rng.random() < 0.37:                 # (a 1-PRB grid has no PRB to leave empty: a third of all cases remain)
        n_run = int(rng.integers(1, n_prb))
        prb_run = [int(rng.integers(0, n_prb - n_run + 1)), n_run]
    zero_syms = []
    if n_sym > 1 and rng.random() < 0.27:
        zero_syms = sorted(int(l) for l in rng.choice(n_sym, int(rng.integers(1, min(n_sym - 1, 3) + 1)), replace=False))
    grid_lead, grid_tail = 2 * int(rng.integers(0, 33)), int(rng.integers(0, 65))
    # ---- the output ----
    layout = str(_pick(rng, TX_LAYOUTS))
    gap = lambda: int(_pick(rng, [0, 1, int(rng.integers(2, 100))]))   # noqa: E731
    lead, row_len, ss, ps = 0, T, R * T, T
    if layout == "longer rows":
        row_len = T + int(rng.integers(1, 41))
        ss, ps = R * row_len, row_len
    elif layout.startswith("ports in slots"):
        ps = T + gap()
        ss = (R - 1) * ps + T + gap()
    elif layout.startswith("slots in ports"):            # one stream per port: slot b right behind slot b - 1, or a gap behind
        ss = T + int(_pick(rng, [0, 0, gap()]))
        ps = B * ss + gap()
    if layout.endswith("odd sample"):
        lead = 2 * int(rng.integers(0, 50)) + 1
    elif layout.startswith(("ports in", "slots in")):
        lead = 2 * int(rng.integers(0, 50))
    via_dem = bool(rng.random() < 0.5)
    advance = int(_pick(rng, [0, min(cp), int(rng.integers(0, min(cp) + 1))])) if via_dem else 0
    return dict(stage="tx", idx=idx, n_fft=N, n_prb_grid=n_prb, n_sym=n_sym, cp_kind=kind, scs=scs, cp_slot=cp_slot, cp_len=cp,
                phasor=str(_pick(rng, TX_PHASORS)), B=B, R=R, prb_run=prb_run, zero_syms=zero_syms, grid_lead=grid_lead, grid_tail=grid_tail,
                layout=layout, lead=lead, row_len=row_len, slot_stride=ss, port_stride=ps, tail=int(rng.integers(0, 100)),
                slot=int(rng.integers(B)), port=int(rng.integers(R)), via_dem=via_dem, advance=advance, seed=int(rng.integers(1 << 30)))


def tx_extent(c):
    """Elements of the stream from the first sample of row (0, 0) to behind the last element of the last row."""
    return (c["B"] - 1) * c["slot_stride"] + (c["R"] - 1) * c["port_stride"] + c["row_len"]


def tx_rows(c):
    """bool [lead + extent + tail]: the elements of the stream the modulator writes -- the first T of each (slot, port) row."""
    _, T = X.symbol_starts(c["n_fft"], c["cp_len"])
    rows = np.zeros(c["lead"] + tx_extent(c) + c["tail"], bool)
    for b in range(c["B"]):
        for r in range(c["R"]):
            o = c["lead"] + b * c["slot_stride"] + r * c["port_stride"]
            assert not rows[o:o + T].any(), (c, b, r)            # the header's rule: no two rows share a sample
            rows[o:o + T] = True
    return rows


def realize_tx(c):
    """grid [B, R, n_sc, n_sym] complex64: CN(0, 1) times an amplitude 10^U(-3, 3) per (slot, port), exact zeros outside the
    PRB run and on the zero symbols; the phasors (unit modulus at seeded angles, or with a modulus in 0.25 .. 4); the float64
    reference ofdm_oracle.modulate [B, R, T] and the rule's per-sample symbol rms (0 on the samples of an all-zero symbol).
    For a case built through `for_demodulator` also the round trip's reference |phi_l|^2 X and its unit's rms: per symbol
    |phi_l|^2 sqrt(sum_k |X[k, l]|^2 / N), the rms of the N samples the demodulator's window holds (the transform is
    unitary), times the |phi_l| of its product at the store."""
    rng = np.random.default_rng(c["seed"])
    N, B, R, n_sym, n_sc = c["n_fft"], c["B"], c["R"], c["n_sym"], 12 * c["n_prb_grid"]
    starts, T = X.symbol_starts(N, c["cp_len"])
    amp = 10.0 ** rng.uniform(-3.0, 3.0, (B, R, 1, 1))
    shape = (B, R, n_sc, n_sym)
    grid = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5) * amp).astype(np.complex64)
    if c["prb_run"] is not None:
        p0, n_run = c["prb_run"]
        grid[:, :, :12 * p0] = 0
        grid[:, :, 12 * (p0 + n_run):] = 0
    grid[:, :, :, c["zero_syms"]] = 0
    phi = None
    if c["phasor"] != "none":
        phi = np.exp(2j * np.pi * rng.random(n_sym))
        if c["phasor"] == "scaled":
            phi = phi * rng.uniform(0.25, 4.0, n_sym)
        phi = phi.astype(np.complex64)
    ref = OO.modulate(grid, N, c["cp_len"], phi)
    d = SimpleNamespace(c=c, T=T, starts=starts, n_sc=n_sc, grid=grid, phi=phi, ref=ref, rms=X.symbol_rms(ref, N, c["cp_len"]))
    if c["via_dem"]:
        p2 = np.ones(n_sym) if phi is None else np.abs(phi.astype(np.complex128)) ** 2
        x = grid.astype(np.complex128)
        d.pair_ref = p2 * x
        d.pair_rms = p2 * np.sqrt((np.abs(x) ** 2).sum(-2, keepdims=True) / N)          # [B, R, 1, n_sym]
    return d


def tx_check(got, ref, rms, n_fft, what, t, rule=X.check):
    """`rule` (ofdm_tx_oracle.check, or ofdm_oracle.check for the round trip) over the outputs whose unit is not 0; where it is
    0 -- the outputs of an all-zero symbol -- the reference is exactly 0 and so must `got` be, in either sign.  Returns the
    rule's ratio."""
    got, rms = np.asarray(got), np.broadcast_to(rms, ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    zero = rms == 0
    assert not np.any(ref[zero]), f"{what}: the reference of an all-zero symbol is not 0"
    assert np.all(got[zero] == 0), f"{what}: {int(np.count_nonzero(got[zero]))} outputs of all-zero symbols are not 0"
    assert not zero.all(), f"{what}: no symbol carries a value"
    return rule(got[~zero], ref[~zero], rms[~zero], n_fft, what, t=t)


def tx_classes(c):
    """The paths of `ce_ofdmtx_kernel` and its wrapper a case reaches, from the library's host view of the plan and the dict."""
    v = OF.derive_host(c["n_fft"], c["n_prb_grid"], c["cp_len"], c["n_sym"], 0)
    N, cp, rpw = c["n_fft"], c["cp_len"], int(v.rows_per_workgroup)
    out = {f"n_fft {N}", "cp " + c["cp_kind"], "phasor " + c["phasor"], "layout " + c["layout"], f"rows_per_workgroup {rpw}"}
    if 0 in cp:
        out.add("cp_len 0 present")
    if N in cp:
        out.add("cp_len N present")
    if any(t % 2 for t in X.symbol_starts(N, cp)[0]):
        out.add("an odd symbol start")
    if rpw > 1 and c["n_sym"] % rpw:
        out.add(f"a partial last workgroup at {rpw} rows")
    if c["n_sym"] > rpw:
        out.add("more than one workgroup per (slot, port)")
    if c["n_prb_grid"] == 1:
        out.add("n_prb_grid 1")
    if c["n_prb_grid"] == N // 12:
        out |= {"n_prb_grid = n_fft // 12", f"n_prb_grid = n_fft // 12 at n_fft {N}"}
    if c["lead"] % 2:
        out.add("an odd first sample")
    if c["layout"] != "dense" and ((c["B"] > 1 and c["slot_stride"] % 2) or (c["R"] > 1 and c["port_stride"] % 2)):
        out.add("an odd row stride")
    if c["B"] * c["R"] > 1:
        out.add("more than one (slot, port)")
    if c["B"] * c["R"] >= 64:
        out.add("B R >= 64")
    if c["prb_run"] is not None:
        out.add("zero PRBs")
    if c["zero_syms"]:
        out.add("a zero symbol")
    if c["grid_lead"]:
        out.add("grid behind the buffer's start")
    if c["via_dem"]:
        out.add("built through for_demodulator")
        if c["advance"] == min(cp) > 0:
            out.add("advance = min cp > 0")
        elif c["advance"] > 0:
            out.add("0 < advance < min cp")
    return out
