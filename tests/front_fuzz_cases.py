"""Seeded random cases for the three PUSCH kernels the first two fuzzes leave at pinned cases -- transform precoding
(csrc/ce_tp.hip `ce_tp_precode_kernel`), the OFDM demodulator (csrc/ce_ofdm.hip) and the DM-RS generator (csrc/ce_dmrs.hip) --
for tests/test_front_fuzz.py (CPU: what the draws must satisfy by themselves) and tests/test_zzzzzzzzzzzzz_hip_front_fuzz.py
(GPU: the kernels against the oracles on them).

The structure is tests/chain_fuzz_cases.py's: `draw_*(idx)` derives a case from np.random.default_rng([BASE_SEED, stage_id,
idx]) as a plain dict of Python values (stage ids 9 .. 11, so no draw of the first two fuzzes changes); `realize_*(case)`
turns it into arrays, seeded by the dict's own "seed"; `*_classes(case)` names the kernel paths it reaches.  References and
comparison rules are the existing oracles' (tp_oracle.precode with tpre_oracle.check, ofdm_oracle.demodulate_ref with
ofdm_oracle.check, dmrs_oracle.pilots_ref bit for bit): nothing is restated here.  Shapes are the smallest that still reach
every kernel path."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import dmrs_oracle as DM
import ofdm_oracle as OO
import tp_oracle as TP
from chain_fuzz_cases import TP_EDGE_PRBS
from srsran_ce_pytorch_amd import deprecode as DP, ofdm as OF, synth as S
from stage_fuzz_cases import BASE_SEED, _pick, _rng   # noqa: F401  (BASE_SEED: the seed all three fuzzes share)

STAGE_PRE, STAGE_OFDM, STAGE_DMRS = 9, 10, 11
N_PRE_SWEEP, N_PRE_MORE = len(TP.VALID_PRBS), 32
N_PRE, N_OFDM, N_DMRS = N_PRE_SWEEP + N_PRE_MORE, 120, 120
assert N_PRE_SWEEP == 53

# T = 4 C as in tpre_oracle.py / ofdm_oracle.py; C = the float32 numpy restatement's largest error ratio over the realized
# draws (tests/test_front_fuzz.py re-measures both and fails if one exceeds its recorded value); never measured on a kernel
C_PRE_FUZZ = 1.0         # measured 0.987 (tpre_oracle.precode_f32 over the 85 precoder draws), rounded up
T_PRE_FUZZ = 4.0 * C_PRE_FUZZ
C_OFDM_FUZZ = 1.1        # measured 1.021 (ofdm_oracle.demodulate_f32 over the 120 demodulator draws), rounded up
T_OFDM_FUZZ = 4.0 * C_OFDM_FUZZ


# ---------------------------------------------------------------- transform precoding: a sweep plus row geometries ----

PRE_FORMS = ["dense", "dense in place", "rows", "rows in place"]
PRE_SMALL_PRBS = [n for n in TP.VALID_PRBS if 12 * n <= 72]          # M <= 72: the row geometry dominates the transform


def _pre_rows(rng, M, S_):
    """(offsets, stride) of one tensor's rows, in complex elements: the rows laid out one behind the other with gaps of 0, 2
    or an even number of up to 2 M elements in front of each, in shuffled order in three quarters of the cases; the slot
    stride is exactly max offset + M in two fifths of them and larger by an even number of up to 4 M elements otherwise."""
    order = rng.permutation(S_) if rng.random() < 0.75 else np.arange(S_)
    offsets, pos = [0] * S_, 0
    for r in order:
        pos += int(_pick(rng, [0, 2, 2 * int(rng.integers(1, M + 1))], [0.4, 0.3, 0.3]))
        offsets[int(r)] = pos
        pos += M
    return offsets, pos if rng.random() < 0.4 else pos + 2 * int(rng.integers(1, 2 * M + 1))


def draw_pre(idx):
    """Case idx < 53 is allocation size tp_oracle.VALID_PRBS[idx]: every valid size, hence every radix sequence, once; the 32
    behind them take a neighbour of threads_per_row's switches (TP_EDGE_PRBS) or a size with M <= 72.  The seed decides S, B,
    the form and, for "rows", the geometries of x and y independently -- one side dense (NULL offsets) in every third case, x and
    y in turn (by idx, and those cases lean to "rows", so that neither count is left to chance); "rows in place" is y = x with
    one scattered geometry."""
    rng = _rng(STAGE_PRE, idx)
    if idx < N_PRE_SWEEP:
        n_prb = int(TP.VALID_PRBS[idx])
        form = str(_pick(rng, PRE_FORMS, [0.22, 0.24, 0.34, 0.2] if idx % 3 else [0.15, 0.2, 0.5, 0.15]))
    else:
        n_prb = int(_pick(rng, TP_EDGE_PRBS)) if rng.random() < 0.3 else int(_pick(rng, PRE_SMALL_PRBS))
        form = str(_pick(rng, PRE_FORMS, [0.0, 0.0, 0.8, 0.2] if idx % 3 else [0.0, 0.0, 1.0, 0.0]))
    M, S_, B = 12 * n_prb, int(rng.integers(1, 15)), int(rng.integers(1, 6))
    x_off = y_off = None
    x_stride = y_stride = S_ * M
    if form == "rows":
        side = "both" if idx % 3 else "x dense" if idx % 6 else "y dense"
        if side != "x dense":
            x_off, x_stride = _pre_rows(rng, M, S_)
        if side != "y dense":
            y_off, y_stride = _pre_rows(rng, M, S_)
    elif form == "rows in place":
        x_off, x_stride = _pre_rows(rng, M, S_)
        y_off, y_stride = list(x_off), x_stride
    return dict(stage="pre", idx=idx, n_prb=n_prb, S=S_, B=B, form=form, x_off=x_off, x_stride=x_stride, y_off=y_off, y_stride=y_stride,
                slot=int(rng.integers(B)), seed=int(rng.integers(1 << 30)))


def pre_offsets(c, side):
    """The row offsets of tensor `side` ("x" or "y"): the drawn ones, or the dense rows r M that NULL stands for."""
    off = c[side + "_off"]
    return [r * 12 * c["n_prb"] for r in range(c["S"])] if off is None else off


def realize_pre(c):
    """x [B, S M] complex64, row r of slot b = CN(0, 1) times its own scale 10^U(-3, 3) (no all-zero row: the rule's unit
    would be 0), and the float64 reference tp_oracle.precode of it."""
    rng = np.random.default_rng(c["seed"])
    M, S_, B = 12 * c["n_prb"], c["S"], c["B"]
    scale = 10.0 ** rng.uniform(-3.0, 3.0, (B, S_, 1))
    x = ((rng.standard_normal((B, S_, M)) + 1j * rng.standard_normal((B, S_, M))) * np.sqrt(0.5) * scale).astype(np.complex64).reshape(B, S_ * M)
    assert np.all(np.abs(x).reshape(B, S_, M).max(-1) > 0)
    return SimpleNamespace(c=c, M=M, S=S_, B=B, x=x, ref=TP.precode(x, M))


def pre_classes(c):
    """The kernel paths of `ce_tp_precode_kernel` a case reaches, from the library's host view of the shape and the geometry."""
    v = DP.derive_host(c["n_prb"], c["S"])
    M = 12 * c["n_prb"]
    out = {"radix " + "x".join(str(int(r)) for r in v.radix[:v.n_passes]), f"threads_per_row {int(v.threads_per_row)}",
           f"rows_per_workgroup {int(v.rows_per_workgroup)}", "form " + c["form"]}
    if c["n_prb"] in TP_EDGE_PRBS:
        out.add(f"n_prb {c['n_prb']}")
    if c["S"] % int(v.rows_per_workgroup):
        out.add("S % rows_per_workgroup != 0")
    if c["B"] > 1:
        out.add("B > 1")
    if c["form"] == "rows":
        if c["x_off"] is None:
            out.add("x dense, y rows")
        elif c["y_off"] is None:
            out.add("x rows, y dense")
        else:
            out.add("x rows, y rows")
            if c["x_off"] != c["y_off"] or c["x_stride"] != c["y_stride"]:
                out.add("x and y geometries differ")
    for side in "xy":
        off = c[side + "_off"]
        if off is None:
            continue
        if off != sorted(off):
            out.add("offsets not ascending")
        s = sorted(off)
        if s[0] > 0 or any(b - a > M for a, b in zip(s, s[1:])):
            out.add("a gap")
        out.add("stride = extent" if c[side + "_stride"] == s[-1] + M else "stride > extent")
    return out


# ---------------------------------------------------------------- OFDM demodulator ----

OFDM_CP_KINDS = ["normal", "extended", "free"]
OFDM_PHASORS = ["none", "unit", "scaled"]
OFDM_LAYOUTS = ["dense", "odd view", "permuted", "port stride 0", "slot stride 0"]
OFDM_SCS = [15e3, 30e3, 60e3, 120e3]


def draw_ofdm(idx):
    """One demodulator case: the transform length, the grid width (1 PRB, all that fit, or between), 1 .. 14 symbols whose
    cyclic prefixes are NR normal ones at a drawn numerology and slot, NR extended ones (N / 4; at most the 12 symbols of such
    a slot) or free per symbol from {0, 1, N, U(0, N), U(0, 40)}; the window advance from {0, min cp, U(0, min cp)}; the
    phasors; B, R, the memory layout of the samples, `out=`, and whether every sample outside the windows is NaN."""
    rng = _rng(STAGE_OFDM, idx)
    N = int(_pick(rng, list(OF.FFT_SIZES)))
    n_prb = int(_pick(rng, [1, N // 12, int(rng.integers(1, N // 12 + 1))]))
    n_sym = int(rng.integers(1, 15))
    kind = str(_pick(rng, OFDM_CP_KINDS))
    scs, slot = float(_pick(rng, OFDM_SCS)), 0
    if kind == "normal":
        slot = int(rng.integers(0, int(scs / 15e3)))
        cp = [int(v) for v in OO.cp_lengths_ref(scs, N, n_sym, slot)]
    elif kind == "extended":
        n_sym = min(n_sym, 12)
        cp = [N // 4] * n_sym
    else:
        cp = [int(_pick(rng, [0, 1, N, int(rng.integers(0, N + 1)), int(rng.integers(0, 41))])) for _ in range(n_sym)]
    advance = int(_pick(rng, [0, min(cp), int(rng.integers(0, min(cp) + 1))]))
    layout = str(_pick(rng, OFDM_LAYOUTS))
    B, R = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    if layout == "port stride 0":
        R = max(R, 2)
    if layout == "slot stride 0":
        B = max(B, 2)
    return dict(stage="ofdm", idx=idx, n_fft=N, n_prb_grid=n_prb, n_sym=n_sym, cp_kind=kind, scs=scs, cp_slot=slot, cp_len=cp, advance=advance,
                phasor=str(_pick(rng, OFDM_PHASORS)), B=B, R=R, layout=layout, lead=2 * int(rng.integers(0, 50)) + 1, tail=int(rng.integers(0, 100)),
                out=bool(rng.random() < 0.5), nan_outside=bool(rng.random() < 0.25), slot=int(rng.integers(B)), port=int(rng.integers(R)),
                seed=int(rng.integers(1 << 30)))


def ofdm_inside(c):
    """bool [T]: the samples of a slot that lie in one of its windows -- the only ones the kernel may read."""
    w, T = OO.geometry(c["n_fft"], c["cp_len"], c["advance"])
    inside = np.zeros(T, bool)
    for w_l in w:
        inside[w_l:w_l + c["n_fft"]] = True
    return inside


def realize_ofdm(c):
    """samples [B, R, T] complex64: CN(0, 1) times an amplitude 10^U(-3, 3) per (slot, port) -- one row repeated where the
    layout's port or slot stride is 0 -- with NaN on every sample outside the windows where the case says so; the phasors
    (unit modulus at seeded angles, or with a modulus in 0.25 .. 4); the float64 reference and the rule's unit: the rms of
    each window, times |phi_l| where phasors are given (the transform's error passes through that product at the store)."""
    rng = np.random.default_rng(c["seed"])
    N, B, R, n_sym = c["n_fft"], c["B"], c["R"], c["n_sym"]
    _, T = OO.geometry(N, c["cp_len"], c["advance"])
    amp = 10.0 ** rng.uniform(-3.0, 3.0, (B, R, 1))
    s = ((rng.standard_normal((B, R, T)) + 1j * rng.standard_normal((B, R, T))) * np.sqrt(0.5) * amp).astype(np.complex64)
    if c["layout"] == "port stride 0":
        s = np.repeat(s[:, :1], R, 1)
    if c["layout"] == "slot stride 0":
        s = np.repeat(s[:1], B, 0)
    if c["nan_outside"]:
        s[:, :, ~ofdm_inside(c)] = complex(np.nan, np.nan)
    phi = None
    if c["phasor"] != "none":
        phi = np.exp(2j * np.pi * rng.random(n_sym))
        if c["phasor"] == "scaled":
            phi = phi * rng.uniform(0.25, 4.0, n_sym)
        phi = phi.astype(np.complex64)
    d = SimpleNamespace(c=c, T=T, samples=s, phi=phi, n_sc=12 * c["n_prb_grid"])
    d.ref = OO.demodulate_ref(s, N, c["n_prb_grid"], c["cp_len"], c["advance"], phi)
    d.rms = OO.window_rms(s, N, c["cp_len"], c["advance"]) * (1.0 if phi is None else np.abs(phi.astype(np.complex128)))
    return d


def ofdm_classes(c):
    v = OF.derive_host(c["n_fft"], c["n_prb_grid"], c["cp_len"], c["n_sym"], c["advance"])
    N, cp, rpw = c["n_fft"], c["cp_len"], int(v.rows_per_workgroup)
    out = {f"n_fft {N}", "cp " + c["cp_kind"], "phasor " + c["phasor"], "layout " + c["layout"], f"rows_per_workgroup {rpw}"}
    if 0 in cp:
        out.add("cp_len 0 present")
    if N in cp:
        out.add("cp_len N present")
    if c["advance"] == min(cp) > 0:
        out.add("advance = min cp > 0")
    elif c["advance"] > 0:
        out.add("0 < advance < min cp")
    if any(w % 2 for w in OO.geometry(N, cp, c["advance"])[0]):
        out.add("an odd window start")
    if rpw > 1 and c["n_sym"] % rpw:
        out.add(f"a partial last workgroup at {rpw} rows")
    if c["n_prb_grid"] == 1:
        out.add("n_prb_grid 1")
    if c["n_prb_grid"] == N // 12:
        out.add("n_prb_grid = n_fft // 12")
    if c["out"]:
        out.add("out=")
    if c["nan_outside"]:
        out.add("NaN outside the windows")
    if c["B"] * c["R"] > 1:
        out.add("more than one (slot, port)")
    return out


# ---------------------------------------------------------------- DM-RS generator ----

DMRS_MASKS = {1: [0x555, 0xAAA], 2: [0x0C3, 0x30C, 0xC30]}          # the standard masks of include/ce_dmrs.h per configuration type
DMRS_WIDE_GRIDS = [52, 106, 273, 341]
DMRS_CRB_LIMIT = (1 << 20) // 6                                     # 6 (grid_start_crb + n_prb_grid) <= 2^20
DMRS_LIMIT_CASES = {22: 0, 52: 1, 82: 0, 112: 1}                    # idx -> grid_start_crb = the header's limit minus this
DMRS_BIG_BATCH_CASES = [37, 97]                                     # B = 257
DMRS_REFUSALS = ["unequal active PRBs", "overlapping hop symbols", "mixed types", "a non-standard mask", "crb one above the limit", "n_sym > n_symb_slot"]
# the exception class of the header's error code: CE_ERR_UNSUPPORTED is NotImplementedError, CE_ERR_INVALID ValueError
DMRS_REFUSAL_CLASS = {k: (NotImplementedError if k == "crb one above the limit" else ValueError) for k in DMRS_REFUSALS}
DMRS_PARAM_FORMS = ["int", "host array", "device tensor", "stride-2 view", "length-1 tensor"]
DMRS_DEVICE_FORMS = DMRS_PARAM_FORMS[2:]
DMRS_BATCH_FORMS = DMRS_PARAM_FORMS[1:4]
DMRS_MAX_BITS = 1200000   # B n_columns (1600 + sequence bits) of a case: keeps the oracle's bit-serial recurrence under a second
DMRS_HOST_WORDS = 1100    # tests/test_front_fuzz.py runs the oracle on every draw whose kept window ends below this word
DMRS_PARAM_RANGE = {"slot": 159, "n_id": 65535, "n_scid": 1}


def _dmrs_refusal(idx):
    """Every fifteenth case is a descriptor the header refuses (8 of 120), the six kinds in turn."""
    return DMRS_REFUSALS[(idx // 15) % len(DMRS_REFUSALS)] if idx % 15 == 14 else ""


def _dmrs_prbs(rng, grid, n_active):
    """(prb_start, mask_prbs or None): n_active PRBs of the grid, a contiguous run, or scattered in two fifths of the cases
    that leave room."""
    if n_active < grid and rng.random() < 0.4:
        return 0, sorted(int(q) for q in rng.choice(grid, n_active, replace=False))
    return int(rng.integers(0, grid - n_active + 1)), None


def draw_dmrs(idx):
    """One generator case.  Four fixed cases sit at the header's limit of grid_start_crb and right below it (one DM-RS
    symbol, one slot: the oracle steps 2.1 M bits once), two have B = 257 (small grids), every fifteenth is a refused
    descriptor; the others draw the grid from {1 .. 24, 52, 106, 273, 341}, the type, L, an ordered pair of distinct masks of
    the type, one or two hops of equal active PRBs (contiguous or scattered) with 1 .. 4 DM-RS symbols each, disjoint, the
    symbol counts, grid_start_crb from three bands, the form of each parameter, `out=` and its alignment.  In a tenth of
    the cases all three parameters are device tensors holding values outside the host ranges."""
    rng = _rng(STAGE_DMRS, idx)
    refuse = _dmrs_refusal(idx)
    limit, big = idx in DMRS_LIMIT_CASES, idx in DMRS_BIG_BATCH_CASES
    grid = int(rng.integers(1, 25)) if big or rng.random() < 0.45 else int(_pick(rng, DMRS_WIDE_GRIDS, [0.2, 0.2, 0.2, 0.4]))
    if refuse in ("unequal active PRBs",):
        grid = max(grid, 2)
    dtype = int(_pick(rng, [1, 2]))
    L = int(rng.integers(1, 5))
    masks = [int(m) for m in rng.permutation(DMRS_MASKS[dtype])[:2]]
    n_sym, nss = (int(v) for v in _pick(rng, [(14, 14), (12, 14), (12, 12), (int(rng.integers(1, 12)), 14), (int(rng.integers(1, 12)), 12)],
                                         [0.35, 0.15, 0.2, 0.15, 0.15]))
    two = bool(n_sym >= 2 and rng.random() < 0.4)
    if refuse in ("unequal active PRBs", "overlapping hop symbols"):
        n_sym, two = max(n_sym, 2), True
    n_active = int(_pick(rng, [1, grid, int(rng.integers(1, grid + 1))], [0.2, 0.4, 0.4]))
    k1 = int(rng.integers(1, 5))
    k2 = int(rng.integers(1, 5)) if two else 0
    if limit:
        two, k1, k2 = False, 1, 0
    if big:
        k1, k2 = min(k1, 2), min(k2, 1)
    k1 = min(k1, n_sym - (1 if two else 0))
    k2 = min(k2, n_sym - k1)
    perm = [int(s) for s in rng.permutation(n_sym)]
    symbols = [sorted(perm[:k1]), sorted(perm[k1:k1 + k2])][:2 if two else 1]
    hops = []
    for sy in symbols:
        start, scattered = _dmrs_prbs(rng, grid, n_active)
        hops.append(dict(dmrs_symbols=sy, prb_start=start, n_prbs=n_active, mask_prbs=scattered))
    band = str(_pick(rng, ["0", "1..274", "275..2199"], [0.25, 0.35, 0.4]))
    crb = 0 if band == "0" or big else int(rng.integers(1, 275)) if band == "1..274" else int(rng.integers(275, 2200))
    if limit:
        band, crb = "limit", DMRS_CRB_LIMIT - grid - DMRS_LIMIT_CASES[idx]
    # ---- what makes a refused descriptor of it ----
    if refuse == "unequal active PRBs":
        other = n_active - 1 if n_active > 1 else n_active + 1
        hops[1].update(prb_start=int(rng.integers(0, grid - other + 1)), n_prbs=other, mask_prbs=None)
    elif refuse == "overlapping hop symbols":
        hops[1]["dmrs_symbols"] = sorted(set(hops[1]["dmrs_symbols"]) | {hops[0]["dmrs_symbols"][0]})
    elif refuse == "mixed types":
        L, masks = max(L, 3), [int(_pick(rng, DMRS_MASKS[1])), int(_pick(rng, DMRS_MASKS[2]))][::1 if rng.random() < 0.5 else -1]
    elif refuse == "a non-standard mask":
        masks[0] = int(_pick(rng, [0x249, 0x0C0, 0xFFF, 0x000, 0x556]))
    elif refuse == "crb one above the limit":
        band, crb = "above the limit", DMRS_CRB_LIMIT - grid + 1
    elif refuse == "n_sym > n_symb_slot":
        n_sym, nss = 14, 12
    # ---- the per-slot parameters ----
    n_cols = sum(len(h["dmrs_symbols"]) for h in hops)
    B = 257 if big else 1 if limit else max(1, min(int(rng.integers(1, 9)), DMRS_MAX_BITS // (n_cols * (1602 + 12 * (crb + grid)))))
    out_of_range = bool(not limit and not big and rng.random() < 0.1)
    forms = [str(_pick(rng, DMRS_DEVICE_FORMS if out_of_range else DMRS_PARAM_FORMS)) for _ in range(3)]
    if B > 1 and not any(f in DMRS_BATCH_FORMS for f in forms):
        forms[int(rng.integers(3))] = str(_pick(rng, DMRS_BATCH_FORMS[1:] if out_of_range else DMRS_BATCH_FORMS))
    if not any(f in DMRS_BATCH_FORMS for f in forms):
        B = 1
    params = {}
    for name, form in zip(("slot", "n_id", "n_scid"), forms):
        n, hi = (B if form in DMRS_BATCH_FORMS else 1), DMRS_PARAM_RANGE[name]
        v = rng.integers(0, hi + 1, n)
        edge = rng.random(n)
        v = np.where(edge < 0.1, 0, np.where(edge < 0.2, hi, v))
        if out_of_range:                                  # int32 values the host forms would refuse
            lo = -(1 << 31) if name == "slot" else hi + 1
            wild = np.where(rng.random(n) < 0.2, [(1 << 31) - 1, lo][int(rng.integers(2))], rng.integers(lo, 1 << 31, n))
            v = np.where(rng.random(n) < 0.7, wild, v)
            v[int(rng.integers(n))] = wild[0]
        params[name] = dict(form=form, values=[int(x) for x in v])
    return dict(stage="dmrs", idx=idx, n_prb_grid=grid, type=dtype, L=L, masks=masks, hops=hops, n_sym=n_sym, n_symb_slot=nss, grid_start_crb=crb,
                crb_band=band, B=B, params=params, out_of_range=out_of_range, refuse=refuse, out=bool(rng.random() < 0.5),
                out_off8=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def dmrs_case_spec(c):
    re_masks = [[(m >> r) & 1 for r in range(12)] for m in c["masks"]]
    hops = [S.hop_spec(h["dmrs_symbols"], h["prb_start"], h["n_prbs"], 0, c["n_sym"], re_masks=re_masks, mask_prbs=h["mask_prbs"]) for h in c["hops"]]
    return S.case_spec("front_fuzz", c["n_prb_grid"], hops, n_layers=c["L"], n_sym=c["n_sym"], seed=c["seed"])


def dmrs_view(c):
    """The library's host view of a case's descriptor; raises what the library refuses it with."""
    from srsran_ce_pytorch_amd import dmrs
    h1, h2, _ = S.numpy_hops(dmrs_case_spec(c))
    return dmrs.derive_host(h1, h2, c["L"], c["n_prb_grid"], c["n_sym"], grid_start_crb=c["grid_start_crb"], n_symb_slot=c["n_symb_slot"])


def dmrs_slot_params(c):
    """[(slot, n_id, n_scid)] of the B slots: a parameter of one value holds for the whole batch."""
    cols = [c["params"][n]["values"] for n in ("slot", "n_id", "n_scid")]
    return [tuple(v[b] if len(v) > 1 else v[0] for v in cols) for b in range(c["B"])]


def dmrs_span(c):
    """(first, last) kept word of the sequence over the hops, from the allocation alone: pilot m sits on bits 2 m, 2 m + 1."""
    ppp = 6 if c["type"] == 1 else 4
    lo, hi = [], []
    for h in c["hops"]:
        prbs = h["mask_prbs"] if h["mask_prbs"] is not None else [h["prb_start"], h["prb_start"] + h["n_prbs"] - 1]
        lo.append(2 * ppp * (c["grid_start_crb"] + min(prbs)) // 32)
        hi.append((2 * (ppp * (c["grid_start_crb"] + max(prbs)) + ppp - 1) + 1) // 32)
    return lo, hi


def realize_dmrs(c):
    """ref [B, n_re, n_dmrs_total, L] complex64: dmrs_oracle.pilots_ref per slot with the slot's own integers -- out-of-range
    ones included: dmrs_oracle.c_init reduces them mod 2^31 as the header's unsigned arithmetic does.  A (slot, n_id, n_scid)
    that repeats in the batch is computed once."""
    assert not c["refuse"], c
    case = dmrs_case_spec(c)
    seen = {}
    for p in dmrs_slot_params(c):
        if p not in seen:
            seen[p] = DM.pilots_ref(case, *p, c["n_symb_slot"], c["grid_start_crb"])
    return SimpleNamespace(c=c, case=case, slots=dmrs_slot_params(c), ref=np.stack([seen[p] for p in dmrs_slot_params(c)]))


def dmrs_classes(c):
    if c["refuse"]:
        return {"refused", "refused: " + c["refuse"]}
    lo, hi = dmrs_span(c)
    n_cols = sum(len(h["dmrs_symbols"]) for h in c["hops"])
    ppp = 6 if c["type"] == 1 else 4
    n_elem = ppp * c["hops"][0]["n_prbs"] * n_cols * c["L"]
    out = {f"type {c['type']}, L {c['L']}", "masks 0x%03X 0x%03X" % tuple(c["masks"]), "crb " + c["crb_band"],
           "n_symb_slot %d" % c["n_symb_slot"], "grid " + (str(c["n_prb_grid"]) if c["n_prb_grid"] in DMRS_WIDE_GRIDS else "<= 24")}
    out |= {f"{name} as {p['form']}" for name, p in c["params"].items()}
    out.add("two hops" if len(c["hops"]) == 2 else "one hop")
    if any(h["mask_prbs"] is not None for h in c["hops"]):
        out.add("scattered")
    if c["grid_start_crb"] % 2:
        out.add("crb odd")
    if max(b - a + 1 for a, b in zip(lo, hi)) >= 128:
        out.add("n_words >= 128")
    if c["n_sym"] < c["n_symb_slot"]:
        out.add("n_sym < n_symb_slot")
    if c["out_of_range"]:
        out.add("out-of-range device values")
    if c["B"] > 1:
        out.add("B > 1")
    if c["B"] == 257:
        out.add("B = 257")
    out.add("store 16 bytes" if n_elem % 2 == 0 and not (c["out"] and c["out_off8"]) else "store 8 bytes")
    if c["out"]:
        out.add("out= 8 bytes off" if c["out_off8"] else "out= aligned")
    return out
