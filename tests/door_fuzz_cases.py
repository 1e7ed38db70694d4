"""Seeded random cases for the four front-door stages the earlier fuzzes leave at their pinned cases -- the channel emulator
(csrc/ce_chan.hip `ce_chan_kernel`), the fronthaul codec (csrc/ce_fh.hip `ce_fh_decompress_kernel`, `ce_fh_compress_kernel`), the
PRACH detector (csrc/ce_prach.hip `ce_prach_kernel`) and the SRS estimator (csrc/ce_srs.hip `ce_srs_profile_kernel`,
`ce_srs_estimate_kernel`) -- for tests/test_door_fuzz.py (CPU: what the draws must satisfy by themselves) and
tests/test_zzzzzzzzzzzzzzzzzzzzz_hip_door_fuzz.py (GPU: the kernels against the oracles on them).

The structure is tests/tx_fuzz_cases.py's: `draw_*(idx)` derives a case from np.random.default_rng([BASE_SEED, STAGE, idx]) as a
plain dict of Python values (stage ids 13 .. 16, behind the earlier fuzzes' 1 .. 12, so none of their draws changes);
`realize_*(case)` turns it into arrays, seeded by the dict's own "seed"; `*_classes(case)` names the kernel paths it reaches, from
the library's host view and the dict alone.  The references are chan_oracle.apply_ref, fh_oracle.compress / decompress,
prach_oracle.detect_ref and srs_oracle.profile_full / window / delay_of / estimate_ref, the rules the oracles' own: none is restated
here.  `prach_check` and `srs_check` call those rules with the fuzz tolerances (srs_oracle.check and the two `gaps` functions read
their module's pinned tolerance, so their delay clauses are spelled out here with `t` as an argument); where a rule's unit is 0 --
an all-zero occasion or item -- the oracles' `_ratio` accepts an exact 0 only."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import chan_oracle as CO
import fh_oracle as FO
import prach_oracle as PO
import srs_oracle as SO
from stage_fuzz_cases import BASE_SEED, _pick, _rng   # noqa: F401  (BASE_SEED: the seed every fuzz shares)

STAGE_CHAN, STAGE_FH, STAGE_PRACH, STAGE_SRS = 13, 14, 15, 16
N_CHAN, N_FH, N_PRACH, N_SRS = 120, 136, 120, 120

# T = 4 C as in the four oracles; C = the float32 numpy restatements' largest error ratio against the float64 oracle over the
# realized draws (tests/test_door_fuzz.py re-measures every one and fails if it exceeds its recorded value); never measured on a
# kernel.  The fronthaul codec has no tolerance: it is defined to the bit.
C_CHAN_FUZZ = 3.3            # measured 3.250 (chan_oracle.apply_f32 over the 120 draws), rounded up
C_PRACH_FUZZ = 6.1           # measured 6.083 (prach_oracle.detect_f32 over the 120 draws), rounded up
# measured 3.111, 0.168, 0.146, 1.224, 0.315 (srs_oracle.profile_f32 / estimate_f32), rounded up
C_SRS_FUZZ = {"profile": 3.2, "h_sb": 0.2, "h_wb": 0.2, "noise": 1.3, "epre": 0.4}
T_CHAN_FUZZ = 4.0 * C_CHAN_FUZZ
T_PRACH_FUZZ = 4.0 * C_PRACH_FUZZ
T_SRS_FUZZ = {k: 4.0 * v for k, v in C_SRS_FUZZ.items()}

NAN = np.complex64(complex(np.nan, np.nan))


# ---------------------------------------------------------------- rows in a flat buffer ----

def extent(n, strides, row):
    """Elements from the first element of row (0, .., 0) to behind the last element of the last row."""
    return sum((k - 1) * s for k, s in zip(n, strides)) + row


def place(buf, rows, lead, strides):
    """rows [n.., row] into the flat `buf` at lead + sum idx strides, in ascending index order (with a stride of 0 the last wins)."""
    for idx in np.ndindex(*rows.shape[:-1]):
        o = lead + sum(i * s for i, s in zip(idx, strides))
        buf[o:o + rows.shape[-1]] = rows[idx]


def gather(buf, n, row, lead, strides):
    """The rows [n.., row] a strided view of `buf` holds: what the kernel reads."""
    out = np.empty(tuple(n) + (row,), buf.dtype)
    for idx in np.ndindex(*n):
        o = lead + sum(i * s for i, s in zip(idx, strides))
        out[idx] = buf[o:o + row]
    return out


def rows_mask(total, n, row, lead, strides, what):
    """bool [total]: the elements of the rows; asserts the header's rule for a written side: no two rows share an element."""
    m = np.zeros(total, bool)
    for idx in np.ndindex(*n):
        o = lead + sum(i * s for i, s in zip(idx, strides))
        assert o + row <= total and not m[o:o + row].any(), (what, idx)
        m[o:o + row] = True
    return m


def _nested(rng, n, row, order, parity=None, q=1):
    """Strides of rows of `row` units nested as `order` (dimension indices, innermost first) with a drawn gap behind every row
    and group: multiples of q; `parity` (one bit per dimension, q = 1 only) fixes each stride's parity."""
    s, ext = [0] * len(n), row
    for d in order:
        st = -(-(ext + int(_pick(rng, [0, 1, int(rng.integers(2, 40))]))) // q) * q
        if parity is not None:
            st += (st ^ parity[d]) & 1
        s[d] = st
        ext += (n[d] - 1) * st
    return s


# ================================================================ channel emulator ====

CHAN_X_LAYOUTS = ["dense", "longer rows", "ports in slots", "slots in ports"]
CHAN_Y_LAYOUTS = ["dense", "ports in slots", "slots in ports"]
CHAN_MAX_WORK = 1 << 23          # B R P K T of a case: the float32 restatement stays near a second
CHAN_FCW = [0, 1, -1, 2 ** 31 - 1, -2 ** 31]


def _two_level(rng, kind, n_out, n_in, T):
    """(row_len, outer stride, inner stride) of [n_out, n_in] rows of T for "dense", "longer rows", "<inner> in <outer>" nestings."""
    gap = lambda: int(_pick(rng, [0, 1, int(rng.integers(2, 100))]))   # noqa: E731
    if kind == "dense":
        return T, n_in * T, T
    if kind == "longer rows":
        L = T + int(rng.integers(1, 41))
        return L, n_in * L, L
    inner = T + gap()
    return T, (n_in - 1) * inner + T + gap(), inner


def draw_chan(idx):
    """One emulator case.  Everything in it is defined by include/ce_tp.h `ce_chan_apply`: 1 .. 4 tx ports, 1 .. 128 taps, x rows
    at free strides >= 0 on 8 bytes, dense taps per slot or shared, int32 fcw / uint32 phase0 / float32 sigma >= 0 per slot or
    one for the batch, any 64-bit seed and int64 first_slot, y rows pairwise disjoint in one of the two nestings.

    P in 1 .. 4; K from {1, 2, 3, 4, 5, U(6, 126), 127, 128}; T from {1, 2, 3, 1022 .. 1026, 2047 .. 2050, U(1, 4500), an odd one in
    5 .. 1023, U(3073, 4500)}; R in
    1 .. 4 and B in 1 .. 3, lowered until B R P K T <= CHAN_MAX_WORK; the taps shared or per slot, with a zero
    row (three of ten), for one (r, p) or for every p of an r -- then the FIR sum of that output row is exactly 0, and the draw always
    has noise, so that the GPU test checks the noise by itself there; CFO and sigma absent, a scalar
    or a tensor, the words from CHAN_FCW or random, a sigma tensor holding one exact 0; the Philox seed with both halves
    non-zero; first_slot 0, negative or above 2^32; an amplitude 10^U(-3, 3) per slot; the layouts of x (always inside a NaN
    buffer) and of y with their leads, strides and tails in elements; the slot of the single-item comparison."""
    rng = _rng(STAGE_CHAN, idx)
    P = int(_pick(rng, [1, 2, 3, 4]))
    K = int(_pick(rng, [1, 2, 3, 4, 5, int(rng.integers(6, 127)), 127, 128]))
    T = int(_pick(rng, [1, 2, 3, int(rng.integers(1022, 1027)), int(rng.integers(2047, 2051)), int(rng.integers(1, 4501)), 2 * int(rng.integers(2, 512)) + 1,
                        int(rng.integers(3073, 4501))]))
    R, B = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    while B * R * P * K * T > CHAN_MAX_WORK:
        B, R = (B, R - 1) if R >= B else (B - 1, R)
    shared = bool(rng.random() < 0.5)
    zero_tap = None
    if rng.random() < 0.3 and max(R, P) > 1:               # (R = P = 1: the one row would be all zero, and the case test nothing)
        zero_tap = [int(rng.integers(R)), int(_pick(rng, [-1, -1, int(rng.integers(P))]))]     # p = -1: every tx port of that r
        if R == 1 and zero_tap[1] < 0:
            zero_tap[1] = int(rng.integers(P))                                                  # one receive port: keep a tx port, so that an output's unit is not 0
    word = lambda: int(_pick(rng, CHAN_FCW + [int(rng.integers(-2 ** 31, 2 ** 31))]))     # noqa: E731
    cfo = str(_pick(rng, ["none", "scalar", "tensor"]))
    fcw = phase0 = None
    if cfo == "scalar":
        fcw, phase0 = word(), int(rng.integers(0, 1 << 32))
    elif cfo == "tensor":
        fcw, phase0 = [word() for _ in range(B)], [int(rng.integers(0, 1 << 32)) for _ in range(B)]
    all_ports = zero_tap is not None and (zero_tap[1] < 0 or P == 1)                       # an output row whose FIR sum is exactly 0: its noise is checked by itself
    noise = str(_pick(rng, ["scalar", "tensor", "tensor"] if all_ports else ["none", "scalar", "tensor"]))
    sg = lambda: float(np.float32(10.0 ** rng.uniform(-3.0, 3.0)))                        # noqa: E731
    sigma = None
    if noise == "scalar":
        sigma = sg()
    elif noise == "tensor":
        sigma = [sg() for _ in range(B)]
        sigma[int(rng.integers(B))] = 0.0
    x_layout, y_layout = str(_pick(rng, CHAN_X_LAYOUTS)), str(_pick(rng, CHAN_Y_LAYOUTS))
    x_row, x_ss, x_ps = _two_level(rng, x_layout, B, P, T)
    if x_layout == "slots in ports":                       # one stream per port: slot b right behind slot b - 1, or a gap behind
        x_ss = T + int(_pick(rng, [0, 0, int(rng.integers(1, 100))]))
        x_ps = B * x_ss + int(rng.integers(0, 100))
    y_row, y_ss, y_ps = _two_level(rng, y_layout, B, R, T)
    if y_layout == "slots in ports":
        y_ss = T + int(_pick(rng, [0, 0, int(rng.integers(1, 100))]))
        y_ps = B * y_ss + int(rng.integers(0, 100))
    return dict(stage="chan", idx=idx, P=P, K=K, T=T, R=R, B=B, shared=shared, zero_tap=zero_tap, cfo=cfo, fcw=fcw, phase0=phase0, noise=noise, sigma=sigma,
                noise_seed=(int(rng.integers(1, 1 << 32)) << 32) | int(rng.integers(1, 1 << 32)),
                first_slot=int(_pick(rng, [0, -int(rng.integers(1, 1 << 40)), (1 << 32) + int(rng.integers(0, 1 << 40))])),
                amp=[float(10.0 ** rng.uniform(-3.0, 3.0)) for _ in range(B)],
                x_layout=x_layout, x_lead=2 * int(rng.integers(0, 70)) + int(rng.integers(2)), x_row=x_row, x_ss=x_ss, x_ps=x_ps, x_tail=int(rng.integers(0, 140)),
                y_layout=y_layout, y_lead=2 * int(rng.integers(0, 50)) + int(rng.integers(2)), y_row=y_row, y_ss=y_ss, y_ps=y_ps, y_tail=int(rng.integers(0, 100)),
                slot=int(rng.integers(B)), seed=int(rng.integers(1 << 30)))


def chan_x_total(c):
    return c["x_lead"] + extent((c["B"], c["P"]), (c["x_ss"], c["x_ps"]), c["T"]) + c["x_tail"]


def chan_y_total(c):
    return c["y_lead"] + extent((c["B"], c["R"]), (c["y_ss"], c["y_ps"]), c["T"]) + c["y_tail"]


def chan_rows(c):
    """bool [lead + extent + tail]: the elements of the stream the emulator writes -- the T samples of each (slot, port) row."""
    return rows_mask(chan_y_total(c), (c["B"], c["R"]), c["T"], c["y_lead"], (c["y_ss"], c["y_ps"]), c)


def realize_chan(c):
    """x complex64 [B, P, T]: CN(0, 2) times the slot's amplitude; h complex64 [B or 1, R, P, K] of unit energy per (r, p) with the
    dict's zero rows; fcw / phase0 / sigma as chan_oracle.inputs holds them (None, a scalar, or int32 / uint32 / float32 [B]);
    ref, A and n of chan_oracle.apply_ref.  `c` itself is the `c` of chan_oracle.ratio (it reads P and K)."""
    rng = np.random.default_rng(c["seed"])
    B, P, R, K, T = c["B"], c["P"], c["R"], c["K"], c["T"]
    amp = np.asarray(c["amp"])[:, None, None]
    x = ((rng.standard_normal((B, P, T)) + 1j * rng.standard_normal((B, P, T))) * amp).astype(np.complex64)
    hs = (1 if c["shared"] else B, R, P, K)
    h = ((rng.standard_normal(hs) + 1j * rng.standard_normal(hs)) / np.sqrt(2.0 * K)).astype(np.complex64)
    if c["zero_tap"] is not None:
        r, p = c["zero_tap"]
        h[:, r, slice(None) if p < 0 else p] = 0
    fcw = phase0 = sigma = None
    if c["cfo"] == "scalar":
        fcw, phase0 = c["fcw"], c["phase0"]
    elif c["cfo"] == "tensor":
        fcw, phase0 = np.array(c["fcw"], np.int32), np.array(c["phase0"], np.uint32)
    if c["noise"] == "scalar":
        sigma = c["sigma"]
    elif c["noise"] == "tensor":
        sigma = np.array(c["sigma"], np.float32)
    ref, A, n = CO.apply_ref(x, h, fcw, phase0, sigma, c["noise_seed"], c["first_slot"])
    return SimpleNamespace(c=c, x=x, h=h, fcw=fcw, phase0=phase0, sigma=sigma, seed=c["noise_seed"], first_slot=c["first_slot"], ref=ref, A=A, n=n)


def chan_zero_rows(c):
    """bool [B, R]: the output rows whose every product has a zero factor (every tap of the row is 0)."""
    z = np.zeros((c["B"], c["R"]), bool)
    if c["zero_tap"] is not None and (c["zero_tap"][1] < 0 or c["P"] == 1):
        z[:, c["zero_tap"][0]] = True
    return z


def chan_classes(c):
    """The paths of `ce_chan_kernel` and its host entry a case reaches, from the dict alone."""
    P, K, T, B = c["P"], c["K"], c["T"], c["B"]
    out = {f"n_tx {P}", "K " + (str(K) if K <= 5 or K >= 127 else ("6..126 odd" if K % 2 else "6..126 even")), f"halo {K & ~1}" if K <= 5 else "halo 6..126",
           "taps " + ("shared" if c["shared"] else "per slot"), "cfo " + c["cfo"], "sigma " + c["noise"], "x " + c["x_layout"], "y " + c["y_layout"],
           "first_slot " + ("0" if c["first_slot"] == 0 else "negative" if c["first_slot"] < 0 else "above 2^32"), f"tiles {min(-(-T // 1024), 4)}{'+' if T > 3072 else ''}"}
    if 3 < K < 127 and K != 12:
        out.add("K never pinned (4..11, 13..126)")
    if K > T:
        out.add("K > T")
    if T <= 3:
        out.add(f"T {T}")
    if T % 1024 == 0:
        out.add("T a multiple of the tile")
    if T > 1024 and T % 2 == 0 and 0 < T % 1024 <= 2:
        out.add("an even T just behind a tile edge")
    if 3 < T < 1024 and T % 2:
        out.add("an odd T in the first tile")
    if T % 2:
        out.add("an odd T")
    if c["zero_tap"] is not None:
        out.add("a zero tap row" + (" for every tx port" if chan_zero_rows(c).any() else ""))
    sig = [] if c["sigma"] is None else (c["sigma"] if isinstance(c["sigma"], list) else [c["sigma"]] * B)
    if chan_zero_rows(c).any() and any(v > 0 for v in sig):
        out.add("noise checked by itself")
        if isinstance(c["sigma"], list) and B > 1:
            out.add("noise checked by itself under a sigma tensor")
        if T > 1024:
            out.add("noise checked by itself over more than one tile")
    words = [] if c["fcw"] is None else (c["fcw"] if isinstance(c["fcw"], list) else [c["fcw"]])
    for w, name in ((0, "fcw 0"), (-2 ** 31, "fcw -2^31"), (2 ** 31 - 1, "fcw 2^31 - 1"), (1, "fcw 1"), (-1, "fcw -1")):
        if w in words:
            out.add(name)
    if isinstance(c["sigma"], list) and any(s > 0 for s in c["sigma"]):
        out.add("sigma 0 beside non-zero values")
    if min(c["amp"]) < 0.1 or max(c["amp"]) > 10.0:
        out.add("an amplitude beyond a decade from 1")
    if c["x_lead"] % 2:
        out.add("x at an odd element")
    if c["y_layout"] != "dense" and c["y_lead"] % 2:
        out.add("y at an odd element")
    if c["x_layout"] in ("ports in slots", "slots in ports") and c["x_lead"] % 2 and c["cfo"] != "none" and c["noise"] != "none":
        out.add("x strided at an odd element with CFO and noise")
    if B > 1:
        out.add("more than one slot")
    return out


# ================================================================ fronthaul codec ====

FH_N_PRB = [1, 2, 3, 63, 64, 65, 127, 128, 129, 273, 341]
FH_BIG_CASES = [16, 33, 50, 67]          # n_prb = 341 (six tiles of 64 PRBs), one row or two: W = 17 -> "none", W = 1, 2, 3
FH_MAX_PRB_ROWS = 1400                   # B R S n_prb of a case: the bit-serial oracle's five passes stay under about a second
FH_NESTINGS = {"port inside slot": (2, 1, 0), "slot inside port": (2, 0, 1), "symbol outside": (0, 1, 2)}      # dimensions (slot, port, symbol), innermost first
FH_PARITIES = ["all even", "all odd", "exactly one odd", "odd only on a dimension of one entry"]
FH_SCALES = ["2^-96", "2^96", "2^-11", "free"]
FH_EDGES = ["zero", "2^(L-1) - 1", "2^(L-1)", "-2^(L-1)"]


def _fh_parity(rng, kind, n):
    """One bit per dimension (slot, port, symbol) for `kind`; a kind the shape cannot hold falls back to the nearest it can."""
    many, one = [d for d in range(3) if n[d] > 1], [d for d in range(3) if n[d] == 1]
    if kind == "odd only on a dimension of one entry" and one:
        p = [0, 0, 0]
        p[int(_pick(rng, one))] = 1
        return p, kind
    if kind == "exactly one odd" and many:
        p = [0, 0, 0]
        p[int(_pick(rng, many))] = 1
        return p, kind
    if kind == "all odd":
        return [1, 1, 1], kind
    return [0, 0, 0], "all even"


def draw_fh(idx):
    """One codec case, run through both kernels.  Everything in it is defined by include/ce_tp.h `ce_fh_decompress` /
    `ce_fh_compress`: W in 1 .. 16 or "none", 1 .. 341 PRBs, a float32 scale in 2^-96 .. 2^96, a payload whose base and strides are
    multiples of 4 bytes, a grid on 8 bytes with strides of any parity, the written side's rows pairwise disjoint in any nesting,
    the read side's strides free (0 repeats a row).

    The format cycles with the index (W = 1 + idx mod 17, 17 standing for "none"), so every width is drawn equally often; n_prb
    from FH_N_PRB or U(1, 341), 341 in FH_BIG_CASES; S in 1 .. 3, R and B in 1 .. 2, lowered until B R S n_prb <= FH_MAX_PRB_ROWS; the
    scale; in a third of the cases a section of a wider grid; per side (grid written, grid read, payload written, payload read) a
    nesting, the parity of base and strides (grid; kind and base cycle with idx // 17, the width's k-th draw, so that every width meets
    the 16-byte and the 8-byte instantiation of both kernels) or the padding behind row_bytes (payload), and for the sides that are read which
    dimensions repeat a row; the PRB of every row that carries each of FH_EDGES; the row of the single-item comparison."""
    rng = _rng(STAGE_FH, idx)
    W = 1 + idx % 17
    method, W = ("none", 16) if W == 17 else ("bfp", W)
    n_prb = 341 if idx in FH_BIG_CASES else int(_pick(rng, FH_N_PRB[:-1] + [int(rng.integers(1, 342))]))
    n = [int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 4))]
    while n[0] * n[1] * n[2] * n_prb > FH_MAX_PRB_ROWS and max(n) > 1:
        n[int(np.argmax(n))] -= 1
    scale_kind = str(_pick(rng, FH_SCALES))
    scale = {"2^-96": 2.0 ** -96, "2^96": 2.0 ** 96, "2^-11": 2.0 ** -11}.get(scale_kind) or float(np.float32(10.0 ** rng.uniform(-6.0, 6.0)))
    start_prb, n_prb_grid = 0, n_prb
    if n_prb < 341 and rng.random() < 0.34:
        n_prb_grid = n_prb + int(rng.integers(1, min(341 - n_prb, 8) + 1))
        start_prb = int(rng.integers(0, n_prb_grid - n_prb + 1))
    n_sc, nb = 12 * n_prb_grid, FO.row_bytes(method, W, n_prb)
    out = dict(stage="fh", idx=idx, method=method, W=W, n_prb=n_prb, B=n[0], R=n[1], S=n[2], scale_kind=scale_kind, scale=scale, start_prb=start_prb, n_prb_grid=n_prb_grid)
    turn = idx // 17                                   # the width's k-th draw: parity kind and base cycle with it, so that every width meets both instantiations of both kernels
    for side, k in (("gw", turn), ("gr", turn + 2)):   # the grid as the decompressor writes it, as the compressor reads it: complex64 elements
        nesting = str(_pick(rng, list(FH_NESTINGS)))
        parity, kind = _fh_parity(rng, FH_PARITIES[k % 4], n)
        st = _nested(rng, n, n_sc, FH_NESTINGS[nesting], parity)
        out.update({side + "_nesting": nesting, side + "_parity": kind, side + "_lead": 2 * int(rng.integers(0, 20)) + (k // 4) % 2, side + "_strides": st,
                    side + "_tail": int(rng.integers(0, 30))})
    for side in ("pw", "pr"):                          # the payload as the compressor writes it, as the decompressor reads it: bytes
        nesting = str(_pick(rng, list(FH_NESTINGS)))
        st = _nested(rng, n, nb + int(_pick(rng, [0, 1, 3, int(rng.integers(0, 9))])), FH_NESTINGS[nesting], q=4)
        out.update({side + "_nesting": nesting, side + "_lead": 4 * int(rng.integers(0, 10)), side + "_strides": st, side + "_tail": int(rng.integers(0, 30))})
    for side in ("gr", "pr"):                          # a read side may repeat a row: stride 0 on drawn dimensions (parity even)
        rep = [d for d in range(3) if n[d] > 1 and rng.random() < 0.2]
        for d in rep:
            out[side + "_strides"][d] = 0
        out[side + "_repeat"] = rep
    out.update(edge_prb=[int(rng.integers(n_prb)) for _ in FH_EDGES], row=[int(rng.integers(k)) for k in n], seed=int(rng.integers(1 << 30)))
    return out


def fh_wide(c, side):
    """Whether the host picks the 16-byte instantiation for the grid of `side` ("gw": decompressor, "gr": compressor), by the
    header's rule: the first RE on 16 bytes (the buffers start on 16 bytes; a PRB is 96 bytes) and every stride of a dimension
    with more than one entry even."""
    n = (c["B"], c["R"], c["S"])
    return c[side + "_lead"] % 2 == 0 and all(k == 1 or s % 2 == 0 for k, s in zip(n, c[side + "_strides"]))


def fh_edge_values(c):
    """Per FH_EDGES the quantised values v (in steps) a PRB gets so that the largest magnitude of v >= 0 ? v : ~v sits on the edge
    of bit_length: all zero; a peak of 2^(L-1) - 1, 2^(L-1), -2^(L-1), L drawn from the widths that change the exponent."""
    L = 1 + (c["seed"] + c["W"]) % 15                                      # 1 .. 15: 2^(L-1) .. 2^14 fit int16
    return L, [0, (1 << (L - 1)) - 1, 1 << (L - 1), -(1 << (L - 1))]


def realize_fh(c):
    """`grid` complex64 [B, R, S, 12 n_prb] as fh_oracle.make_grid draws it, with the edge PRBs of every row overwritten (exact
    multiples of the scale: v * scale is exact for |v| < 2^15, and v * scale * inv_scale rounds back to v); `payload` uint8
    [B, R, S, row_bytes] of random bytes (every exponent, random reserved nibbles).  Rows a read side repeats are made equal first,
    so what the oracle sees is what the strided view holds.  packed / unpacked / restored / repacked as fh_oracle.inputs."""
    rng = np.random.default_rng(c["seed"])
    n, n_prb = (c["B"], c["R"], c["S"]), c["n_prb"]
    s32 = np.float32(c["scale"])
    grid = FO.make_grid(rng, n + (12 * n_prb,), c["scale"]).copy()
    L, edges = fh_edge_values(c)
    for idx in np.ndindex(*n):
        for p, v in zip(c["edge_prb"], edges):
            sign = -1.0 if v < 0 else 1.0
            prb = (rng.integers(0, max(abs(v), 1), 24) * sign).astype(np.float32)            # below the peak in magnitude, on its side
            prb[int(rng.integers(24))] = np.float32(v)
            grid[idx][12 * p:12 * p + 12] = (prb * s32).view(np.complex64) if v else 0
    nb = FO.row_bytes(c["method"], c["W"], n_prb)
    payload = rng.integers(0, 256, n + (nb,), dtype=np.uint8)
    for rep, a in ((c["gr_repeat"], grid), (c["pr_repeat"], payload)):
        for d in rep:
            a[:] = np.take(a, [a.shape[d] - 1], axis=d)                                     # the last index wins, as `place` does
    d = SimpleNamespace(c=c, grid=grid, payload=payload, row_bytes=nb, L=L, packed=FO.compress(grid, c["scale"], c["method"], c["W"]),
                        unpacked=FO.decompress(payload, n_prb, c["scale"], c["method"], c["W"]))
    d.restored = FO.decompress(d.packed, n_prb, c["scale"], c["method"], c["W"])
    d.repacked = FO.compress(d.restored, c["scale"], c["method"], c["W"])
    return d


def fh_classes(c):
    """The paths of the two kernels and their host entries a case reaches, from the dict alone."""
    n, n_prb = (c["B"], c["R"], c["S"]), c["n_prb"]
    pb = FO.prb_bytes(c["method"], c["W"])
    out = {f"W {c['W']}" if c["method"] == "bfp" else "method none", f"prb_bytes {pb}", "scale " + c["scale_kind"],
           "decompressor: " + ("16-byte" if fh_wide(c, "gw") else "8-byte") + " accesses", "compressor: " + ("16-byte" if fh_wide(c, "gr") else "8-byte") + " accesses",
           "grid written: " + c["gw_nesting"], "grid written: " + c["gw_parity"], "grid read: " + c["gr_parity"], "payload written: " + c["pw_nesting"],
           f"row_bytes mod 4 = {n_prb * pb % 4}", "tiles of 64 PRBs: " + (str(-(-n_prb // 64)) if n_prb <= 192 else "4 or more")}
    if n_prb in FH_N_PRB:
        out.add(f"n_prb {n_prb}")
    if c["n_prb_grid"] > n_prb:
        out.add("a section of a wider grid")
    if c["gw_lead"] % 2:
        out.add("grid written at an odd element")
    if c["gr_repeat"]:
        out.add("grid read with a repeated row (stride 0)")
    if c["pr_repeat"]:
        out.add("payload read with a repeated row (stride 0)")
    if any(st > n_prb * pb for k, st in zip(n, c["pw_strides"]) if k > 1):
        out.add("payload written with bytes behind row_bytes")
    if n[0] * n[1] * n[2] > 1:
        out.add("more than one row")
    return out


# ================================================================ PRACH detector ====

PRACH_PAIRS = [(L, N) for L in PO.L_RA for N in PO.FFT_SIZES if N > L]
PRACH_64_ROOT_CASES = [7, 47, 87]        # n_roots = 64, the limit
PRACH_64_PORT_CASES = [23, 63, 103]      # R = 64, the limit
PRACH_MAX_POINTS = 1 << 22               # B n_roots terms N of a case: the float64 reference stays under about two seconds
PRACH_TYPICAL_NCS = {139: [2, 4, 6, 8, 10, 12, 13, 15, 17, 19, 23, 27, 34, 46, 69], 839: [13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419],
                     571: [8, 10, 12, 15, 17, 21, 25, 30, 35, 44, 52, 63, 82, 104, 127], 1151: [17, 21, 25, 30, 35, 44, 52, 63, 82, 104, 127, 164, 230, 383, 575]}
# The delay rule's condition needs a peak that stands clear of its neighbour on the N grid.  A preamble 0.2 samples off the grid
# leads its neighbour by 0.6 x 3.3 (L / N)^2 of the peak (the main lobe's curvature); a second root in the occasion adds a ripple of
# 2 / sqrt(L) of the peak (the roots' cross-correlation), noise of power s one of 2 sqrt(s / L).  So where N >= 2 L the preambles
# of an occasion share one root (its other windows; the occasions still differ), and the noise power per RE is capped at
# PRACH_NOISE_CAP L (L / N)^4: a ripple of a quarter of that lead.
PRACH_NOISE_CAP = 0.05
PRACH_ROWS_PER_WORKGROUP = {256: 4, 512: 2, 1024: 2}     # of the library's host view (tests/test_door_fuzz.py compares); 1 beyond
PRACH_LAYOUTS = ["dense", "longer rows", "port outside", "repetition outside", "stride 0 over ports", "stride 0 over repetitions"]


def prach_min_ncs(L, N):
    """The smallest n_cs > 0 whose window holds the guard and two more indices: floor(n_cs N / L) >= ceil(N / L) + 2.  A shorter
    window does not hold the peak of its own preamble, so no transmitted preamble could meet the delay rule's condition."""
    g, n_cs = -(-N // L), 1
    while n_cs * N // L < g + 2:
        n_cs += 1
    return n_cs


def draw_prach(idx):
    """One detector case.  Everything in it is defined by include/ce_tp.h `ce_prach_*`: a legal (L, N), 1 .. 64 distinct roots in
    1 .. L - 1, 0 <= n_cs < L, 1 .. 64 windows with n_shifts n_cs <= L (one where n_cs = 0), 1 .. 64 ports and 1 .. 12 repetitions,
    y rows on 8 bytes at free strides >= 0.

    (L, N) uniform over the 13 legal pairs; n_roots from {1, 2, 3, U(4, 12)}, 64 in PRACH_64_ROOT_CASES, the roots distinct draws
    with 1 and L - 1 each forced in one case of four; n_cs from {0, small, NR-typical, large} (never below prach_min_ncs);
    n_shifts from {1, the largest legal up to 64, between}; combine; R from {1 .. 5, U(6, 16)}, 64 in PRACH_64_PORT_CASES; S in
    1 .. 12, and in two draws of five at N <= 1024 as many terms as the workgroup has rows, or one fewer; B in 1 .. 3 occasions of
    kind signal / noise / zero, one signal at least; S, B, n_roots and R lowered in that order until B n_roots terms N <=
    PRACH_MAX_POINTS; per signal occasion one to three preambles on distinct (root, window) pairs (one root per occasion where
    N >= 2 L, see PRACH_NOISE_CAP), each at a drawn index inside its window behind the guard (realize_prach moves it 0.2 samples
    behind that index with prach_oracle.off_half_sample); an amplitude 10^U(-3, 3) and a noise power from {0.03, 0.1, 0.25} under
    the cap per occasion; the layout of y with its lead, row
    length and strides in elements; return_profile; the occasion and the root of the single-item comparisons."""
    rng = _rng(STAGE_PRACH, idx)
    L, N = PRACH_PAIRS[int(rng.integers(len(PRACH_PAIRS)))]
    big_roots, big_ports = idx in PRACH_64_ROOT_CASES, idx in PRACH_64_PORT_CASES
    n_roots = 64 if big_roots else int(_pick(rng, [1, 2, 3, int(rng.integers(4, 13))]))
    lo = prach_min_ncs(L, N)
    kind = str(_pick(rng, ["0", "small", "typical", "large"]))
    n_cs = {"0": 0, "small": lo + int(rng.integers(0, 6)), "typical": max(int(_pick(rng, PRACH_TYPICAL_NCS[L])), lo), "large": int(rng.integers(L // 3, L))}[kind]
    most = min(64, L // n_cs) if n_cs else 1
    n_shifts = int(_pick(rng, [1, most, int(rng.integers(1, most + 1))]))
    combine = int(rng.integers(2))
    R = 64 if big_ports else int(_pick(rng, [1, 2, 3, 4, 5, int(rng.integers(6, 17))]))
    S, B = int(rng.integers(1, 13)), int(rng.integers(1, 4))
    rpw, fit = PRACH_ROWS_PER_WORKGROUP.get(N, 1), str(_pick(rng, ["free", "free", "free", "equal", "fewer"]))
    if rpw > 1 and fit != "free" and not big_ports:        # two draws of five where a workgroup holds several rows: as many terms as rows, or one fewer
        terms = rpw if fit == "equal" else rpw - 1
        R, S = (terms, 1) if combine or rng.random() < 0.5 else (1, terms)
    points =lambda: B * n_roots * (R if combine else R * S) * N                           # noqa: E731
    while points() > PRACH_MAX_POINTS:
        if S > 1 and not combine:
            S -= 1
        elif B > 1:
            B -= 1
        elif n_roots > 1 and not big_roots:
            n_roots -= 1
        else:
            assert R > 1 and not big_ports, idx
            R -= 1
    roots = sorted(int(u) for u in 1 + rng.choice(L - 1, n_roots, replace=False))
    for forced in (1, L - 1):
        if rng.random() < 0.25 and forced not in roots:
            roots[0 if forced == 1 else -1] = forced
    assert len(set(roots)) == n_roots, idx
    roots = [int(u) for u in rng.permutation(roots)]
    kinds = [str(_pick(rng, ["signal", "noise", "zero"], [2, 1, 1])) for _ in range(B)]
    if "signal" not in kinds:
        kinds[int(rng.integers(B))] = "signal"
    g = -(-N // L)
    win_len = n_cs * N // L if n_cs else N
    span = win_len - g - 1 if n_cs else N - 1                                              # indices behind the zero-delay peak that stay inside the window
    preambles = []
    for b, k in enumerate(kinds):
        if k != "signal":
            continue
        pairs, one_root = set(), int(rng.integers(n_roots))
        for _ in range(int(rng.integers(1, 4))):
            pairs.add((int(rng.integers(n_roots)) if N < 2 * L else one_root, int(rng.integers(n_shifts))))
        preambles += [[b, i, v, int(rng.integers(0, max(span, 1)))] for i, v in sorted(pairs)]
    layout = str(_pick(rng, PRACH_LAYOUTS))
    gap = lambda: int(_pick(rng, [0, 1, int(rng.integers(2, 60))]))                        # noqa: E731
    W = L + (int(rng.integers(1, 41)) if layout == "longer rows" or rng.random() < 0.3 else 0)
    if layout in ("dense", "longer rows"):
        W = L if layout == "dense" else max(W, L + 1)
        st = [R * S * W, S * W, W]
    elif layout == "port outside":
        st = _nested(rng, (B, R, S), W, (2, 1, 0))
    elif layout == "repetition outside":
        st = _nested(rng, (B, R, S), W, (1, 2, 0))
    elif layout == "stride 0 over ports":
        rs = W + gap()
        st = [(S - 1) * rs + W + gap(), 0, rs]
    else:
        ps = W + gap()
        st = [(R - 1) * ps + W + gap(), ps, 0]
    return dict(stage="prach", idx=idx, L=L, N=N, roots=roots, n_cs_kind=kind, n_cs=n_cs, n_shifts=n_shifts, combine=combine, R=R, S=S, occasions=kinds, preambles=preambles,
                amp=[float(10.0 ** rng.uniform(-3.0, 3.0)) for _ in range(B)], noise=[float(min(_pick(rng, [0.03, 0.1, 0.25]), PRACH_NOISE_CAP * L * (L / N) ** 4)) for _ in range(B)],
                layout=layout, lead=2 * int(rng.integers(0, 30)) + int(rng.integers(2)), row_len=W, strides=[int(s) for s in st], tail=int(rng.integers(0, 80)),
                return_profile=bool(rng.random() < 0.5), occasion=int(rng.integers(B)), root=int(rng.integers(n_roots)), seed=int(rng.integers(1 << 30)))


def prach_total(c):
    return c["lead"] + extent((len(c["occasions"]), c["R"], c["S"]), c["strides"], c["row_len"]) + c["tail"]


def realize_prach(c):
    """y complex64 [B, R, S, L] as prach_oracle.inputs builds it -- per preamble and port a seeded phase, the same over the
    repetitions, complex normal noise of the occasion's power, all times the occasion's amplitude; a zero occasion all zero --
    then placed into the case's buffer and read back through its strides, so a stride of 0 repeats a row for the oracle as it does
    for the kernel.  `host` is that NaN-filled buffer; ref = prach_oracle.detect_ref; `sent` the (occasion, root index, window)
    triples, the shape prach_oracle.check and hit_miss read."""
    rng = np.random.default_rng(c["seed"])
    L, N, R, S, B = c["L"], c["N"], c["R"], c["S"], len(c["occasions"])
    y = np.zeros((B, R, S, L), np.complex128)
    for b, kind in enumerate(c["occasions"]):
        if kind != "zero":
            y[b] = np.sqrt(c["noise"][b] / 2.0) * (rng.standard_normal((R, S, L)) + 1j * rng.standard_normal((R, S, L)))
    for b, i, v, j in c["preambles"]:
        delay = PO.off_half_sample(L, N, v * c["n_cs"], j * L / N)
        y[b] += np.exp(2j * np.pi * rng.random(R))[:, None, None] * PO.preamble_freq(c["roots"][i], v * c["n_cs"], L, delay)[None, None, :]
    y = (y * np.asarray(c["amp"])[:, None, None, None]).astype(np.complex64)
    host = np.full(prach_total(c), NAN, np.complex64)
    place(host, y, c["lead"], c["strides"])
    y = gather(host, (B, R, S), L, c["lead"], c["strides"])
    ref = PO.detect_ref(y, L, N, c["roots"], c["n_cs"], c["n_shifts"], c["combine"])
    return SimpleNamespace(c=c, L=L, N=N, roots=tuple(c["roots"]), y=y, host=host, ref=ref, sent=tuple(sorted({(b, i, v) for b, i, v, _ in c["preambles"]})))


def prach_gaps(d, t):
    """prach_oracle.signal_gaps with the tolerance `t`: per transmitted preamble (the oracle's gap between the largest and the
    second-largest value of its window, the two tolerances involved)."""
    ref, N, out = d.ref, d.N, []
    for (b, i, v) in d.sent:
        w = ref.profile[b, i, (int(ref.win_start[v]) + np.arange(ref.win_len)) % N]
        o = np.argsort(w)[::-1]
        u = PO.profile_unit(w[o[:2]], ref.mean[b, i], N)
        out.append((float(w[o[0]] - w[o[1]]), float(t * (u[0] + u[1]))))
    return out


def prach_check(got, d, what, t):
    """prach_oracle.check under `t`, and the clause for an all-zero occasion: every output of it is exactly 0."""
    r = PO.check(got, d, what, t=t)
    for b, kind in enumerate(d.c["occasions"]):
        if kind == "zero":
            assert not d.ref.profile[b].any(), f"{what}: the reference of an all-zero occasion is not 0"
            assert not np.asarray(got.peak)[b].any() and not np.asarray(got.delay)[b].any() and not np.asarray(got.mean)[b].any(), f"{what}: occasion {b} is all zero, its outputs are not"
            assert getattr(got, "profile", None) is None or not np.asarray(got.profile)[b].any(), f"{what}: occasion {b} is all zero, its profile is not"
    return r


def prach_classes(c, view):
    """The paths of `ce_prach_kernel` a case reaches, from the library's host view and the dict."""
    L, N, R, S, B = c["L"], c["N"], c["R"], c["S"], len(c["occasions"])
    rpw, terms, n_roots = int(view.rows_per_workgroup), (R if c["combine"] else R * S), len(c["roots"])
    out = {f"L {L}", f"N {N}", f"(L, N) = ({L}, {N})", f"rows_per_workgroup {rpw}", f"outputs per thread {N // int(view.threads_per_row)}",
           "n_roots " + (str(n_roots) if n_roots <= 3 or n_roots == 64 else "4..12"), "n_cs " + c["n_cs_kind"], "combine " + ("coherent" if c["combine"] else "noncoherent"),
           "R " + (str(R) if R <= 5 or R == 64 else "6..16"), "layout " + c["layout"], "profile " + ("returned" if c["return_profile"] else "not returned")}
    if n_roots != 3 or sorted(c["roots"]) != sorted(PO.case_roots(L)):
        out.add("roots other than 1, L - 1, L // 2 + 1")
    if 1 in c["roots"]:
        out.add("root 1 present")
    if L - 1 in c["roots"]:
        out.add("root L - 1 present")
    if terms < rpw:
        out.add("fewer terms than rows_per_workgroup")
    if terms == rpw and rpw > 1:
        out.add("as many terms as rows_per_workgroup")
    if terms % rpw:
        out.add("terms no multiple of rows_per_workgroup")
    if terms > 12:
        out.add("more than 12 terms")
    if R > 5:
        out.add("more than 5 ports")
    if c["n_shifts"] % 4 and n_roots > 3:
        out.add("n_shifts no multiple of 4 with more than three roots")
    if c["n_shifts"] == 1:
        out.add("n_shifts 1")
    if c["n_shifts"] == 64:
        out.add("n_shifts 64")
    if L == 139 and N >= 2048:
        out.add("L 139 at 8 or 16 outputs per thread")
    if c["lead"] % 2:
        out.add("y at an odd element")
    if c["row_len"] > L:
        out.add("rows longer than L")
    for k in ("signal", "noise", "zero"):
        if k in c["occasions"]:
            out.add("an occasion of " + k)
    if B > 1:
        out.add("more than one occasion")
    if min(c["amp"]) < 0.1 or max(c["amp"]) > 10.0:
        out.add("an amplitude beyond a decade from 1")
    if max(sum(1 for p in c["preambles"] if p[0] == b) for b in range(B)) > 1:
        out.add("more than one preamble in an occasion")
    return out


# ================================================================ SRS estimator ====

SRS_272_CASES = [11, 51, 91]             # m_srs = 272, the widest
SRS_64_PORT_CASES = [29, 69, 109]        # R = 64, the limit
SRS_MAX_RES = 1 << 18                    # B R n_sym n_sc of a case
SRS_MAX_RATIO = 32                       # N <= SRS_MAX_RATIO M: beyond, the profile's main lobe is so flat that the oracle's own gap
#                                          between the peak and its neighbour (3.3 (M / N)^2 of the peak) falls below 100 tolerance pairs
SRS_LAYOUTS = ["dense", "grid view", "longer rows", "ports outside items", "odd element, NaN outside the combs"]
SRS_SLOTS_PER_FRAME = [10, 20, 40, 80, 160]
SRS_WIN_KINDS = ["default", "1", "N", "free"]


def draw_srs(idx):
    """One estimator case.  Everything in it is defined by include/ce_tp.h `ce_srs_*`: the comb, ports, cyclic shift and comb
    offset in their ranges, m_srs a multiple of 4 in 4 .. 272, n_symb in {1, 2, 4} from l0 inside n_sym <= n_symb_slot, start_prb per
    symbol inside the grid, N a listed size above M, 1 <= win_len <= N, slot in 0 .. 2^31 - 1, n_id in 0 .. 65535, 1 .. 64 receive
    ports, y rows on 8 bytes at free strides.

    m_srs from {4, 8, 12, 16, 20, 24, 4 U(1, 17)}, 272 in SRS_272_CASES; N from {the smallest size above M, the largest size up to
    SRS_MAX_RATIO M, any between}; win_len default, 1, or free in 1 .. default -- and N or free in 1 .. N only with one sounding port:
    with two or four ports on a comb the full profile repeats every N / 2 or N / 4 indices (each port's term sees the others
    shifted), so a window beyond the default holds several equal maxima and the delay rule's condition cannot hold; R from
    {1 .. 5}, 64 in SRS_64_PORT_CASES; B in 1 .. 3, lowered with n_prb_grid until B R n_sym n_sc <= SRS_MAX_RES; item kinds
    signal / zero, one signal at least; per item an index of the stored window (the transmitted delay is that index minus the
    guard), an amplitude 10^U(-3, 3); slot and n_id as ints or per-item values."""
    rng = _rng(STAGE_SRS, idx)
    k_tc, n_ap = int(_pick(rng, [2, 4])), int(_pick(rng, [1, 2, 4]))
    n_cs, k_bar = int(rng.integers(SO.n_cs_max(k_tc))), int(rng.integers(k_tc))
    m_srs = 272 if idx in SRS_272_CASES else int(_pick(rng, [4, 8, 12, 16, 20, 24, 4 * int(rng.integers(1, 18))]))
    M = 12 * m_srs // k_tc
    sizes = [n for n in (128, 256, 512, 1024, 2048, 4096) if M < n <= SRS_MAX_RATIO * M]
    N = int(_pick(rng, [sizes[0], sizes[-1], sizes[int(rng.integers(len(sizes)))]]))
    n_symb, n_symb_slot = int(_pick(rng, [1, 2, 4])), int(_pick(rng, [12, 14]))
    n_sym = int(rng.integers(n_symb, n_symb_slot + 1))
    l0 = int(rng.integers(0, n_sym - n_symb + 1))
    R = 64 if idx in SRS_64_PORT_CASES else int(rng.integers(1, 6))
    B = int(rng.integers(1, 4))
    while B > 1 and B * R * n_sym * 12 * m_srs > SRS_MAX_RES:
        B -= 1
    while R * n_sym * 12 * m_srs > SRS_MAX_RES:                                            # (64 ports of a wide band: fewer symbols in the grid)
        n_sym -= 1
        l0 = min(l0, n_sym - n_symb)
    assert n_sym >= n_symb, idx
    widest = min(341, SRS_MAX_RES // (B * R * n_sym * 12))
    n_prb_grid = int(_pick(rng, [m_srs, widest, int(rng.integers(m_srs, widest + 1))]))
    start_prb = [int(rng.integers(0, n_prb_grid - m_srs + 1)) for _ in range(n_symb)]
    hopping = str(_pick(rng, ["neither", "group", "sequence"]))
    per_item = bool(rng.random() < 0.5)
    n_val = B if per_item else 1
    slot = [int(_pick(rng, [int(rng.integers(0, 200)), 2 ** 31 - 1, int(rng.integers(0, 2 ** 31))])) for _ in range(n_val)]
    n_id = [int(_pick(rng, [int(rng.integers(0, 1024)), int(rng.integers(1024, 65536)), 65535])) for _ in range(n_val)]
    ncs = SO.n_cs_max(k_tc)
    ports = SO.ports(k_tc, n_ap, n_cs, k_bar)
    fullest = max(sum(1 for comb, _ in ports if comb == k) for k in {comb for comb, _ in ports})
    g = -(-N // M)
    default = N * (ncs // fullest) // ncs - g
    win_kind = str(_pick(rng, SRS_WIN_KINDS))
    if win_kind == "N" and n_ap > 1:
        win_kind = "free"
    win_len = {"default": None, "1": 1, "N": N, "free": int(rng.integers(1, (N if n_ap == 1 else default) + 1))}[win_kind]
    stored = default if win_len is None else win_len
    kinds = [str(_pick(rng, ["signal", "zero"], [4, 1])) for _ in range(B)]
    if "signal" not in kinds:
        kinds[int(rng.integers(B))] = "signal"
    layout = str(_pick(rng, SRS_LAYOUTS))
    n_sc = 12 * n_prb_grid
    W = n_sc + (int(rng.integers(1, 25)) if layout in ("longer rows", "odd element, NaN outside the combs") else 0)
    st = _nested(rng, (B, R, n_sym), W, (2, 0, 1)) if layout == "ports outside items" else [R * n_sym * W, n_sym * W, W]
    lead = 2 * int(rng.integers(0, 20)) + (1 if layout.startswith("odd element") else 0)
    return dict(stage="srs", idx=idx, k_tc=k_tc, n_ap=n_ap, n_cs=n_cs, k_bar=k_bar, m_srs=m_srs, N=N, n_symb=n_symb, n_symb_slot=n_symb_slot, n_sym=n_sym, l0=l0,
                n_prb_grid=n_prb_grid, start_prb=start_prb, slots_per_frame=int(_pick(rng, SRS_SLOTS_PER_FRAME)), hopping=hopping, per_item=per_item, slot=slot, n_id=n_id,
                win_kind=win_kind, win_len=win_len, R=R, B=B, items=kinds, window_index=[int(rng.integers(stored)) for _ in range(B)],
                amp=[float(10.0 ** rng.uniform(-3.0, 3.0)) for _ in range(B)], layout=layout, lead=lead, row_len=W, strides=[int(s) for s in st], tail=int(rng.integers(0, 40)),
                shift=int(rng.integers(1, 2 ** 30 // N)) * int(_pick(rng, [1, -1])), item=int(rng.integers(B)), port=int(rng.integers(R)), seed=int(rng.integers(1 << 30)))


def srs_case(c):
    """The plan values of a draw as srs_oracle.case derives them (any geometry serves as the base: every value is overridden)."""
    return SO.case("a_c4_4p_one_comb_m36", c["hopping"], k_tc=c["k_tc"], n_ap=c["n_ap"], n_cs=c["n_cs"], k_bar=c["k_bar"], m_srs=c["m_srs"], n_symb=c["n_symb"], N=c["N"],
                   R=c["R"], B=c["B"], l0=c["l0"], start_prb=tuple(c["start_prb"]), n_prb_grid=c["n_prb_grid"], n_sym=c["n_sym"], n_symb_slot=c["n_symb_slot"],
                   slots_per_frame=c["slots_per_frame"], slot=tuple(c["slot"]), n_id=tuple(c["n_id"]), win_len=c["win_len"])


def srs_total(c):
    return c["lead"] + extent((c["B"], c["R"], c["n_sym"]), c["strides"], c["row_len"]) + c["tail"]


def srs_used(k):
    """bool [n_sym, n_sc]: the elements of the used combs, all the estimator may read."""
    used = np.zeros((k.n_sym, k.n_sc), bool)
    for comb in k.combs:
        for s in range(k.n_symb):
            used[k.l0 + s, 12 * k.start_prb[s] + comb:12 * k.start_prb[s] + comb + k.k_tc * k.M:k.k_tc] = True
    return used


def realize_srs(c):
    """y complex64 [B, R, n_sym, n_sc] as srs_oracle.draw builds it -- unit-variance clutter on every RE outside the used combs
    (NaN instead in the layout that says so), on the used combs sum_i H r_i exp(-j 2 pi k delay / (N k_tc)) + noise of sigma =
    srs_oracle.SIGMA, with the item's delay window_index - g -- times the item's amplitude; a zero item is exactly 0 on the used
    combs.  `host` is the NaN-filled buffer that holds it at the case's strides.  The oracle's results by srs_oracle.finish."""
    k = srs_case(c)
    rng = np.random.default_rng(c["seed"])
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)                 # noqa: E731
    y = cn(k.B, k.R, k.n_sym, k.n_sc)
    H = cn(k.B, k.R, k.n_ap) + 0.5
    delays = np.array(c["window_index"], np.int64) - k.g
    n = np.arange(k.M)
    for b in range(k.B):
        seq = SO.sequence(k, SO._item(k.slot, b), SO._item(k.n_id, b))
        for comb in k.combs:
            for s in range(k.n_symb):
                kk = 12 * k.start_prb[s] + comb + k.k_tc * n
                tx = sum(H[b, :, i, None] * seq[i, s][None, :] for i, (ci, _) in enumerate(k.ports) if ci == comb)
                y[b][:, k.l0 + s, kk] = tx * np.exp(-2j * np.pi * kk * delays[b] / (k.N * k.k_tc))[None, :] + SO.SIGMA * cn(k.R, k.M)
    used = srs_used(k)
    y = y * np.asarray(c["amp"])[:, None, None, None]
    for b, kind in enumerate(c["items"]):
        if kind == "zero":
            y[b][:, used] = 0
    y = y.astype(np.complex64)
    if c["layout"].endswith("NaN outside the combs"):
        y[:, :, ~used] = NAN
    host = np.full(srs_total(c), NAN, np.complex64)
    place(host, y, c["lead"], c["strides"])
    d = SO.finish(k, y, H, delays)
    d.host, d.draw, d.used = host, c, used
    return d


def srs_gaps(d, t):
    """srs_oracle.gaps with the profile tolerance `t`: per item (the oracle's gap between the largest and the second-largest
    value of sum_r profile -- infinite for a window of one index --, the two tolerances involved)."""
    tot, unit = d.prof.sum(1), t * SO.units(d.c, d)["profile"].sum(1)
    out = []
    for b in range(tot.shape[0]):
        o = np.argsort(tot[b])[::-1]
        out.append((np.inf, 0.0) if tot.shape[1] < 2 else (float(tot[b, o[0]] - tot[b, o[1]]), float(unit[b, o[0]] + unit[b, o[1]])))
    return out


def srs_check(d, tol, prof=None, delay=None, est=None, what=""):
    """srs_oracle.check's clauses under the tolerances `tol` (a dict per quantity): the value rules through srs_oracle.ratios, whose
    `_ratio` accepts nothing but an exact 0 where the unit is 0 (a zero item); the delay rule; equality of the delay on every item
    that carries a signal (at win_len = 1 that is -g).  A zero item's profile is all zero: every index of its window is a maximum.
    Returns the ratios."""
    c, draw = d.c, d.draw
    r = SO.ratios(d, prof, est)
    print(f"{what}: max error / unit: " + ", ".join(f"{k} {v:.3f} (bound {tol[k]:g})" for k, v in r.items()))
    if prof is not None:
        assert np.asarray(prof).dtype == np.float32 and np.asarray(prof).shape == d.prof.shape and np.all(np.isfinite(prof)), what
    if est is not None:
        assert est.h_sb.dtype == np.complex64 == est.h_wb.dtype and est.noise.dtype == np.float32 == est.epre.dtype, what
        assert est.h_sb.shape == d.est.h_sb.shape and est.h_wb.shape == d.est.h_wb.shape and est.noise.shape == d.est.noise.shape == est.epre.shape, what
        assert all(np.all(np.isfinite(np.asarray(getattr(est, k)).view(np.float32))) for k in ("h_sb", "h_wb", "noise", "epre")), f"{what}: non-finite output"
    for k, v in r.items():
        assert v <= tol[k], f"{what}: {k} error ratio {v:.3f} > {tol[k]:g}"
    if delay is not None:
        delay = np.asarray(delay)
        assert delay.dtype == np.int32 and delay.shape == d.delay.shape, (what, delay.dtype, delay.shape)
        assert delay.min() >= -c.g and delay.max() < c.win_len - c.g, f"{what}: a delay outside the window"
        tot, unit = d.prof.sum(1), tol["profile"] * SO.units(c, d)["profile"].sum(1)
        for b in range(len(delay)):
            at, best = int(delay[b]) + c.g, int(d.delay[b]) + c.g
            assert tot[b, at] >= tot[b, best] - (unit[b, at] + unit[b, best]), f"{what}: delay {delay[b]} of item {b} is no maximum of the oracle's profile"
            if draw["items"][b] == "signal":
                assert delay[b] == d.delay[b], f"{what}: delay {delay[b]} of item {b}, the oracle has {d.delay[b]}"
    return r


def srs_classes(c, hv):
    """The paths of the two SRS kernels a case reaches, from the library's host view and the dict."""
    k_tc, n_ap, N, M = c["k_tc"], c["n_ap"], c["N"], hv.m
    tpr, rpw = int(hv.view.threads_per_row), int(hv.view.rows_per_workgroup)
    ncs = SO.n_cs_max(k_tc)
    out = {f"k_tc {k_tc}", f"n_ap {n_ap}", f"N {N}", f"N {N}: {tpr} threads per row, {rpw} rows per workgroup, {N // tpr} outputs per thread", f"n_symb {c['n_symb']}",
           f"n_symb_slot {c['n_symb_slot']}", f"slots_per_frame {c['slots_per_frame']}", "hopping " + c["hopping"], "win_len " + c["win_kind"], "layout " + c["layout"],
           "R " + str(c["R"]), "slot and n_id " + ("per item" if c["per_item"] else "as ints"), f"n_combs {hv.n_combs}", "M " + (str(M) if M <= 72 else "above 72")}
    if c["n_sym"] < 14:
        out.add("n_sym < 14")
    if max(c["n_id"]) > 1023:
        out.add("n_id above 1023")
    if any(v & (1 << 12) for v in c["n_id"]) and c["hopping"] != "neither":
        out.add("bit 12 of c_init set with hopping")
    if max(c["slot"]) >= 2 ** 30:
        out.add("slot above 2^30")
    stored = hv.default_win_len if c["win_len"] is None else c["win_len"]
    if c["win_len"] is not None and stored > hv.default_win_len:
        out.add("win_len above the default")
    if stored > N - hv.guard:
        out.add("win_len above N - g")
    if n_ap == 4 and k_tc == 2 and c["n_cs"] < ncs // 2:
        out.add("four ports on one comb at k_tc 2")
    if n_ap == 1 and k_tc == 4:
        out.add("n_ap 1 at k_tc 4")
    if 36 <= M < 72 and M not in (36, 48):
        out.add("M 60")
    if M == 72:
        out.add("M 72: sequence hopping live" if c["hopping"] == "sequence" else "M 72")
    if M < 36:
        out.add("a phi-table sequence")
    if N == min(n for n in (128, 256, 512, 1024, 2048, 4096) if n > M):
        out.add("N the smallest size above M")
    if c["m_srs"] == 272:
        out.add("m_srs 272")
    if len(set(c["start_prb"])) > 1:
        out.add("start_prb differs between symbols")
    if "zero" in c["items"]:
        out.add("a zero item")
    if c["B"] > 1:
        out.add("more than one item")
    if min(c["amp"]) < 0.1 or max(c["amp"]) > 10.0:
        out.add("an amplitude beyond a decade from 1")
    if hv.v_live and c["hopping"] == "sequence":
        out.add("sequence hopping live")
    return out
