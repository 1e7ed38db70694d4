"""Seeded random cases for the five PUSCH stages added behind the first fuzz -- transform de-precoding (csrc/ce_tp.hip), the LDPC
decoder (csrc/ce_ldpc.hip), transport-block assembly (csrc/ce_tb.hip), the transport-block encoder (csrc/ce_enc.hip) and the
modulator (csrc/ce_mod.hip) -- for tests/test_chain_fuzz.py (CPU: what the draws must satisfy by themselves) and
tests/test_zzzzzzzzzz_hip_chain_fuzz.py (GPU: the kernels against the oracles on them).

The structure is tests/stage_fuzz_cases.py's: `draw_*(idx)` derives a case from np.random.default_rng([BASE_SEED, stage_id,
idx]) as a plain dict of Python values (stage ids 4 .. 8, so no draw of the first fuzz changes); `realize_*(case)` turns it
into arrays, seeded by the dict's own "seed"; `*_classes(case)` names the kernel paths it reaches.  References and comparison
rules are the existing oracles' (tp_oracle, ldpc_oracle, tb_oracle, enc_oracle, mod_oracle, rm_oracle): nothing is restated
here.  Shapes are the smallest that still reach every kernel path."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import demod_oracle as D
import dmrs_oracle
import enc_oracle as E
import eq_oracle as Q
import ldpc_oracle as O
import mod_oracle as M
import rm_oracle as R
import tb_oracle as T
import tp_oracle as TP
from srsran_ce_pytorch_amd import deprecode as DP, ldpc as LD, synth as S
from stage_fuzz_cases import BASE_SEED, DM_BAD_NVAR, DM_BAD_X, RM_MAX_G, _eq_geometry, _pick, _rng   # noqa: F401  (BASE_SEED: the seed both fuzzes share)

STAGE_TP, STAGE_LDPC, STAGE_TB, STAGE_ENC, STAGE_MOD = 4, 5, 6, 7, 8
N_TP, N_LDPC, N_TB, N_ENC, N_MOD = len(TP.VALID_PRBS), 80, 100, 100, 100
NR_ZC = list(R.ZC_SET)                                  # the 51 lifting sizes of TS 38.212 Table 5.3.2-1
assert N_TP == 53 and len(NR_ZC) == 51

# T = 4 C as in tp_oracle.py; C = the float32 numpy restatement's largest error ratio over the 53 realized sweep cases
# (tests/test_chain_fuzz.py re-measures it and fails if it exceeds the recorded value); never measured on the kernel
C_TP_FUZZ = 1.3          # measured 1.204 (deprecode_f32 over the 53 sweep cases), rounded up
T_TP_FUZZ = 4.0 * C_TP_FUZZ


# ---------------------------------------------------------------- transform de-precoding: a sweep ----

TP_EDGE_PRBS = [32, 36, 96, 100]                         # either side of threads_per_row's switches at M = 384 and M = 1152


def draw_tp(idx):
    """Case idx is allocation size tp_oracle.VALID_PRBS[idx]: every valid size, hence every radix sequence, once.  The seed
    decides S, B, whether the call is in place (a third) and whether one row is fully dropped (a fifth)."""
    rng = _rng(STAGE_TP, idx)
    B = int(rng.integers(1, 6))
    return dict(stage="tp", idx=idx, n_prb=int(TP.VALID_PRBS[idx]), S=int(rng.integers(1, 15)), B=B, in_place=bool(rng.random() < 1 / 3),
                dropped_row=bool(rng.random() < 0.2), slot=int(rng.integers(B)), seed=int(rng.integers(1 << 30)))


def realize_tp(c):
    """tp_oracle.draw's signal (precoded 16QAM + CN(0, nvar_k), nvar_k = 10^U(-3, 0.5)) with 2 % of the REs erased by the
    special values of stage_fuzz_cases.realize_dm and, where drawn, one row dropped by every one of them in turn; and the
    float64 reference."""
    rng = np.random.default_rng(c["seed"])
    M_, S_, B = 12 * c["n_prb"], c["S"], c["B"]
    n = S_ * M_
    x_tx = D.modulate(rng.integers(0, 2, (B, n * 4)), 4)
    nvar = 10.0 ** rng.uniform(-3.0, 0.5, (B, n))
    noise = (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))) * np.sqrt(nvar / 2.0)
    x = (TP.precode(x_tx, M_) + noise).astype(np.complex64)
    nvar = nvar.astype(np.float32)
    erased = rng.random((B, n)) < 0.02
    which = rng.integers(0, len(DM_BAD_NVAR) + len(DM_BAD_X), (B, n))
    row = None
    if c["dropped_row"]:
        row = (int(rng.integers(B)), int(rng.integers(S_)))
        erased[row[0], row[1] * M_:(row[1] + 1) * M_] = True
        which[row[0], row[1] * M_:(row[1] + 1) * M_] = np.arange(M_) % (len(DM_BAD_NVAR) + len(DM_BAD_X))
    for k, v in enumerate(DM_BAD_NVAR):
        nvar[erased & (which == k)] = v
    for k, v in enumerate(DM_BAD_X):
        x[erased & (which == len(DM_BAD_NVAR) + k)] = v
    d = SimpleNamespace(c=c, M=M_, S=S_, B=B, x_hat=x, nvar=nvar, erased=erased, row=row)
    d.ref_x, d.ref_nv = TP.deprecode_ref(x, nvar, M_)
    return d


def tp_classes(c, d=None):
    """The kernel paths of csrc/ce_tp.hip a sweep case reaches, from the library's host view of the shape."""
    v = DP.derive_host(c["n_prb"], c["S"])
    out = {"radix " + "x".join(str(int(r)) for r in v.radix[:v.n_passes]), f"threads_per_row {int(v.threads_per_row)}",
           f"rows_per_workgroup {int(v.rows_per_workgroup)}"}
    if c["n_prb"] in TP_EDGE_PRBS:
        out.add(f"n_prb {c['n_prb']}")
    if c["S"] % int(v.rows_per_workgroup):
        out.add("S % rows_per_workgroup != 0")
    if c["in_place"]:
        out.add("in place")
    if c["dropped_row"]:
        out.add("a dropped row")
    if d is not None and d.erased.any():
        out.add("erasures")
    return out


# ---------------------------------------------------------------- LDPC decoder ----

LDPC_WG_THREADS, LDPC_WG_LDS = 256, 80896                # the two caps of blocks_per_workgroup (csrc/ce_ldpc.hip)
LDPC_ODD_ZC = [17, 33, 63, 65, 127, 129, 255, 257, 383]  # either side of a wave, of two, of four; no NR size among them
LDPC_ITERS = [1, 2, 3, 8, 20]
LDPC_ROW_KINDS = ["zero", "random", "3 dB", "1 dB", "clean", "random", "-2.5 dB"]      # the mix of ldpc_oracle.mixed_inputs


def ldpc_graph(c):
    """Rows of (col, shift) of a case: row r ends with its own column n_sys + r at shift 0; its other degrees[r] - 1 edges are
    distinct columns below n_sys + r at random shifts -- lower-triangular, so ldpc_oracle.encode yields codewords."""
    rng = np.random.default_rng(c["graph_seed"])
    n_sys, zc = c["n_sys"], c["zc"]
    rows = []
    for r, deg in enumerate(c["degrees"]):
        cols = sorted(rng.choice(n_sys + r, deg - 1, replace=False).tolist())
        rows.append([(int(col), int(rng.integers(zc))) for col in cols] + [(n_sys + r, 0)])
    return rows


def ldpc_view(c):
    return LD.derive_host(LD.LdpcGraph(ldpc_graph(c), c["n_sys"] + len(c["degrees"])), c["zc"], c["n_in"], c["k_out"], n_punctured_cols=c["n_punct"],
                          dtype=torch.int8 if c["dtype"] == "i8" else torch.float32, llr_scale=c["llr_scale"], max_iters=c["max_iters"],
                          early_stop=c["early_stop"])


def draw_ldpc(idx):
    """One decoder case.  zc: the 51 NR lifting sizes in cases 0 .. 50, then 2 .. 384 with half of the weight on
    LDPC_ODD_ZC.  Graph: n_sys in 2 .. 22, n_rows in 1 .. 46; one row is forced to degree 2 + idx mod 18, so that every
    instance ldpc_row<DEG> / ldpc_parity<DEG> runs; the others are uniform up to what the row admits, or small.  nb is chosen
    against the library's blocks_per_workgroup: below it, a multiple of it, or more than one workgroup with a partial last
    one."""
    rng = _rng(STAGE_LDPC, idx)
    zc = NR_ZC[idx] if idx < len(NR_ZC) else int(_pick(rng, LDPC_ODD_ZC)) if rng.random() < 0.5 else int(rng.integers(2, 385))
    forced = 2 + idx % 18
    n_sys = max(int(rng.integers(2, 23)), forced - 1)     # row 0 admits degrees up to n_sys + 1
    n_rows = int(rng.integers(1, 47))
    degrees = []
    for r in range(n_rows):
        top = min(O.MAX_ROW_DEGREE, n_sys + r + 1)
        degrees.append(int(rng.integers(2, top + 1)) if rng.random() < 0.5 else int(rng.integers(2, min(6, top) + 1)))
    degrees[int(rng.integers(n_rows))] = forced
    n_cols = n_sys + n_rows
    n_punct = int(_pick(rng, [0, 1, 2, int(rng.integers(0, n_sys + 1))], [0.2, 0.15, 0.45, 0.2]))
    full = (n_cols - n_punct) * zc
    n_in = int(_pick(rng, [full, full - 1, min(full, int(rng.integers(1, full + 1)) | 1), 1], [0.5, 0.2, 0.2, 0.1]))
    k_max = n_sys * zc
    k = int(rng.integers(1, k_max + 1))
    k32 = 32 * max(1, k // 32)
    k_out = min(k_max, int(_pick(rng, [k_max, k, 128 * max(1, k // 128), k32 if k32 % 128 else k32 + 32, k | 1], [0.3, 0.2, 0.15, 0.15, 0.2])))
    dtype = "i8" if rng.random() < 0.5 else "f32"
    c = dict(stage="ldpc", idx=idx, zc=zc, n_sys=n_sys, degrees=degrees, graph_seed=int(rng.integers(1 << 30)), n_punct=n_punct, n_in=n_in, k_out=k_out,
             max_iters=int(_pick(rng, LDPC_ITERS)), early_stop=bool(rng.random() < 0.75), dtype=dtype,
             llr_scale=float(_pick(rng, [1.0, 4.0, 1.3])) if dtype == "f32" else 1.0)
    bpw = int(ldpc_view(c).blocks_per_workgroup)
    kind = str(_pick(rng, ["below", "multiple", "partial"], [0.25, 0.25, 0.5]))
    if kind == "below":
        nb = int(rng.integers(1, bpw)) if bpw > 1 else 1
    elif kind == "multiple":
        nb = bpw * int(rng.integers(1, 3))
    else:
        nb = bpw * int(rng.integers(1, 3)) + (int(rng.integers(1, bpw)) if bpw > 1 else 0) + (bpw == 1)
    c.update(nb=nb, nb_kind=kind, first_row=int(rng.integers(len(LDPC_ROW_KINDS))), seed=int(rng.integers(1 << 30)))
    return c


def realize_ldpc(c):
    """nb input rows in the mix of ldpc_oracle.mixed_inputs, row i of kind LDPC_ROW_KINDS[(first_row + i) mod 7]: an all-zero
    row, a clean codeword, noisy codewords at 3, 1 and -2.5 dB, random rows over the full int8 range (-128 included).  A
    float32 case holds (int8 value + U(-0.49, 0.49)) / llr_scale, with NaN, +-inf and +-1e9 on a few positions of the random
    rows.  The reference is decode_ref of the quantised rows."""
    rng = np.random.default_rng(c["seed"])
    rows, n_sys, zc, nb, n_in = ldpc_graph(c), c["n_sys"], c["zc"], c["nb"], c["n_in"]
    n_cols = n_sys + len(rows)
    cw = O.encode(rows, n_sys, zc, rng.integers(0, 2, (nb, n_sys * zc)))[:, c["n_punct"] * zc: c["n_punct"] * zc + n_in]
    kinds = [LDPC_ROW_KINDS[(c["first_row"] + i) % len(LDPC_ROW_KINDS)] for i in range(nb)]
    llr = np.zeros((nb, n_in), np.int8)
    for i, kind in enumerate(kinds):
        if kind == "random":
            llr[i] = rng.integers(-128, 128, n_in)
        elif kind == "clean":
            llr[i] = O.noisy_llr(rng, cw[i], 40.0, 1.0)
        elif kind != "zero":
            llr[i] = O.noisy_llr(rng, cw[i], float(kind.split()[0]), O.SCALE)
    x = llr
    if c["dtype"] == "f32":
        x = ((llr.astype(np.float64) + rng.uniform(-0.49, 0.49, llr.shape)) / c["llr_scale"]).astype(np.float32)
        x[llr == 0] = 0.0                                  # the all-zero row stays all zero
        special = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, -0.0, 3e38], np.float32)
        for i, kind in enumerate(kinds):
            if kind == "random":
                where = rng.integers(0, n_in, len(special))
                x[i, where] = special
    d = SimpleNamespace(c=c, rows=rows, n_cols=n_cols, kinds=kinds, llr=x)
    d.L, d.status, _ = O.decode_ref(rows, n_cols, zc, O.channel(O.quantise(x, c["llr_scale"]), n_cols, zc, c["n_punct"]), c["max_iters"], c["early_stop"])
    d.hard = O.pack(d.L, c["k_out"])
    return d


def ldpc_caps(c, v):
    """(threads cap, LDS cap) of blocks_per_workgroup = max(1, min of the two)."""
    return LDPC_WG_THREADS // c["zc"], LDPC_WG_LDS // int(v.lds_bytes_per_block)


def ldpc_classes(c):
    v = ldpc_view(c)
    bpw, nb = int(v.blocks_per_workgroup), c["nb"]
    by_threads, by_lds = ldpc_caps(c, v)
    out = {f"degree {d}" for d in c["degrees"]} | {"nb " + c["nb_kind"], "dtype " + c["dtype"], f"max_iters {c['max_iters']}"}
    if bpw == 1:
        out.add("bpw = 1")
    elif by_lds < by_threads:
        out.add("bpw capped by LDS")
    else:
        out.add("bpw capped by threads")
    if int(v.threads) % 64:
        out.add("threads % 64 != 0")
    if (c["zc"] % 64) and bpw > 1:
        out.add("a block straddles a wave")
    if nb > bpw:
        out.add("more than one workgroup")
        if nb % bpw:
            out.add("a partial last workgroup")
    if c["dtype"] == "f32":
        out |= {"f32 input", f"scale {c['llr_scale']:g}"}
    if not c["early_stop"]:
        out.add("early_stop off")
    out.add(f"n_punct {c['n_punct']}" if c["n_punct"] <= 2 else "n_punct > 2")
    if c["zc"] in NR_ZC:
        out.add("an NR lifting size")
    if c["n_in"] < (c["n_sys"] + len(c["degrees"]) - c["n_punct"]) * c["zc"]:
        out.add("n_in below full")
    if c["k_out"] % 32:
        out.add("k_out % 32 != 0")
    elif c["k_out"] % 128:
        out.add("k_out % 128 != 0")
    else:
        out.add("k_out % 128 == 0")
    return out


def ladder_graph(zc=7, n_sys=2):
    """The degree ladder: row r has degree r + 2, r = 0 .. 17 -- the narrowest graph that holds every degree 2 .. 19."""
    rng = np.random.default_rng(BASE_SEED)
    rows = []
    for r in range(O.MAX_ROW_DEGREE - 1):
        cols = sorted(rng.choice(n_sys + r, r + 1, replace=False).tolist())
        rows.append([(int(col), int(rng.integers(zc))) for col in cols] + [(n_sys + r, 0)])
    return SimpleNamespace(rows=rows, n_sys=n_sys, n_cols=n_sys + len(rows), zc=zc)


# ---------------------------------------------------------------- transport-block assembly ----

TB_MAX_A = 90000          # c152 stays the pinned large case
TB_PIECES = [(multi, piece) for multi in (False, True) for piece in range(1, 6)]       # the instances tb_residues<MULTI, PIECE>
TB_CORRUPTIONS = ["untouched", "payload flips", "crc24b flips", "tb crc flips", "refreshed crc24b", "random rows"]


def tb_derive(c):
    """tb_oracle.derive of a case, or the ValueError the oracle refuses the size with."""
    try:
        return T.derive(c["bg"], c["A"])
    except ValueError as e:
        return e


def tb_piece(d):
    return -(-d.in_row_bytes // 256)       # dwords per lane of a 64-lane wave: ce_tb_host_view.piece_dwords


def _tb_valid(bg, A):
    return not isinstance(tb_derive(dict(bg=bg, A=A)), Exception)


def _tb_edges():
    """(bg, A): either side of the CRC16 / CRC24A change, of BG1's last single block, and of each change of C up to C = 11 --
    the last valid size with C blocks and the first valid one with C + 1; for C <= 2 also the size right behind the change as
    it is, which B mod C may refuse (BG1's 8425 is such a size)."""
    out = [(bg, A) for bg in (1, 2) for A in (3824, 3825)] + [(1, 8424), (1, 8425)]

    def blocks(A, k_cb):                                           # 5.2.2's C, whether or not B mod C then refuses the size
        B = A + (24 if A > 3824 else 16)
        return 1 if B <= k_cb else -(-B // (k_cb - 24))

    for bg, k_cb in ((1, 8448), (2, 3840)):
        for C in range(1, 11):
            top = next(A for A in range(C * k_cb, 0, -1) if blocks(A, k_cb) <= C)
            lo = next(A for A in range(top, 0, -1) if _tb_valid(bg, A))
            hi = next(A for A in range(top + 1, top + 64) if _tb_valid(bg, A))
            assert T.derive(bg, lo).C == C and T.derive(bg, hi).C == C + 1, (bg, C, lo, hi)
            out += [(bg, lo), (bg, hi)] + [(bg, top + 1)] * (C <= 2)
    return sorted(set(out))


TB_EDGES = _tb_edges()
TB_NAMED_EDGES = [(1, 3824), (1, 3825), (1, 8424), (1, 8425)]     # 8425: B = 8449 is no multiple of C = 2, refused


def draw_tb(idx):
    """One assembly case.  Every fifth case takes (bg, A) from the edges (TB_NAMED_EDGES, then drawn from TB_EDGES); the others take the ten (C = 1 or C > 1, piece)
    instances in turn -- eight cases each: a uniform or log-uniform A would leave (C = 1, piece 3) at two -- with bg and a
    log-uniform A redrawn until the oracle's integers are that instance's.  Only an edge may be a size the oracle refuses.
    Then S, the kind of corruption and the number of flipped bits."""
    rng = _rng(STAGE_TB, idx)
    source = "edge" if idx % 5 == 4 else "instance"
    tries = 0
    if source == "edge":                                  # the four named BG1 edges first, then any
        bg, A = TB_NAMED_EDGES[idx // 5] if idx // 5 < len(TB_NAMED_EDGES) else (int(v) for v in _pick(rng, TB_EDGES))
    else:
        want = TB_PIECES[(idx - idx // 5) % len(TB_PIECES)]
        while True:
            tries += 1
            assert tries < 200000, (idx, want)
            bg, A = int(rng.integers(1, 3)), min(TB_MAX_A, int(10.0 ** rng.uniform(0.0, np.log10(TB_MAX_A))))
            d = tb_derive(dict(bg=bg, A=A))
            if not isinstance(d, Exception) and (d.C > 1, tb_piece(d)) == want:
                break
    return dict(stage="tb", idx=idx, bg=bg, A=A, S=int(rng.integers(1, 13)), source=source, tries=tries,
                corruption=str(_pick(rng, TB_CORRUPTIONS, [0.15, 0.25, 0.15, 0.15, 0.15, 0.15])), n_flips=int(rng.integers(1, 4)), seed=int(rng.integers(1 << 30)))


def tb_corruption(c, d):
    """The corruption a case applies: a single block has no CRC24B field, so those two kinds fall back to the transport
    block's own CRC."""
    return "tb crc flips" if d.C == 1 and c["corruption"] in ("crc24b flips", "refreshed crc24b") else c["corruption"]


def realize_tb(c):
    """segment()'s valid rows of S random transport blocks with random bits behind K', then the case's corruption: flipped
    bits at tb_oracle.boundary_bits and at random positions of the payload, of a CRC24B field or of the transport-block CRC;
    a block whose CRC24B is recomputed after a payload flip; or fully random rows.  The reference is assemble_ref."""
    d = tb_derive(c)
    assert not isinstance(d, Exception), c
    rng = np.random.default_rng(c["seed"])
    S_ = c["S"]
    tb_bits = rng.integers(0, 2, (S_, d.A)).astype(np.uint8)
    bits = np.zeros((S_, d.C, 8 * d.in_row_bytes), np.uint8)
    bits[..., :d.Kp] = T.segment(tb_bits, c["bg"]).reshape(S_, d.C, d.Kp)
    bits[..., d.Kp:] = rng.integers(0, 2, bits[..., d.Kp:].shape)
    rows = np.packbits(bits, axis=-1)
    kind, flips = tb_corruption(c, d), []
    if kind == "random rows":
        rows = rng.integers(0, 256, rows.shape).astype(np.uint8)
    elif kind != "untouched":
        for _ in range(c["n_flips"]):
            b = int(rng.integers(S_))
            if kind == "crc24b flips":
                r, i = int(rng.integers(d.C)), int(_pick(rng, [d.P, d.Kp - 1, int(rng.integers(d.P, d.Kp))]))
            else:
                lo, hi = (d.A, d.B) if kind == "tb crc flips" else (0, d.A)
                edge = [s for s in T.boundary_bits(d) if lo <= s < hi]
                s = int(_pick(rng, edge)) if edge and rng.random() < 0.5 else int(rng.integers(lo, hi))
                r, i = divmod(s, d.P)
            rows = T.flip(rows, b, r, i)
            if kind == "refreshed crc24b":
                rows = T.refresh_cb_crc(rows, d, b, r)
            flips.append((b, r, i))
    x = SimpleNamespace(c=c, d=d, tb_bits=tb_bits, rows=rows, kind=kind, flips=flips)
    x.tb, x.tb_status, x.cb_status = T.assemble_ref(rows, d)
    return x


def tb_classes(c):
    d = tb_derive(c)
    if isinstance(d, Exception):
        return {"refused"}
    out = {f"C {'> 1' if d.C > 1 else '= 1'}, piece {tb_piece(d)}", "CRC" + d.which, tb_corruption(c, d), "source " + c["source"], f"bg {c['bg']}"}
    if d.P % 32:
        out.add("P % 32 != 0")
    if d.P % 8:
        out.add("P % 8 != 0")
    if (c["S"] * d.C) % 4:
        out.add("S C % 4 != 0")
    if d.C % 4:
        out.add("C % 4 != 0")
    if d.C > 4:
        out.add("C > 4")
    return out


# ---------------------------------------------------------------- encoder ----

ENC_FORMS = [0, 1, 2, "tri"]
ENC_BAD_GRAPHS = ["three shifts", "extension column", "parity column twice"]
ENC_BIG_ZC = [288, 320, 352, 384] * 3 + [144, 176, 208, 240, 160, 192, 224, 256]       # cases 51 .. 70: the rare col_dwords 5 .. 12
ENC_MAX_TRIES = 100000


def _enc_descriptor(rng, refuse, want_zc):
    """(bg, A, qm, L, G, n_ref, tries) as stage_fuzz_cases.draw_rm draws a rate-recovery descriptor -- A from three bands,
    n_ref from {0, K - 2 Zc, K - 2 Zc + 1, uniform in [K - 2 Zc, N]}, q = G / (L Qm) from three bands cut to G <= RM_MAX_G,
    `refuse` one of draw_rm's four refusals or "" -- redrawn until R.derive yields the lifting size `want_zc`, if given."""
    tries = 0
    while True:
        tries += 1
        assert tries < ENC_MAX_TRIES, (refuse, want_zc)
        bg, qm, L = int(rng.integers(1, 3)), int(_pick(rng, [2, 4, 6, 8])), int(rng.integers(1, 5))
        band = int(rng.choice(3, p=[0.25, 0.25, 0.5]))
        A = int([rng.integers(1, 401), rng.integers(400, 4001), 8 * rng.integers(500, 2201)][band])
        try:
            g = R.derive(bg, A, 2, 1, 2 * 10000)
        except ValueError:
            g = None
        if refuse == "B mod C":
            if g is None:
                return bg, A, qm, L, L * qm * 50, 0, tries
            continue
        if g is None or (refuse == "q < C" and g.C == 1) or (want_zc and g.Zc != want_zc):
            continue
        lo = g.K - 2 * g.Zc
        kind = int(rng.choice(4, p=[0.15, 0.25, 0.2, 0.4]))
        n_ref = [0, lo, lo + 1, int(rng.integers(lo, g.N + 1))][kind]
        N_cb = g.N if n_ref == 0 else min(g.N, n_ref)
        P = N_cb - (g.K - g.Kp)
        lq = L * qm
        q_max = RM_MAX_G // lq
        q_band = int(rng.choice(3, p=[0.2, 0.3, 0.5]))
        if q_band == 0:
            q = max(g.C, int(rng.integers(1, 41)))
        else:
            q = max(g.C, int((rng.uniform(0.2, 1.0) if q_band == 1 else rng.uniform(1.0, 3.5)) * g.C * P / lq))
        if q > q_max:
            q = int(rng.integers(max(g.C, q_max // 2), q_max + 1))
        if q_band == 2 and q % g.C == 0 and q < q_max and rng.random() < 0.7:
            q += 1                                # unequal E_r among the code blocks
        if g.C > 1 and q >= 32 * g.C and rng.random() < 0.4:
            q -= q % (32 * g.C)                   # every E_r a multiple of 32: the blocks meet at dword boundaries of g
        G = lq * q
        if refuse == "q < C":
            G = lq * (g.C - 1)
        elif refuse == "G":
            G += 1
        elif refuse == "n_ref":
            n_ref = lo - 1
        return bg, A, qm, L, G, n_ref, tries


def enc_derive(c):
    try:
        return R.derive(c["bg"], c["A"], c["qm"], c["L"], c["G"], c["n_ref"])
    except ValueError as e:
        return e


def draw_enc(idx):
    """One encoder case.  Cases 0 .. 50 are pinned one to each NR lifting size and cases 51 .. 70 to the large sizes whose
    col_dwords = ceil(Zc / 32) one NR size each would leave at one or two cases; both kinds are accepted descriptors.  Of
    the rest about a quarter are descriptors the oracle refuses and a sixth graphs that break the stated form (7 % and 5 %
    of all cases).  The graph is enc_oracle.nr_core_graph (variant 0, 1, 2) or the triangular ldpc_oracle.random_graph,
    truncated in half of the cases where n_ref makes N_cb fit a prefix of rows."""
    rng = _rng(STAGE_ENC, idx)
    want_zc = NR_ZC[idx] if idx < len(NR_ZC) else ENC_BIG_ZC[idx - len(NR_ZC)] if idx - len(NR_ZC) < len(ENC_BIG_ZC) else 0
    refuse = bad_graph = ""
    if not want_zc:
        refuse = str(_pick(rng, ["B mod C", "q < C", "G", "n_ref"])) if rng.random() < 0.24 else ""
        bad_graph = str(_pick(rng, ENC_BAD_GRAPHS)) if not refuse and rng.random() < 0.22 else ""
    bg, A, qm, L, G, n_ref, tries = _enc_descriptor(rng, refuse, want_zc)
    form = _pick(rng, [0, 1] if bad_graph == "three shifts" else ENC_FORMS)
    form = form if isinstance(form, str) else int(form)
    sh = E.SHAPE[bg]
    n_rows = sh["n_rows"]
    d = enc_derive(dict(bg=bg, A=A, qm=qm, L=L, G=G, n_ref=n_ref))
    if not isinstance(d, Exception) and not bad_graph:
        fit = max(4, -(-d.N_cb // d.Zc) + 2 - sh["n_sys"])            # the fewest rows with (n_cols - 2) Zc >= N_cb
        if fit < n_rows and rng.random() < 0.5:
            n_rows = int(rng.integers(fit, n_rows + 1))
    if bad_graph == "three shifts" and not isinstance(d, Exception) and d.Zc < 3:
        bad_graph = "extension column"                                # three distinct shifts need Zc >= 3
    S_ = int(rng.integers(1, 7))
    rv_kind = str(_pick(rng, ["tensor", "strided", "scalar"]))
    rvs = [int(v) for v in rng.integers(0, 4, S_)]
    if rv_kind == "scalar":
        rvs = [rvs[0]] * S_
    return dict(stage="enc", idx=idx, bg=bg, A=A, qm=qm, L=L, G=G, n_ref=n_ref, form=form, n_rows=n_rows, graph_seed=int(rng.integers(1 << 30)),
                bad_graph=bad_graph, want_zc=int(want_zc), tries=tries, S=S_, rvs=rvs, rv_kind=rv_kind, want_cw=bool(rng.random() < 0.5),
                seed=int(rng.integers(1 << 30)))


def enc_graph(c, zc):
    """SimpleNamespace(rows, n_cols, n_sys, zc) of a case at lifting size zc, with the case's defect where it has one:
    "three shifts": column n_sys at three distinct shifts; "extension column": row 5 touches row 4's parity column;
    "parity column twice": row 6's own column in core row 0 too."""
    sh = E.SHAPE[c["bg"]]
    n_sys = sh["n_sys"]
    rng = np.random.default_rng(c["graph_seed"])
    if c["form"] == "tri":
        rows = O.random_graph(rng, n_sys, sh["n_rows"], zc, sh["core_degree"], sh["ext"])
    else:
        rows = E.nr_core_graph(rng, n_sys, sh["n_rows"], zc, sh["core_degree"], sh["ext"], c["form"])
    rows = [list(row) for row in rows[:c["n_rows"]]]
    if c["bad_graph"] == "three shifts":
        first = int(rng.integers(zc))
        shifts = iter([first, (first + 1) % zc, (first + 2) % zc])
        rows[:4] = [[(col, next(shifts)) if col == n_sys else (col, s) for col, s in row] for row in rows[:4]]
    elif c["bad_graph"] == "extension column":
        rows[5] = [e for e in rows[5] if e[0] != n_sys + 4][1:] + [(n_sys + 4, int(rng.integers(zc)))]
        rows[5].sort(key=lambda e: (e[0] == n_sys + 5, e[0]))
    elif c["bad_graph"] == "parity column twice":
        rows[0] = rows[0][1:] + [(n_sys + 6, int(rng.integers(zc)))]
    return SimpleNamespace(rows=rows, n_cols=n_sys + len(rows), n_sys=n_sys, zc=zc)


def enc_view(c, g):
    from srsran_ce_pytorch_amd import encoder as EN
    return EN.derive_host(c["bg"], c["A"], c["qm"], c["L"], c["G"], LD.LdpcGraph(g.rows, g.n_cols), c["n_ref"])


def realize_enc(c):
    """S random transport blocks as packed rows with random bits behind bit A, and enc_oracle.transmit of them under the
    case's rv per slot, packed as the kernel writes g and cw."""
    d = enc_derive(c)
    assert not isinstance(d, Exception) and not c["bad_graph"], c
    rng = np.random.default_rng(c["seed"])
    g = enc_graph(c, d.Zc)
    tb_bits = rng.integers(0, 2, (c["S"], d.A)).astype(np.uint8)
    full = rng.integers(0, 2, (c["S"], 128 * -(-d.A // 128))).astype(np.uint8)
    full[:, :d.A] = tb_bits
    bits, cw = E.transmit(d, g, tb_bits, c["rvs"])
    return SimpleNamespace(c=c, d=d, graph=g, tb_bits=tb_bits, tb_rows=np.packbits(full, axis=-1), g=T.pack(bits, 16 * -(-d.G // 128)),
                           cw=T.pack(cw, 16 * -(-cw.shape[-1] // 128)))


def enc_classes(c):
    d = enc_derive(c)
    if isinstance(d, Exception):
        return {"refused descriptor"}
    g = enc_graph(c, d.Zc)
    if c["bad_graph"]:
        return {"refused graph", "refused graph: " + c["bad_graph"]}
    v = enc_view(c, g)
    out = {f"col_dwords {int(v.col_dwords)}", f"form {c['form']}", "CRC24A" if d.A > 3824 else "CRC16", "rv " + c["rv_kind"], f"bg {c['bg']}",
           "core nr" if v.core_form == 1 else "core triangular"}
    if d.Zc % 32 == 0:
        out.add("Zc % 32 == 0")
    if d.C > 1:
        out.add("cw_required, C > 1" if v.cw_required else "C > 1, no cw_required")
    if int(v.rows_needed) < len(g.rows):
        out.add("rows_needed < n_rows")
    if len(g.rows) < E.SHAPE[c["bg"]]["n_rows"]:
        out.add("truncated graph")
    if max(d.E) > d.P:
        out.add("repetition")
    if any(d.f0 <= d.k0[rv] < d.f1 for rv in c["rvs"]):
        out.add("k0[rv] in the fillers")
    if len(set(d.E)) > 1:
        out.add("unequal E_r")
    if c["want_cw"]:
        out.add("cw requested")
    return out


# ---------------------------------------------------------------- modulator ----

MOD_WIDE_GRIDS = [52, 106, 273]
MOD_DMRS = {"T1": Q.T1, "T2": Q.T2, "T1_CDM0": [S.TYPE1_CDM0], "T1_CDM1": [S.TYPE1_CDM1]}
# reserved_re_mask -> the DM-RS combs that lie inside it (ce_mod.h refuses a pilot RE that is a data RE too) with the layers
# each admits.  The masks 0, 0x001 and 0x800 of EQ_MASKS hold no type-1 or type-2 comb: the draw replaces them.
MOD_COMBS = {0xFFF: [("T1", 4), ("T2", 4)], 0x555: [("T1_CDM0", 2)], 0xAAA: [("T1_CDM1", 2)], 0x3CF: [("T2", 4)]}
MOD_MAX_BITS = 150000     # G B of a case: keeps the oracle's bit-serial Gold sequences fast
MOD_TILE_SC = 256


def _mod_data_res(hops, mask):
    free = 12 - bin(mask).count("1")
    return sum(h["n_prbs"] * (12 * (h["n_alloc"] - len(h["dmrs_symbols"])) + free * len(h["dmrs_symbols"])) for h in hops)


def draw_mod(idx):
    """One modulator case.  The geometry is stage_fuzz_cases._eq_geometry's (grid <= 24 PRB); a quarter of the cases put the
    allocation (still <= 24 PRB) at a random prb_start of a 52-, 106- or 273-PRB grid.  What ce_mod.h refuses is drawn away:
    the second hop takes the first one's n_prbs, and a mask without room for a DM-RS comb is replaced by one of the four
    others.  Redrawn while there is no data RE."""
    rng = _rng(STAGE_MOD, idx)
    wide = bool(rng.random() < 0.25)
    while True:
        grid, n_sym, mask, hops = _eq_geometry(rng)
        if wide:
            grid = int(_pick(rng, MOD_WIDE_GRIDS))
        if mask not in MOD_COMBS:
            mask = int(_pick(rng, sorted(MOD_COMBS)))
        for h in hops:
            h["n_prbs"] = hops[0]["n_prbs"]
            if wide or h is not hops[0]:
                h["prb_start"] = int(rng.integers(0, grid - h["n_prbs"] + 1))
        if _mod_data_res(hops, mask) > 0:
            break
    dmrs, l_max = _pick(rng, MOD_COMBS[mask])
    L, qm = int(rng.integers(1, l_max + 1)), int(_pick(rng, [2, 4, 6, 8]))
    G = _mod_data_res(hops, mask) * L * qm
    B = max(1, min(int(rng.integers(1, 7)), MOD_MAX_BITS // G))

    def ident(hi):
        v = rng.integers(0, hi + 1, B)
        edge = rng.random(B)
        return [int(x) for x in np.where(edge < 0.1, 0, np.where(edge < 0.2, hi, v))]

    kind = str(_pick(rng, ["scalar", "tensor", "stride0"]))
    rnti, n_id = ident(65535), ident(1023)
    if kind != "tensor":
        rnti, n_id = [rnti[0]] * B, [n_id[0]] * B
    beta = float(_pick(rng, [1.0, 1.4125, float(np.float32(rng.uniform(0.25, 4.0)))]))
    return dict(stage="mod", idx=idx, n_prb_grid=grid, n_sym=n_sym, hops=hops, mask=mask, dmrs=str(dmrs), L=L, qm=qm, B=B, wide=wide,
                scramble=bool(rng.random() < 0.75), rnti=rnti, n_id=n_id, param_kind=kind, pilots_per_slot=bool(rng.random() < 0.5), beta=beta,
                out_nan=bool(rng.random() < 0.5), slot=int(rng.integers(B)), seed=int(rng.integers(1 << 30)))


def mod_case_spec(c):
    hops = [S.hop_spec(h["dmrs_symbols"], h["prb_start"], h["n_prbs"], h["start_symbol"], h["n_alloc"], re_masks=MOD_DMRS[c["dmrs"]]) for h in c["hops"]]
    return S.case_spec("chain_fuzz", c["n_prb_grid"], hops, n_layers=c["L"], n_sym=c["n_sym"], seed=c["seed"])


def mod_view(c):
    from srsran_ce_pytorch_amd import modulator as MO
    h1, h2, _ = S.numpy_hops(mod_case_spec(c))
    return MO.derive_host(h1, h2, c["L"], c["n_prb_grid"], c["qm"], c["n_sym"], reserved_re_mask=c["mask"], scramble=c["scramble"])


def realize_mod(c):
    """Random bits as packed rows with random bits behind G, pilots with iid normal parts (the beta multiply rounds), one
    tensor for the batch or one per slot, and mod_oracle.modulate_ref of them."""
    case = mod_case_spec(c)
    rng = np.random.default_rng(c["seed"])
    B, L, qm = c["B"], c["L"], c["qm"]
    n_data_re = len(Q.data_re_ref(case, c["mask"]))
    G = n_data_re * L * qm
    g_bits = rng.integers(0, 2, (B, G)).astype(np.uint8)
    hs = dmrs_oracle.hops_of(case)
    n_re, n_cols = int(hs[0][1].sum() * hs[0][2][:, 0].sum()), sum(len(sy) for sy, _, _ in hs)
    shape = ((B,) if c["pilots_per_slot"] else ()) + (n_re, n_cols, L)
    pilots = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    d = SimpleNamespace(c=c, case=case, B=B, L=L, qm=qm, G=G, n_data_re=n_data_re, g_bits=g_bits, g_rows=M.pack(g_bits, 16 * -(-G // 128), rng),
                        pilots=pilots, n_re=n_re, n_cols=n_cols)
    d.ref = M.modulate_ref(case, c["mask"], qm, g_bits, pilots, c["beta"], np.array(c["rnti"]), np.array(c["n_id"]), scramble=c["scramble"])
    return d


def mod_classes(c):
    v = mod_view(c)
    hops, n_sym = c["hops"], c["n_sym"]
    out = {f"Qm {c['qm']}", f"L {c['L']}", "params " + c["param_kind"], "scrambling " + ("on" if c["scramble"] else "off"), "dmrs " + c["dmrs"],
           f"mask 0x{c['mask']:03x}", "pilots per slot" if c["pilots_per_slot"] else "pilots shared",
           "beta " + ("1" if c["beta"] == 1.0 else "1.4125" if c["beta"] == 1.4125 else "drawn")}
    if len(hops) == 2:
        out.add("two hops")
    if hops[0]["start_symbol"] > 0:
        out.add("first hop starts after symbol 0")
    if any(not any(h["start_symbol"] <= s < h["start_symbol"] + h["n_alloc"] for h in hops) for s in range(n_sym)):
        out.add("symbols in no hop")
    if int(v.tiles_per_symbol) > 1:
        out.add("tiles_per_symbol > 1")
    if any(12 * h["prb_start"] // MOD_TILE_SC != (12 * (h["prb_start"] + h["n_prbs"]) - 1) // MOD_TILE_SC for h in hops):
        out.add("an allocation crossing a tile edge")
    if any(12 * h["prb_start"] >= MOD_TILE_SC for h in hops):
        out.add("a tile beyond the first")
    if c["mask"] != 0xFFF:
        out.add("data on DM-RS symbols")
    per_sym = {int(v.data_res_per_prb[s]) * hops[int(v.sym_hop[s])]["n_prbs"] * c["L"] * c["qm"] for s in range(n_sym) if v.sym_hop[s] >= 0}
    if any(n % 32 for n in per_sym):
        out.add("bits per symbol % 32 != 0")
    if c["wide"]:
        out.add("wide grid")
    if c["out_nan"]:
        out.add("out= prefilled with NaN")
    if c["B"] > 1:
        out.add("B > 1")
    for name, hi in (("rnti", 65535), ("n_id", 1023)):
        if c["scramble"] and 0 in c[name]:
            out.add(name + " 0")
        if c["scramble"] and hi in c[name]:
            out.add(f"{name} {hi}")
    return out
