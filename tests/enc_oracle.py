"""Oracle of the transport-block encoder extension (include/ce_enc.h): seeded random graphs whose four core rows have the
NR form (`nr_core_graph`: a dual diagonal plus one weight-3 column), an encoder for them in numpy (`encode_nr`, the lambda
method of ce_enc.h on plain bit arrays; forward substitution where the core is triangular), and the whole forward chain
`transmit` = tb_oracle.segment -> encode_nr -> rm_oracle.slot_map.  Nothing here uses the kernel's forms (periodic column
images, the four-step core program, chunked CRCs, rank / unrank): the CRCs are tb_oracle's, the positions rm_oracle's walk.
Everything is bits; results are compared by value (np.array_equal), without a tolerance.

The base-graph tables of TS 38.212 5.3.2 are not in this repository; the NR-core form is this project's reading of their
shape and nothing here is, or claims to be, a test against them."""
import functools
from types import SimpleNamespace

import numpy as np

import ldpc_oracle as O
import rm_oracle as R
import tb_oracle as T

HOLDERS = {0: (0, 1, 3), 1: (0, 2, 3), 2: (0, 1, 3)}      # variant -> the core rows that hold column n_sys
SHAPE = {1: dict(n_sys=22, n_rows=46, core_degree=16, ext=(3, 9)),      # 16 + 3 core edges: no row exceeds 19
         2: dict(n_sys=10, n_rows=42, core_degree=8, ext=(3, 5))}


def nr_core_graph(rng, n_sys, n_rows, zc, core_degree, ext, variant):
    """ldpc_oracle.random_graph with the four core rows rewritten into the NR core: column n_sys + j (j = 1, 2, 3) in rows
    j - 1 and j at shift 0; column n_sys in rows {0, 1, 3} (variant 0) or {0, 2, 3} (variant 1), the first and the last of
    them at one shift a, the middle one at a shift b drawn independently (so b = a happens too); variant 2 is variant 0
    with b = a always.  The systematic edges and the extension rows are random_graph's."""
    rows = [list(row) for row in O.random_graph(rng, n_sys, n_rows, zc, core_degree, ext)]
    a, b = int(rng.integers(zc)), int(rng.integers(zc))
    if variant == 2:
        b = a
    hold = HOLDERS[variant]
    for i in range(4):
        row = [(c, s) for c, s in rows[i] if c < n_sys]
        if i in hold:
            row.append((n_sys, b if i == hold[1] else a))
        if i >= 1:
            row.append((n_sys + i, 0))
        if i <= 2:
            row.append((n_sys + i + 1, 0))
        assert len(row) <= O.MAX_ROW_DEGREE
        rows[i] = row
    return rows


def _rot(x, s):
    """x[..., (z + s) mod zc]: what an edge (c, s) contributes, as in ldpc_oracle._vars."""
    return np.roll(x, -s, axis=-1)


def is_triangular(rows, n_sys):
    return all((n_sys + i, 0) in rows[i] and all(c <= n_sys + i for c, _ in rows[i]) and sum(c == n_sys + i for c, _ in rows[i]) == 1
               for i in range(min(4, len(rows))))


def encode_nr(rows, n_sys, zc, info):
    """Codeword [nb, (n_sys + n_rows) zc] of info[nb, n_sys zc].  Core: with lambda_i the XOR of row i's rotated systematic
    columns, the sum of the four rows leaves column n_sys rotated by the one shift that does not cancel; rows 0, 1, 2 then
    give columns n_sys + 1, + 2, + 3.  A triangular core is solved row by row.  Rows >= 4 end with their own column."""
    info = np.asarray(info, np.int64)
    nb, n_rows = info.shape[0], len(rows)
    col = [info[:, c * zc:(c + 1) * zc] for c in range(n_sys)] + [None] * n_rows

    def row_sum(r, skip):
        acc = np.zeros((nb, zc), np.int64)
        for c, s in rows[r]:
            if c not in skip:
                acc ^= _rot(col[c], s)
        return acc

    if is_triangular(rows, n_sys):
        first_ext = 0
    else:
        core = set(range(n_sys, n_sys + 4))
        lam = [row_sum(i, core) for i in range(4)]
        shifts = [s for i in range(4) for c, s in rows[i] if c == n_sys]
        assert len(shifts) == 3
        left = [s for s in shifts if shifts.count(s) % 2 == 1]       # the equal pair cancels; three equal leave one
        rem = left[0]
        col[n_sys] = _rot(lam[0] ^ lam[1] ^ lam[2] ^ lam[3], -rem)     # rot(p0, rem) = the sum  =>  p0 = the sum rotated back
        for j in (1, 2, 3):                                            # row j - 1: everything but column n_sys + j is known
            col[n_sys + j] = row_sum(j - 1, {n_sys + j})
        first_ext = 4
    for r in range(first_ext, n_rows):
        assert sum(c == n_sys + r for c, _ in rows[r]) == 1 and (n_sys + r, 0) in rows[r]
        col[n_sys + r] = row_sum(r, {n_sys + r})
    return np.concatenate(col, axis=1)


def transmit(d, graph, tb_bits, rvs):
    """(g bits [S, G], codewords [S, C, n_cols Zc]) of tb_bits[S, A] under one rv per slot: segment, fill to K with zeros,
    encode, and read every bit of the slot's row where rm_oracle.slot_map says it comes from."""
    tb_bits = np.asarray(tb_bits, np.uint8)
    S = tb_bits.shape[0]
    blocks = T.segment(tb_bits, d.bg).reshape(S, d.C, d.Kp)
    info = np.zeros((S, d.C, d.K), np.int64)
    info[:, :, :d.Kp] = blocks
    assert graph.zc == d.Zc and graph.n_sys * graph.zc == d.K and (graph.n_cols - 2) * graph.zc >= d.N_cb
    cw = encode_nr(graph.rows, graph.n_sys, graph.zc, info.reshape(S * d.C, d.K)).reshape(S, d.C, -1)
    g = np.empty((S, d.G), np.uint8)
    for b in range(S):
        blk, pos, _ = R.slot_map(d, int(rvs[b]))
        g[b] = cw[b, blk, pos + 2 * d.Zc]
    return g, cw.astype(np.uint8)


# ---- the pinned cases ----

def enc_case(name, bg, A, qm, L, G, zc, form, n_ref=0, n_rows=None, slots=3, **pinned):
    """form: 0 / 1 / 2 = nr_core_graph's variant, "tri" = ldpc_oracle.random_graph as it is."""
    pinned["Zc"] = zc
    return dict(name=name, bg=bg, A=A, qm=qm, L=L, G=G, zc=zc, form=form, n_ref=n_ref, n_rows=n_rows, slots=slots, pinned=pinned)


CASES = [
    enc_case("bg1_z2", 1, 24, 2, 1, 120, 2, 0, C=1, Kp=40, K=44, N_cb=132),                                   # sub-dword columns
    enc_case("bg2_z7_rep", 2, 24, 2, 1, 480, 7, 1, C=1, K_b=6, N_cb=350, f0=26, f1=56, P=320),                # G > P: repetition
    enc_case("bg2_z7_rep3", 2, 24, 2, 1, 1200, 7, 2, slots=2, C=1, k0=(0, 91, 175, 301)),                     # G > 2 N_cb; three equal shifts
    enc_case("bg2_z7_tri", 2, 24, 2, 1, 480, 7, "tri", C=1),                                                  # a triangular core
    enc_case("bg1_z6_k0_in_filler", 1, 96, 4, 1, 240, 6, 0, f0=100, f1=120, k0=(0, 102, 198, 336)),           # rv 1 starts inside the fillers
    enc_case("bg1_z15", 1, 300, 2, 1, 600, 15, 1, C=1, Kp=316),                                               # odd Zc
    enc_case("bg1_z15_rows12", 1, 300, 4, 1, 400, 15, 0, n_ref=480, n_rows=12, N_cb=480),                     # a truncated graph, limited buffer
    enc_case("bg2_z36_kb8", 2, 256, 2, 1, 512, 36, 0, C=1, K_b=8, Kp=272, K=360),                             # just over 32; filler columns
    enc_case("bg2_z72_kb9", 2, 600, 6, 1, 1200, 72, 1, C=1, K_b=9, Kp=616),
    enc_case("bg2_z104_kb10", 2, 1000, 2, 2, 2000, 104, 0, C=1, K_b=10, Kp=1016),
    enc_case("bg1_crc16_top", 1, 3824, 2, 1, 6000, 176, 0, slots=2, C=1, B=3840),                             # the last CRC16 size
    enc_case("bg1_crc24_first", 1, 3825, 2, 1, 6000, 176, 1, slots=2, C=1, B=3849),                           # the first CRC24A size
    enc_case("bg2_z208_c2", 2, 3848, 4, 2, 12000, 208, 0, slots=2, C=2, E=[6000, 6000]),                      # the blocks meet inside a dword
    enc_case("bg2_z208_c2_aligned", 2, 3848, 2, 1, 12032, 208, 1, slots=2, C=2, E=[6016, 6016]),              # ... at a dword boundary: one launch
    enc_case("bg1_z208_c2", 1, 8448, 2, 1, 24000, 208, 1, slots=2, C=2, Kp=4260, N_cb=13728),
    enc_case("bg1_z208_lbrm", 1, 8448, 4, 3, 16812, 208, 0, n_ref=9000, slots=2, C=2, N_cb=9000, P=8684, E=[8400, 8412]),
    enc_case("bg2_z352_c5", 2, 16976, 2, 1, 30006, 352, 0, slots=2, C=5, Kp=3424, E=[6000, 6000, 6002, 6002, 6002]),   # unequal E_r
    enc_case("bg1_z384_c9", 1, 71976, 2, 1, 108008, 384, 1, slots=2, C=9, B=72000, Kp=8024, E=[12000] * 5 + [12002] * 4),       # A > 2 * 32768: three CRC chunks
    enc_case("bg1_z384", 1, 8424, 2, 1, 10000, 384, 0, slots=2, C=1, Kp=8448, K=8448, N_cb=25344),            # the largest Zc, no fillers, G < N_cb
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
# the shapes of the whole loop encoder -> LLRs -> rate recovery -> decoder -> assembly (CPU: tests/test_enc.py, from the oracles alone)
LOOPS = {"bg2_z7_rep": dict(bg=2, A=24, qm=2, L=1, G=480, pinned=dict(Zc=7, K_b=6)),
         "bg2_z208_c2": dict(bg=2, A=3848, qm=4, L=2, G=12000, pinned=dict(C=2, Zc=208)),
         "bg1_z208_c2": dict(bg=1, A=8448, qm=2, L=1, G=24000, pinned=dict(C=2, Zc=208))}


@functools.lru_cache(maxsize=None)
def case_derive(name):
    c = CASE_BY_NAME[name]
    d = R.derive(c["bg"], c["A"], c["qm"], c["L"], c["G"], c["n_ref"])
    for k, v in c["pinned"].items():
        assert getattr(d, k) == v, (name, k, getattr(d, k))
    return d


@functools.lru_cache(maxsize=None)
def graph(name):
    """SimpleNamespace(rows, n_cols, n_sys, zc) of a named case; shared, do not modify."""
    c = CASE_BY_NAME[name]
    sh = SHAPE[c["bg"]]
    rng = np.random.default_rng(12000 + CASES.index(c))
    if c["form"] == "tri":
        rows = O.random_graph(rng, sh["n_sys"], sh["n_rows"], c["zc"], sh["core_degree"], sh["ext"])
    else:
        rows = nr_core_graph(rng, sh["n_sys"], sh["n_rows"], c["zc"], sh["core_degree"], sh["ext"], c["form"])
    if c["n_rows"]:
        rows = rows[:c["n_rows"]]
    return SimpleNamespace(name=name, rows=rows, n_cols=sh["n_sys"] + len(rows), n_sys=sh["n_sys"], zc=c["zc"])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(tb_bits[S, A], the packed tb rows with random bits behind A) of a named case; shared and read-only."""
    c, d = CASE_BY_NAME[name], case_derive(name)
    rng = np.random.default_rng(13000 + CASES.index(c))
    tb_bits = rng.integers(0, 2, (c["slots"], d.A)).astype(np.uint8)
    row_bytes = 16 * -(-d.A // 128)
    noise = rng.integers(0, 2, (c["slots"], row_bytes * 8)).astype(np.uint8)
    noise[:, :d.A] = tb_bits
    return _frozen(tb_bits, np.packbits(noise, axis=-1))


def rvs_of(name, shift):
    """One rv per slot; shift = 0 .. 3 brings every rv to every slot."""
    return [(b + shift) & 3 for b in range(CASE_BY_NAME[name]["slots"])]


@functools.lru_cache(maxsize=None)
def reference(name, shift):
    """(g rows [S, 16 ceil(G / 128)], cw rows [S, C, 16 ceil(n_cols Zc / 128)]) packed, under rvs_of(name, shift)."""
    d, gr = case_derive(name), graph(name)
    g, cw = transmit(d, gr, inputs(name)[0], rvs_of(name, shift))
    return _frozen(T.pack(g, 16 * -(-d.G // 128)), T.pack(cw, 16 * -(-cw.shape[-1] // 128)))
