"""Oracle of the LDPC decoder extension (include/ce_ldpc.h): the layered normalised min-sum operator restated in numpy
int64 (`decode_ref`, vectorised over the blocks of a batch and over z, never over rows or edges; `decode_loop`, the same as
plain Python loops over (r, z, e) for one block), the quantiser, seeded random graphs of the NR shape with their
forward-substitution encoder, and the pinned cases the CPU and GPU tests share.  All arithmetic is integer: results are
compared by value (np.array_equal), without a tolerance.

The base-graph tables of TS 38.212 5.3.2 are not in this repository; nothing here is, or claims to be, a test against them."""
import functools
from types import SimpleNamespace

import numpy as np

MAX_ROW_DEGREE, L_BOUND = 19, 4497


def quantise(x, scale=1.0):
    """q of include/ce_ldpc.h as int64: int8 -> the value, -128 taken as -127; float32 -> one float32 multiplication by
    `scale`, NaN -> 0, clamp to [-127, 127], round half to even."""
    x = np.asarray(x)
    if x.dtype == np.int8:
        return np.maximum(x.astype(np.int64), -127)
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(scale)
    assert v.dtype == np.float32
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.clip(v, np.float32(-127), np.float32(127))).astype(np.int64)


def channel(q, n_cols, zc, n_punct):
    """ch[nb, n_cols zc] from the quantised input rows q[nb, n_in]."""
    ch = np.zeros((q.shape[0], n_cols * zc), np.int64)
    ch[:, n_punct * zc: n_punct * zc + q.shape[1]] = q
    return ch


def _vars(rows, zc):
    z = np.arange(zc)
    return [np.stack([c * zc + (z + s) % zc for c, s in row]) for row in rows]      # per row: [degree, zc]


def syndrome(rows, zc, bits):
    """[..., n_rows, zc]: XOR of the bits of every lifted check."""
    bits = np.asarray(bits).astype(np.int64)
    return np.stack([bits[..., v].sum(-2) & 1 for v in _vars(rows, zc)], axis=-2)


def decode_ref(rows, n_cols, zc, ch, max_iters, early_stop):
    """The operator of include/ce_ldpc.h on ch[nb, n_cols zc] (int64).  Returns L[nb, n_cols zc], status[nb, 2] and the
    final R per row ([nb, degree, zc]) for the identity L = ch + sum R."""
    ch = np.asarray(ch, np.int64)
    nb = ch.shape[0]
    var = _vars(rows, zc)
    L = ch.copy()
    R = [np.zeros((nb, len(row), zc), np.int64) for row in rows]
    status = np.zeros((nb, 2), np.int64)
    alive = np.ones(nb, bool)
    for it in range(1, max_iters + 1):
        act = np.flatnonzero(alive)
        if act.size == 0:
            break
        for r, v in enumerate(var):
            t = L[act][:, v] - R[r][act]                                   # [na, degree, zc]
            s = t < 0
            a = np.minimum(np.abs(t), 127)
            two = np.sort(a, axis=1)[:, :2]
            min1, min2 = two[:, 0], two[:, 1]
            idx = np.argmin(a, axis=1)
            sgn = np.logical_xor.reduce(s, axis=1)
            own = np.arange(len(v))[None, :, None] == idx[:, None, :]
            m = (3 * np.where(own, min2[:, None, :], min1[:, None, :])) >> 2
            rn = np.where(sgn[:, None, :] ^ s, -m, m)
            R[r][act] = rn
            L[act[:, None, None], v[None]] = t + rn                         # a row's variables are distinct
        if early_stop or it == max_iters:
            ok = ~syndrome(rows, zc, L[act] < 0).any(axis=(-1, -2))
            stop = ok | (it == max_iters)
            status[act[stop], 0] = it
            status[act[stop], 1] = ok[stop]
            alive[act[stop]] = False
    return L, status, R


def decode_loop(rows, n_cols, zc, ch, max_iters, early_stop):
    """decode_ref for ONE block ch[n_cols zc] as plain Python loops over (r, z, e); ties take the first edge."""
    L = [int(x) for x in ch]
    R = [[[0] * zc for _ in row] for row in rows]
    for it in range(1, max_iters + 1):
        for r, row in enumerate(rows):
            for z in range(zc):
                var = [c * zc + (z + s) % zc for c, s in row]
                t = [L[v] - R[r][e][z] for e, v in enumerate(var)]
                a = [min(abs(x), 127) for x in t]
                idx = min(range(len(row)), key=lambda e: (a[e], e))
                min1 = a[idx]
                min2 = min(a[e] for e in range(len(row)) if e != idx)
                sgn = 0
                for x in t:
                    sgn ^= x < 0
                for e, v in enumerate(var):
                    m = (3 * (min2 if e == idx else min1)) >> 2
                    R[r][e][z] = -m if sgn ^ (t[e] < 0) else m
                    L[v] = t[e] + R[r][e][z]
        if early_stop or it == max_iters:
            ok = all(sum(L[c * zc + (z + s) % zc] < 0 for c, s in row) % 2 == 0 for row in rows for z in range(zc))
            if ok or it == max_iters:
                return np.array(L, np.int64), np.array([it, int(ok)], np.int64)
    raise AssertionError("unreachable")


def pack(L, k_out):
    """hard[nb, 16 ceil(k_out / 128)] uint8 of include/ce_ldpc.h from L[nb, >= k_out]: MSB first, padding 0."""
    row_bytes = 16 * -(-k_out // 128)
    bits = np.zeros((L.shape[0], row_bytes * 8), np.uint8)
    bits[:, :k_out] = L[:, :k_out] < 0
    return np.packbits(bits, axis=-1)


def random_graph(rng, n_sys, n_rows, zc, core_degree, ext_degree_range):
    """Rows of (col, shift) over n_sys + n_rows columns in the NR shape.  Rows 0-3 (the core): `core_degree` random
    systematic columns, the row's parity column n_sys + i at shift 0 and, for i >= 1, column n_sys + i - 1 at a random
    shift.  Rows >= 4: a random draw of columns < n_sys + 4 and the row's own parity column at shift 0 (degree 1)."""
    rows = []
    for i in range(n_rows):
        if i < 4:
            cols = sorted(rng.choice(n_sys, core_degree, replace=False).tolist())
            row = [(c, int(rng.integers(zc))) for c in cols]
            if i >= 1:
                row.append((n_sys + i - 1, int(rng.integers(zc))))
        else:
            d = int(rng.integers(ext_degree_range[0], ext_degree_range[1] + 1))
            cols = sorted(rng.choice(n_sys + 4, d, replace=False).tolist())
            row = [(c, int(rng.integers(zc))) for c in cols]
        row.append((n_sys + i, 0))
        assert 2 <= len(row) <= MAX_ROW_DEGREE
        rows.append(row)
    return rows


def encode(rows, n_sys, zc, info):
    """Codeword [nb, (n_sys + n_rows) zc] of info[nb, n_sys zc] by forward substitution: row r ends with its own parity
    column n_sys + r at shift 0 and touches earlier columns only."""
    info = np.asarray(info, np.int64)
    cw = np.zeros((info.shape[0], (n_sys + len(rows)) * zc), np.int64)
    cw[:, :n_sys * zc] = info
    z = np.arange(zc)
    for r, row in enumerate(rows):
        assert row[-1] == (n_sys + r, 0) and all(c < n_sys + r for c, _ in row[:-1])
        p = np.zeros((info.shape[0], zc), np.int64)
        for c, s in row[:-1]:
            p ^= cw[:, c * zc + (z + s) % zc]
        cw[:, (n_sys + r) * zc: (n_sys + r + 1) * zc] = p
    return cw


def noisy_llr(rng, bits, esn0_db, scale=8.0):
    """int8 LLRs of BPSK over AWGN: y = 1 - 2 b + n, LLR = 2 y / sigma^2, times `scale`, rounded and clamped to +-127."""
    sigma2 = 1.0 / (2.0 * 10.0 ** (esn0_db / 10.0))
    y = 1.0 - 2.0 * bits + rng.standard_normal(bits.shape) * np.sqrt(sigma2)
    return np.clip(np.rint(2.0 * y / sigma2 * scale), -127, 127).astype(np.int8)


# ---- the pinned cases ----

TINY_ROWS = [[(0, 1), (2, 0)], [(1, 1), (3, 0)]]            # 2 rows x 4 columns, degree 2, at zc = 2
ESN0_DB, SCALE = 1.0, 8.0                                    # the noisy codewords: rate 1/3, int8 scale 8


def case(name, bg, zc, seed, n_rows=None, n_punct=2, esn0_db=ESN0_DB):
    return dict(name=name, bg=bg, zc=zc, seed=seed, n_rows=n_rows, n_punct=n_punct, esn0_db=esn0_db)


CASES = [
    case("tiny_z2", 0, 2, 0, n_punct=1),
    case("bg2_z7", 2, 7, 11), case("bg2_z36", 2, 36, 12), case("bg2_z64", 2, 64, 13), case("bg2_z72", 2, 72, 14),
    case("bg1_z15", 1, 15, 21), case("bg1_z208", 1, 208, 22), case("bg1_z384", 1, 384, 23),
    case("bg1_z15_rows12", 1, 15, 21, n_rows=12, esn0_db=5.0),      # 22 / 32: a high rate needs the higher Es/N0
    case("bg2_z7_nopunct", 2, 7, 11, n_punct=0),
    case("bg2_z8", 2, 8, 15),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
CODEWORD_CASES = [c["name"] for c in CASES if c["bg"]]
SMALL_CASES = ["tiny_z2", "bg2_z7", "bg1_z15_rows12", "bg2_z7_nopunct"]      # where decode_loop is affordable
SHAPE = {1: dict(n_sys=22, n_rows=46, core_degree=17, ext=(3, 9)),           # rows 1-3 have 19 edges
         2: dict(n_sys=10, n_rows=42, core_degree=8, ext=(3, 5))}


@functools.lru_cache(maxsize=None)
def graph(name):
    """SimpleNamespace(rows, n_cols, n_sys, zc, n_punct, n_in, k_out) of a named case; shared, do not modify."""
    c = CASE_BY_NAME[name]
    if c["bg"] == 0:
        rows, n_sys = TINY_ROWS, 2
    else:
        sh = SHAPE[c["bg"]]
        n_sys = sh["n_sys"]
        rows = random_graph(np.random.default_rng(c["seed"]), n_sys, sh["n_rows"], c["zc"], sh["core_degree"], sh["ext"])
        if c["n_rows"]:
            rows = rows[:c["n_rows"]]
    n_cols = n_sys + len(rows)
    return SimpleNamespace(name=name, rows=rows, n_cols=n_cols, n_sys=n_sys, zc=c["zc"], n_punct=c["n_punct"],
                           n_in=(n_cols - c["n_punct"]) * c["zc"], k_out=n_sys * c["zc"], n_bits=n_cols * c["zc"])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def random_inputs(name, nb=3):
    """int8 rows over the full range (-128 included): not codewords, so most never converge."""
    g = graph(name)
    rng = np.random.default_rng(5000 + CASES.index(CASE_BY_NAME[name]))
    return _frozen(rng.integers(-128, 128, (nb, g.n_in)).astype(np.int8))[0]


@functools.lru_cache(maxsize=None)
def codeword_inputs(name, nb=3):
    """(info bits [nb, n_sys zc], int8 LLR rows [nb, n_in]) of noisy codewords."""
    g = graph(name)
    rng = np.random.default_rng(6000 + CASES.index(CASE_BY_NAME[name]))
    info = rng.integers(0, 2, (nb, g.n_sys * g.zc))
    cw = encode(g.rows, g.n_sys, g.zc, info)
    llr = noisy_llr(rng, cw[:, g.n_punct * g.zc:], CASE_BY_NAME[name]["esn0_db"], SCALE)
    return _frozen(info, llr)


MIXED_CASES = ["bg2_z7", "bg2_z36", "bg1_z15"]


@functools.lru_cache(maxsize=None)
def mixed_inputs(name):
    """One batch where neighbouring blocks stop at different iterations: an all-zero row (stops at 1), a clean codeword,
    noisy codewords at three noise levels and random rows, interleaved twice over."""
    g = graph(name)
    rng = np.random.default_rng(7000 + CASES.index(CASE_BY_NAME[name]))
    info = rng.integers(0, 2, (4, g.n_sys * g.zc))
    tx = encode(g.rows, g.n_sys, g.zc, info)[:, g.n_punct * g.zc:]
    rows = [np.zeros(g.n_in, np.int8), noisy_llr(rng, tx[0], 40.0, 1.0), rng.integers(-128, 128, g.n_in).astype(np.int8),
            noisy_llr(rng, tx[1], 3.0, SCALE), noisy_llr(rng, tx[2], 1.0, SCALE), rng.integers(-128, 128, g.n_in).astype(np.int8),
            noisy_llr(rng, tx[3], -2.5, SCALE)]
    order = [0, 2, 3, 4, 1, 5, 6, 4, 0, 3, 5, 1, 6, 2, 3]
    return _frozen(np.stack([rows[i] for i in order]))[0]


@functools.lru_cache(maxsize=None)
def reference(name, kind, max_iters, early_stop):
    """(L, status, hard) of decode_ref for the named case's inputs of `kind` ("random", "codeword", "mixed"); shared."""
    g = graph(name)
    llr = {"random": random_inputs, "mixed": mixed_inputs, "codeword": lambda n: codeword_inputs(n)[1]}[kind](name)
    L, status, _ = decode_ref(g.rows, g.n_cols, g.zc, channel(quantise(llr), g.n_cols, g.zc, g.n_punct), max_iters, early_stop)
    return _frozen(L, status, pack(L, g.k_out))


# ---- the packing of the kernel's per-check state (include/ce_ldpc.h), restated ----

IDX_SHIFT, MAG_SHIFT = 19, 24


def state_pack(neg_bits, idx, m1, m2):
    return (neg_bits | (idx << IDX_SHIFT) | (m1 << MAG_SHIFT)).astype(np.uint32), m2.astype(np.uint8)


def state_unpack(word, byte, degree):
    """R_e of every edge e < degree from the 5 bytes."""
    word, byte = word.astype(np.int64), byte.astype(np.int64)
    e = np.arange(degree)[:, None]
    m = np.where(e == ((word >> IDX_SHIFT) & 31)[None], byte[None], (word >> MAG_SHIFT)[None])
    return np.where((word[None] >> e) & 1, -m, m)


# ---- the chain behind rate recovery (tests/rm_oracle.py) ----

CHAINS = {"bg2": dict(bg=2, A=24, qm=2, L=1, G=480, graph="bg2_z7", pinned=dict(Zc=7, N_cb=350, f0=26, f1=56, C=1, Kp=40)),
          "bg1_c2": dict(bg=1, A=8448, qm=2, L=1, G=24000, graph="bg1_z208", pinned=dict(Zc=208, N_cb=13728, C=2, Kp=4260))}
CHAIN_SLOTS = 2


@functools.lru_cache(maxsize=None)
def chain_inputs(which):
    """K' random bits plus zero fillers per code block, encoded with the named random graph, placed at the transmitted
    positions of rv 0 and rv 2 through rm_oracle.slot_map and turned into noisy int8 LLR rows [slots, G]; with the rate
    recovery's expected soft buffers (rm_oracle.recover) for rv 0 alone and for rv 0 then rv 2 combined."""
    import rm_oracle as R
    c = CHAINS[which]
    d = R.derive(c["bg"], c["A"], c["qm"], c["L"], c["G"])
    for k, v in c["pinned"].items():
        assert getattr(d, k) == v, (which, k, getattr(d, k))
    g = graph(c["graph"])
    assert g.zc == d.Zc and g.n_sys * g.zc == d.K and (g.n_cols - 2) * g.zc == d.N_cb
    rng = np.random.default_rng(8000 + sorted(CHAINS).index(which))
    info = np.zeros((CHAIN_SLOTS, d.C, d.K), np.int64)
    info[:, :, :d.Kp] = rng.integers(0, 2, (CHAIN_SLOTS, d.C, d.Kp))
    cw = encode(g.rows, g.n_sys, g.zc, info.reshape(-1, d.K)).reshape(CHAIN_SLOTS, d.C, -1)
    x = SimpleNamespace(c=c, d=d, g=g, bits=info[:, :, :d.Kp].astype(np.uint8), llr={}, soft={})
    for rv in (0, 2):
        blk, pos, _ = R.slot_map(d, rv)
        x.llr[rv] = np.ascontiguousarray(noisy_llr(rng, cw[:, blk, pos + 2 * d.Zc], ESN0_DB, SCALE))
    x.soft[(0,)], _ = R.recover(d, x.llr[0], [0] * CHAIN_SLOTS)
    x.soft[(0, 2)], _ = R.recover(d, x.llr[2], [2] * CHAIN_SLOTS, harq=x.soft[(0,)])
    _frozen(x.bits, *x.llr.values(), *x.soft.values())
    return x
