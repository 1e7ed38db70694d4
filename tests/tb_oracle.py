"""Oracle of the transport-block assembly extension (include/ce_tb.h): the CRCs of TS 38.212 5.1 as the bit-serial
division (`crc_bits`) and as a 16-bit-table form vectorised over a batch (`crc_fast`), 5.1 / 5.2.2 forward (`segment`: attach
the transport-block CRC, split, attach CRC24B per block -- no filler bits, the decoder outputs K' bits only), and the
inverse the kernel computes restated twice: `assemble_ref` on plain bit arrays, `assemble_loop` as a literal per-bit loop.
Nothing here uses the kernel's closed form (chunk residues advanced by powers of x): every residue is the CRC of a whole
bit string, a block's share t_r the CRC of the stream with every other block zeroed.  All arithmetic is integer; results
are compared by value (np.array_equal), without a tolerance."""
import functools
from types import SimpleNamespace

import numpy as np

import rm_oracle as R

POLY = {"24A": (0x864CFB, 24), "24B": (0x800063, 24), "16": (0x1021, 16)}
CHECK = {"24A": 0xCDE703, "24B": 0x23EF52, "16": 0x31C3}            # of the nine bytes "123456789" (the catalogue values)
CHECK_BITS = np.unpackbits(np.frombuffer(b"123456789", np.uint8))


def crc_bits(bits, which):
    """5.1, literal: the remainder of bits(x) x^L divided by g, one bit at a time, MSB first, from a zero register."""
    g, L = POLY[which]
    reg = 0
    for b in bits:
        top = ((reg >> (L - 1)) & 1) ^ int(b)
        reg = (reg << 1) & ((1 << L) - 1)
        if top:
            reg ^= g
    return reg


@functools.lru_cache(maxsize=None)
def _table16(which):
    g, L = POLY[which]
    reg = np.arange(1 << 16, dtype=np.int64) << (L - 16)
    for _ in range(16):
        reg = ((reg << 1) & ((1 << L) - 1)) ^ np.where((reg >> (L - 1)) & 1, g, 0)
    return reg


def _words(bits):
    """bits[..., n] -> big-endian uint16 words [..., ceil(n / 16)].  Leading zeros leave a zero register where it is, so
    the string is padded in FRONT."""
    bits = np.asarray(bits, np.uint8)
    pad = -bits.shape[-1] % 16
    if pad:
        bits = np.concatenate([np.zeros(bits.shape[:-1] + (pad,), np.uint8), bits], axis=-1)
    by = np.packbits(bits, axis=-1).astype(np.uint16)
    return (by[..., 0::2] << 8) | by[..., 1::2]


def _crc_words(words, which):
    """The CRC of each row of words[batch, n] (uint16), 16 bits per step from a 65536-entry table."""
    g, L = POLY[which]
    tab, mask = _table16(which), (1 << L) - 1
    reg = np.zeros(words.shape[0], np.int64)
    for w in np.ascontiguousarray(words.T):
        reg = ((reg << 16) & mask) ^ tab[((reg >> (L - 16)) ^ w) & 0xFFFF]
    return reg


def crc_fast(bits, which):
    """crc_bits over the last axis of bits[..., n], vectorised over the leading axes."""
    bits = np.asarray(bits, np.uint8)
    words = _words(bits)
    return _crc_words(words.reshape(-1, words.shape[-1]), which).reshape(bits.shape[:-1])


def _to_bits(value, L):
    return np.array([(value >> (L - 1 - i)) & 1 for i in range(L)], np.uint8)


def derive(bg, A):
    """Every integer of include/ce_tb.h; the segmentation comes from rm_oracle.derive (QPSK, one layer, 8192 LLRs: values
    that do not enter it)."""
    d = R.derive(bg, A, 2, 1, 8192)
    which = "24A" if A > 3824 else "16"
    L_tb = POLY[which][1]
    L_cb = 24 if d.C > 1 else 0
    assert d.B == A + L_tb and (d.Kp - L_cb) * d.C == d.B
    return SimpleNamespace(bg=bg, A=A, B=d.B, K_cb=d.K_cb, C=d.C, Bp=d.Bp, Kp=d.Kp, which=which, L_tb=L_tb, g_tb=POLY[which][0], L_cb=L_cb,
                           g_cb=POLY["24B"][0], P=d.Kp - L_cb, in_row_bytes=16 * -(-d.Kp // 128), tb_row_bytes=16 * -(-A // 128))


def segment(tb_bits, bg):
    """5.1 and 5.2.2 forward: tb_bits[..., A] -> code blocks [..., C, K'] (payload, then CRC24B when C > 1)."""
    tb_bits = np.asarray(tb_bits, np.uint8)
    d = derive(bg, tb_bits.shape[-1])
    lead = tb_bits.shape[:-1]
    crc = crc_fast(tb_bits, d.which)
    par = ((crc[..., None] >> (d.L_tb - 1 - np.arange(d.L_tb))) & 1).astype(np.uint8)
    s = np.concatenate([tb_bits, par], axis=-1).reshape(lead + (d.C, d.P))
    if d.C == 1:
        return s
    cb = crc_fast(s, "24B")
    par = ((cb[..., None] >> (23 - np.arange(24))) & 1).astype(np.uint8)
    return np.concatenate([s, par], axis=-1)


def pack(bits, row_bytes):
    """bits[..., n] of 0 / 1 -> uint8 [..., row_bytes], MSB first, zero padding."""
    bits = np.asarray(bits, np.uint8)
    out = np.zeros(bits.shape[:-1] + (row_bytes * 8,), np.uint8)
    out[..., :bits.shape[-1]] = bits
    return np.packbits(out, axis=-1)


def assemble_ref(hard_rows, d):
    """(tb[S, tb_row_bytes] uint8, tb_status[S, 2], cb_status[S, C, 2] int32) of include/ce_tb.h for
    hard_rows[S, C, in_row_bytes]; bits >= K' of a row are dropped before anything looks at them."""
    hard_rows = np.asarray(hard_rows, np.uint8)
    S = hard_rows.shape[0]
    assert hard_rows.shape == (S, d.C, d.in_row_bytes)
    bits = np.unpackbits(hard_rows, axis=-1)[..., :d.Kp]
    s = bits[..., :d.P].reshape(S, d.B)
    tb = pack(s[:, :d.A], d.tb_row_bytes)
    tb_res = crc_fast(s, d.which)
    cb = np.zeros((S, d.C, 2), np.int64)
    cb[..., 0] = crc_fast(bits, "24B") if d.C > 1 else tb_res[:, None]
    alone = np.zeros(d.B, np.uint8)                      # t_r: the CRC of the stream with every block but r zeroed
    words = np.empty((S, d.C, -(-d.B // 16)), np.uint16)
    for b in range(S):
        for r in range(d.C):
            alone[r * d.P:(r + 1) * d.P] = bits[b, r, :d.P]
            words[b, r] = _words(alone)
            alone[r * d.P:(r + 1) * d.P] = 0
    cb[..., 1] = _crc_words(words.reshape(S * d.C, -1), d.which).reshape(S, d.C)
    status = np.stack([tb_res, (cb[..., 0] != 0).sum(-1)], axis=-1)
    return tb, status.astype(np.int32), cb.astype(np.int32)


def assemble_loop(hard_rows, d):
    """assemble_ref as plain Python loops over single bits (small cases only)."""
    S = len(hard_rows)
    tb = np.zeros((S, d.tb_row_bytes), np.uint8)
    status = np.zeros((S, 2), np.int32)
    cb = np.zeros((S, d.C, 2), np.int32)
    for b in range(S):
        bit = lambda r, i: (int(hard_rows[b][r][i // 8]) >> (7 - i % 8)) & 1      # noqa: E731
        s = []
        for r in range(d.C):
            block = [bit(r, i) for i in range(d.Kp)]
            s += block[:d.P]
            cb[b, r, 1] = crc_bits(block[:d.P] + [0] * ((d.C - 1 - r) * d.P), d.which)
            if d.C > 1:
                cb[b, r, 0] = crc_bits(block, "24B")
        assert len(s) == d.B
        status[b, 0] = crc_bits(s, d.which)
        if d.C == 1:
            cb[b, 0, 0] = status[b, 0]
        status[b, 1] = sum(int(cb[b, r, 0] != 0) for r in range(d.C))
        for i in range(d.A):
            tb[b, i // 8] |= s[i] << (7 - i % 8)
    return tb, status, cb


# ---- the pinned cases ----

def tb_case(name, bg, A, slots=3, **pinned):
    return dict(name=name, bg=bg, A=A, slots=slots, pinned=pinned)


CASES = [
    tb_case("c1_tiny", 2, 24, C=1, which="16", Kp=40, P=40, in_row_bytes=16, tb_row_bytes=16),       # one partly filled chunk
    tb_case("c1_8bit", 2, 8, C=1, which="16", Kp=24, P=24),                                          # the smallest byte-sized block
    tb_case("c1_odd", 2, 13, C=1, which="16", Kp=29, P=29),                                          # A no multiple of 8
    tb_case("c1_crc16_top", 2, 3824, C=1, which="16", B=3840, Kp=3840, K_cb=3840),                   # the last CRC16 size, B = K_cb
    tb_case("c2_crc24_first", 2, 3832, C=2, which="24A", Kp=1952, P=1928),                           # the first CRC24A size; C = 2 on BG2
    tb_case("c1_bg1_same", 1, 3832, C=1, which="24A", Kp=3856, P=3856),                              # the same A with C = 1 on BG1
    tb_case("c1_max", 1, 8424, C=1, which="24A", Kp=8448, P=8448, in_row_bytes=1056),                # 66 chunks: more than one per lane
    tb_case("c2_bits", 1, 8448, C=2, which="24A", Kp=4260, P=4236),                                  # P mod 32 = 12: a boundary 12 bits into a dword
    tb_case("c2_bytes", 1, 8472, C=2, which="24A", Kp=4272, P=4248),                                 # P = 531 bytes: 3 bytes into a dword
    tb_case("c5_bytes", 2, 16976, C=5, which="24A", Kp=3424, P=3400),
    tb_case("c5_bits", 2, 16981, C=5, which="24A", Kp=3425, P=3401),                                 # every boundary at another bit offset
    tb_case("c152", 1, 1277992, slots=2, C=152, which="24A", Kp=8432, P=8408, B=1278016),            # the largest NR transport block
    # three dwords per lane in one block, four in one block, four in each of two (appended: the seeds above keep their index)
    tb_case("c1_piece3", 1, 4300, C=1, which="24A", Kp=4324, in_row_bytes=544),
    tb_case("c1_piece4", 1, 7000, C=1, which="24A", Kp=7024, in_row_bytes=880),
    tb_case("c2_piece4", 1, 13928, C=2, which="24A", Kp=7000, in_row_bytes=880),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
SMALL_CASES = ["c1_tiny", "c1_8bit", "c1_odd", "c2_crc24_first", "c5_bits"]      # where assemble_loop is affordable
CORRUPTION_CASES = ["c2_bits", "c5_bits", "c1_tiny"]


@functools.lru_cache(maxsize=None)
def case_derive(name):
    c = CASE_BY_NAME[name]
    d = derive(c["bg"], c["A"])
    for k, v in c["pinned"].items():
        assert getattr(d, k) == v, (name, k, getattr(d, k))
    return d


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(tb_bits[S, A], hard rows of the valid code blocks segment() makes of them, random rows that are no codewords --
    with random bits behind K' too), drawn once and shared read-only."""
    c, d = CASE_BY_NAME[name], case_derive(name)
    rng = np.random.default_rng(9000 + CASES.index(c))
    tb_bits = rng.integers(0, 2, (c["slots"], d.A)).astype(np.uint8)
    valid = pack(segment(tb_bits, c["bg"]), d.in_row_bytes)
    rand = rng.integers(0, 256, (c["slots"], d.C, d.in_row_bytes)).astype(np.uint8)
    return _frozen(tb_bits, valid, rand)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """assemble_ref of inputs(name)'s "valid" or "random" rows; shared and read-only."""
    _, valid, rand = inputs(name)
    return _frozen(*assemble_ref(valid if kind == "valid" else rand, case_derive(name)))


def boundary_bits(d):
    """Stream bit positions worth corrupting: the first, the last (of the payload and of the whole stream), and the bits
    either side of every block boundary."""
    pos = {0, d.A - 1, d.B - 1}
    for r in range(1, d.C):
        pos |= {r * d.P - 1, r * d.P}
    return sorted(pos)


def flip(rows, b, r, i):
    """A copy of hard rows with bit i of block r of slot b flipped."""
    out = np.array(rows)
    out[b, r, i // 8] ^= 0x80 >> (i % 8)
    return out


def refresh_cb_crc(rows, d, b, r):
    """A copy with block r's CRC24B field recomputed from its payload (C > 1)."""
    out = np.array(rows)
    bits = np.unpackbits(out[b, r])
    bits[d.P:d.Kp] = _to_bits(int(crc_fast(bits[:d.P], "24B")), 24)
    out[b, r] = np.packbits(bits)
    return out


# ---- the chain behind the LDPC decoder (tests/ldpc_oracle.py CHAINS) ----

CHAIN_ESN0_DB = 1.0      # ldpc_oracle.ESN0_DB: the CPU oracle decodes every block of both chains there (tests/test_tb.py)


@functools.lru_cache(maxsize=None)
def chain_inputs(which):
    """A random transport block -> segment() -> the named random graph's codewords -> the transmitted positions of rv 0
    (rm_oracle.slot_map) -> noisy int8 LLR rows [slots, G], as ldpc_oracle.chain_inputs makes them; `llr_neg` is the same
    batch with the last slot's row negated.  `soft` / `soft_neg` are the rate recovery's expected buffers."""
    import ldpc_oracle as O
    c = O.CHAINS[which]
    d = R.derive(c["bg"], c["A"], c["qm"], c["L"], c["G"])
    for k, v in c["pinned"].items():
        assert getattr(d, k) == v, (which, k, getattr(d, k))
    t, g = derive(c["bg"], c["A"]), O.graph(c["graph"])
    assert (t.C, t.Kp) == (d.C, d.Kp) and g.zc == d.Zc and g.n_sys * g.zc == d.K
    rng = np.random.default_rng(9500 + sorted(O.CHAINS).index(which))
    tb_bits = rng.integers(0, 2, (O.CHAIN_SLOTS, t.A)).astype(np.uint8)
    blocks = segment(tb_bits, c["bg"])
    info = np.zeros((O.CHAIN_SLOTS, d.C, d.K), np.int64)
    info[:, :, :d.Kp] = blocks
    cw = O.encode(g.rows, g.n_sys, g.zc, info.reshape(-1, d.K)).reshape(O.CHAIN_SLOTS, d.C, -1)
    blk, pos, _ = R.slot_map(d, 0)
    llr = np.ascontiguousarray(O.noisy_llr(rng, cw[:, blk, pos + 2 * d.Zc], CHAIN_ESN0_DB, O.SCALE))
    llr_neg = llr.copy()
    llr_neg[-1] = -llr_neg[-1]
    soft, _ = R.recover(d, llr, [0] * O.CHAIN_SLOTS)
    soft_neg, _ = R.recover(d, llr_neg, [0] * O.CHAIN_SLOTS)
    _frozen(tb_bits, blocks, llr, llr_neg, soft, soft_neg)
    return SimpleNamespace(c=c, d=d, t=t, g=g, tb_bits=tb_bits, blocks=blocks, llr=llr, llr_neg=llr_neg, soft=soft, soft_neg=soft_neg)
