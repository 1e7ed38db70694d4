"""Oracle of the rate-recovery extension (include/ce_rm.h): TS 38.212 5.2.2 (segmentation), 5.4.2.1 (bit selection), 5.4.2.2
(bit interleaving) and 5.5 (concatenation) restated as the specification's own loops -- a NULL-marked circular buffer, the
`while k < E` walk, the interleaver's double loop, concatenation -- which yield, for every element of a slot's LLR row, the
code block r and the buffer position n it belongs to.  Accumulation is in source order of k, in np.float32 additions or in
int64 with one clamp.  Nothing here uses the kernel's closed form (rank, k mod P).  Results are compared by value
(np.array_equal; -0.0 == 0.0), without a tolerance."""
import functools
from types import SimpleNamespace

import numpy as np

ZC_SET = sorted(a << j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if (a << j) <= 384)
K0_NUM = {1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}
MAX_BITS = 1 << 21
NULL = -1


def select_base_graph(tbs, rate):
    """38.212 7.2.2."""
    return 2 if tbs <= 292 or (tbs <= 3824 and rate <= 0.67) or rate <= 0.25 else 1


def derive(bg, A, qm, L, G, n_ref=0):
    """Every derived value of include/ce_rm.h; raises ValueError where the descriptor is to be refused."""
    if bg not in (1, 2) or qm not in (2, 4, 6, 8) or not 1 <= L <= 4 or A < 1:
        raise ValueError("unsupported")
    B = A + 24 if A > 3824 else A + 16
    K_cb = 8448 if bg == 1 else 3840
    if B <= K_cb:
        C, Bp = 1, B
    else:
        C = -(-B // (K_cb - 24))
        Bp = B + 24 * C
    if B % C:
        raise ValueError("B mod C")
    Kp = Bp // C
    K_b = 22 if bg == 1 else 10 if B > 640 else 9 if B > 560 else 8 if B > 192 else 6
    if Kp > K_b * 384:
        raise ValueError("K'")
    Zc = min(z for z in ZC_SET if K_b * z >= Kp)
    K, N = (22 * Zc, 66 * Zc) if bg == 1 else (10 * Zc, 50 * Zc)
    if n_ref != 0 and n_ref < K - 2 * Zc:
        raise ValueError("n_ref")
    N_cb = N if n_ref == 0 else min(N, n_ref)
    f0, f1 = Kp - 2 * Zc, K - 2 * Zc
    if G % (L * qm) or G > MAX_BITS or G < 1:
        raise ValueError("G")
    q = G // (L * qm)
    if q < C:
        raise ValueError("q < C")
    E = [L * qm * (q // C) if r <= C - (q % C) - 1 else L * qm * -(-q // C) for r in range(C)]
    den = 66 if bg == 1 else 50
    k0 = tuple((num * N_cb) // (den * Zc) * Zc for num in K0_NUM[bg])
    return SimpleNamespace(bg=bg, A=A, qm=qm, L=L, G=G, n_ref=n_ref, B=B, K_cb=K_cb, C=C, Bp=Bp, Kp=Kp, K_b=K_b, Zc=Zc, K=K, N=N,
                           N_cb=N_cb, f0=f0, f1=f1, P=N_cb - (f1 - f0), E=E, k0=k0)


def walk(d, rv, E):
    """5.4.2.1: position n_k of e_k, k = 0 .. E-1, in a circular buffer whose filler bits are marked NULL."""
    buf = np.zeros(d.N_cb, np.int64)
    buf[d.f0:d.f1] = NULL                      # [K' - 2 Zc, K - 2 Zc) of the buffer: the filler bits, as far as N_cb reaches
    pos = np.empty(E, np.int64)
    k = j = 0
    k0 = d.k0[rv]
    while k < E:
        n = (k0 + j) % d.N_cb
        if buf[n] != NULL:
            pos[k] = n
            k += 1
        j += 1
    return pos


@functools.lru_cache(maxsize=None)
def _slot_map(key, rv):
    d = derive(*key)
    blk = np.empty(d.G, np.int64)
    pos = np.empty(d.G, np.int64)
    kk = np.empty(d.G, np.int64)
    start = 0
    for r, E in enumerate(d.E):                # 5.5: block r's f_0 .. f_{E-1} follow those of blocks 0 .. r-1
        n_of_e = walk(d, rv, E)
        for j in range(E // d.qm):             # 5.4.2.2: f_{i + j Qm} = e_{i E/Qm + j}
            for i in range(d.qm):
                src = start + i + j * d.qm
                k = i * (E // d.qm) + j
                blk[src], pos[src], kk[src] = r, n_of_e[k], k
        start += E
    assert start == d.G
    for a in (blk, pos, kk):
        a.setflags(write=False)
    return blk, pos, kk


def slot_map(d, rv):
    """(r, n, k) of every element of a slot's LLR row under redundancy version rv; shared and read-only."""
    return _slot_map((d.bg, d.A, d.qm, d.L, d.G, d.n_ref), rv & 3)


def recover(d, llr, rvs, harq=None, filler=127.0):
    """out[slot][r][n] of include/ce_rm.h for llr [B, G] (np.float32 or np.int8) and one rv per slot."""
    i8 = llr.dtype == np.int8
    assert i8 or llr.dtype == np.float32
    B = llr.shape[0]
    out = np.zeros((B, d.C, d.N_cb), np.int64 if i8 else np.float32)
    if harq is not None:
        assert harq.dtype == llr.dtype and harq.shape == out.shape
        out[...] = harq
    hits = np.zeros(out.shape, np.int64)
    for b in range(B):
        blk, pos, kk = slot_map(d, int(rvs[b]))
        order = np.lexsort((kk, blk))          # ascending k inside each block
        idx = (blk[order], pos[order])
        np.add.at(out[b], idx, llr[b][order].astype(out.dtype))     # unbuffered: one addition per source, in this order
        np.add.at(hits[b], idx, 1)
    if i8:
        out = np.where(hits > 0, np.clip(out, -127, 127), out)
    out[:, :, d.f0:d.f1] = 127 if i8 else np.float32(filler)
    hits[:, :, d.f0:d.f1] = 0
    return out.astype(llr.dtype), hits


def recover_loop(d, llr, rvs, harq=None, filler=127.0):
    """recover() with the accumulation as a plain Python loop (checks that np.add.at adds in the stated order)."""
    i8 = llr.dtype == np.int8
    B = llr.shape[0]
    out = np.zeros((B, d.C, d.N_cb), np.int64 if i8 else np.float32)
    if harq is not None:
        out[...] = harq
    hit = np.zeros(out.shape, bool)
    for b in range(B):
        blk, pos, kk = slot_map(d, int(rvs[b]))
        for src in np.lexsort((kk, blk)):
            r, n = blk[src], pos[src]
            out[b, r, n] = out[b, r, n] + (int(llr[b, src]) if i8 else llr[b, src])
            hit[b, r, n] = True
    if i8:
        out = np.where(hit, np.clip(out, -127, 127), out)
    out[:, :, d.f0:d.f1] = 127 if i8 else np.float32(filler)
    return out.astype(llr.dtype)


def rm_case(name, bg, A, qm, L, G, n_ref=0, rep=False, pinned=None):
    return dict(name=name, bg=bg, A=A, qm=qm, L=L, G=G, n_ref=n_ref, rep=rep, pinned=pinned or {})


CASES = [
    rm_case("bg2_a24_rep", 2, 24, 2, 1, 1200, rep=True,
            pinned=dict(C=1, Zc=7, N=350, f0=26, f1=56, P=320, k0=(0, 91, 175, 301))),
    rm_case("bg1_a96_k0_in_filler", 1, 96, 4, 1, 240,
            pinned=dict(Zc=6, N=396, f0=100, f1=120, k0=(0, 102, 198, 336))),
    rm_case("bg1_a96_rep", 1, 96, 4, 2, 1208, rep=True, pinned=dict(Zc=6, N=396, f0=100, f1=120, k0=(0, 102, 198, 336))),
    rm_case("bg2_a3848_c2", 2, 3848, 6, 2, 10812,
            pinned=dict(C=2, Zc=208, N=10400, f0=1544, f1=1664, E=[5400, 5412], k0=(0, 2704, 5200, 8944))),
    rm_case("bg1_a8448_c2", 1, 8448, 8, 1, 12008,
            pinned=dict(C=2, Zc=208, N=13728, f0=3844, f1=4160, E=[6000, 6008], k0=(0, 3536, 6864, 11648))),
    rm_case("bg1_a8448_lbrm", 1, 8448, 4, 3, 16812, n_ref=9000,
            pinned=dict(C=2, Zc=208, N=13728, N_cb=9000, P=8684, E=[8400, 8412], k0=(0, 2288, 4368, 7488))),
    rm_case("bg1_a16896_c3", 1, 16896, 8, 4, 32000, pinned=dict(C=3, E=[10656, 10656, 10688])),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
N_SLOTS = 3
FILLER = 40.5            # the float32 cases' filler_llr: a value no sum of the drawn inputs takes


def case_derive(c):
    return derive(c["bg"], c["A"], c["qm"], c["L"], c["G"], c["n_ref"])


def rvs_of(shift):
    """Three slots with distinct rv; shift = 0 .. 3 brings every rv to every slot."""
    return [(b + shift) & 3 for b in range(N_SLOTS)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """llr and harq of a named case in both formats, drawn once and shared read-only.  int8: full range where positions
    are hit repeatedly (sums saturate), |x| <= 60 elsewhere (llr + harq never saturates); recover() results under every
    rv rotation are cached by reference()."""
    c = CASE_BY_NAME[name]
    d = case_derive(c)
    rng = np.random.default_rng(3000 + CASES.index(c))
    lim = 127 if c["rep"] else 60
    x = SimpleNamespace(c=c, d=d, name=name)
    x.llr_i8 = rng.integers(-lim, lim + 1, (N_SLOTS, d.G)).astype(np.int8)
    x.harq_i8 = rng.integers(-lim, lim + 1, (N_SLOTS, d.C, d.N_cb)).astype(np.int8)
    x.llr_f32 = (rng.standard_normal((N_SLOTS, d.G)) * 4.0).astype(np.float32)
    x.harq_f32 = (rng.standard_normal((N_SLOTS, d.C, d.N_cb)) * 4.0).astype(np.float32)
    for a in (x.llr_i8, x.harq_i8, x.llr_f32, x.harq_f32):
        a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, fmt, shift, with_harq):
    """(out, hits) of recover() for inputs(name) in format `fmt` ("i8" / "f32") under rvs_of(shift); asserts the int8
    saturation property of the draw: sums leave [-127, 127] in the repetition cases and nowhere else."""
    x = inputs(name)
    llr = x.llr_i8 if fmt == "i8" else x.llr_f32
    harq = (x.harq_i8 if fmt == "i8" else x.harq_f32) if with_harq else None
    out, hits = recover(x.d, llr, rvs_of(shift), harq, FILLER)
    if fmt == "i8":
        wide, _ = recover(x.d, llr.astype(np.float32), rvs_of(shift), None if harq is None else harq.astype(np.float32), FILLER)
        wide[:, :, x.d.f0:x.d.f1] = 0
        saturated = bool(np.any(np.abs(wide) > 127))
        assert saturated == x.c["rep"], (name, shift, with_harq, saturated)
    out.setflags(write=False)
    hits.setflags(write=False)
    return out, hits
