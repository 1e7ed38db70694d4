"""Seeded random cases for the three PUSCH stages behind the channel estimate -- equalizer (csrc/ce_eq.hip), soft demapper
(csrc/ce_demod.hip), LDPC rate recovery (csrc/ce_rm.hip) -- for tests/test_stage_fuzz.py (CPU: what the draws must satisfy by
themselves) and tests/test_zzzz_hip_stage_fuzz.py (GPU: the kernels against the oracles on them).

`draw_*(idx)` derives a case from np.random.default_rng([BASE_SEED, stage_id, idx]) as a plain dict of Python values (a
failing case is replayed from that dict alone; the GPU file's LOGGED_CASES hold such dicts); `realize_*(case)` turns it into
arrays, seeded by the dict's own "seed".  References and comparison rules are the existing oracles' (eq_oracle,
demod_oracle, rm_oracle): nothing is restated here.  Shapes are the smallest that still reach every kernel path."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import demod_oracle as D
import eq_oracle as Q
import rm_oracle as R
from srsran_ce_pytorch_amd import synth as S

BASE_SEED = 20261020
N_CASES = 150
STAGE_EQ, STAGE_DEMOD, STAGE_RM = 1, 2, 3

# T = 4 C as in eq_oracle.py / demod_oracle.py; C = the float32 numpy restatement's largest error ratio over these draws
# (tests/test_stage_fuzz.py re-measures both and fails if one exceeds its recorded value)
C_EQ_FUZZ = 4.5          # measured 4.49 (equalize_f32 over the 150 equalizer draws), rounded up
T_EQ_FUZZ = 4.0 * C_EQ_FUZZ
C_DEMOD_FUZZ = 3.0       # measured 2.98 (llr_f32 over the 150 demapper draws), rounded up
T_DEMOD_FUZZ = 4.0 * C_DEMOD_FUZZ


def _rng(stage, idx):
    return np.random.default_rng([BASE_SEED, stage, idx])


def _pick(rng, values, weights=None):
    w = None if weights is None else np.asarray(weights, float) / np.sum(weights)
    return values[int(rng.choice(len(values), p=w))]


# ---------------------------------------------------------------- rate recovery ----

RM_MAX_G = 24000          # keeps the oracle's Python walk fast
RM_GUARD = 64             # elements either side of a guarded output: keeps 16-byte alignment in both formats
RM_FILLER = R.FILLER
RM_TILE_ELEMS = 4 * 1024  # int8 elements of one tile (CE_RM_TILE_UNITS units of 4)


def _rm_geometry(bg, A):
    """(C, Zc, K, N, K') of a transport block, or None where segmentation refuses it (B mod C)."""
    try:
        d = R.derive(bg, A, 2, 1, 2 * 10000)
    except ValueError:
        return None
    return d.C, d.Zc, d.K, d.N, d.Kp


def draw_rm(idx):
    """One rate-recovery case.  A from three bands; n_ref from {0, K - 2 Zc, K - 2 Zc + 1, uniform in [K - 2 Zc, N], the
    same forced odd}, where half of the forced-odd draws take the odd value 4096 m - 1 of that range if there is one: only
    there can `lead` push an int8 buffer's last unit into a tile of its own, and a uniform draw would not find it;
    q = G / (L Qm) from three bands, cut to G <= RM_MAX_G.  About 7 % of the cases are descriptors the oracle refuses, the
    kind of refusal drawn among four."""
    rng = _rng(STAGE_RM, idx)
    refuse = str(_pick(rng, ["B mod C", "q < C", "G", "n_ref"])) if rng.random() < 0.07 else ""
    while True:
        bg, qm, L = int(rng.integers(1, 3)), int(_pick(rng, [2, 4, 6, 8])), int(rng.integers(1, 5))
        band = int(rng.choice(3, p=[0.25, 0.25, 0.5]))
        A = int([rng.integers(1, 401), rng.integers(400, 4001), 8 * rng.integers(500, 2201)][band])
        geo = _rm_geometry(bg, A)
        if refuse == "B mod C":
            if geo is None:
                n_ref, G = 0, L * qm * 50
                break
            continue
        if geo is None:
            continue
        C, Zc, K, N, Kp = geo
        if refuse == "q < C" and C == 1:
            continue
        lo = K - 2 * Zc
        kind = int(rng.choice(5, p=[0.12, 0.2, 0.15, 0.13, 0.4] if C == 1 else [0.08, 0.27, 0.2, 0.1, 0.35]))
        if kind == 0:
            n_ref = 0
        elif kind == 1:
            n_ref = lo
        elif kind == 2:
            n_ref = lo + 1
        else:
            n_ref = int(rng.integers(lo, N + 1))
            if kind == 4:
                n_ref |= 1
                edge = [v for v in range(RM_TILE_ELEMS - 1, N + 1, RM_TILE_ELEMS) if v >= lo]
                if edge and rng.random() < 0.5:
                    n_ref = int(_pick(rng, edge))
        N_cb = N if n_ref == 0 else min(N, n_ref)
        P = N_cb - ((K - 2 * Zc) - (Kp - 2 * Zc))
        lq = L * qm
        q_max = RM_MAX_G // lq
        q_band = int(rng.choice(3, p=[0.2, 0.3, 0.5]))
        if q_band == 0:
            q = max(C, int(rng.integers(1, 41)))
        else:
            q = int(rng.uniform(0.2, 1.0) * C * P / lq) if q_band == 1 else int(rng.uniform(1.0, 3.5) * C * P / lq)
            q = max(q, C)
        if q > q_max:
            q = int(rng.integers(max(C, q_max // 2), q_max + 1))
        if q_band == 2 and q % C == 0 and q < q_max and rng.random() < 0.7:
            q += 1                                # unequal E_r among the code blocks
        G = lq * q
        if refuse == "q < C":
            G = lq * (C - 1)
        elif refuse == "G":
            G += 1
        elif refuse == "n_ref":
            n_ref = lo - 1
        break
    B = int(rng.integers(9, 21)) if rng.random() < 0.45 else int(rng.integers(1, 9))
    rv_kind = str(_pick(rng, ["tensor", "strided", "scalar"]))
    rvs = [int(v) for v in rng.integers(0, 4, B)]
    if rv_kind == "scalar":
        rvs = [rvs[0]] * B
    return dict(stage="rm", idx=idx, bg=bg, A=A, qm=qm, L=L, G=G, n_ref=n_ref, B=B, rvs=rvs, rv_kind=rv_kind,
                harq=str(_pick(rng, ["none", "separate", "in_place"])), guarded=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def rm_derive(c):
    """The oracle's derivation of a case, or the ValueError it refuses the descriptor with."""
    try:
        return R.derive(c["bg"], c["A"], c["qm"], c["L"], c["G"], c["n_ref"])
    except ValueError as e:
        return e


def realize_rm(c):
    """llr and harq of an accepted case in both formats.  int8: the full range where a position is hit repeatedly (sums
    saturate), |x| <= 60 elsewhere, as rm_oracle.inputs; float32: 4 N(0, 1)."""
    d = rm_derive(c)
    assert not isinstance(d, Exception), c
    rng = np.random.default_rng(c["seed"])
    B = c["B"]
    lim = 127 if max(d.E) > d.P else 60
    x = SimpleNamespace(c=c, d=d, B=B)
    x.llr_i8 = rng.integers(-lim, lim + 1, (B, d.G)).astype(np.int8)
    x.harq_i8 = rng.integers(-lim, lim + 1, (B, d.C, d.N_cb)).astype(np.int8)
    x.llr_f32 = (rng.standard_normal((B, d.G)) * 4.0).astype(np.float32)
    x.harq_f32 = (rng.standard_normal((B, d.C, d.N_cb)) * 4.0).astype(np.float32)
    return x


def rm_leads(d, B, unit=4):
    """`lead` of every (slot, block): how far into a 4-byte unit of the flat output its buffer starts."""
    return [((b * d.C + r) * d.N_cb) % unit for b in range(B) for r in range(d.C)]


def rm_classes(c):
    """The kernel paths of csrc/ce_rm.hip a case reaches (names as tests/test_stage_fuzz.py counts them)."""
    d = rm_derive(c)
    if isinstance(d, Exception):
        return {"refused"}
    B, out = c["B"], set()
    leads = rm_leads(d, B)
    tile_units = RM_TILE_ELEMS // 4
    tiles = lambda units: -(-units // tile_units)   # noqa: E731
    if B > 8:
        out.add("B > 8")
        if B % 8:
            out.add("B > 8, B % 8 != 0")
    if d.N_cb % 2 and d.C > 1:
        out.add("odd N_cb, C > 1")
    if any(v in (1, 3) for v in leads):
        out.add("lead 1 or 3")
    if any(v and d.C > 1 for v in leads):
        out.add("lead != 0, C > 1")
    if any(tiles(-(-(v + d.N_cb) // 4)) > tiles(-(-d.N_cb // 4)) for v in leads):
        out.add("extra tile")
    if d.N_cb == d.K - 2 * d.Zc:
        out.add("N_cb == K - 2 Zc")
    if max(d.E) > d.P:
        out.add("repetition")
        if max(d.E) > 2 * d.P:
            out.add("max E > 2 P")
        if d.C > 1 and len(set(d.E)) > 1:
            out.add("repetition, C > 1, e_lo != e_hi")
    if any(d.f0 <= d.k0[rv] < d.f1 for rv in c["rvs"]):
        out.add("k0[rv] in the fillers")
    for k in ("tensor", "strided", "scalar"):
        if c["rv_kind"] == k:
            out.add("rv " + k)
    out.add("harq " + c["harq"])
    if c["guarded"]:
        out.add("guarded")
    return out


# ---------------------------------------------------------------- equalizer ----

EQ_N_SYM = [1, 2, 4, 7, 10, 12, 13, 14]
EQ_MASKS = [0xFFF, 0x555, 0xAAA, 0x3CF, 0, 0x001, 0x800]
EQ_SCALES = [1e-3, 1.0, 1e3]


def _eq_geometry(rng):
    grid = int(rng.integers(1, 25))
    n_sym = int(_pick(rng, EQ_N_SYM))
    mask = int(_pick(rng, EQ_MASKS))
    spans = []
    if n_sym >= 2 and rng.random() < 0.45:        # two hops on disjoint symbol ranges; the first may start at symbol 1
        s1 = 1 if n_sym >= 3 and rng.random() < 0.4 else 0
        m = int(rng.integers(s1 + 1, n_sym))
        m2 = m if rng.random() < 0.7 else int(rng.integers(m, n_sym))
        spans = [(s1, m - s1), (m2, int(rng.integers(1, n_sym - m2 + 1)) if rng.random() < 0.5 else n_sym - m2)]
    else:                                         # one hop with any start symbol and length
        s1 = int(rng.integers(0, n_sym)) if rng.random() < 0.5 else 0
        spans = [(s1, int(rng.integers(1, n_sym - s1 + 1)) if rng.random() < 0.5 else n_sym - s1)]
    hops = []
    for start, n_alloc in spans:
        n_prbs = int(rng.integers(1, grid + 1))
        nd = min(int(rng.integers(1, 4)), n_alloc)
        dm = sorted(int(s) for s in rng.choice(np.arange(start, start + n_alloc), size=nd, replace=False))
        hops.append(dict(dmrs_symbols=dm, prb_start=int(rng.integers(0, grid - n_prbs + 1)), n_prbs=n_prbs, start_symbol=start, n_alloc=n_alloc))
    return grid, n_sym, mask, hops


def draw_eq(idx):
    """One equalizer case.  The geometry is redrawn while it holds no data RE (every allocated symbol a fully reserved
    DM-RS symbol): the library refuses that, and the oracle has nothing to say about it.
    R >= L: with fewer ports than layers at this SNR b = 1 - [A^-1]_ll approaches 0, the rule's 1 / b term makes any
    tolerance vacuous and oracle and kernel can disagree on the b > 0 predicate itself -- a question about the stated
    contract, not one a fuzz answers."""
    rng = _rng(STAGE_EQ, idx)
    while True:
        grid, n_sym, mask, hops = _eq_geometry(rng)
        free = 12 - bin(mask).count("1")
        if sum(h["n_prbs"] * (12 * (h["n_alloc"] - len(h["dmrs_symbols"])) + free * len(h["dmrs_symbols"])) for h in hops) > 0:
            break
    L = int(rng.integers(1, 5))
    R_ = int(rng.integers(L, 9))
    B = int(rng.integers(1, 13))
    return dict(stage="eq", idx=idx, n_prb_grid=grid, n_sym=n_sym, hops=hops, mask=mask, L=L, R=R_, B=B, scale=float(_pick(rng, EQ_SCALES)),
                layout=int(rng.integers(3)), slot=int(rng.integers(B)), seed=int(rng.integers(1 << 30)))


def eq_case_spec(c):
    hops = [S.hop_spec(h["dmrs_symbols"], h["prb_start"], h["n_prbs"], h["start_symbol"], h["n_alloc"]) for h in c["hops"]]
    return S.case_spec("stage_fuzz", c["n_prb_grid"], hops, n_layers=c["L"], n_sym=c["n_sym"], seed=c["seed"])


def realize_eq(c):
    """eq_oracle.draw's inputs for the case (iid channel inside the hops, unrelated rx off the data REs, noise
    10^-1.5 U(0.5, 2)), then rx and ch_est times a and noise times a^2, and the float64 reference of those inputs."""
    d = Q.draw(dict(case=eq_case_spec(c), L=c["L"], R=c["R"], B=c["B"], mask=c["mask"]))
    a = np.float32(c["scale"])
    d.rx = (d.rx * a).astype(np.complex64)
    d.ch_est = (d.ch_est * a).astype(np.complex64)
    d.noise = d.noise * float(c["scale"]) ** 2
    d.ref = Q.equalize_ref(d.rx, d.ch_est, d.noise, d.data_re)
    return d


def eq_check(x, nvar, ref, what):
    """eq_oracle.check's rule with the fuzz constant."""
    x, nvar = np.asarray(x), np.asarray(nvar)
    assert x.shape == ref.x_hat.shape and nvar.shape == ref.nvar.shape, (what, x.shape, nvar.shape, ref.x_hat.shape)
    rx_, rn_ = Q.error_ratios(x, nvar, ref)
    print(f"{what}: max error / (2^-24 (kappa + 1/b) scale): x_hat {rx_.max():.2f}, nvar {rn_.max():.2f}  (T = {T_EQ_FUZZ:g})")
    assert rx_.max() <= T_EQ_FUZZ, f"{what}: x_hat error ratio {rx_.max():.2f} > T = {T_EQ_FUZZ:g}"
    assert rn_.max() <= T_EQ_FUZZ, f"{what}: nvar error ratio {rn_.max():.2f} > T = {T_EQ_FUZZ:g}"


def eq_classes(c):
    out = {f"n_sym {c['n_sym']}", f"R {c['R']}", f"mask 0x{c['mask']:03x}", f"scale {c['scale']:g}", f"layout {c['layout']}"}
    hops = c["hops"]
    if c["B"] > 5:
        out.add("B > 5")
    if any(h["prb_start"] not in (0, 1, 2, 3, 30) for h in hops):
        out.add("another PRB start")
    if hops[0]["start_symbol"] > 0:
        out.add("first hop starts after symbol 0")
    if len(hops) == 2:
        out.add("two hops")
        if hops[0]["n_prbs"] != hops[1]["n_prbs"]:
            out.add("two hops of unequal width")
        sets = [set(range(h["prb_start"], h["prb_start"] + h["n_prbs"])) for h in hops]
        for chunk in range(-(-c["n_prb_grid"] // Q.CHUNK_PRB)):
            own = set(range(chunk * Q.CHUNK_PRB, (chunk + 1) * Q.CHUNK_PRB))
            if sets[0] & own and sets[1] & own and sets[0] & own != sets[1] & own:
                out.add("two hops overlapping partly inside a chunk")
    return out


# ---------------------------------------------------------------- demapper ----

DM_EDGE_M = [1023, 1024, 1025, 2047, 2048, 2049]
DM_BAD_NVAR = [np.inf, 0.0, -1.0, np.nan, -np.inf]                     # the special values of
DM_BAD_X = [complex(np.inf, 0.1), complex(0.1, -np.inf), complex(np.nan, 0.2), complex(0.3, np.nan)]   # test_special_values_are_erasures


def draw_dm(idx):
    """One demapper case.  M from {1..40}, {40..1100}, {1000..3200} and the tile boundaries DM_EDGE_M; rnti / n_id over
    their ranges with a tenth of the values at each extreme, one pair for the batch (as Python ints or stride-0 tensors) or
    one per slot."""
    rng = _rng(STAGE_DEMOD, idx)
    qm = int(_pick(rng, [2, 4, 6, 8]))
    band = int(rng.choice(4, p=[0.25, 0.3, 0.2, 0.25]))
    M = int([rng.integers(1, 41), rng.integers(40, 1101), rng.integers(1000, 3201), _pick(rng, DM_EDGE_M)][band])
    B = int(rng.integers(1, 12))

    def ident(hi):
        v = rng.integers(0, hi + 1, B)
        edge = rng.random(B)
        return [int(x) for x in np.where(edge < 0.1, 0, np.where(edge < 0.2, hi, v))]

    kind = str(_pick(rng, ["scalar", "tensor", "stride0"]))
    rnti, n_id = ident(65535), ident(1023)
    if kind != "tensor":
        rnti, n_id = [rnti[0]] * B, [n_id[0]] * B
    return dict(stage="demod", idx=idx, qm=qm, M=M, B=B, sigma2=float(10.0 ** rng.uniform(-3.5, 0.0)), descramble=bool(rng.random() < 0.6),
                rnti=rnti, n_id=n_id, param_kind=kind, scale_factor=1.3 if rng.random() < 1 / 3 else 1.0, seed=int(rng.integers(1 << 30)))


def realize_dm(c):
    """x_hat = a constellation point + CN(0, sigma2), 5 % of the symbols times U(1, 6) (beyond the outer level);
    nvar = sigma2 10^U(-1, 1); 2 % of the symbols erased by a special value.  Reference, unit tolerance and int8 scale from
    demod_oracle; the scale (times 1.3 in a third of the cases) is rounded to float32, the format the plan holds it in, so
    that input rounding is no part of the error."""
    rng = np.random.default_rng(c["seed"])
    B, M, qm, s2 = c["B"], c["M"], c["qm"], c["sigma2"]
    bits = rng.integers(0, 2, (B, M * qm))
    noise = (rng.standard_normal((B, M)) + 1j * rng.standard_normal((B, M))) * np.sqrt(s2 / 2.0)
    x = D.modulate(bits, qm) + noise
    x = np.where(rng.random((B, M)) < 0.05, x * rng.uniform(1.0, 6.0, (B, M)), x).astype(np.complex64)
    nvar = (s2 * 10.0 ** rng.uniform(-1.0, 1.0, (B, M))).astype(np.float32)
    erased = rng.random((B, M)) < 0.02
    which = rng.integers(0, len(DM_BAD_NVAR) + len(DM_BAD_X), (B, M))
    for k, v in enumerate(DM_BAD_NVAR):
        nvar[erased & (which == k)] = v
    for k, v in enumerate(DM_BAD_X):
        x[erased & (which == len(DM_BAD_NVAR) + k)] = v
    d = SimpleNamespace(c=c, qm=qm, M=M, B=B, G=M * qm, bits=bits, x=x, nvar=nvar, erased=erased, rnti=c["rnti"], n_id=c["n_id"])
    d.ref = D.llr_ref(x, nvar, qm)
    d.tol = D.unit_tolerance(x, nvar, qm)
    live = d.ref[d.ref != 0]
    d.scale = float(np.float32((D.int8_scale(live) if live.size else 1.0) * c["scale_factor"]))   # (a slot batch of erasures only: any scale)
    d.flips = D.flips(dict(M=M, qm=qm, rnti=c["rnti"], n_id=c["n_id"]))
    return d


def dm_classes(c, d=None):
    out = {f"Qm {c['qm']}", "params " + c["param_kind"], "descramble" if c["descramble"] else "plain"}
    if c["M"] in DM_EDGE_M:
        out |= {"M at a tile boundary", f"M {c['M']}"}
    if c["B"] > 3:
        out.add("B > 3")
    if c["M"] % 2 and c["B"] > 1:
        out.add("odd M, B > 1")
    if c["scale_factor"] != 1.0:
        out.add("scale no power of two")
    for name, hi in (("rnti", 65535), ("n_id", 1023)):
        if 0 in c[name]:
            out.add(name + " 0")
        if hi in c[name]:
            out.add(f"{name} {hi}")
    if d is not None:
        ok = D.usable(d.x, d.nvar)
        if d.erased.any():
            out.add("erasures")
        if ok.any() and d.nvar[ok].max() > 16.0 * d.nvar[ok].min():
            out.add("nvar spread above x16")
        if ok.any() and max(np.abs(d.x.real[ok]).max(), np.abs(d.x.imag[ok]).max()) > 1.5 * D.a_max(c["qm"]):
            out.add("beyond the outer level")
    return out
