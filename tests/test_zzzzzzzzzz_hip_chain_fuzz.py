"""A bounded, deterministic differential fuzz on the GPU of the five PUSCH stages added behind the first fuzz: the seeded draws
of tests/chain_fuzz_cases.py through PuschTransformDeprecoder (a sweep over every valid allocation size), PuschLdpcDecoder,
PuschTransportBlock, PuschTransportEncoder and PuschModulator, each against its oracle under the oracle's own rule -- the
de-precoder under tp_oracle.check with T = 4 C, the constant tests/test_chain_fuzz.py calibrates on these same cases; the
other four by value, on integers, bits or float32 bit patterns, without a tolerance.  A descriptor or graph the oracle
refuses must be refused with the same exception class; nothing is skipped.  One pinned decoder test, the degree ladder, runs
every instance ldpc_row<DEG> / ldpc_parity<DEG>, DEG = 2 .. 19, in one launch.

Every assertion message carries the case's dict: `realize_*` of that dict replays the case on the CPU.  Every input is one
the oracle and the header define.

The file's name sorts it behind test_zzzzzzzzz_hip_mod.py: every earlier GPU test keeps its place in the run."""
import numpy as np
import pytest
import torch

import chain_fuzz_cases as F
import ldpc_oracle as O
import mod_oracle as M
import tp_oracle as TP
from srsran_ce_pytorch_amd import deprecode as DP, encoder as EN, ldpc as LD, modulator as MO, synth as S, transportblock as TB

pytestmark = pytest.mark.gpu

# Cases a run flagged, kept exactly as they were drawn (the dicts of chain_fuzz_cases.draw_*); they run after the seeded ones.
LOGGED_TP_CASES = []
LOGGED_LDPC_CASES = []
LOGGED_TB_CASES = []
LOGGED_ENC_CASES = []
LOGGED_MOD_CASES = []


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())


def _case(draw, n, logged, idx):
    return draw(idx) if idx < n else logged[idx - n]


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


# ---------------------------------------------------------------- transform de-precoding ----

@pytest.mark.parametrize("idx", range(F.N_TP + len(LOGGED_TP_CASES)))
def test_deprecoder_sweep_case(idx):
    c = _case(F.draw_tp, F.N_TP, LOGGED_TP_CASES, idx)
    what = f"tp {c}"
    d = F.realize_tp(c)
    tp = DP.PuschTransformDeprecoder(c["n_prb"], c["S"], device=_dev())
    xh, nh = _t(d.x_hat), _t(d.nvar)
    x, nv = tp(xh, nh, out=xh, nvar_out=nh) if c["in_place"] else tp(xh, nh)
    torch.cuda.synchronize()
    assert not c["in_place"] or (x is xh and nv is nh), what
    assert tuple(x.shape) == tuple(nv.shape) == (c["B"], c["S"] * d.M), what
    TP.check(x.cpu().numpy(), nv.cpu().numpy(), d.ref_x, d.ref_nv, DP.derive_host(c["n_prb"], c["S"]), what, t=F.T_TP_FUZZ)
    if c["B"] > 1:                                   # a slot of the batch against its own single-slot call, bit for bit
        b = c["slot"]
        ox, on = tp(_t(d.x_hat[b:b + 1]), _t(d.nvar[b:b + 1]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ox)[0], _bits(x)[b]) and np.array_equal(_bits(on)[0], _bits(nv)[b]), f"{what}: slot {b} alone differs"


# ---------------------------------------------------------------- LDPC decoder ----

def _decode(rows, n_cols, c, llr):
    dec = LD.PuschLdpcDecoder(LD.LdpcGraph(rows, n_cols), c["zc"], c["n_in"], c["k_out"], n_punctured_cols=c["n_punct"],
                              dtype=torch.int8 if c["dtype"] == "i8" else torch.float32, llr_scale=c["llr_scale"], max_iters=c["max_iters"],
                              early_stop=c["early_stop"], device=_dev())
    out = dec(_t(llr), return_post=True)
    torch.cuda.synchronize()
    return dec, tuple(o.cpu().numpy() for o in out)


def _same_decode(got, hard, status, L, what):
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[2].dtype == np.int16, what
    assert np.array_equal(got[1], status), f"{what}: status {got[1].tolist()} != {status.tolist()}"
    assert np.array_equal(got[2], L), f"{what}: post differs, first at (block, bit) {np.argwhere(got[2] != L)[:4].tolist()}"
    assert np.array_equal(got[0], hard), f"{what}: hard differs, first at (block, byte) {np.argwhere(got[0] != hard)[:4].tolist()}"


@pytest.mark.parametrize("idx", range(F.N_LDPC + len(LOGGED_LDPC_CASES)))
def test_decoder_fuzz_case(idx):
    c = _case(F.draw_ldpc, F.N_LDPC, LOGGED_LDPC_CASES, idx)
    what = f"ldpc {c}"
    d = F.realize_ldpc(c)
    dec, got = _decode(d.rows, d.n_cols, c, d.llr)
    assert dec.blocks_per_workgroup == F.ldpc_view(c).blocks_per_workgroup, what
    assert got[0].shape == (c["nb"], dec.row_bytes) and got[1].shape == (c["nb"], 2) and got[2].shape == (c["nb"], d.n_cols * c["zc"]), what
    _same_decode(got, d.hard, d.status, d.L, what)


def test_degree_ladder_runs_every_row_instance():
    """zc = 7, one graph whose 18 rows have the degrees 2 .. 19, three noisy codewords and three random rows in one workgroup:
    the narrowest run that executes all 18 instances of ldpc_row<DEG> and ldpc_parity<DEG>."""
    g = F.ladder_graph()
    rng = np.random.default_rng(F.BASE_SEED + 1)
    c = dict(zc=g.zc, n_in=(g.n_cols - 1) * g.zc, k_out=g.n_sys * g.zc, n_punct=1, dtype="i8", llr_scale=1.0, max_iters=8, early_stop=True)
    cw = O.encode(g.rows, g.n_sys, g.zc, rng.integers(0, 2, (3, g.n_sys * g.zc)))[:, g.zc:]
    llr = np.concatenate([O.noisy_llr(rng, cw, 3.0, O.SCALE), rng.integers(-128, 128, (3, c["n_in"])).astype(np.int8)])
    L, status, _ = O.decode_ref(g.rows, g.n_cols, g.zc, O.channel(O.quantise(llr), g.n_cols, g.zc, 1), 8, True)
    assert len(set(status[:, 0].tolist())) > 1                   # the six blocks do not all stop together
    dec, got = _decode(g.rows, g.n_cols, c, llr)
    assert dec.blocks_per_workgroup >= 6
    _same_decode(got, O.pack(L, c["k_out"]), status, L, "degree ladder")


# ---------------------------------------------------------------- transport-block assembly ----

@pytest.mark.parametrize("idx", range(F.N_TB + len(LOGGED_TB_CASES)))
def test_assembly_fuzz_case(idx):
    c = _case(F.draw_tb, F.N_TB, LOGGED_TB_CASES, idx)
    what = f"tb {c}"
    d = F.tb_derive(c)
    if isinstance(d, Exception):                     # the oracle refuses the size: so must the library, alike
        with pytest.raises(type(d)):
            TB.PuschTransportBlock(c["bg"], c["A"], device=_dev())
        return
    x = F.realize_tb(c)
    asm = TB.PuschTransportBlock(c["bg"], c["A"], device=_dev())
    assert (asm.c, asm.k_prime, asm.in_row_bytes, asm.tb_row_bytes) == (d.C, d.Kp, d.in_row_bytes, d.tb_row_bytes), what
    tb, tb_status, cb_status = (o.cpu().numpy() for o in asm(_t(x.rows)))
    assert tb.dtype == np.uint8 and tb_status.dtype == np.int32 and cb_status.dtype == np.int32, what
    assert tb.shape == x.tb.shape and tb_status.shape == x.tb_status.shape and cb_status.shape == x.cb_status.shape, what
    assert np.array_equal(cb_status, x.cb_status), f"{what} ({x.kind} {x.flips}): cb_status differs at (slot, block, field) {np.argwhere(cb_status != x.cb_status)[:4].tolist()}"
    assert np.array_equal(tb_status, x.tb_status), f"{what} ({x.kind} {x.flips}): tb_status {tb_status.tolist()[:4]} != {x.tb_status.tolist()[:4]}"
    assert np.array_equal(tb, x.tb), f"{what} ({x.kind} {x.flips}): tb differs at (slot, byte) {np.argwhere(tb != x.tb)[:4].tolist()}"


# ---------------------------------------------------------------- encoder ----

@pytest.mark.parametrize("idx", range(F.N_ENC + len(LOGGED_ENC_CASES)))
def test_encoder_fuzz_case(idx):
    c = _case(F.draw_enc, F.N_ENC, LOGGED_ENC_CASES, idx)
    what = f"enc {c}"
    d = F.enc_derive(c)
    args = (c["bg"], c["A"], c["qm"], c["L"], c["G"])
    if isinstance(d, Exception) or c["bad_graph"]:   # refused by the oracle, or a graph outside the stated form: refused alike
        g = F.enc_graph(c, 2 if isinstance(d, Exception) else d.Zc)
        with pytest.raises(type(d) if isinstance(d, Exception) else ValueError):
            EN.PuschTransportEncoder(*args, LD.LdpcGraph(g.rows, g.n_cols), n_ref=c["n_ref"], device=_dev())
        return
    x = F.realize_enc(c)
    enc = EN.PuschTransportEncoder(*args, LD.LdpcGraph(x.graph.rows, x.graph.n_cols), n_ref=c["n_ref"], device=_dev())
    rvs = c["rvs"]
    if c["rv_kind"] == "scalar":
        rv = rvs[0]
    elif c["rv_kind"] == "tensor":
        rv = _t(rvs, torch.int32)
    else:                                            # an element stride of 3; the values between are other rvs
        rv = _t(np.stack([rvs, (np.array(rvs) + 1) & 3, (np.array(rvs) + 2) & 3], 1).reshape(-1), torch.int32)[::3]
        assert rv.stride(0) == 3
    out = enc(_t(x.tb_rows), rv=rv, return_codeword=c["want_cw"])
    torch.cuda.synchronize()
    g, cw = out if c["want_cw"] else (out, None)
    g = g.cpu().numpy()
    assert g.dtype == np.uint8 and g.shape == x.g.shape == (c["S"], enc.g_row_bytes), what
    if cw is not None:
        cw = cw.cpu().numpy()
        assert cw.shape == x.cw.shape, (what, cw.shape, x.cw.shape)
        assert np.array_equal(cw, x.cw), f"{what}: cw differs, first at (slot, block, byte) {np.argwhere(cw != x.cw)[:4].tolist()}"
    assert np.array_equal(g, x.g), f"{what}: g differs, first at (slot, byte) {np.argwhere(g != x.g)[:4].tolist()}"


# ---------------------------------------------------------------- modulator ----

def _mod_param(values, kind, B):
    if kind == "scalar":
        return values[0]
    if kind == "stride0":
        t = _t(values[:1], torch.int32).expand(B)
        assert t.stride(0) == 0 or B == 1
        return t
    return _t(values, torch.int32)


@pytest.mark.parametrize("idx", range(F.N_MOD + len(LOGGED_MOD_CASES)))
def test_modulator_fuzz_case(idx):
    c = _case(F.draw_mod, F.N_MOD, LOGGED_MOD_CASES, idx)
    what = f"mod {c}"
    d = F.realize_mod(c)
    h1, h2, _ = S.numpy_hops(d.case)
    mod = MO.PuschModulator(h1, h2, c["L"], c["n_prb_grid"], c["qm"], n_sym=c["n_sym"], reserved_re_mask=c["mask"], scramble=c["scramble"], device=_dev())
    assert (mod.n_bits, mod.n_data_re, mod.g_row_bytes, mod.n_re, mod.n_dmrs_total) == (d.G, d.n_data_re, d.g_rows.shape[1], d.n_re, d.n_cols), what
    B = c["B"]

    def run(sl):
        n = sl.stop - sl.start
        ids = dict(rnti=_mod_param(c["rnti"][sl], c["param_kind"], n), n_id=_mod_param(c["n_id"][sl], c["param_kind"], n)) if c["scramble"] else {}
        out = torch.full((n, c["L"], c["n_sym"], 12 * c["n_prb_grid"]), float("nan"), dtype=torch.complex64, device=_dev()) if c["out_nan"] else None
        tx = mod(_t(d.g_rows[sl]), _t(d.pilots[sl] if c["pilots_per_slot"] else d.pilots), c["beta"], out=out, **ids)
        torch.cuda.synchronize()
        assert out is None or tx.data_ptr() == out.data_ptr(), what
        return np.ascontiguousarray(tx.permute(0, 1, 3, 2).cpu().numpy())      # the oracle's [B, L, n_sym, n_sc]

    got = run(slice(0, B))
    assert got.dtype == np.complex64 and got.shape == d.ref.shape, (what, got.shape, d.ref.shape)
    assert M.same(got, d.ref), f"{what}: tx differs, first at (slot, layer, symbol, subcarrier) {np.argwhere(got.view(np.uint64) != np.ascontiguousarray(d.ref).view(np.uint64))[:4].tolist()}"
    if B > 1:                                        # a slot of the batch against its own single-slot call, bit for bit
        b = c["slot"]
        assert M.same(run(slice(b, b + 1))[0], got[b]), f"{what}: slot {b} alone differs"
