"""A bounded, deterministic differential fuzz of the three PUSCH stages behind the channel estimate on the GPU: the N_CASES
seeded draws per stage of tests/stage_fuzz_cases.py through PuschEqualizer, PuschDemapper and PuschRateRecovery, each against
its oracle under the oracle's own rule (rate recovery: by value, without a tolerance; equalizer and demapper: T = 4 C with
the constants tests/test_stage_fuzz.py calibrates on these same draws).  A descriptor the oracle refuses must be refused
with the same exception class; nothing is skipped.  Two deterministic rate-recovery tests pin what depends on no draw: slot
batches beyond one group of 8, and buffers of an odd N_cb, which start 1 and 3 bytes into a 4-byte unit of the int8 output.

Every assertion message carries the case's dict: `realize_*` of that dict replays the case on the CPU.

The file's name sorts it behind test_zzz_hip_rm.py: every earlier GPU test keeps its place in the run."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import demod_oracle as D
import rm_oracle as R
import stage_fuzz_cases as F
from srsran_ce_pytorch_amd import demod as DM, equalizer as EQ, ratematch as RM, synth as S

pytestmark = pytest.mark.gpu
FORMATS = [("f32", torch.float32), ("i8", torch.int8)]
FILL = {"f32": -5.0, "i8": 77}                      # sentinel of the guard regions

# Cases a run flagged, kept exactly as they were drawn (the dicts of stage_fuzz_cases.draw_*); they run after the seeded ones.
LOGGED_EQ_CASES = []
LOGGED_DEMOD_CASES = []
LOGGED_RM_CASES = []


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=_dev())


def _case(draw, logged, idx):
    return draw(idx) if idx < F.N_CASES else logged[idx - F.N_CASES]


# ---------------------------------------------------------------- equalizer ----

def _rx_layout(rx, layout):
    """The three layouts of test_z_hip_eq.py::test_rx_layouts_give_identical_bits."""
    if layout == 0:                                  # permuted view of a [B, R, n_sym, n_sc] buffer
        return _t(np.asarray(rx).transpose(0, 1, 3, 2)).contiguous().permute(0, 1, 3, 2)
    if layout == 1:                                  # contiguous [B, R, n_sc, n_sym]
        return _t(rx)
    B, R_, n_sc, n_sym = rx.shape                    # neither axis has unit stride
    wide = torch.zeros((B, R_, n_sc, 2 * n_sym + 1), dtype=torch.complex64, device=_dev())
    wide[..., ::2][..., :n_sym] = _t(rx)
    return wide[..., ::2][..., :n_sym]


@pytest.mark.parametrize("idx", range(F.N_CASES + len(LOGGED_EQ_CASES)))
def test_equalizer_fuzz_case(idx):
    c = _case(F.draw_eq, LOGGED_EQ_CASES, idx)
    what = f"eq {c}"
    d = F.realize_eq(c)
    h1, h2, _ = S.numpy_hops(F.eq_case_spec(c))
    eq = EQ.PuschEqualizer(h1, h2, c["L"], c["n_prb_grid"], c["n_sym"], reserved_re_mask=c["mask"], device=_dev())
    assert eq.n_data_re == len(d.data_re) and np.array_equal(eq.data_re(), d.data_re), what
    x, nv = eq(_rx_layout(d.rx, c["layout"]), _t(d.ch_est), _t(d.noise))
    torch.cuda.synchronize()
    shape = (c["B"], len(d.data_re), c["L"])
    assert tuple(x.shape) == shape == tuple(nv.shape) and x.dtype == torch.complex64 and nv.dtype == torch.float32, what
    F.eq_check(x.cpu().numpy(), nv.cpu().numpy(), d.ref, what)
    if c["B"] > 1:                                   # a slot of the batch against its own single-slot call, bit for bit
        b = c["slot"]
        xb, nb = eq(_rx_layout(d.rx[b:b + 1], c["layout"]), _t(d.ch_est[b:b + 1]), _t(d.noise[b:b + 1]))
        torch.cuda.synchronize()
        bits = lambda t: t.cpu().numpy().view(np.int32)   # noqa: E731
        assert np.array_equal(bits(xb[0]), bits(x[b])) and np.array_equal(bits(nb[0]), bits(nv[b])), f"{what}: slot {b} alone differs"


# ---------------------------------------------------------------- demapper ----

def _dm_param(values, kind, B):
    if kind == "scalar":
        return values[0]
    if kind == "stride0":
        t = _t(values[:1], torch.int32).expand(B)
        assert t.stride(0) == 0 or B == 1
        return t
    return _t(values, torch.int32)


@pytest.mark.parametrize("idx", range(F.N_CASES + len(LOGGED_DEMOD_CASES)))
def test_demapper_fuzz_case(idx):
    c = _case(F.draw_dm, LOGGED_DEMOD_CASES, idx)
    what = f"demod {c}"
    d = F.realize_dm(c)
    x, nvar = _t(d.x), _t(d.nvar)
    for fmt, dt in FORMATS:
        scale = d.scale if fmt == "i8" else None
        plain = DM.PuschDemapper(d.qm, d.M, out_dtype=dt, llr_scale=d.scale, device=_dev())(x, nvar)
        torch.cuda.synchronize()
        assert tuple(plain.shape) == (d.B, d.G) and plain.dtype == dt, what
        p = plain.cpu().numpy()
        D.check(p, d.ref, d.tol, f"{what} {fmt}", scale=scale, t=F.T_DEMOD_FUZZ)
        if not c["descramble"]:
            continue
        dem = DM.PuschDemapper(d.qm, d.M, out_dtype=dt, llr_scale=d.scale, descramble=True, device=_dev())
        q = dem(x, nvar, rnti=_dm_param(c["rnti"], c["param_kind"], d.B), n_id=_dm_param(c["n_id"], c["param_kind"], d.B))
        torch.cuda.synchronize()
        q = q.cpu().numpy()
        D.check(q, np.where(d.flips, -d.ref, d.ref), d.tol, f"{what} {fmt} descrambled", scale=scale, t=F.T_DEMOD_FUZZ)
        # descrambling is the plain result with the signs flipped where c = 1, exactly (-0.0 == 0.0; int8 never holds -128)
        assert np.array_equal(q, np.where(d.flips, -p, p)), f"{what} {fmt}: {int(np.sum(q != np.where(d.flips, -p, p)))} LLRs are not the plain ones sign-flipped"


# ---------------------------------------------------------------- rate recovery ----

def _rm_plan(c, dt):
    return RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], dtype=dt, n_ref=c["n_ref"], filler_llr=F.RM_FILLER, device=_dev())


def _rm_buffers(B, d, fmt, dt, harq, guarded, in_place):
    """(out, harq tensor, whole buffer or None): the output alone or inside a buffer with RM_GUARD sentinel elements
    either side (which keeps it 16-byte aligned), the kept buffer separate or the output itself."""
    n = B * d.C * d.N_cb
    buf = out = None
    if guarded:
        buf = torch.full((n + 2 * F.RM_GUARD,), FILL[fmt], dtype=dt, device=_dev())
        out = buf[F.RM_GUARD:F.RM_GUARD + n].view(B, d.C, d.N_cb)
    hq = None if harq is None else _t(harq)
    if in_place:
        if out is None:
            out = hq
        else:
            out.copy_(hq)
            hq = out
    return out, hq, buf


def _rm_compare(got, out, buf, ref, hits, d, fmt, harq, what):
    B = ref.shape[0]
    assert out is None or got is out, what
    assert tuple(got.shape) == (B, d.C, d.N_cb), what
    g = got.cpu().numpy()
    bad = np.argwhere(g != ref)
    assert bad.size == 0, f"{what} {fmt}: {len(bad)} positions differ from the oracle, the first at (slot, block, n) = {bad[0].tolist()}"
    # fillers hold the filler value whatever harq holds there; a position nothing reaches keeps harq, or 0
    assert np.all(g[:, :, d.f0:d.f1] == (127 if fmt == "i8" else np.float32(F.RM_FILLER))), f"{what} {fmt}: fillers"
    live = np.ones(d.N_cb, bool)
    live[d.f0:d.f1] = False
    untouched = (hits == 0) & live
    kept = np.zeros_like(ref) if harq is None else harq
    assert np.array_equal(g[untouched], kept[untouched]), f"{what} {fmt}: a position nothing reaches changed"
    if buf is not None:
        h = buf.cpu().numpy()
        assert np.all(h[:F.RM_GUARD] == FILL[fmt]) and np.all(h[-F.RM_GUARD:] == FILL[fmt]), f"{what} {fmt}: a guard region was written"


@pytest.mark.parametrize("idx", range(F.N_CASES + len(LOGGED_RM_CASES)))
def test_rate_recovery_fuzz_case(idx):
    c = _case(F.draw_rm, LOGGED_RM_CASES, idx)
    what = f"rm {c}"
    d = F.rm_derive(c)
    if isinstance(d, Exception):                     # the oracle refuses the descriptor: so must the library, alike
        for _, dt in FORMATS:
            with pytest.raises(type(d)):
                _rm_plan(c, dt)
        return
    x = F.realize_rm(c)
    B, rvs = c["B"], c["rvs"]
    for fmt, dt in FORMATS:
        llr = x.llr_i8 if fmt == "i8" else x.llr_f32
        harq = None if c["harq"] == "none" else (x.harq_i8 if fmt == "i8" else x.harq_f32)
        ref, hits = R.recover(d, llr, rvs, harq, F.RM_FILLER)
        if c["rv_kind"] == "scalar":
            rv = rvs[0]
        elif c["rv_kind"] == "tensor":
            rv = _t(rvs, torch.int32)
        else:                                        # an element stride of 3; the values between are other rvs
            rv = _t(np.stack([rvs, (np.array(rvs) + 1) & 3, (np.array(rvs) + 2) & 3], 1).reshape(-1), torch.int32)[::3]
            assert rv.stride(0) == 3
        out, hq, buf = _rm_buffers(B, d, fmt, dt, harq, c["guarded"], c["harq"] == "in_place")
        got = _rm_plan(c, dt)(_t(llr), rv, harq=hq, out=out)
        torch.cuda.synchronize()
        _rm_compare(got, out, buf, ref, hits, d, fmt, harq, what)


def _named_inputs(name, B, seed):
    c = R.CASE_BY_NAME[name]
    d = R.case_derive(c)
    rng = np.random.default_rng(seed)
    lim = 127 if c["rep"] else 60
    x = SimpleNamespace(d=d, c=dict(bg=c["bg"], A=c["A"], qm=c["qm"], L=c["L"], G=c["G"], n_ref=c["n_ref"]))
    x.llr_i8 = rng.integers(-lim, lim + 1, (B, d.G)).astype(np.int8)
    x.harq_i8 = rng.integers(-lim, lim + 1, (B, d.C, d.N_cb)).astype(np.int8)
    x.llr_f32 = (rng.standard_normal((B, d.G)) * 4.0).astype(np.float32)
    x.harq_f32 = (rng.standard_normal((B, d.C, d.N_cb)) * 4.0).astype(np.float32)
    return x


def test_rate_recovery_batches_of_9_16_and_17_slots():
    """The workgroup-to-slot map b = 8 grp + (blockIdx & 7) beyond its first group, with a last group that is full (16) and
    one that holds a single slot (9, 17): against the oracle, and every slot against its own single-slot call."""
    for name in ("bg2_a24_rep", "bg1_a8448_c2"):
        x = _named_inputs(name, 17, 4100)
        d = x.d
        rvs = [b & 3 for b in range(17)]
        for fmt, dt in FORMATS:
            llr, harq = (x.llr_i8, x.harq_i8) if fmt == "i8" else (x.llr_f32, x.harq_f32)
            rm = _rm_plan(x.c, dt)
            alone = []
            for b in range(17):
                alone.append(rm(_t(llr[b:b + 1]), rvs[b], harq=_t(harq[b:b + 1])).cpu().numpy()[0])
            for B in (9, 16, 17):
                what = f"{name} {fmt} B={B}"
                ref, hits = R.recover(d, llr[:B], rvs[:B], harq[:B], F.RM_FILLER)
                got = rm(_t(llr[:B]), _t(rvs[:B], torch.int32), harq=_t(harq[:B]))
                torch.cuda.synchronize()
                _rm_compare(got, None, None, ref, hits, d, fmt, harq[:B], what)
                g = got.cpu().numpy()
                for b in range(B):
                    assert np.array_equal(g[b].view(np.uint8), alone[b].view(np.uint8)), f"{what}: slot {b} differs from its single-slot call"


def test_rate_recovery_odd_n_cb_starts_buffers_at_every_byte_of_a_unit():
    """N_cb = 349, C = 1, five slots: the buffers start 0, 1, 2, 3, 0 bytes into a 4-byte unit of the int8 output; and two
    code blocks of N_cb = 9001.  Both formats, harq combined in place inside a guarded buffer."""
    one = dict(bg=2, A=24, qm=2, L=1, G=1200, n_ref=349)
    two = dict(bg=1, A=8448, qm=4, L=3, G=16812, n_ref=9001)
    B = 5
    assert F.rm_leads(F.rm_derive(one), B) == [0, 1, 2, 3, 0]
    assert F.rm_leads(F.rm_derive(two), B) == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1] and F.rm_derive(two).C == 2
    for k, desc in enumerate((one, two)):
        c = dict(desc, B=B, seed=4200 + k)
        d = F.rm_derive(c)
        assert d.N_cb == desc["n_ref"] and (max(d.E) > d.P) == (k == 0)
        x = F.realize_rm(c)
        rvs = [(b + 1) & 3 for b in range(B)]
        for fmt, dt in FORMATS:
            llr, harq = (x.llr_i8, x.harq_i8) if fmt == "i8" else (x.llr_f32, x.harq_f32)
            ref, hits = R.recover(d, llr, rvs, harq, F.RM_FILLER)
            out, hq, buf = _rm_buffers(B, d, fmt, dt, harq, True, True)
            assert hq is out
            got = _rm_plan(c, dt)(_t(llr), _t(rvs, torch.int32), harq=hq, out=out)
            torch.cuda.synchronize()
            _rm_compare(got, out, buf, ref, hits, d, fmt, harq, f"rm {desc} B={B} rvs={rvs}")
