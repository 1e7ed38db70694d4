"""Every kernel variant the plan can select, against the float64 oracle (one test per representative of
tests/kernel_variants.py; the test id is the selection tuple).

Two Rx ports, both input layouts, and the diagnostic launch: the channel estimate, noise, RSRP, EPRE and CFO are compared
with oracle/ce_oracle.py run on complex128 copies of the same grid and pilots (the oracle keeps the dtype end to end) at
the suite's bars; the time alignment exactly with the complex64 oracle's, or a near-tie neighbour of it; each hop's
pilot-RE estimate before and after smoothing, its CFO and its TA bin with the oracle's stages, which places a
disagreement in a stage."""
import numpy as np
import pytest
import torch

from conftest import TA_TIE_RATIO, check_outputs, ta_alternatives_from

import ce_oracle as O
import kernel_variants as K
from srsran_ce_pytorch_amd import estimator as E, synth as S

pytestmark = pytest.mark.gpu

TOL_CH = 2e-5     # of max|h| (tests/test_hip_parity.py)
TOL_SC = 2e-5     # relative
TOL_P = 2e-6      # pilot-RE stages, of max|P| (tests/test_hip_stages.py)

REPS = K.representatives()


def _oracle(b, it, interp, dtype):
    stages = []
    r = O.srs_channel_estimator(b.grids[it].astype(dtype), b.pilots.astype(dtype), b.beta, b.hop1, b.hop2, b.config,
                                interp=interp, stages=stages)
    return r, stages


@pytest.mark.parametrize("rep", REPS, ids=[r[0] for r in REPS])
def test_variant_matches_float64_oracle(rep):
    vid, want, case, interp = rep
    assert K.variant_of(K.derive_case(case, interp), case["n_sym"], interp) == want, f"{vid}: the policy moved"
    dev = torch.device("cuda:0")
    b = S.build_case(case, 2)
    n_hops, L = len(case["hops"]), case["n_layers"]
    plan = E.make_plan(b.hop1, b.hop2, b.config, b.beta, L, case["n_prb_grid"], case["n_sym"], dev, interp)
    pil = torch.as_tensor(b.pilots, device=dev)
    g_ref = torch.as_tensor(b.grids, device=dev)[None]                               # [1 slot, 2 ports, n_sc, n_sym]
    g_sym = g_ref.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    outs = {"ref": E.estimate_with_plan(plan, g_ref, pil), "sym_major": E.estimate_with_plan(plan, g_sym, pil)}
    diag, st_p, st_s = E.estimate_stages(plan, g_sym, pil, n_hops)
    torch.cuda.synchronize()
    for a, c in zip(outs["sym_major"], diag):                                         # the dump changes nothing
        assert torch.equal(a, c) or (torch.isnan(a).all() and torch.isnan(c).all())
    outs = {k: [t[0].cpu().numpy() for t in v] for k, v in outs.items()}
    st_p, st_s = st_p[0].cpu().numpy(), st_s[0].cpu().numpy()

    for it in range(2):
        (ch128, n128, r128, e128, _, c128), stages128 = _oracle(b, it, interp, np.complex128)
        (_, _, _, _, ta64, _), stages64 = _oracle(b, it, interp, np.complex64)
        # check_outputs loosens its bars where RSRP < EPRE / 16; these inputs must never need that
        assert 16.0 * r128 >= e128, f"{vid}[{it}]: ill-conditioned input (rsrp {r128}, epre {e128})"
        ref_sc = [n128, r128, e128, ta64, np.nan if c128 is None else c128]
        bins = [int(st["ta_bin"]) for st in stages64]
        alts = ta_alternatives_from(bins, [st["ta_pw"] for st in stages64], case["scs"])
        for layout, o in outs.items():
            got = [o[1][it], o[2][it], o[3][it], o[4][it], o[5][it]]
            check_outputs(o[0][it], got, ch128, ref_sc, TOL_CH, TOL_SC, f"{vid}[{it}]/{layout}", alts)
        assert len(stages128) == n_hops
        for h in range(n_hops):
            for k, key in enumerate(("p_ls", "p_smooth")):
                ref = stages128[h][key].T                                             # (n_re, L) -> [L][n_re]
                err = np.abs(st_p[it, k, h] - ref).max() / np.abs(ref).max()
                assert err <= TOL_P, f"{vid}[{it}] hop {h} {key}: {err:.2e}"
            cfo = stages128[h]["cfo_hop"]
            if cfo is None:
                assert np.isnan(st_s[it, h, 0]), f"{vid}[{it}] hop {h}: cfo should be 'not estimated'"
            else:
                assert abs(st_s[it, h, 0] - cfo) <= 2e-6 * max(abs(cfo), 1e-3), f"{vid}[{it}] hop {h} cfo {st_s[it, h, 0]} vs {cfo}"
            lo, top, hi = stages64[h]["ta_pw"]
            ok = {bins[h]} | {bins[h] + d for d, pw in ((-1, lo), (1, hi)) if pw >= 0.0 and pw >= (1.0 - TA_TIE_RATIO) * top}
            assert int(st_s[it, h, 1]) in ok, f"{vid}[{it}] hop {h} TA bin {st_s[it, h, 1]} vs {bins[h]}"
