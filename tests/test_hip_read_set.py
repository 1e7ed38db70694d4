"""Every kernel variant reads its read set and nothing else (one test per representative of tests/kernel_variants.py).

tests/test_hip_kernel_variants.py proves that each variant computes the right numbers from the right REs; this module
proves the converse.  The kernels load past the band and discard what they loaded (``load_hop`` / ``finish_hop`` of
ce_estimate_kernel.h, the staging loads and the writer's ``pick`` of ce_narrow_kernel.h); that is exact only while the
value is selected away -- multiplied by zero, an Inf or a NaN there would still poison the outputs, and no finite input
shows the difference.  So the inputs here are not finite where the kernels must not look:

* outside the read set (tests/read_set.py) the grid holds NaN ([sc][sym] layout) or +-Inf ([sym][sc] layout, odd row
  pitch), and the pilots are cut from a wider tensor that holds the same: all six outputs must be bit-identical to the
  dense, clean run;
* one read-set RE of one item and one pilot entry of another slot hold NaN: every other item must be bit-identical to
  the clean run, and the poisoned items' noise, RSRP, EPRE and CFO must be NaN exactly where the complex128 oracle's are.

B = 5 slots x R = 2 ports: the wave-per-item kernel (four items per workgroup, ce_narrow_kernel.h) fills two workgroups and
leaves a ragged third; the poisoned item sits in the middle of the second, the poisoned slot is the ragged third."""
import zlib

import numpy as np
import pytest
import torch

import ce_oracle as O
import kernel_variants as K
import read_set as RS
from srsran_ce_pytorch_amd import estimator as E, synth as S

pytestmark = pytest.mark.gpu

B, R = 5, 2
POISON_SLOT, POISON_PORT = 2, 1          # item 5: the second of the wave-per-item kernel's workgroups, not at its edge
POISON_PILOT_SLOT = 4                    # items 8, 9: the ragged last workgroup
NAN = complex(np.nan, np.nan)
PAD_SC, PAD_SYM = 12, 1                  # outside the view: subcarriers below and above, symbols before and after

REPS = K.representatives()
NAMES = ("ch_est", "noise", "rsrp", "epre", "ta", "cfo")


def _bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int64)


def _run(plan, g, p):
    out = E.estimate_with_plan(plan, g, p)
    torch.cuda.synchronize()
    return [_bits(t).cpu() for t in out]


def _same(got, ref, what, skip=()):
    for nm, g, r in zip(NAMES, got, ref):
        diff = (g != r).reshape(B * R, -1).any(dim=1)
        bad = [i for i in torch.nonzero(diff).flatten().tolist() if i not in skip]
        assert not bad, f"{what}: {nm} of item(s) {bad} differs from the clean run"


@pytest.mark.parametrize("rep", REPS, ids=[r[0] for r in REPS])
def test_variant_reads_only_its_read_set(rep):
    vid, want, case, interp = rep
    assert K.variant_of(K.derive_case(case, interp), case["n_sym"], interp) == want, f"{vid}: the policy moved"
    dev = torch.device("cuda:0")
    b = S.build_case(case, B * R)
    n_sc, n_sym, L = 12 * case["n_prb_grid"], case["n_sym"], case["n_layers"]
    n_re, n_dm = b.pilots.shape[:2]
    plan = E.make_plan(b.hop1, b.hop2, b.config, b.beta, L, case["n_prb_grid"], n_sym, dev, interp)
    grids = b.grids.reshape(B, R, n_sc, n_sym)
    pilots = np.broadcast_to(b.pilots, (B, n_re, n_dm, L)).copy()
    rs = RS.read_set(case)
    ref = _run(plan, torch.as_tensor(grids, device=dev), torch.as_tensor(pilots, device=dev))

    # NaN outside the read set, [sc][sym] layout: a slice of a NaN-filled buffer with an extra port, subcarriers and symbols
    big = np.full((B, R + 1, n_sc + 2 * PAD_SC, n_sym + 2 * PAD_SYM), NAN, np.complex64)
    inner = big[:, :R, PAD_SC:PAD_SC + n_sc, PAD_SYM:PAD_SYM + n_sym]
    inner[:, :, rs] = grids[:, :, rs]
    wide = np.full((B, n_re + 1, n_dm + 1, L + 1), NAN, np.complex64)
    wide[:, :n_re, :n_dm, :L] = pilots
    g = torch.as_tensor(big, device=dev)[:, :R, PAD_SC:PAD_SC + n_sc, PAD_SYM:PAD_SYM + n_sym]
    p = torch.as_tensor(wide, device=dev)[:, :n_re, :n_dm, :L]
    _same(_run(plan, g, p), ref, f"{vid}: NaN outside the read set")

    # +Inf (even items) / -Inf (odd items) outside the read set, [sym][sc] layout with a row pitch of n_sc + 1
    sign = np.ones((B, R + 1))                                                      # the spare port: +Inf
    sign[:, :R] = np.where(np.arange(B * R).reshape(B, R) % 2 == 0, 1.0, -1.0)      # item s R + r
    big = np.empty((B, R + 1, n_sym + 2 * PAD_SYM, n_sc + 1), np.complex64)
    big.real[...] = big.imag[...] = (sign * np.inf)[:, :, None, None]
    inner = big[:, :R, PAD_SYM:PAD_SYM + n_sym, :n_sc].transpose(0, 1, 3, 2)
    inner[:, :, rs] = grids[:, :, rs]
    wide = np.full((B, n_re + 1, n_dm + 1, L + 1), complex(np.inf, -np.inf), np.complex64)
    wide[:, :n_re, :n_dm, :L] = pilots
    g = torch.as_tensor(big, device=dev)[:, :R, PAD_SYM:PAD_SYM + n_sym, :n_sc].permute(0, 1, 3, 2)
    p = torch.as_tensor(wide, device=dev)[:, :n_re, :n_dm, :L]
    _same(_run(plan, g, p), ref, f"{vid}: +-Inf outside the read set, sym-major rows")

    # item isolation: NaN at one read-set RE of one item and at one pilot entry of another slot
    rng = np.random.default_rng(zlib.crc32(vid.encode()))
    members = np.argwhere(rs)
    sc, sym = members[rng.integers(len(members))]
    pe = tuple(int(rng.integers(n)) for n in (n_re, n_dm, L))
    pg, pp = grids.copy(), pilots.copy()
    pg[POISON_SLOT, POISON_PORT, sc, sym] = NAN
    pp[(POISON_PILOT_SLOT,) + pe] = NAN
    got = _run(plan, torch.as_tensor(pg, device=dev), torch.as_tensor(pp, device=dev))
    hit = {POISON_SLOT * R + POISON_PORT: (POISON_SLOT, POISON_PORT)} | {POISON_PILOT_SLOT * R + r: (POISON_PILOT_SLOT, r) for r in range(R)}
    what = f"{vid}: NaN at RE ({sc}, {sym}) of item {POISON_SLOT * R + POISON_PORT} and pilot {pe} of slot {POISON_PILOT_SLOT}"
    _same(got, ref, what, skip=hit)
    scal = [t.view(torch.float64).numpy().reshape(B * R) for t in got[1:]]
    for i, (s, r) in hit.items():
        _, noise, rsrp, epre, _, cfo = O.srs_channel_estimator(pg[s, r].astype(np.complex128), pp[s].astype(np.complex128),
                                                               b.beta, b.hop1, b.hop2, b.config, interp=interp)
        for nm, k, o in (("noise", 0, noise), ("rsrp", 1, rsrp), ("epre", 2, epre)) + ((("cfo", 4, cfo),) if cfo is not None else ()):
            assert np.isnan(scal[k][i]) == np.isnan(o), f"{what}: item {i} {nm} {scal[k][i]} vs the oracle's {o}"
