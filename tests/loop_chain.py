"""What the loop tests "transport block in, transport block out" share (test_zzzzzzzzz_hip_mod.py, test_zzzzzzzzzzz_hip_precode.py,
test_zzzzzzzzzzzz_hip_ofdm.py): the stage objects of one loop geometry of enc_oracle.LOOPS / mod_oracle.loop_case with the
encoded transport blocks and the pilots, and the receive side from the resource grid to the transport block.  Between the two
each test puts its own channel; every assertion stays in the test that makes it."""
from types import SimpleNamespace

import numpy as np
import torch

import enc_oracle as E
import mod_oracle as MO
import tb_oracle as TBO
from srsran_ce_pytorch_amd import demod as DM, deprecode as DP, dmrs as DR, encoder as EN, equalizer as EQ, estimator as ES, ldpc as LD
from srsran_ce_pytorch_amd import modulator as MD, precode as PR, ratematch as RM, synth as S, transportblock as TB


def build(name, dev):
    """The chain of loop geometry `name` on `dev`: the oracle's records (c, lp, case), the hops (h1, h2, cfg), L, qm and
    n_prb_grid, the stages rm, enc, dec, asm, eq, mod, dem, the transform pair pre, tp (None where the geometry has more than
    one layer, data on DM-RS symbols or a PRB count with a prime factor above 5), the packed transport blocks `sent` ([B, ..]
    uint8, host), their code bits `g` at rv 0 and the PuschDmrs pilots `pil`."""
    ch = SimpleNamespace(name=name, dev=dev, c=E.CASE_BY_NAME[name], lp=E.LOOPS[name], case=MO.loop_case(name))
    c, gr = ch.c, E.graph(name)
    ch.h1, ch.h2, ch.cfg = S.numpy_hops(ch.case)
    ch.L, ch.qm, ch.n_prb_grid = ch.lp["L"], ch.lp["qm"], ch.case["n_prb_grid"]
    graph = LD.LdpcGraph(gr.rows, gr.n_cols)
    ch.rm = RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], device=dev)
    ch.enc = EN.PuschTransportEncoder.for_rate_recovery(ch.rm, graph)
    ch.dec = LD.PuschLdpcDecoder.for_rate_recovery(ch.rm, graph)
    ch.asm = TB.PuschTransportBlock.for_rate_recovery(ch.rm)
    ch.eq = EQ.PuschEqualizer(ch.h1, ch.h2, ch.L, ch.n_prb_grid, device=dev)
    ch.mod = MD.PuschModulator.for_equalizer(ch.eq, ch.qm, scramble=True)
    ch.dem = DM.PuschDemapper(ch.qm, ch.eq.n_data_re * ch.L, out_dtype=torch.int8, llr_scale=4.0, descramble=True, device=dev)
    try:
        ch.pre, ch.tp = PR.PuschTransformPrecoder.for_modulator(ch.mod), DP.PuschTransformDeprecoder.for_equalizer(ch.eq)
    except ValueError:
        ch.pre = ch.tp = None
    ch.sent = TBO.pack(np.array(E.inputs(name)[0]), ch.enc.tb_row_bytes)
    ch.B = len(ch.sent)
    ch.g = ch.enc(torch.as_tensor(np.array(ch.sent), device=dev), rv=0)
    ch.pil = DR.PuschDmrs(ch.h1, ch.h2, ch.L, ch.n_prb_grid, device=dev)(MO.LOOP_SLOT, MO.LOOP_N_ID, MO.LOOP_N_SCID)
    return ch


def modulate(ch):
    """tx [B, L, n_sc, n_sym] of the chain's code bits and pilots, scrambled with LOOP_RNTI / LOOP_SCR_ID; a new tensor per call."""
    return ch.mod(ch.g, ch.pil[0].contiguous(), ch.case["beta"], rnti=MO.LOOP_RNTI, n_id=MO.LOOP_SCR_ID)


def receive(ch, rx, rnti=MO.LOOP_RNTI, deprecode=False):
    """(out, tb_status) on the host of the received grid rx [B, R, n_sc, n_sym]: estimate -> PuschEqualizer ->
    (PuschTransformDeprecoder) -> PuschDemapper(descramble, int8) -> PuschRateRecovery -> PuschLdpcDecoder -> PuschTransportBlock."""
    ch_est, noise, *_ = ES.estimate(rx, ch.pil[0], ch.case["beta"], ch.h1, ch.h2, ch.cfg)
    x, nv = ch.eq(rx, ch_est, noise)
    if deprecode:
        x, nv = ch.tp(x, nv)
    soft = ch.rm(ch.dem(x, nv, rnti=rnti, n_id=MO.LOOP_SCR_ID), rv=0)
    hard, status = ch.dec(soft)
    out, tb_status, cb_status = ch.asm(hard)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tb_status.cpu().numpy()
