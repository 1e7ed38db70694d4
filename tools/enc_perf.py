#!/usr/bin/env python3
"""Dev tool (GPU box): what the transport-block encoder extension (include/ce_enc.h) costs on random transport blocks, on
seeded random graphs with the NR core (tests/enc_oracle.py `nr_core_graph`), at

  8192 slots of A = 8424 on BG1, QPSK, G = 16896            C = 1, Zc = 384: one launch, g gathered from LDS
  64 slots of A = 1277992 on BG1, 64QAM x 4 layers          C = 152, Zc = 384 (the largest NR transport block), twice:
      G = 1896960   every E_r = 12480, a multiple of 32: one launch
      G = 1897032   E_r = 12480 / 12504: blocks meet inside a dword of g, so the codewords go through `cw` and a second
                    launch gathers g from them

Timings alternate in one process, all through preallocated tensors:

  (a) ce_enc_encode                                         device events, LAUNCHES launches per repeat
  (b) a device-to-device Tensor.copy_ of the same `g` bytes the same
  (c) PuschLdpcDecoder on the same blocks: the rate recovery of +-64 LLRs of (a)'s g, 8 iterations at most, early stop -- clean
      codewords, so the least a decode costs
  (d) the same decoder without early stop: 8 iterations

Writes ms per call (mean and range over the repeats), (a)/(b), (a)/(c), (a)/(d) and code blocks/s to profiles/enc_perf.txt
(--out).  (a) and (b) at the second shape are a few tens of microseconds of device work per call, so their figures hold the
launch path too; kernel times come from a kernel trace of this tool, in a run of its own.  There is no pass mark.
`--rehearse` runs the host-side logic without a GPU and measures nothing."""
import ctypes as C
import statistics
import sys

import numpy as np
import torch

from _perf_common import ROOT, finish, gpu, parser, stats, timed

sys.path.insert(0, str(ROOT / "tests"))
import enc_oracle as E  # noqa: E402

from srsran_ce_pytorch_amd import encoder as EN, ldpc as LD, ratematch as RM  # noqa: E402

SHAPES = ((8192, 1, 8424, 2, 1, 16896), (64, 1, 1277992, 6, 4, 1896960), (64, 1, 1277992, 6, 4, 1897032))      # slots, base graph, A, Qm, layers, G


def graph(bg, zc):
    sh = E.SHAPE[bg]
    rows = E.nr_core_graph(np.random.default_rng(31), sh["n_sys"], sh["n_rows"], zc, sh["core_degree"], sh["ext"], 0)
    return LD.LdpcGraph(rows, sh["n_sys"] + sh["n_rows"])


def describe(slots, bg, A, qm, L, G):
    v = RM.derive_host(bg, A, qm, L, G)
    gr = graph(bg, v.zc)
    e = EN.derive_host(bg, A, qm, L, G, gr)
    launches = "two launches, g gathered from cw" if e.cw_required else "one launch, g gathered from LDS"
    return gr, e, (f"{slots} slots x A = {A} on BG{bg}, Qm = {qm}, {L} layers, G = {G}: C = {e.c}, Zc = {e.zc}, K' = {e.k_prime}, N_cb = {e.n_cb}, E_r = {e.e_lo}"
                   f"{'' if e.n_lo == e.c else f' / {e.e_hi}'}, {e.rows_needed} of {gr.n_rows} rows reach the buffer; tb {slots * e.tb_row_bytes / 1e6:.2f} MB, "
                   f"g {slots * e.g_row_bytes / 1e6:.2f} MB, cw {slots * e.c * e.cw_row_bytes / 1e6:.2f} MB; {slots * e.c} workgroups of {e.threads} threads, "
                   f"{e.lds_bytes} B LDS; {launches}")


def llr_of(g, n_bits):
    shifts = torch.arange(7, -1, -1, device=g.device, dtype=torch.int16)
    bits = ((g.to(torch.int16).unsqueeze(-1) >> shifts) & 1).reshape(g.shape[0], -1)[:, :n_bits]
    return (64 - 128 * bits).to(torch.int8).contiguous()


def measure(args):
    dev = gpu("enc_perf")
    gen = torch.Generator(device=dev)
    gen.manual_seed(19)
    lines = []
    for slots, bg, A, qm, L, G in SHAPES:
        S = max(1, int(slots * args.slots_scale))
        gr, e, text = describe(S, bg, A, qm, L, G)
        rm = RM.PuschRateRecovery(bg, A, qm, L, G, device=dev)
        enc = EN.PuschTransportEncoder.for_rate_recovery(rm, gr)
        tb = torch.empty((S, enc.tb_row_bytes), dtype=torch.uint8, device=dev).random_(generator=gen)
        rv = torch.zeros(1, dtype=torch.int32, device=dev)
        g, cw = enc(tb, rv=0, return_codeword=True)      # creates the plan; the launches below reuse these tensors
        soft = rm(llr_of(g, G), rv=0)
        decs = [LD.PuschLdpcDecoder.for_rate_recovery(rm, gr, max_iters=8, early_stop=stop) for stop in (True, False)]
        hard, status = decs[0](soft)
        ok = bool((status[..., 1] == 1).all())
        dst = torch.empty_like(g)
        ptrs = [C.c_void_p(t.data_ptr()) for t in (tb, rv, g, cw)]
        a = lambda: enc._launch(ptrs[0], ptrs[1], 0, S, ptrs[2], ptrs[3] if enc.needs_codeword else None)      # noqa: E731
        b = lambda: dst.copy_(g)                                                                                  # noqa: E731
        c, d = (lambda dec=dec: dec(soft) for dec in decs)
        for fn in (a, b, c, d):
            timed(fn, 2)
        t = {k: [] for k in "abcd"}
        for _ in range(args.repeats):
            t["a"].append(timed(a, args.launches))
            t["b"].append(timed(b, args.launches))
            t["c"].append(timed(c, args.dec_launches))
            t["d"].append(timed(d, args.dec_launches))
        m = {k: statistics.mean(v) for k, v in t.items()}
        nb = S * e.c
        lines += [f"{text}",
                  f"  (a) ce_enc_encode                      {stats(t['a'])}   {nb / m['a'] / 1e3:8.2f} M code blocks/s   {g.numel() / m['a'] / 1e6:8.1f} GB/s of g written",
                  f"  (b) copy_ of g, {g.numel() / 1e6:7.2f} MB             {stats(t['b'])}   {g.numel() / m['b'] / 1e6:8.1f} GB/s read and as much written",
                  f"  (c) decoder, early stop (all parity ok: {ok})   {stats(t['c'])}   {nb / m['c'] / 1e3:8.2f} M code blocks/s",
                  f"  (d) decoder, 8 iterations              {stats(t['d'])}   {nb / m['d'] / 1e3:8.2f} M code blocks/s",
                  f"  (a)/(b) = {m['a'] / m['b']:.3f}   (a)/(c) = {m['a'] / m['c']:.4f}   (a)/(d) = {m['a'] / m['d']:.4f}"]
        del enc, rm, decs, tb, g, cw, soft, hard, status, dst
        torch.cuda.empty_cache()
    return lines


def main():
    ap = parser(__doc__, "enc_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    ap.add_argument("--dec-launches", type=int, default=3, help="launches per repeat of the decoder timings")
    args = ap.parse_args()
    if args.launches < 50 and not args.rehearse:
        args.launches = 50                                          # tens of microseconds per call: a window of 20 calls times the clock
    head = [f"tools/enc_perf.py: random transport blocks, rv 0; {args.launches} launches x {args.repeats} repeats of (a) (b), {args.dec_launches} of (c) (d), alternating"]
    if args.rehearse:
        print("\n".join(head + [describe(*s)[2] + " -- not measured" for s in SHAPES]))
        return
    lines = head + measure(args)
    lines[0] += f"; {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    finish(lines, args.out)


if __name__ == "__main__":
    main()
