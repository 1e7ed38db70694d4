#!/usr/bin/env python3
"""Dev tool (GPU box): what the low-PAPR DM-RS generator (include/ce_dmrs.h `ce_dmrs_lp_generate`) costs -- at 273 PRB and at
6 PRB, DM-RS symbols [2, 11], 8192 slots, group hopping, per-slot device parameters.  Three timings alternate in one process:

  (a) PuschLowPaprDmrs                                                        device events, LAUNCHES launches per repeat
  (b) a plain device fill of the same number of bytes (the floor of this store stream)        the same
  (c) PuschDmrs, the Gold / QPSK generator, at the same shape (one layer)                     the same

Writes means and spread, (a)/(b), (c)/(b) and (a)/(c) to profiles/dmrs_lp_perf.txt (--out).  `--rehearse` builds the plans'
host views on a few slots without a GPU and measures nothing."""
import statistics

import numpy as np

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import dmrs, synth as S

SHAPES = [(273, 273), (6, 24)]      # (allocated PRBs, grid PRBs)


def main():
    ap = parser(__doc__, "dmrs_lp_perf", rehearse_help="host derivation only, no GPU, nothing measured, nothing written")
    ap.add_argument("--slots", type=int, default=8192)
    ap.add_argument("--hopping", default="group", choices=sorted(dmrs.HOPPING))
    args = ap.parse_args()

    rng = np.random.default_rng(1)
    B = 4 if args.rehearse else args.slots
    slots, n_ids = rng.integers(0, 20, B).astype(np.int32), rng.integers(0, 1008, B).astype(np.int32)
    lines = [f"tools/dmrs_lp_perf.py: DM-RS [2, 11], {B} slots, {args.hopping} hopping; {args.launches} launches x {args.repeats} repeats, alternating (a) (b) (c)"]
    cases = [(n_prb, S.case_spec(f"lp{n_prb}", grid, [S.hop_spec([2, 11], 0, n_prb)])) for n_prb, grid in SHAPES]
    if args.rehearse:
        for n_prb, case in cases:
            h1, h2, _ = S.numpy_hops(case)
            v = dmrs.derive_host_low_papr(h1, h2, case["n_prb_grid"], hopping=args.hopping, slots_per_frame=20)
            print(f"{n_prb} PRB: n_re {v.n_re}, {v.n_dmrs_total} columns, N = {v.n_zc}, {v.n_words} hopping words per row -- not measured")
        return

    import torch
    dev = gpu("dmrs_lp_perf")
    d_slot, d_id = torch.as_tensor(slots, device=dev), torch.as_tensor(n_ids, device=dev)
    d_scid = torch.zeros(1, dtype=torch.int32, device=dev)
    for n_prb, case in cases:
        h1, h2, _ = S.numpy_hops(case)
        lp = dmrs.PuschLowPaprDmrs(h1, h2, case["n_prb_grid"], hopping=args.hopping, slots_per_frame=20, device=dev)
        gold = dmrs.PuschDmrs(h1, h2, 1, case["n_prb_grid"], device=dev)
        out = torch.empty((B, lp.n_re, lp.n_dmrs_total, 1), dtype=torch.complex64, device=dev)
        out_gold = torch.empty_like(out)
        fill = torch.empty_like(out).view(torch.float32)
        nbytes = out.numel() * 8
        a = lambda: lp(d_slot, d_id, out=out)                             # noqa: E731
        b = lambda: fill.fill_(0.70710677)                                # noqa: E731
        c = lambda: gold(d_slot, d_id, d_scid, out=out_gold)              # noqa: E731
        for fn in (a, b, c):                                              # warm-up: code objects, allocator
            timed(fn, 3)
        ta, tb, tc = [], [], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb.append(timed(b, args.launches))
            tc.append(timed(c, args.launches))
        ma, mb, mc = (statistics.mean(x) for x in (ta, tb, tc))
        lines += [f"{n_prb} PRB: {nbytes / 1e6:.1f} MB per step ({nbytes // B} B per slot)",
                  f"  (a) PuschLowPaprDmrs kernel, per-slot device parameters   {stats(ta, 9)}   {nbytes / ma / 1e6:8.1f} GB/s",
                  f"  (b) device fill of the same bytes                         {stats(tb, 9)}   {nbytes / mb / 1e6:8.1f} GB/s",
                  f"  (c) PuschDmrs (Gold / QPSK) at the same shape, L = 1      {stats(tc, 9)}   {nbytes / mc / 1e6:8.1f} GB/s",
                  f"  (a)/(b) = {ma / mb:.3f}    (c)/(b) = {mc / mb:.3f}    (a)/(c) = {ma / mc:.3f}"]
        del out, out_gold, fill
        torch.cuda.empty_cache()
    lines.append("profiles/dmrs_perf.txt, the Gold generator's own run at 273 PRB, L = 1: (a)/(b) = 1.838")
    finish(lines, args.out)


if __name__ == "__main__":
    main()
