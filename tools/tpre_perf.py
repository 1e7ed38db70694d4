#!/usr/bin/env python3
"""Dev tool (GPU box): what transform precoding (include/ce_tp.h `ce_tp_precode`) costs -- slots of S = 12 data symbols at
n_prbs = 4, 25, 125 and 270 (M = 48, 300, 1500, 3240), complex64 in and out (16 bytes per RE).  Four timings alternate in one
process:

  (a) PuschTransformPrecoder.grid_: in place on the data rows of a 273-PRB grid      device events, LAUNCHES launches per repeat
      [B, 1, 14, 3276] (allocation at PRB 3, DM-RS on symbols 2 and 11)
  (b) PuschTransformPrecoder on dense rows [B, S M], in place (out = x)               the same
  (c) PuschTransformDeprecoder at the same M, S and B, out of place (24 bytes per RE) the same
  (d) an in-place elementwise pass over the dense rows (float32 mul_ by 1)            the same

(d) reads and writes what (a) and (b) read and write.  Writes the four times, their spread, the GB/s each implies on its
own bytes, (a)/(d), (b)/(d) and (b) against 16/24 of (c) to profiles/tpre_perf.txt (--out).  `--rehearse` runs the
host-side logic without a GPU and measures nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import deprecode as DP, modulator as MD, precode as PR, synth as S

SYMBOLS, N_PRB_GRID, PRB_START = 12, 273, 3
SHAPES = ((4, 8192), (25, 8192), (125, 4096), (270, 2048))          # (n_prbs, slots): at least 24576 workgroups per launch


def modulator(n_prbs, device=None):
    case = S.case_spec("tpre_perf", N_PRB_GRID, [S.hop_spec([2, 11], PRB_START, n_prbs)])
    h1, h2, _ = S.numpy_hops(case)
    return MD.PuschModulator(h1, h2, 1, N_PRB_GRID, "16qam", device=device)


def describe(n_prbs, B):
    v = DP.derive_host(n_prbs, SYMBOLS)
    pre = PR.PuschTransformPrecoder.for_modulator(modulator(n_prbs))
    assert pre.n_symbols == SYMBOLS and pre.row_offsets[0] == 12 * PRB_START
    radix = " ".join(str(r) for r in v.radix[:v.n_passes])
    return v, (f"n_prbs={n_prbs}: M = {v.m_sc}, {B} slots, radices {radix}; {v.rows_per_workgroup} row(s) per workgroup of {v.threads} threads "
               f"({v.threads_per_row} per row), {B * v.n_workgroups_per_slot} workgroups, {v.lds_bytes} B LDS; grid rows at "
               f"{pre.row_offsets[0]}, {pre.row_offsets[1]}, .. of a slot of {pre.slot_stride}")


def main():
    ap = parser(__doc__, "tpre_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    shapes = [(n, max(1, int(B * args.slots_scale))) for n, B in SHAPES]

    lines = [f"tools/tpre_perf.py: S = {SYMBOLS} data symbols; {args.launches} launches x {args.repeats} repeats, alternating (a) (b) (c) (d)"]
    if args.rehearse:
        print("\n".join(lines + [describe(n, B)[1] + " -- not measured" for n, B in shapes]))
        return

    dev = gpu("tpre_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    for n_prbs, B in shapes:
        v, text = describe(n_prbs, B)
        n = SYMBOLS * v.m_sc
        grid_pre = PR.PuschTransformPrecoder.for_modulator(modulator(n_prbs, device=dev))
        pre = PR.PuschTransformPrecoder(n_prbs, SYMBOLS, device=dev)
        tp = DP.PuschTransformDeprecoder(n_prbs, SYMBOLS, device=dev)
        tx = torch.view_as_complex(torch.empty((B, 1, 14, 12 * N_PRB_GRID, 2), dtype=torch.float32, device=dev).normal_(generator=g)).permute(0, 1, 3, 2)
        x = torch.view_as_complex(torch.empty((B, n, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        xr = torch.view_as_real(x)
        x_hat = torch.view_as_complex(torch.empty((B, n, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        nvar = torch.empty((B, n), dtype=torch.float32, device=dev).uniform_(0.01, 2.0, generator=g)
        out, nvar_out = torch.empty_like(x_hat), torch.empty_like(nvar)
        fns = dict(a=lambda: grid_pre.grid_(tx), b=lambda: pre(x, out=x), c=lambda: tp(x_hat, nvar, out=out, nvar_out=nvar_out), d=lambda: xr.mul_(1.0))
        for fn in fns.values():                                      # warm-up: code objects, allocator
            timed(fn, 3)
        assert bool(torch.isfinite(xr[:: max(1, B // 8)]).all()) and bool(torch.isfinite(torch.view_as_real(tx[:: max(1, B // 8)])).all())
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        b16, b24 = B * n * 16, B * n * 24
        ratio = lambda p, q, f=1.0: f"{m[p] / (f * m[q]):.3f}   (per repeat {min(u / (f * w) for u, w in zip(t[p], t[q])):.3f} .. {max(u / (f * w) for u, w in zip(t[p], t[q])):.3f})"   # noqa: E731
        lines += [text,
                  f"  (a) precoder, in place on the grid     {stats(t['a'])}   {m['a'] * 1e6 / (B * SYMBOLS):8.2f} ns per row   {b16 / m['a'] / 1e6:8.1f} GB/s on {b16 / 1e9:.3f} GB",
                  f"  (b) precoder, dense rows in place      {stats(t['b'])}   {m['b'] * 1e6 / (B * SYMBOLS):8.2f} ns per row   {b16 / m['b'] / 1e6:8.1f} GB/s on {b16 / 1e9:.3f} GB",
                  f"  (c) de-precoder, out of place          {stats(t['c'])}   {m['c'] * 1e6 / (B * SYMBOLS):8.2f} ns per row   {b24 / m['c'] / 1e6:8.1f} GB/s on {b24 / 1e9:.3f} GB",
                  f"  (d) elementwise mul_ in place          {stats(t['d'])}   {'':8}               {b16 / m['d'] / 1e6:8.1f} GB/s on {b16 / 1e9:.3f} GB",
                  f"  (a)/(d) = {ratio('a', 'd')}",
                  f"  (b)/(d) = {ratio('b', 'd')}",
                  f"  (b)/(16/24 (c)) = {ratio('b', 'c', 16.0 / 24.0)}"]
        del grid_pre, pre, tp, tx, x, xr, x_hat, nvar, out, nvar_out, fns
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
