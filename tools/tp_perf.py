#!/usr/bin/env python3
"""Dev tool (GPU box): what the transform de-precoding extension (include/ce_tp.h) costs -- 8192 slots of S = 12 data
symbols at n_prbs = 1, 6, 25, 100 and 270 (M = 12 n_prbs), x_hat complex64 and nvar float32 in, x_out and nvar_out out
(24 bytes per RE).  Two timings alternate in one process:

  (a) PuschTransformDeprecoder out of place, one launch                             device events, LAUNCHES launches per repeat
  (b) a device-to-device Tensor.copy_ of a buffer of (input + output bytes) / 2     the same

(b) reads and writes the same total as (a) reads and writes.  Writes per-row time, means and spread, (a)/(b) and the TB/s
each implies on its own bytes to profiles/tp_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and
measures nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import deprecode as DP

SLOTS, SYMBOLS, PRBS = 8192, 12, (1, 6, 25, 100, 270)


def describe(n_prbs):
    v = DP.derive_host(n_prbs, SYMBOLS)
    radix = " ".join(str(r) for r in v.radix[:v.n_passes])
    return v, (f"n_prbs={n_prbs}: M = {v.m_sc}, radices {radix}; {v.rows_per_workgroup} row(s) per workgroup of {v.threads} threads "
               f"({v.threads_per_row} per row), {v.n_workgroups_per_slot} workgroup(s) per slot, {v.lds_bytes} B LDS, {v.twiddle_bytes} B twiddles")


def main():
    ap = parser(__doc__, "tp_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch size (a smaller card)")
    args = ap.parse_args()
    B = max(1, int(SLOTS * args.slots_scale))

    lines = [f"tools/tp_perf.py: {B} slots x S = {SYMBOLS} data symbols; {args.launches} launches x {args.repeats} repeats, alternating (a) (b)"]
    if args.rehearse:
        print("\n".join(lines + [describe(n)[1] + " -- not measured" for n in PRBS]))
        return

    dev = gpu("tp_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for n_prbs in PRBS:
        v, text = describe(n_prbs)
        n = SYMBOLS * v.m_sc
        tp = DP.PuschTransformDeprecoder(n_prbs, SYMBOLS, device=dev)
        x_hat = torch.view_as_complex(torch.empty((B, n, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        nvar = torch.empty((B, n), dtype=torch.float32, device=dev).uniform_(0.01, 2.0, generator=g)
        out, nvar_out = torch.empty_like(x_hat), torch.empty_like(nvar)
        bytes_a = B * n * 24
        src = torch.empty((bytes_a // 2,), dtype=torch.uint8, device=dev).random_(generator=g)
        dst = torch.empty_like(src)
        a = lambda: tp(x_hat, nvar, out=out, nvar_out=nvar_out)      # noqa: E731
        b = lambda: dst.copy_(src)                                   # noqa: E731
        for fn in (a, b):                                            # warm-up: code objects, allocator
            timed(fn, 3)
        assert bool(torch.isfinite(nvar_out[:: max(1, B // 8)]).all()) and bool(torch.isfinite(torch.view_as_real(out[:: max(1, B // 8)])).all())
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb.append(timed(b, args.launches))
        ma, mb = statistics.mean(ta), statistics.mean(tb)
        rows = B * SYMBOLS
        lines += [text,
                  f"  (a) PuschTransformDeprecoder, one launch   {stats(ta)}   {ma * 1e6 / rows:8.2f} ns per row   {bytes_a / ma / 1e9:6.2f} TB/s on {bytes_a / 1e9:.3f} GB (x_hat, nvar in; x_out, nvar_out out)",
                  f"  (b) copy_ of {src.numel() / 1e9:6.3f} GB                     {stats(tb)}   {'':8}               {2 * src.numel() / mb / 1e9:6.2f} TB/s on {2 * src.numel() / 1e9:.3f} GB (read + written)",
                  f"  (a)/(b) = {ma / mb:.3f}   (per repeat {min(p / q for p, q in zip(ta, tb)):.3f} .. {max(p / q for p, q in zip(ta, tb)):.3f})"]
        del tp, x_hat, nvar, out, nvar_out, src, dst
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
