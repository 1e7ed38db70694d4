#!/usr/bin/env python3
"""Dev tool (GPU box): what the soft-demapper extension (include/ce_demod.h) costs at the headline geometry -- 8192 slots
of M = 273 * 12 * 12 symbols (273 PRB, DM-RS on symbols 2 and 11, L = 1), Qm = 2 and 8, float32 and int8 output,
descrambling off and on (per-slot rnti / n_id on the device).  Two timings alternate in one process:

  (a) PuschDemapper, one launch                                                     device events, LAUNCHES launches per repeat
  (b) a device-to-device Tensor.copy_ of a buffer of (input + output bytes) / 2     the same

(b) reads and writes the same total as (a) reads and writes.  Writes means and spread, (a)/(b) and the TB/s each implies on
its own bytes to profiles/demod_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import demod as DM

SLOTS, M = 8192, 273 * 12 * 12
CONFIGS = [(qm, fmt, descr) for qm in (2, 8) for fmt in (torch.float32, torch.int8) for descr in (False, True)]


def main():
    ap = parser(__doc__, "demod_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch size (a smaller card)")
    args = ap.parse_args()
    B = max(1, int(SLOTS * args.slots_scale))

    lines = [f"tools/demod_perf.py: {B} slots x {M} symbols (273 PRB x 12 data symbols, L = 1); {args.launches} launches x {args.repeats} repeats, alternating (a) (b)"]
    if args.rehearse:
        for qm, fmt, descr in CONFIGS:
            v = DM.derive_host(qm, M, fmt, 4.0, descr)
            print(f"Qm={qm} {fmt} descramble={descr}: {v.n_bits} LLRs per slot, {v.n_tiles} workgroups per slot, {v.n_blocks} Gold blocks, "
                  f"{v.table_bytes} table bytes -- not measured")
        return

    dev = gpu("demod_perf")

    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = torch.empty((B, M), dtype=torch.complex64, device=dev)
    torch.view_as_real(x).normal_(std=0.7071, generator=g)
    nvar = 10.0 ** -1.5 * (0.5 + 1.5 * torch.rand((B, M), dtype=torch.float32, device=dev, generator=g))
    rnti = torch.randint(0, 65536, (B,), dtype=torch.int32, device=dev, generator=g)
    n_id = torch.randint(0, 1024, (B,), dtype=torch.int32, device=dev, generator=g)
    for qm, fmt, descr in CONFIGS:
        dem = DM.PuschDemapper(qm, M, out_dtype=fmt, llr_scale=4.0, descramble=descr, device=dev)
        out = torch.empty((B, M * qm), dtype=fmt, device=dev)
        bytes_a = B * M * 12 + out.numel() * out.element_size()
        src = torch.empty((bytes_a // 2,), dtype=torch.uint8, device=dev).random_(generator=g)
        dst = torch.empty_like(src)
        a = (lambda: dem(x, nvar, rnti=rnti, n_id=n_id, out=out)) if descr else (lambda: dem(x, nvar, out=out))   # noqa: E731
        b = lambda: dst.copy_(src)                                   # noqa: E731
        for fn in (a, b):                                            # warm-up: code objects, allocator
            timed(fn, 3)
        assert bool(torch.isfinite(out[:: max(1, B // 8)].float()).all())
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb.append(timed(b, args.launches))
        ma, mb = statistics.mean(ta), statistics.mean(tb)
        name = "float32" if fmt == torch.float32 else "int8"
        lines += [f"Qm={qm}, {name} out, descrambling {'on' if descr else 'off'}: in {B * M * 12 / 1e9:.2f} GB, out {out.numel() * out.element_size() / 1e9:.2f} GB",
                  f"  (a) PuschDemapper, one launch            {stats(ta)}   {bytes_a / ma / 1e9:6.2f} TB/s on {bytes_a / 1e9:.2f} GB (x_hat and nvar in, LLRs out)",
                  f"  (b) copy_ of {src.numel() / 1e9:5.2f} GB                     {stats(tb)}   {2 * src.numel() / mb / 1e9:6.2f} TB/s on {2 * src.numel() / 1e9:.2f} GB (read + written)",
                  f"  (a)/(b) = {ma / mb:.3f}   (per repeat {min(p / q for p, q in zip(ta, tb)):.3f} .. {max(p / q for p, q in zip(ta, tb)):.3f})"]
        del dem, out, src, dst
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
