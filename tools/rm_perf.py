#!/usr/bin/env python3
"""Dev tool (GPU box): what the rate-recovery extension (include/ce_rm.h) costs at the headline geometry -- 8192 slots of
G = 273 * 12 * 12 * Qm LLRs (273 PRB, 12 data symbols, L = 1), Qm = 2 and 8, float32 and int8, without and with a kept HARQ
buffer (a separate tensor of the output's shape), one rv per slot on the device.  The transport block is the largest
A <= G / 2 (a multiple of 8) on base graph 1 that segments evenly and keeps every E_r <= P, so no position is hit twice; the
tool prints A, the base graph and the resulting C.  Two timings alternate in one process:

  (a) PuschRateRecovery, one launch                                                 device events, LAUNCHES launches per repeat
  (b) a device-to-device Tensor.copy_ of a buffer of (input + output bytes) / 2     the same

(b) reads and writes the same total as (a) reads and writes.  Writes means and spread, (a)/(b) and the TB/s each implies on
its own bytes to profiles/rm_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import ratematch as RM

SLOTS, M, BG, LAYERS = 8192, 273 * 12 * 12, 1, 1
CONFIGS = [(qm, fmt, harq) for qm in (2, 8) for fmt in (torch.float32, torch.int8) for harq in (False, True)]


def choose_tbs(qm):
    """The largest A <= G / 2, a multiple of 8, that the library accepts on BG1 with every E_r <= P."""
    G = M * qm
    for A in range(G // 2 // 8 * 8, 0, -8):
        try:
            v = RM.derive_host(BG, A, qm, LAYERS, G)
        except ValueError:
            continue
        if v.e_hi <= v.p:
            return A, v
    raise SystemExit(f"no transport block size fits G={G}")


def main():
    ap = parser(__doc__, "rm_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch size (a smaller card)")
    args = ap.parse_args()
    B = max(1, int(SLOTS * args.slots_scale))

    lines = [f"tools/rm_perf.py: {B} slots x G = {M} x Qm LLRs (273 PRB x 12 data symbols, L = {LAYERS}); {args.launches} launches x {args.repeats} repeats, alternating (a) (b)"]
    shapes = {}
    for qm in (2, 8):
        A, v = choose_tbs(qm)
        shapes[qm] = (A, v)
        lines.append(f"Qm={qm}: G = {M * qm}, A = {A} on BG{BG} (rate {A / (M * qm):.3f}): C = {v.c}, Zc = {v.zc}, N_cb = {v.n_cb}, fillers [{v.f0}, {v.f1}), "
                     f"P = {v.p}, E_r = {v.e_lo} x {v.n_lo} + {v.e_hi} x {v.c - v.n_lo}; output {v.c * v.n_cb} elements per slot")
    if args.rehearse:
        print("\n".join(lines))
        for qm, fmt, harq in CONFIGS:
            v = RM.derive_host(BG, shapes[qm][0], qm, LAYERS, M * qm, fmt)
            print(f"Qm={qm} {fmt} harq={harq}: {v.n_tiles} workgroups per slot of {v.unit_elems} element(s) per 4-byte unit -- not measured")
        return

    dev = gpu("rm_perf")

    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def draw(shape, fmt):
        if fmt == torch.int8:
            return torch.randint(-60, 61, shape, dtype=torch.int8, device=dev, generator=g)
        return torch.empty(shape, dtype=torch.float32, device=dev).normal_(std=4.0, generator=g)

    rv = torch.randint(0, 4, (B,), dtype=torch.int32, device=dev, generator=g)
    for qm, fmt, with_harq in CONFIGS:
        A, v = shapes[qm]
        G, es = M * qm, 1 if fmt == torch.int8 else 4
        rm = RM.PuschRateRecovery(BG, A, qm, LAYERS, G, dtype=fmt, filler_llr=100.0, device=dev)
        llr = draw((B, G), fmt)
        harq = draw((B, v.c, v.n_cb), fmt) if with_harq else None
        out = torch.empty((B, v.c, v.n_cb), dtype=fmt, device=dev)
        bytes_in = (llr.numel() + (harq.numel() if with_harq else 0)) * es
        bytes_a = bytes_in + out.numel() * es
        src = torch.empty((bytes_a // 2,), dtype=torch.uint8, device=dev).random_(generator=g)
        dst = torch.empty_like(src)
        a = lambda: rm(llr, rv, harq=harq, out=out)                  # noqa: E731
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
        lines += [f"Qm={qm}, {name}, harq {'on' if with_harq else 'off'}: in {bytes_in / 1e9:.2f} GB, out {out.numel() * es / 1e9:.2f} GB",
                  f"  (a) PuschRateRecovery, one launch        {stats(ta)}   {bytes_a / ma / 1e9:6.2f} TB/s on {bytes_a / 1e9:.2f} GB (LLRs{' and harq' if with_harq else ''} in, buffers out)",
                  f"  (b) copy_ of {src.numel() / 1e9:5.2f} GB                     {stats(tb)}   {2 * src.numel() / mb / 1e9:6.2f} TB/s on {2 * src.numel() / 1e9:.2f} GB (read + written)",
                  f"  (a)/(b) = {ma / mb:.3f}   (per repeat {min(p / q for p, q in zip(ta, tb)):.3f} .. {max(p / q for p, q in zip(ta, tb)):.3f})"]
        del rm, llr, harq, out, src, dst
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
