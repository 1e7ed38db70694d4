#!/usr/bin/env python3
"""Dev tool (GPU box): what PRACH preamble detection (include/ce_tp.h `ce_prach_detect`) costs at one long-format load
(L = 839, N = 1024: 64 windows of N_CS = 13, 8 roots, 4 ports x 1 repetition, 256 occasions) and one short-format load (L = 139,
N = 256: 10 windows of N_CS = 13, 6 roots, 4 ports x 12 repetitions, 512 occasions), both non-coherent, each with enough
(occasion, root) workgroups to fill the chip several times.  Three timings alternate in one process:

  (a) PrachDetector, one launch per batch (peak, delay and mean; no profile)            device events, LAUNCHES launches per repeat
  (b) the torch composition of the same operator: the zero-padded product with the      the same
      root table, torch.fft.ifft over N, abs()^2 summed over the terms, the mean, and
      the maximum over the gathered windows
  (c) PuschOfdmDemodulator (14 symbols x 4 ports per slot, the widest grid N holds)       the same
      running the same number of N-point transforms: the project's own transform rate

Writes the times, their spread, the time per N-point transform, (a)/(b) and (a)/(c), and how far (a) and (b) agree, to
profiles/prach_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

import numpy as np
import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import ofdm as OF, prach as PR

# (L, N, n_cs, n_shifts, roots, ports, repetitions, occasions)
LOADS = ((839, 1024, 13, 64, (1, 838, 420, 2, 837, 3, 836, 5), 4, 1, 256),
         (139, 256, 13, 10, (1, 138, 70, 2, 137, 3), 4, 12, 512))


def describe(L, N, n_cs, n_shifts, roots, R, S, B):
    view, ws, wl = PR.derive_host(L, N, roots, n_cs, n_shifts)
    radix = " ".join(str(r) for r in view.radix[:view.n_passes])
    n_tr = B * len(roots) * R * S
    return view, ws, wl, n_tr, (f"L={L}, N={N}, N_CS={n_cs}: {n_shifts} windows of {wl}, {len(roots)} roots, {R} ports x {S} repetitions (non-coherent), {B} occasions: "
                                f"{B * len(roots)} workgroups of {view.threads} threads, {view.rows_per_workgroup} term(s) at a time ({view.threads_per_row} threads each), "
                                f"radices {radix}, {view.lds_bytes} B LDS, {n_tr} transforms of {N} points, {8 * B * R * S * L / 1e6:.1f} MB of y")


def main():
    ap = parser(__doc__, "prach_perf")
    ap.add_argument("--occasions-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    loads = [(*ld[:-1], max(1, int(ld[-1] * args.occasions_scale))) for ld in LOADS]

    lines = [f"tools/prach_perf.py: {args.launches} launches x {args.repeats} repeats, alternating (a) (b) (c)"]
    if args.rehearse:
        print("\n".join(lines + [describe(*ld)[-1] + " -- not measured" for ld in loads]))
        return

    dev = gpu("prach_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(19)
    for ld in loads:
        L, N, n_cs, n_shifts, roots, R, S, B = ld
        view, ws, wl, n_tr, text = describe(*ld)
        det = PR.PrachDetector(L, N, roots, n_cs, n_shifts, device=dev)
        # noise of power 0.25 and, in every occasion, one unit preamble of root 0 in window 1, 0.4 N_CS late
        y = torch.view_as_complex(torch.empty((B, R, S, L, 2), dtype=torch.float32, device=dev).normal_(std=float(np.sqrt(0.125)), generator=g))
        y += torch.as_tensor(PR.prach_preamble_freq(roots[0], n_cs, L, 0.4 * n_cs).astype(np.complex64), device=dev)
        _, table = PR.tables(L, N, roots)
        table_d = torch.as_tensor(table, device=dev)
        idx = torch.as_tensor((ws.astype(np.int64)[:, None] + np.arange(wl)[None, :]) % N, device=dev)
        zpad = torch.zeros((B, len(roots), R * S, N), dtype=torch.complex64, device=dev)

        def composition():
            zpad[..., :L] = y.reshape(B, 1, R * S, L) * table_d[None, :, None, :]
            t = torch.fft.ifft(zpad, dim=-1)
            P = (t.real.square() + t.imag.square()).sum(2) * float((N / L) ** 2)
            peak, d = P[..., idx].max(-1)
            return peak, d, P.mean(-1)

        # (c): the same number of N-point transforms through the OFDM demodulator
        cp = OF.nr_cp_lengths(30e3, N)
        n_prb = min(N // 12, 275)
        dem = OF.PuschOfdmDemodulator(N, n_prb, cp, device=dev)
        slots = -(-n_tr // (14 * 4))
        samples = torch.view_as_complex(torch.empty((slots, 4, dem.n_samples, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        grid = torch.empty((slots, 4, 14, 12 * n_prb), dtype=torch.complex64, device=dev)

        fns = dict(a=lambda: det(y), b=composition, c=lambda: dem(samples, out=grid))
        for fn in fns.values():                                      # warm-up: code objects, plans, allocator
            timed(fn, 3)
        out, (peak_b, d_b, mean_b) = det(y), composition()
        torch.cuda.synchronize()
        rel = float(((out.peak - peak_b).abs() / peak_b).max())
        same = float((out.delay == d_b).float().mean())
        rel_mean = float(((out.mean - mean_b).abs() / mean_b).max())
        found = float((out.peak[:, 0, 1] > 10.0 * out.mean[:, 0]).float().mean())
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        ratio = lambda p, q_: f"{m[p] / m[q_]:.3f}   (per repeat {min(u / w for u, w in zip(t[p], t[q_])):.3f} .. {max(u / w for u, w in zip(t[p], t[q_])):.3f})"   # noqa: E731
        per = lambda k, n: f"{m[k] * 1e6 / n:8.2f} ns per transform"   # noqa: E731
        lines += [text,
                  f"  (a) detector, one launch                 {stats(t['a'])}   {per('a', n_tr)}   {B * len(roots) / m['a'] / 1e3:.2f} M (occasion, root) per s",
                  f"  (b) torch composition                    {stats(t['b'])}   {per('b', n_tr)}",
                  f"  (c) OFDM demodulator, {slots * 56} transforms   {stats(t['c'])}   {per('c', slots * 56)}",
                  f"  (a)/(b) = {ratio('a', 'b')}",
                  f"  (a)/(c) = {ratio('a', 'c')}   per transform: {(m['a'] / n_tr) / (m['c'] / (slots * 56)):.3f}",
                  f"  (a) against (b): max relative difference of peak {rel:.2e}, of mean {rel_mean:.2e}; equal delays in {100 * same:.2f} % of the windows; "
                  f"the preamble found (peak > 10 mean) in {100 * found:.1f} % of the occasions"]
        del det, dem, y, zpad, samples, grid, fns, table_d, idx
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
