#!/usr/bin/env python3
"""Dev tool (GPU box): what OFDM modulation (include/ce_tp.h `ce_ofdmtx_modulate`) costs -- the shapes of tools/ofdm_perf.py,
slots of 14 symbols on 4 ports at (N, n_prb_grid) = (4096, 273) and (1024, 52) at 30 kHz and (128, 10) at 15 kHz, the complex64
grid in (8 n_sc bytes per symbol) and the samples out (8 (N + cp) bytes per symbol), with symbol phasors.  Three timings
alternate in one process:

  (a) PuschOfdmModulator, one launch per batch                                        device events, LAUNCHES launches per repeat
  (b) PuschOfdmDemodulator on the same shapes (advance of half the short prefix), the   the same
      modulator's samples in, one launch per batch
  (d) a traffic twin of (a) in two torch launches: a strided copy of the grid's n_sc    the same
      values of every symbol into the first n_sc samples of the symbol, and a fill of
      the other N + cp - n_sc samples -- 8 n_sc bytes read and 8 (N + cp) written per
      symbol, the symbols at the uniform stride N + min cp (the same byte counts and
      pattern, not the same addresses: symbol 0's longer prefix is not written)

Writes the times, their spread, the time per symbol, the GB/s each implies on its own bytes, (a)/(d) and (a)/(b) to
profiles/ofdm_tx_perf.txt (--out), next to the demodulator's own ratio to its twin from profiles/ofdm_perf.txt.  `--rehearse`
runs the host-side logic without a GPU and measures nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import ofdm as OF

PORTS, SYMBOLS = 4, 14
SHAPES = ((4096, 273, 30e3, 256), (1024, 52, 30e3, 1024), (128, 10, 15e3, 8192))   # (N, n_prb_grid, scs, slots): ~0.5 GB of samples each
DEMODULATOR_OVER_ITS_TWIN = {4096: 4.06, 1024: 2.72, 128: 2.42}                    # (a)/(d) of profiles/ofdm_perf.txt


def describe(N, n_prb, scs, B):
    cp = OF.nr_cp_lengths(scs, N)
    a = min(cp) // 2
    v = OF.derive_host(N, n_prb, cp, SYMBOLS, 0)
    radix = " ".join(str(r) for r in v.radix[:v.n_passes])
    T = sum(cp) + SYMBOLS * N
    return cp, a, v, T, (f"N={N}, n_prb_grid={n_prb} (n_sc = {12 * n_prb}), {scs / 1e3:g} kHz: T = {T}, {B} slots x {PORTS} ports, radices {radix}; "
                         f"{v.rows_per_workgroup} symbol(s) per workgroup of {v.threads} threads ({v.threads_per_row} per symbol), "
                         f"{B * PORTS * v.n_workgroups_per_slot} workgroups, {v.lds_bytes} B LDS")


def main():
    ap = parser(__doc__, "ofdm_tx_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    shapes = [(N, p, scs, max(1, int(B * args.slots_scale))) for N, p, scs, B in SHAPES]

    lines = [f"tools/ofdm_tx_perf.py: {SYMBOLS} symbols x {PORTS} ports; {args.launches} launches x {args.repeats} repeats, alternating (a) (b) (d)"]
    if args.rehearse:
        print("\n".join(lines + [describe(*s)[-1] + " -- not measured" for s in shapes]))
        return

    dev = gpu("ofdm_tx_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    for N, n_prb, scs, B in shapes:
        cp, a, v, T, text = describe(N, n_prb, scs, B)
        n_sc = 12 * n_prb
        phi = OF.nr_symbol_phasors(3.5e9, scs, N, cp)
        dem = OF.PuschOfdmDemodulator(N, n_prb, cp, window_advance=a, sym_phasor=phi, device=dev)
        mod = OF.PuschOfdmModulator.for_demodulator(dem)
        dense = torch.view_as_complex(torch.empty((B, PORTS, SYMBOLS, n_sc, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        grid = dense.permute(0, 1, 3, 2)
        s = torch.empty((B, PORTS, T), dtype=torch.complex64, device=dev)
        back = torch.empty((B, PORTS, SYMBOLS, n_sc), dtype=torch.complex64, device=dev)
        # (d): the symbols at a uniform stride, n_sc values copied in, the rest filled
        step = N + min(cp)
        assert (SYMBOLS - 1) * step + step <= T
        s_d = torch.empty_like(s)
        head = s_d.as_strided((B, PORTS, SYMBOLS, n_sc), (PORTS * T, T, step, 1))
        tail = torch.view_as_real(s_d).as_strided((B, PORTS, SYMBOLS, 2 * (step - n_sc)), (2 * PORTS * T, 2 * T, 2 * step, 1), 2 * n_sc)

        def twin():
            head.copy_(dense)
            tail.fill_(1.0)

        fns = dict(a=lambda: mod(grid, out=s), b=lambda: dem(s, out=back), d=twin)
        for fn in fns.values():                                      # warm-up: code objects, allocator
            timed(fn, 3)
        assert bool(torch.isfinite(torch.view_as_real(s[:: max(1, B // 8)])).all())
        err = float((back - dense).abs().max())                      # the demodulator returns the grid
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        n_symbols = B * PORTS * SYMBOLS
        bytes_tx, bytes_rx = 8 * (B * PORTS * T + n_symbols * n_sc), 8 * n_symbols * (N + n_sc)
        ratio = lambda p, q_: f"{m[p] / m[q_]:.3f}   (per repeat {min(u / w for u, w in zip(t[p], t[q_])):.3f} .. {max(u / w for u, w in zip(t[p], t[q_])):.3f})"   # noqa: E731
        per = lambda k, nbytes: f"{m[k] * 1e6 / n_symbols:8.2f} ns per symbol   {nbytes / m[k] / 1e6:8.1f} GB/s on {nbytes / 1e9:.3f} GB"   # noqa: E731
        lines += [text,
                  f"  (a) modulator, one launch              {stats(t['a'])}   {per('a', bytes_tx)}",
                  f"  (b) demodulator, one launch            {stats(t['b'])}   {per('b', bytes_rx)}",
                  f"  (d) traffic twin of (a), copy + fill   {stats(t['d'])}   {per('d', bytes_tx)}",
                  f"  (a)/(d) = {ratio('a', 'd')};  the demodulator over its own twin in profiles/ofdm_perf.txt: {DEMODULATOR_OVER_ITS_TWIN[N]:.2f}",
                  f"  (a)/(b) = {ratio('a', 'b')};  max |demodulate(modulate(X)) - X| = {err:.2e} at rms 1.41 grid values"]
        del dem, mod, dense, grid, s, back, s_d, head, tail, fns
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
