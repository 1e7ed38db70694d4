#!/usr/bin/env python3
"""Dev tool (GPU box): what OFDM demodulation (include/ce_tp.h `ce_ofdm_demodulate`) costs -- slots of 14 symbols on 4 ports at
(N, n_prb_grid) = (4096, 273) and (1024, 52) at 30 kHz and (128, 10) at 15 kHz, complex64 samples in (8 N bytes per window
read, the cyclic prefixes skipped) and the grid out (8 n_sc bytes per symbol), with a window advance of half the short prefix
and symbol phasors.  Three timings alternate in one process:

  (a) PuschOfdmDemodulator, one launch per batch                                      device events, LAUNCHES launches per repeat
  (d) a traffic twin in two torch launches: a strided copy of n_sc samples of every    the same
      window into the output, and a sum over the other N - n_sc samples of the window
      -- 8 n_sym N bytes read and 8 n_sym n_sc written per (slot, port), the windows at
      the uniform stride N + min cp (the same byte counts and pattern, not the same
      addresses: symbol 0's longer prefix is not skipped)
  (e) torch: gather of the windows, torch.fft.fft (norm="ortho"), gather of the bins,  the same
      product with the advance-and-phasor table -- the same result in four launches
      and three intermediates; skipped, and said so, if torch's FFT does not run here

Writes the times, their spread, the GB/s each implies on (a)'s bytes, (a)/(d), (a)/(e) and the largest |a - e| to
profiles/ofdm_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

import numpy as np
import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import ofdm as OF

PORTS, SYMBOLS = 4, 14
SHAPES = ((4096, 273, 30e3, 256), (1024, 52, 30e3, 1024), (128, 10, 15e3, 8192))   # (N, n_prb_grid, scs, slots): ~0.5 GB of samples each


def describe(N, n_prb, scs, B):
    cp = OF.nr_cp_lengths(scs, N)
    a = min(cp) // 2
    v = OF.derive_host(N, n_prb, cp, SYMBOLS, a)
    radix = " ".join(str(r) for r in v.radix[:v.n_passes])
    T = sum(cp) + SYMBOLS * N
    return cp, a, v, T, (f"N={N}, n_prb_grid={n_prb} (n_sc = {12 * n_prb}), {scs / 1e3:g} kHz: T = {T}, advance {a}, {B} slots x {PORTS} ports, radices {radix}; "
                         f"{v.rows_per_workgroup} window(s) per workgroup of {v.threads} threads ({v.threads_per_row} per window), "
                         f"{B * PORTS * v.n_workgroups_per_slot} workgroups, {v.lds_bytes} B LDS")


def main():
    ap = parser(__doc__, "ofdm_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    shapes = [(N, p, scs, max(1, int(B * args.slots_scale))) for N, p, scs, B in SHAPES]

    lines = [f"tools/ofdm_perf.py: {SYMBOLS} symbols x {PORTS} ports; {args.launches} launches x {args.repeats} repeats, alternating (a) (d) (e)"]
    if args.rehearse:
        print("\n".join(lines + [describe(*s)[-1] + " -- not measured" for s in shapes]))
        return

    dev = gpu("ofdm_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    for N, n_prb, scs, B in shapes:
        cp, a, v, T, text = describe(N, n_prb, scs, B)
        n_sc = 12 * n_prb
        phi = OF.nr_symbol_phasors(3.5e9, scs, N, cp)
        dem = OF.PuschOfdmDemodulator(N, n_prb, cp, window_advance=a, sym_phasor=phi, device=dev)
        s = torch.view_as_complex(torch.empty((B, PORTS, T, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        out = torch.empty((B, PORTS, SYMBOLS, n_sc), dtype=torch.complex64, device=dev)
        # (d): the windows at a uniform stride, n_sc samples copied, the rest summed
        step = N + min(cp)
        assert (SYMBOLS - 1) * step + N <= T
        head = s.as_strided((B, PORTS, SYMBOLS, n_sc), (PORTS * T, T, step, 1))
        tail = torch.view_as_real(s).as_strided((B, PORTS, SYMBOLS, 2 * (N - n_sc)), (2 * PORTS * T, 2 * T, 2 * step, 1), 2 * n_sc)
        out_d, sink = torch.empty_like(out), torch.empty((B, PORTS, SYMBOLS), dtype=torch.float32, device=dev)

        def twin():
            out_d.copy_(head)
            torch.sum(tail, dim=-1, out=sink)

        # (e): torch's FFT over the gathered windows
        starts = np.cumsum([0] + [c + N for c in cp[:-1]]) + np.array(cp) - a
        win = torch.as_tensor((starts[:, None] + np.arange(N)[None, :]).reshape(-1), device=dev)
        q = np.arange(n_sc) - n_sc // 2
        bins = torch.as_tensor(q % N, device=dev)
        table = torch.as_tensor((phi.astype(np.complex128)[:, None] * np.exp(2j * np.pi * q * a / N)[None, :]).astype(np.complex64), device=dev)

        def torch_fft():
            x = s.index_select(2, win).view(B, PORTS, SYMBOLS, N)
            return torch.fft.fft(x, dim=-1, norm="ortho").index_select(3, bins) * table

        fns = dict(a=lambda: dem(s, out=out), d=twin)
        fft_note = ""
        try:
            ref = torch_fft()
            torch.cuda.synchronize()
            fns["e"] = torch_fft
        except Exception as e:   # noqa: BLE001 -- whatever torch's FFT backend raises on this box
            fft_note = f"  (e) torch.fft.fft does not run on this box: {type(e).__name__}: {str(e).splitlines()[0][:120]}"
        for fn in fns.values():                                      # warm-up: code objects, allocator, FFT plans
            timed(fn, 3)
        assert bool(torch.isfinite(torch.view_as_real(out[:: max(1, B // 8)])).all())
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        nbytes = B * PORTS * SYMBOLS * 8 * (N + n_sc)
        ratio = lambda p, q_: f"{m[p] / m[q_]:.3f}   (per repeat {min(u / w for u, w in zip(t[p], t[q_])):.3f} .. {max(u / w for u, w in zip(t[p], t[q_])):.3f})"   # noqa: E731
        per = lambda k: f"{m[k] * 1e6 / (B * PORTS * SYMBOLS):8.2f} ns per window   {nbytes / m[k] / 1e6:8.1f} GB/s on {nbytes / 1e9:.3f} GB"   # noqa: E731
        lines += [text,
                  f"  (a) demodulator, one launch            {stats(t['a'])}   {per('a')}",
                  f"  (d) traffic twin, copy + sum           {stats(t['d'])}   {per('d')}",
                  f"  (a)/(d) = {ratio('a', 'd')}"]
        if "e" in fns:
            err = float((out - ref).abs().max())
            lines += [f"  (e) torch gather + fft + gather + mul  {stats(t['e'])}   {per('e')}",
                      f"  (a)/(e) = {ratio('a', 'e')};  max |a - e| = {err:.2e} at rms 1 samples"]
            del ref
        else:
            lines.append(fft_note)
        del dem, s, out, out_d, sink, head, tail, fns
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
