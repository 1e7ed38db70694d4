#!/usr/bin/env python3
"""Dev tool (GPU box): what the time-domain channel emulator (include/ce_tp.h `ce_chan_apply`) costs -- the slots of
tools/ofdm_perf.py, T = 61440 / 15360 / 1920 samples (N = 4096 and 1024 at 30 kHz, 128 at 15 kHz) in batches of 256 / 1024 /
8192, one tx port, four rx ports, K = 1, 12 and 64 taps shared by the batch; 8 T bytes in and 32 T out per slot.  The timings
alternate in one process, device events around LAUNCHES launches per repeat:

  (a)  PuschChannelEmulator with taps + CFO + noise (device tensors of per-slot control words and sigmas), one launch
  (b1) the same with sigma=None, (b2) with cfo=None, (b0) with neither: what the noise and the oscillator cost
  (c)  a traffic twin in one torch launch: the tx row copied to the four rx rows (8 T read, 32 T written per slot)
  (d)  the torch composition a user would write today: K shifted, scaled sums (a multiply and an add per tap, all ports at
       once), a product with a phasor row kept from call to call, normal_() into a kept buffer and a scaled add

Writes the times, their spread, ns per output sample, (a)/(d), (a)/(c) and (b0)/(c) with the range over the repeats to
profiles/chan_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

import numpy as np
import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import channel as CH, ofdm as OF

N_TX, N_RX = 1, 4
SHAPES = ((4096, 30e3, 256), (1024, 30e3, 1024), (128, 15e3, 8192))     # (N, scs, slots): ~0.5 GB of rx samples each
TAPS = (1, 12, 64)


def describe(N, scs, B, K):
    T = sum(OF.nr_cp_lengths(scs, N)) + 14 * N
    tiles = (T + 1023) // 1024
    lds = 8 * (N_TX * (1024 + (K & ~1)) + N_TX * K)
    return T, (f"N={N}, {scs / 1e3:g} kHz: T = {T}, {B} slots, {N_TX} tx x {N_RX} rx ports, K = {K}: {B * N_RX * tiles} workgroups of 256 threads, "
               f"{lds} B LDS")


def main():
    ap = parser(__doc__, "chan_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    shapes = [(N, scs, max(1, int(B * args.slots_scale))) for N, scs, B in SHAPES]
    lines = [f"tools/chan_perf.py: {N_TX} tx x {N_RX} rx ports; {args.launches} launches x {args.repeats} repeats, alternating (a) (b1) (b2) (b0) (c) (d)"]
    if args.rehearse:
        print("\n".join(lines + [describe(N, scs, B, K)[1] + " -- not measured" for N, scs, B in shapes for K in TAPS]))
        return

    dev = gpu("chan_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(15)
    rng = np.random.default_rng(15)
    for N, scs, B in shapes:
        T, _ = describe(N, scs, B, 1)
        fs = scs * N
        x = torch.view_as_complex(torch.empty((B, N_TX, T, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        y = torch.empty((B, N_RX, T), dtype=torch.complex64, device=dev)
        y_d, noise = torch.empty_like(y), torch.empty_like(y)
        fcw = torch.as_tensor(rng.integers(-CH.cfo_word(2e3, fs), CH.cfo_word(2e3, fs), B).astype(np.int32), device=dev)
        sigma = torch.as_tensor((0.05 + 0.1 * rng.random(B)).astype(np.float32), device=dev)
        word = CH.cfo_word(350.0, fs)
        phasor = torch.as_tensor(np.exp(2j * np.pi * ((word * np.arange(T)) % (1 << 32)) * 2.0 ** -32).astype(np.complex64), device=dev)[None, None]
        for K in TAPS:
            text = describe(N, scs, B, K)[1]
            emu = CH.PuschChannelEmulator(N_TX, N_RX, K, device=dev)
            h = ((rng.standard_normal((1, N_RX, N_TX, K)) + 1j * rng.standard_normal((1, N_RX, N_TX, K))) / np.sqrt(2 * K)).astype(np.complex64)
            taps = torch.as_tensor(h, device=dev)
            hk = [taps[0, :, 0, k].reshape(1, N_RX, 1).clone() for k in range(K)]

            def composition():
                torch.mul(x, hk[0], out=y_d)
                for k in range(1, K):
                    y_d[:, :, k:].add_(x[:, :, :T - k] * hk[k])
                y_d.mul_(phasor)
                torch.view_as_real(noise).normal_(generator=g)
                y_d.add_(noise, alpha=0.1)

            fns = {"a": lambda: emu(x, taps, cfo=fcw, sigma=sigma, seed=1, out=y), "b1": lambda: emu(x, taps, cfo=fcw, out=y),
                   "b2": lambda: emu(x, taps, sigma=sigma, seed=1, out=y), "b0": lambda: emu(x, taps, out=y),
                   "c": lambda: y.copy_(x.expand(B, N_RX, T)), "d": composition}
            for fn in fns.values():                                  # warm-up: code objects, allocator
                timed(fn, 2)
            emu(x, taps, out=y)                                      # the kernel's sums are the composition's
            torch.mul(x, hk[0], out=y_d)
            for k in range(1, K):
                y_d[:, :, k:].add_(x[:, :, :T - k] * hk[k])
            err = float((y[:: max(1, B // 8)] - y_d[:: max(1, B // 8)]).abs().max())
            t = {k: [] for k in fns}
            for _ in range(args.repeats):
                for k, fn in fns.items():
                    t[k].append(timed(fn, args.launches))
            m = {k: statistics.mean(ts) for k, ts in t.items()}
            n_out = B * N_RX * T
            nbytes = 8 * (B * N_TX * T + n_out)
            ratio = lambda p, q_: f"{m[p] / m[q_]:.3f}   (per repeat {min(u / w for u, w in zip(t[p], t[q_])):.3f} .. {max(u / w for u, w in zip(t[p], t[q_])):.3f})"   # noqa: E731
            per = lambda k: f"{m[k] * 1e6 / n_out:7.4f} ns per output sample   {nbytes / m[k] / 1e6:8.1f} GB/s on {nbytes / 1e9:.3f} GB"   # noqa: E731
            lines += [text,
                      f"  (a)  emulator: taps + CFO + noise       {stats(t['a'])}   {per('a')}",
                      f"  (b1) emulator: sigma=None               {stats(t['b1'])}   {per('b1')}",
                      f"  (b2) emulator: cfo=None                 {stats(t['b2'])}   {per('b2')}",
                      f"  (b0) emulator: taps alone               {stats(t['b0'])}   {per('b0')}",
                      f"  (c)  traffic twin, one copy             {stats(t['c'])}   {per('c')}",
                      f"  (d)  torch: {2 * K - 1:3d} + 3 launches             {stats(t['d'])}   {per('d')}",
                      f"  (a)/(d) = {ratio('a', 'd')};  (a)/(c) = {ratio('a', 'c')};  (b0)/(c) = {ratio('b0', 'c')}",
                      f"  noise (a) - (b1) = {m['a'] - m['b1']:.4f} ms, oscillator (a) - (b2) = {m['a'] - m['b2']:.4f} ms;  max |emulator - shifted sums| = {err:.2e}"]
            del emu, taps, hk, fns
        del x, y, y_d, noise, phasor
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
