#!/usr/bin/env python3
"""Dev tool (GPU box): what the equalizer extension (include/ce_eq.h) costs at the headline geometry -- 273 PRB, DM-RS
symbols [2, 11], 4 Rx, L = 1 at 8192 slots and L = 4 at 2048 slots.  Two timings alternate in one process:

  (a) PuschEqualizer on ch_est / rx / noise as estimate() lays them out            device events, LAUNCHES launches per repeat
  (b) a device pass that only reads the same ch_est and rx tensors: torch.sum over their float32 views   the same

(a) reads the data REs only (12 of the 14 symbols with the default reserved_re_mask) and writes x_hat and nvar; (b) reads
every byte of both tensors and writes two scalars.  Writes means and spread, (a)/(b) and the TB/s each implies on its own
bytes to profiles/eq_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import equalizer as EQ, synth as S

SHAPES = [(1, 8192), (4, 2048)]     # (layers, slots)
PORTS = 4


def main():
    ap = parser(__doc__, "eq_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale both batch sizes (a smaller card)")
    args = ap.parse_args()

    lines = [f"tools/eq_perf.py: 273 PRB, DM-RS [2, 11], {PORTS} Rx; {args.launches} launches x {args.repeats} repeats, alternating (a) (b)"]
    if args.rehearse:
        for L, B in SHAPES:
            h1, h2, _ = S.numpy_hops(S.bench_case("filter", L))
            eq = EQ.PuschEqualizer(h1, h2, L, 273)
            print(f"L={L}: {B} slots, {eq.n_data_re} data REs per slot, first rows {eq.data_re()[:2].tolist()} -- not measured")
        return

    import torch
    dev = gpu("eq_perf")

    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for L, B in SHAPES:
        B = max(1, int(B * args.slots_scale))
        h1, h2, _ = S.numpy_hops(S.bench_case("filter", L))
        eq = EQ.PuschEqualizer(h1, h2, L, 273, device=dev)
        n_sc, n_sym, R = 3276, 14, PORTS
        rx_buf = torch.empty((B, R, n_sym, n_sc), dtype=torch.complex64, device=dev)        # subcarrier-contiguous, as bench.py feeds estimate()
        ch = torch.empty((B, R, n_sc, n_sym, L), dtype=torch.complex64, device=dev)
        for b0 in range(0, B, 64):                                                           # filled in slices: no second copy of 12 GB
            torch.view_as_real(rx_buf[b0:b0 + 64]).normal_(generator=g)
            torch.view_as_real(ch[b0:b0 + 64]).normal_(std=0.7071, generator=g)
        rx = rx_buf.permute(0, 1, 3, 2)
        noise = 10.0 ** -1.5 * (0.5 + 1.5 * torch.rand((B, R), dtype=torch.float64, device=dev, generator=g))
        out = (torch.empty((B, eq.n_data_re, L), dtype=torch.complex64, device=dev), torch.empty((B, eq.n_data_re, L), dtype=torch.float32, device=dev))
        rx_f, ch_f = torch.view_as_real(rx_buf), torch.view_as_real(ch)
        a = lambda: eq(rx, ch, noise, out=out)                   # noqa: E731
        b = lambda: (ch_f.sum(), rx_f.sum())                     # noqa: E731
        bytes_a = B * eq.n_data_re * (R * 8 * (L + 1) + 12 * L)  # h and y of every data RE on every port, x_hat and nvar out
        bytes_b = (rx_buf.numel() + ch.numel()) * 8
        for fn in (a, b):                                        # warm-up: code objects, allocator
            timed(fn, 3)
        assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(torch.view_as_real(out[0])).all())
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb.append(timed(b, args.launches))
        ma, mb = statistics.mean(ta), statistics.mean(tb)
        lines += [f"L={L}, {B} slots: ch_est {ch.numel() * 8 / 1e9:.2f} GB, rx {rx_buf.numel() * 8 / 1e9:.2f} GB, x_hat + nvar {B * eq.n_data_re * L * 12 / 1e9:.2f} GB",
                  f"  (a) PuschEqualizer, one launch                     {stats(ta, 9)}   {bytes_a / ma / 1e9:6.2f} TB/s on {bytes_a / 1e9:.2f} GB (data REs in, results out)",
                  f"  (b) torch.sum over both tensors' float32 views     {stats(tb, 9)}   {bytes_b / mb / 1e9:6.2f} TB/s on {bytes_b / 1e9:.2f} GB (every byte in)",
                  f"  (a)/(b) = {ma / mb:.3f}"]
        del rx_buf, rx, ch, out, rx_f, ch_f
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
