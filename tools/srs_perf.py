#!/usr/bin/env python3
"""Dev tool (GPU box): what SRS channel estimation (include/ce_tp.h `ce_srs_profile`, `ce_srs_estimate`) costs at two loads, each
with enough (item, receive port) workgroups to fill the chip several times:

  wide    64 receive ports x 16 items x 4 symbols x 272 PRB, comb 2, 2 ports, N = 2048
  narrow  64 receive ports x 64 items x 1 symbol x 48 PRB, comb 4, 4 ports, N = 256

Timings alternate in one process, device events round LAUNCHES launches per repeat:

  (a1) SrsEstimator.profile: launch 1 and the wrapper's sum / argmax           (a2) SrsEstimator(...): launch 2 at that delay
  (b1) the torch composition of launch 1: the comb gather, the products with    (b2) the torch composition of launch 2: the products, the
       conj(r) and conj(rho), torch.fft.ifft over N, abs()^2 summed over the         block means, the residual and its energy, the mean
       terms, the window, sum / argmax                                               energy, the wideband mean
  (c)  a read-only pass over the same bytes of y (the rows of the sounding symbols over the sounding band): the floor of launch 2
  (d)  PuschOfdmDemodulator (14 symbols x 4 ports per slot, the widest grid N holds) running the number of N-point transforms of
       launch 1: the project's own transform rate

Writes the times, their spread, the ratios and how far (a) and (b) agree to profiles/srs_perf.txt (--out).  `--rehearse` runs the
host-side logic without a GPU and measures nothing."""
import statistics

import numpy as np
import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import ofdm as OF, srs as S

# name, (k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, N), receive ports, items
LOADS = (("wide", (2, 2, 3, 1, 272, 4, 2048), 64, 16),
         ("narrow", (4, 4, 2, 1, 48, 1, 256), 64, 64))
SLOT, N_ID, DELAY = 7, 777, 5


def describe(name, geo, R, B):
    k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, N = geo
    hv = S.derive_host(k_tc, n_ap, n_cs, k_bar, m_srs, m_srs + 1, N, n_symb=n_symb, n_sym=n_symb, hopping="group")
    n_tr = B * R * n_symb * n_ap
    radix = " ".join(str(r) for r in hv.view.radix[:hv.view.n_passes])
    return hv, n_tr, (f"{name}: {R} receive ports x {B} items x {n_symb} symbols x {m_srs} PRB, comb {k_tc}, {n_ap} ports on {hv.n_combs} comb(s), N={N}: "
                      f"M={hv.m}, {hv.n_blocks} blocks of Q={hv.q_len}, window {hv.default_win_len} behind a guard of {hv.guard}; {B * R} workgroups of 256 threads, "
                      f"{hv.view.rows_per_workgroup} term(s) at a time, radices {radix}, {hv.view.lds_bytes} B LDS of buffers; {n_tr} transforms of {N} points, "
                      f"{8 * B * R * n_symb * 12 * m_srs / 1e6:.1f} MB of y rows")


def main():
    ap = parser(__doc__, "srs_perf")
    ap.add_argument("--items-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    loads = [(n, g, R, max(1, int(B * args.items_scale))) for n, g, R, B in LOADS]
    lines = [f"tools/srs_perf.py: {args.launches} launches x {args.repeats} repeats, alternating (a1) (a2) (b1) (b2) (c) (d)"]
    if args.rehearse:
        print("\n".join(lines + [describe(*ld)[-1] + " -- not measured" for ld in loads]))
        return

    dev = gpu("srs_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    for name, geo, R, B in loads:
        k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, N = geo
        hv, n_tr, text = describe(name, geo, R, B)
        n_prb_grid, M, Q, nb, ncs, guard = m_srs + 1, hv.m, hv.q_len, hv.n_blocks, S.n_cs_max(k_tc), hv.guard
        est = S.SrsEstimator(k_tc, n_ap, n_cs, k_bar, m_srs, n_prb_grid, N, n_symb=n_symb, n_sym=n_symb, start_prb=1, hopping="group", device=dev)
        wl, ports = est.win_len, est.ports
        # noise of power 0.01 and every port at unit gain, DELAY grid steps late
        seq = S.srs_sequence(k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, 0, SLOT, N_ID, "group")
        tx = S.srs_map(seq, k_tc, n_ap, n_cs, k_bar, 1, 0, n_prb_grid, n_symb).sum(0).T                       # [n_symb, n_sc]
        tx = tx * np.exp(-2j * np.pi * np.arange(12 * n_prb_grid) * DELAY / (N * k_tc))[None]
        y = torch.view_as_complex(torch.empty((B, R, n_symb, 12 * n_prb_grid, 2), dtype=torch.float32, device=dev).normal_(std=float(np.sqrt(0.005)), generator=g))
        y += torch.as_tensor(tx.astype(np.complex64), device=dev)
        base = torch.as_tensor(np.conj(seq[0] / np.exp(2j * np.pi * ((ports[0][1] * np.arange(M)) % ncs) / ncs)).astype(np.complex64), device=dev)   # conj(rbar) [n_symb, M]
        rho = torch.as_tensor(np.stack([np.exp(2j * np.pi * ((cs * np.arange(M)) % ncs) / ncs) for _, cs in ports]).astype(np.complex64), device=dev)  # [n_ap, M]
        combs = sorted({c for c, _ in ports})
        w = torch.as_tensor(np.exp(2j * np.pi * ((np.arange(M) * DELAY) % N) / N).astype(np.complex64), device=dev)
        win = torch.as_tensor((np.arange(wl) - guard) % N, device=dev)
        dof = n_symb * len(combs) * M - n_symb * n_ap * nb
        delay_t = torch.full((B,), DELAY, dtype=torch.int32, device=dev)

        def comb_rows(c):
            return y[..., 12 + c:12 + c + k_tc * M:k_tc]                                                     # [B, R, n_symb, M]

        def composition_1():
            P = 0
            for i, (c, _) in enumerate(ports):
                z = torch.fft.ifft(comb_rows(c) * base * rho[i].conj(), n=N, dim=-1)
                P = P + (z.real.square() + z.imag.square()).sum(2)
            prof = P[..., win] * float((N / M) ** 2)
            return prof, (prof.sum(1).argmax(-1) - guard).to(torch.int32)

        def composition_2():
            h_sb = torch.empty((B, R, n_ap, n_symb, nb), dtype=torch.complex64, device=dev)
            num = en = 0
            for c in combs:
                yc = comb_rows(c)
                gc = yc * base * w
                e = gc
                for i, (ci, _) in enumerate(ports):
                    if ci == c:
                        h = (gc * rho[i].conj()).reshape(B, R, n_symb, nb, Q).mean(-1)
                        h_sb[:, :, i] = h
                        e = e - h.repeat_interleave(Q, dim=-1) * rho[i]
                num = num + (e.real.square() + e.imag.square()).sum((2, 3))
                en = en + (yc.real.square() + yc.imag.square()).sum((2, 3))
            return h_sb, h_sb.mean((3, 4)), num / dof, en / (n_symb * len(combs) * M)

        band = torch.view_as_real(y[..., 12:12 + 12 * m_srs])

        # (d): the same number of N-point transforms through the OFDM demodulator
        cp = OF.nr_cp_lengths(30e3, N)
        n_prb = min(N // 12, 275)
        dem = OF.PuschOfdmDemodulator(N, n_prb, cp, device=dev)
        slots = -(-n_tr // (14 * 4))
        samples = torch.view_as_complex(torch.empty((slots, 4, dem.n_samples, 2), dtype=torch.float32, device=dev).normal_(generator=g))
        grid = torch.empty((slots, 4, 14, 12 * n_prb), dtype=torch.complex64, device=dev)

        fns = dict(a1=lambda: est.profile(y, SLOT, N_ID), a2=lambda: est(y, SLOT, N_ID, delay=delay_t), b1=composition_1, b2=composition_2,
                   c=lambda: band.sum(), d=lambda: dem(samples, out=grid))
        for fn in fns.values():                                      # warm-up: code objects, plans, allocator
            timed(fn, 3)
        p, out, (prof_b, delay_b), (h_b, hw_b, noise_b, epre_b) = est.profile(y, SLOT, N_ID), est(y, SLOT, N_ID, delay=delay_t), composition_1(), composition_2()
        torch.cuda.synchronize()
        rel_p = float(((p.profile - prof_b).abs().amax(-1) / prof_b.amax(-1)).max())
        same = float((p.delay == delay_b).float().mean())
        found = float((p.delay == DELAY).float().mean())
        rel_h = float(((out.h_sb - h_b).abs() / h_b.abs().amax()).max())
        rel_n, rel_e = float(((out.noise - noise_b).abs() / noise_b).max()), float(((out.epre - epre_b).abs() / epre_b).max())
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        ratio = lambda a, b: f"{m[a] / m[b]:.3f}   (per repeat {min(u / v for u, v in zip(t[a], t[b])):.3f} .. {max(u / v for u, v in zip(t[a], t[b])):.3f})"   # noqa: E731
        mb = 8 * B * R * n_symb * 12 * m_srs / 1e6
        lines += [text,
                  f"  (a1) profile + argmax                    {stats(t['a1'])}   {m['a1'] * 1e6 / n_tr:8.2f} ns per transform",
                  f"  (b1) torch composition of launch 1       {stats(t['b1'])}   {m['b1'] * 1e6 / n_tr:8.2f} ns per transform",
                  f"  (d)  OFDM demodulator, {slots * 56} transforms   {stats(t['d'])}   {m['d'] * 1e6 / (slots * 56):8.2f} ns per transform",
                  f"  (a2) estimate                            {stats(t['a2'])}   {mb / m['a2']:8.1f} GB/s of y rows",
                  f"  (b2) torch composition of launch 2       {stats(t['b2'])}",
                  f"  (c)  read-only pass over the y rows       {stats(t['c'])}   {mb / m['c']:8.1f} GB/s",
                  f"  (a1)/(b1) = {ratio('a1', 'b1')}",
                  f"  (a1)/(d)  = {ratio('a1', 'd')}   per transform: {(m['a1'] / n_tr) / (m['d'] / (slots * 56)):.3f}",
                  f"  (a2)/(b2) = {ratio('a2', 'b2')}",
                  f"  (a2)/(c)  = {ratio('a2', 'c')}",
                  f"  (a) against (b): profile max difference / peak {rel_p:.2e}; equal delays in {100 * same:.1f} % of the items, the sent delay in {100 * found:.1f} %; "
                  f"h_sb max difference / max {rel_h:.2e}; noise {rel_n:.2e}, epre {rel_e:.2e} relative"]
        del est, dem, y, samples, grid, fns, band, base, rho
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
