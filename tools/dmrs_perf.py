#!/usr/bin/env python3
"""Dev tool (GPU box): what the DM-RS generation extension (include/ce_dmrs.h) costs at the headline geometry -- 273 PRB,
DM-RS symbols [2, 11], 8192 slots, L = 1 and L = 4.  Three timings alternate in one process:

  (a) PuschDmrs with per-slot device parameters                                   device events, LAUNCHES launches per repeat
  (b) a plain device fill of the same number of bytes (the floor of this store stream)        device events, the same
  (c) what a caller does without the extension: numpy generation of the same tensor on the host (table method,
      vectorised over the batch) + the copy to the device              host clock around a synchronise, once per repeat

and, for scale, the estimation step the pilots feed (headline workload: 4 Rx, RC filter, L = 1) in the same run.
Writes means and spread, (a)/(b) and (c)/(a) to profiles/dmrs_perf.txt (--out).  `--rehearse` runs the host-side logic on
a few slots without a GPU and measures nothing."""
import statistics
import time

import numpy as np

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import dmrs, synth as S


def host_pilots(view, n_layers, slots, n_ids, n_scids, n_symb_slot=14):
    """[B, n_re, n_dmrs_total, L] complex64 in numpy from the plan's host view: the kernel's arithmetic, vectorised over B."""
    u = np.uint32
    B, n_re, n_cols = len(slots), view.n_re, view.n_dmrs_total
    sl, ni, ns = (np.asarray(v).astype(np.uint32) for v in (slots, n_ids, n_scids))
    out = np.empty((B, n_re, n_cols, n_layers, 2), np.uint32)
    for col in range(n_cols):
        h, sym = view.col_hop[col], view.col_sym[col]
        ci = ((((u(n_symb_slot) * sl + u(sym + 1)) * (u(2) * ni + u(1))) << u(17)) + u(2) * ni + ns) & u(0x7FFFFFFF)
        nw = view.n_words[h]
        words = np.tile(np.array(view.x1[h][:nw], np.uint32), (B, 1))
        for i in range(31):
            words ^= np.array(view.t[h][i][:nw], np.uint32)[None, :] * ((ci >> u(i)) & u(1))[:, None]
        m = np.array(view.m[h][:n_re], np.int64)
        br = 2 * m - 32 * view.word0[h]
        two = words[:, br >> 5] >> (br & 31).astype(np.uint32)[None, :]
        for l in range(n_layers):
            flip = (m & 1).astype(np.uint32)[None, :] if l % 2 else u(0)
            out[:, :, col, l, 0] = u(0x3F3504F3) ^ (((two ^ flip) & u(1)) << u(31))
            out[:, :, col, l, 1] = u(0x3F3504F3) ^ ((((two >> u(1)) ^ flip) & u(1)) << u(31))
    return out.view(np.float32).view(np.complex64)[..., 0]


def main():
    ap = parser(__doc__, "dmrs_perf", rehearse_help="host logic only, on 4 slots; no GPU, nothing measured, nothing written")
    ap.add_argument("--slots", type=int, default=8192)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--no-estimate", action="store_true", help="skip the estimation step (12 GB of received grids at 8192 slots)")
    args = ap.parse_args()

    rng = np.random.default_rng(1)
    B = 4 if args.rehearse else args.slots
    slots, n_ids, n_scids = (rng.integers(0, hi, B).astype(np.int32) for hi in (160, 65536, 2))
    lines = [f"tools/dmrs_perf.py: 273 PRB, DM-RS [2, 11], {B} slots; {args.launches} launches x {args.repeats} repeats, alternating (a) (b) (c)"]
    if args.rehearse:
        for L in args.layers:
            h1, h2, _ = S.numpy_hops(S.bench_case("filter", L))
            view = dmrs.derive_host(h1, h2, L, 273, 14)
            p = host_pilots(view, L, slots, n_ids, n_scids)
            print(f"L={L}: host tensor {p.shape}, {p.nbytes // B} B per slot, |p|^2 == 1: {bool(np.allclose(np.abs(p) ** 2, 1.0))} -- not measured")
        return

    import torch
    from srsran_ce_pytorch_amd import estimator as E
    dev = gpu("dmrs_perf")

    for L in args.layers:
        case = S.bench_case("filter", L)
        h1, h2, cfg = S.numpy_hops(case)
        gen = dmrs.PuschDmrs(h1, h2, L, 273, 14, device=dev)
        view = dmrs.derive_host(h1, h2, L, 273, 14)
        d_slot, d_id, d_scid = (torch.as_tensor(v, device=dev) for v in (slots, n_ids, n_scids))
        out = torch.empty((B, gen.n_re, gen.n_dmrs_total, L), dtype=torch.complex64, device=dev)
        fill = torch.empty_like(out).view(torch.float32)
        staged = torch.empty_like(out)
        nbytes = out.numel() * 8
        step = None
        if L == 1 and not args.no_estimate:
            plan = E.make_plan(h1, h2, cfg, case["beta"], 1, 273, 14, dev)
            rx, _ = S.torch_inputs(case, B, 4, dev, seed=1234)
            est_out = E.estimate_with_plan(plan, rx, gen(d_slot, d_id, d_scid, out=out))
            step = lambda: E.estimate_with_plan(plan, rx, out, est_out)   # noqa: E731
        a = lambda: gen(d_slot, d_id, d_scid, out=out)                    # noqa: E731
        b = lambda: fill.fill_(0.70710677)                                # noqa: E731

        def c():
            t0 = time.perf_counter()
            staged.copy_(torch.from_numpy(host_pilots(view, L, slots, n_ids, n_scids)))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for fn in (a, b) + ((step,) if step else ()):                     # warm-up: code objects, allocator
            timed(fn, 3)
        ms_c0 = c()
        assert torch.equal(staged.view(torch.float32), out.view(torch.float32)), "host generation and kernel disagree"
        ta, tb, tc, ts = [], [], [ms_c0], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb.append(timed(b, args.launches))
            tc.append(c())
            if step:
                ts.append(timed(step, args.launches))
        ma, mb, mc = (statistics.mean(x) for x in (ta, tb, tc[1:]))
        lines += [f"L={L}: {nbytes / 1e6:.1f} MB per step ({nbytes // B} B per slot)",
                  f"  (a) PuschDmrs kernel, per-slot device parameters   {stats(ta, 9)}   {nbytes / ma / 1e6:8.1f} GB/s",
                  f"  (b) device fill of the same bytes                  {stats(tb, 9)}   {nbytes / mb / 1e6:8.1f} GB/s",
                  f"  (c) numpy on the host + copy to the device         {stats(tc[1:], 9)}   (first, untimed-for-mean run: {ms_c0:.1f} ms)",
                  f"  (a)/(b) = {ma / mb:.3f}    (c)/(a) = {mc / ma:.1f}"]
        if ts:
            ms = statistics.mean(ts)
            lines += [f"  estimation step fed by these pilots (4 Rx, RC filter)  {stats(ts, 9)}",
                      f"  (a) / estimation step = {ma / ms:.4f}    (c) / estimation step = {mc / ms:.2f}"]
        del out, fill, staged
        if step:
            del rx, est_out, step
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
