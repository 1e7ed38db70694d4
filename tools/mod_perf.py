#!/usr/bin/env python3
"""Dev tool (GPU box): what the modulator extension (include/ce_mod.h) costs against the least a pass that writes the same
bytes can cost, at

  273 PRB x {1, 4} layers x {QPSK, 256QAM}, DM-RS symbols [2, 11], 14 symbols      the full band; 256 slots per launch (94 MB of tx at 1 layer, 376 MB at 4)
  3 PRB inside a 52-PRB grid, 1 layer, 16QAM, DM-RS symbols [2, 11]                a narrow allocation: most of tx is zeros; 1024 slots

Timings alternate in one process, round by round, all through preallocated tensors:

  (a) ce_mod_modulate, scrambling on, per-slot rnti / n_id and pilots            device events, LAUNCHES launches per repeat
  (b) Tensor.zero_() of the same tx buffer: a plain device fill of the same bytes  the same

Writes ms per call (mean and range over the repeats), GB/s of tx bytes written and (a)/(b) to profiles/mod_perf.txt (--out).
The yardstick is (b) in the same process; boxes of one pool differ by a few percent, so a margin below that means nothing.
Kernel times come from a kernel trace of this tool, in a run of its own.  There is no pass mark.
`--rehearse` runs the host-side logic without a GPU and measures nothing."""
import ctypes as C
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import modulator as MO, synth as S  # noqa: E402

T1 = [S.TYPE1_CDM0, S.TYPE1_CDM1]
SHAPES = [(256, 273, 0, 273, L, qm) for L in (1, 4) for qm in (2, 8)] + [(1024, 52, 10, 3, 1, 4)]      # slots, grid PRBs, first PRB, PRBs, layers, Qm


def hops(n_prb_grid, prb_start, n_prbs, L):
    case = S.case_spec("mod_perf", n_prb_grid, [S.hop_spec([2, 11], prb_start, n_prbs, re_masks=T1 if L > 2 else None)], n_layers=L)
    return S.numpy_hops(case)[:2]


def describe(slots, n_prb_grid, prb_start, n_prbs, L, qm):
    v = MO.derive_host(*hops(n_prb_grid, prb_start, n_prbs, L), L, n_prb_grid, qm)
    tx_bytes = slots * L * 14 * 12 * n_prb_grid * 8
    return v, tx_bytes, (f"{slots} slots x {n_prbs} PRB in {n_prb_grid}, {L} layers, Qm = {qm}: G = {v.n_bits}, tx {tx_bytes / 1e6:.2f} MB, g {slots * v.g_row_bytes / 1e6:.2f} MB, "
                         f"pilots {slots * v.n_re * v.n_dmrs_total * L * 8 / 1e6:.2f} MB; {slots * v.workgroups_per_slot} workgroups of {v.threads} threads "
                         f"({v.workgroups_per_slot} per slot, at most {v.max_tile_blocks} Gold blocks each), {v.lds_bytes} B LDS")


def measure(args):
    dev = gpu("mod_perf")
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    lines = []
    for slots, n_prb_grid, prb_start, n_prbs, L, qm in SHAPES:
        B = max(1, int(slots * args.slots_scale))
        v, tx_bytes, text = describe(B, n_prb_grid, prb_start, n_prbs, L, qm)
        mod = MO.PuschModulator(*hops(n_prb_grid, prb_start, n_prbs, L), L, n_prb_grid, qm, device=dev)
        g = torch.empty((B, mod.g_row_bytes), dtype=torch.uint8, device=dev).random_(generator=gen)
        pil = torch.view_as_complex(torch.randn((B, mod.n_re, mod.n_dmrs_total, L, 2), generator=gen, device=dev))
        rnti = torch.randint(0, 65536, (B,), generator=gen, device=dev, dtype=torch.int32)
        n_id = torch.randint(0, 1024, (B,), generator=gen, device=dev, dtype=torch.int32)
        out = torch.empty((B, L, 14, 12 * n_prb_grid), dtype=torch.complex64, device=dev)
        mod(g, pil, 1.4125, rnti=rnti, n_id=n_id, out=out)      # creates the plan; the launches below reuse these tensors
        ptrs = [C.c_void_p(t.data_ptr()) for t in (g, pil, rnti, n_id, out)]
        strides = (C.c_int64 * 2)(1, 1)
        a = lambda: mod._launch(ptrs[0], ptrs[1], pil[0].numel(), C.c_float(1.4125), ptrs[2], ptrs[3], strides, B, ptrs[4])      # noqa: E731
        b = lambda: out.zero_()                                                                                                  # noqa: E731
        for fn in (a, b):
            timed(fn, 3)
        t = {k: [] for k in "ab"}
        for _ in range(args.repeats):
            t["a"].append(timed(a, args.launches))
            t["b"].append(timed(b, args.launches))
        m = {k: statistics.mean(x) for k, x in t.items()}
        lines += [text,
                  f"  (a) ce_mod_modulate    {stats(t['a'])}   {tx_bytes / m['a'] / 1e6:8.1f} GB/s of tx written",
                  f"  (b) zero_() of tx      {stats(t['b'])}   {tx_bytes / m['b'] / 1e6:8.1f} GB/s",
                  f"  (a)/(b) = {m['a'] / m['b']:.3f}"]
        del mod, g, pil, out
        torch.cuda.empty_cache()
    return lines


def main():
    ap = parser(__doc__, "mod_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    args = ap.parse_args()
    if args.launches < 100 and not args.rehearse:
        args.launches = 100                                         # tens of microseconds per call: a window of 20 calls times the clock
    head = [f"tools/mod_perf.py: random bits and pilots, scrambling on; {args.launches} launches x {args.repeats} repeats of (a) (b), alternating"]
    if args.rehearse:
        print("\n".join(head + [describe(*s)[2] + " -- not measured" for s in SHAPES]))
        return
    lines = head + measure(args)
    lines[0] += f"; {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    finish(lines, args.out)


if __name__ == "__main__":
    main()
