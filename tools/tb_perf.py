#!/usr/bin/env python3
"""Dev tool (GPU box): what the transport-block assembly extension (include/ce_tb.h) costs on random `hard` rows at

  8192 slots of A = 8424 on BG1      C = 1, K' = 8448: one launch
  64 slots of A = 1277992 on BG1     C = 152, K' = 8432 (the largest NR transport block): the assembly and the fold launch

Two timings alternate in one process, both through preallocated tensors:

  (a) ce_tb_assemble                                       device events, LAUNCHES launches per repeat
  (b) a device-to-device Tensor.copy_ of the same `hard`   the same

Writes ms per call (mean and range over the repeats), (a)/(b), code blocks/s and the GB/s of `hard` each implies to
profiles/tb_perf.txt (--out).  Both are a few microseconds of device work per call, so the figures hold the launch path of
each too; kernel times come from a kernel trace of this tool, in a run of its own.  `--variant NAME=LIB` runs the same
measurement in a child process on a diagnostic build of the library (tools/variants_build.sh with -DCE_TB_NIBBLE: the
replicated 16-entry CRC table; -DCE_TB_NO_FOLD: the first launch alone, which gives the fold launch by difference) and appends its
lines.  There is no pass mark.  `--rehearse` runs the host-side logic without a GPU and measures nothing."""
import ctypes as C
import os
import statistics
import subprocess
import sys

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import transportblock as TB

SHAPES = ((8192, 1, 8424), (64, 1, 1277992))      # slots, base graph, A


def describe(slots, bg, A):
    v = TB.derive_host(bg, A)
    n_wg = -(-slots * v.c // v.blocks_per_workgroup)
    fold = f" + {-(-slots // v.fold_slots_per_workgroup)} for the fold" if v.c > 1 else ", no fold launch"
    return v, (f"{slots} slots x A = {A} on BG{bg}: C = {v.c}, K' = {v.k_prime}, P = {v.p}, {v.piece_dwords} dwords of a row per lane; hard {slots * v.c * v.in_row_bytes / 1e6:.2f} MB, "
               f"tb {slots * v.tb_row_bytes / 1e6:.2f} MB; {n_wg} workgroups of {v.threads} threads ({v.blocks_per_workgroup} code blocks each, {v.lds_bytes} B LDS){fold}")


def measure(args, label):
    dev = gpu("tb_perf")
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    lines = []
    for slots, bg, A in SHAPES:
        S = max(1, int(slots * args.slots_scale))
        v, text = describe(S, bg, A)
        asm = TB.PuschTransportBlock(bg, A, device=dev)
        hard = torch.empty((S, v.c, v.in_row_bytes), dtype=torch.uint8, device=dev).random_(generator=g)
        tb, tb_status, cb_status = asm(hard)                       # creates the plan; the launches below reuse these tensors
        dst = torch.empty_like(hard)
        ptrs = [C.c_void_p(t.data_ptr()) for t in (hard, tb, tb_status, cb_status)]
        a = lambda: asm._launch(ptrs[0], S, ptrs[1], ptrs[2], ptrs[3])      # noqa: E731
        b = lambda: dst.copy_(hard)                                          # noqa: E731
        for fn in (a, b):
            timed(fn, 3)
        ta, tb_ = [], []
        for _ in range(args.repeats):
            ta.append(timed(a, args.launches))
            tb_.append(timed(b, args.launches))
        ma, mb = statistics.mean(ta), statistics.mean(tb_)
        nbytes = hard.numel()
        lines += [f"[{label}] {text}",
                  f"  (a) ce_tb_assemble{', both launches' if v.c > 1 else '':16s} {stats(ta)}   {S * v.c / ma / 1e3:8.2f} M code blocks/s   {nbytes / ma / 1e6:8.1f} GB/s of hard read",
                  f"  (b) copy_ of hard, {nbytes / 1e6:6.2f} MB       {stats(tb_)}   {nbytes / mb / 1e6:8.1f} GB/s read and as much written",
                  f"  (a)/(b) = {ma / mb:.3f}   (per repeat {min(p / q for p, q in zip(ta, tb_)):.3f} .. {max(p / q for p, q in zip(ta, tb_)):.3f})"]
        del asm, hard, dst, tb, tb_status, cb_status
        torch.cuda.empty_cache()
    return lines


def main():
    ap = parser(__doc__, "tb_perf")
    ap.add_argument("--slots-scale", type=float, default=1.0, help="scale the batch sizes (a smaller card)")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB", help="also measure a diagnostic build of the library, in a child process")
    ap.add_argument("--child", default="", help=argparse_suppress())
    args = ap.parse_args()
    if args.launches < 200 and not args.rehearse and not args.child:
        args.launches = 200                                         # microseconds per call: a window of 20 calls times the clock
    head = [f"tools/tb_perf.py: random hard rows; {args.launches} launches x {args.repeats} repeats, alternating (a) (b)"]
    if args.rehearse:
        print("\n".join(head + [describe(*s)[1] + " -- not measured" for s in SHAPES]))
        return
    if args.child:                                                  # a variant's measurement: lines on stdout, nothing written
        print("\n".join(measure(args, args.child)))
        return
    lines = head + measure(args, "shipped library")
    lines[0] += f"; {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    for item in args.variant:
        name, _, lib = item.partition("=")
        if not os.path.exists(lib):
            raise SystemExit(f"--variant {item}: {lib} does not exist")
        cmd = [sys.executable, __file__, "--child", name, "--launches", str(args.launches), "--repeats", str(args.repeats), "--slots-scale", str(args.slots_scale)]
        out = subprocess.run(cmd, env=dict(os.environ, CE_HIP_LIB=os.path.abspath(lib)), check=True, capture_output=True, text=True, timeout=300)
        lines += out.stdout.rstrip("\n").split("\n")
    finish(lines, args.out)


def argparse_suppress():
    import argparse
    return argparse.SUPPRESS


if __name__ == "__main__":
    main()
