#!/usr/bin/env python3
"""Dev tool (GPU box): what the LDPC decoder extension (include/ce_ldpc.h) costs -- 8192 slots' worth of code blocks (one
per slot) of random int8 soft values on seeded random graphs of the NR shape (tests/ldpc_oracle.py `random_graph`; the
base-graph tables of TS 38.212 are not in this repository): 46 x 68 with 19-edge core rows at zc = 384 and 64, and
42 x 52 at zc = 36; early_stop off, 8 iterations, no post output.

  PuschLdpcDecoder, one launch                device events, LAUNCHES launches per repeat

Writes ms per launch (mean and range over the repeats), blocks/s, information Gbit/s (k_out = n_sys zc bits per block),
ns per block-iteration, and the LDS traffic the layout implies per block-iteration (per edge and lifted check 2 bytes of L
read and 2 written, per lifted check 5 bytes of state read and 5 written; the single parity pass at the end reads 2
bytes per edge and check once) with the LDS rate that implies, to profiles/ldpc_perf.txt (--out).  There is no pass mark.
`--rehearse` runs the host-side logic without a GPU and measures nothing."""
import statistics
import sys

import numpy as np
import torch

from _perf_common import ROOT, finish, gpu, parser, stats, timed

sys.path.insert(0, str(ROOT / "tests"))
import ldpc_oracle as O  # noqa: E402

from srsran_ce_pytorch_amd import ldpc as LD  # noqa: E402

BLOCKS, ITERS = 8192, 8
SHAPES = (("46 x 68", 1, 384, 31), ("46 x 68", 1, 64, 32), ("42 x 52", 2, 36, 33))


def describe(label, bg, zc, seed):
    sh = O.SHAPE[bg]
    rows = O.random_graph(np.random.default_rng(seed), sh["n_sys"], sh["n_rows"], zc, sh["core_degree"], sh["ext"])
    graph = LD.LdpcGraph(rows, sh["n_sys"] + sh["n_rows"])
    n_in, k_out = (graph.n_cols - 2) * zc, sh["n_sys"] * zc
    v = LD.derive_host(graph, zc, n_in, k_out, max_iters=ITERS, early_stop=False)
    lds_per_iter = zc * (4 * v.n_edges + 10 * graph.n_rows) + zc * 2 * v.n_edges / ITERS
    text = (f"{label} random graph, zc = {zc}: {v.n_edges} edges, row degree <= {v.max_row_degree}, n_in = {n_in}, k_out = {k_out}; "
            f"{v.blocks_per_workgroup} block(s) per workgroup of {v.threads} threads, {v.lds_bytes} B LDS; "
            f"{lds_per_iter / 1e3:.1f} kB of LDS traffic per block-iteration")
    return graph, n_in, k_out, lds_per_iter, text


def main():
    ap = parser(__doc__, "ldpc_perf")
    ap.add_argument("--blocks-scale", type=float, default=1.0, help="scale the batch size (a smaller card)")
    args = ap.parse_args()
    B = max(1, int(BLOCKS * args.blocks_scale))

    lines = [f"tools/ldpc_perf.py: {B} code blocks, early_stop off, {ITERS} iterations; {args.launches} launches x {args.repeats} repeats"]
    if args.rehearse:
        print("\n".join(lines + [describe(*s)[4] + " -- not measured" for s in SHAPES]))
        return

    dev = gpu("ldpc_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    for shape in SHAPES:
        graph, n_in, k_out, lds_per_iter, text = describe(*shape)
        dec = LD.PuschLdpcDecoder(graph, shape[2], n_in, k_out, max_iters=ITERS, early_stop=False, device=dev)
        soft = torch.randint(-127, 128, (B, n_in), dtype=torch.int8, device=dev, generator=g)
        a = lambda: dec(soft)      # noqa: E731
        timed(a, 3)                # warm-up: code object, allocator
        hard, status = dec(soft)
        assert bool((status[:, 0] == ITERS).all())
        ta = [timed(a, args.launches) for _ in range(args.repeats)]
        ma = statistics.mean(ta)
        lines += [text,
                  f"  PuschLdpcDecoder, one launch   {stats(ta)}   {B / ma / 1e3:8.3f} M blocks/s   {B * k_out / ma / 1e6:7.2f} information Gbit/s   "
                  f"{ma * 1e6 / (B * ITERS):8.1f} ns per block-iteration   {B * ITERS * lds_per_iter / ma / 1e9:6.2f} TB/s of LDS traffic by the layout's count"]
        del dec, soft, hard, status
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
