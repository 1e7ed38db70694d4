#!/usr/bin/env python3
"""Dev tool (GPU box): what fronthaul I/Q (de)compression (include/ce_tp.h `ce_fh_decompress`, `ce_fh_compress`) costs at
273 PRB x 14 symbols x 4 ports, for BFP of 9 and of 14 bits and for plain int16, in a batch of --slots slots (256: 0.38 GB of
grid, beyond the Infinity Cache).  The timings alternate in one process, device events around LAUNCHES launches per repeat:

  (a)  PuschFronthaulDecompressor, one launch              (b)  PuschFronthaulCompressor, one launch
  (ca) (cb) traffic twins that move the same bytes with torch: for (a) a copy of the payload's bytes and a fill of the rest
       of the grid's (reads the payload's bytes, writes the grid's); for (b) a copy of the payload's bytes and a sum over the
       rest of the grid's (reads the grid's bytes, writes the payload's)
  (da) (db) the torch compositions a user would write today: for (a) three byte gathers, shifts and masks, the sign, the
       exponent shift, the conversion and the product; for (b) the quantiser, the per-PRB maximum, frexp for the bit length,
       the shift, the mantissas' bits spread out and summed into bytes.  Both are compared with the kernels' outputs, by bits.

Writes the times, their spread, GB/s on the bytes the kernels must move and (a)/(ca), (a)/(da), (b)/(cb), (b)/(db) with the
range over the repeats to profiles/fh_perf.txt (--out).  `--rehearse` runs the host-side logic without a GPU and measures
nothing."""
import statistics

import torch

from _perf_common import finish, gpu, parser, stats, timed

from srsran_ce_pytorch_amd import fronthaul as FH

N_PRB, N_SYM, N_PORTS = 273, 14, 4
FORMATS = (("bfp", 9), ("bfp", 14), ("none", 16))
SCALE = 2.0 ** -11


def describe(method, W, B):
    nb = N_PRB * (1 + 3 * W if method == "bfp" else 48)
    rows = B * N_PORTS * N_SYM
    return nb, rows, (f"{method} W={W}: {B} slots x {N_PORTS} ports x {N_SYM} symbols x {N_PRB} PRB: rows of {nb} bytes <-> {12 * N_PRB} REs, "
                      f"{rows * nb / 1e6:.1f} MB of payload, {rows * 96 * N_PRB / 1e6:.1f} MB of grid, {rows * 5} workgroups of 256 threads")


def torch_decompress(rows3, hdr, W, scale, idx, shift):
    """uint8 [rows, n_prb, prb_bytes] -> float32 [rows, n_prb, 24]: shift-and-mask over three gathered bytes per mantissa."""
    word = (rows3[..., idx].to(torch.int32) << 16) | (rows3[..., idx + 1].to(torch.int32) << 8) | rows3[..., idx + 2].to(torch.int32)
    m = (word >> shift) & ((1 << W) - 1)
    m = (m ^ (1 << (W - 1))) - (1 << (W - 1))
    if hdr:
        m = m << (rows3[..., :1].to(torch.int32) & 15)
    return m.to(torch.float32) * scale


def torch_compress(x, hdr, W, inv_scale, weights):
    """float32 [rows, n_prb, 24] -> uint8 [rows, n_prb, prb_bytes]."""
    v = torch.nan_to_num(torch.round(x * inv_scale), nan=0.0).clamp_(-32768.0, 32767.0).to(torch.int32)
    parts = []
    if hdr:
        peak = torch.where(v >= 0, v, ~v).amax(-1, keepdim=True)
        e = (torch.frexp(peak.to(torch.float32))[1] + 1 - W).clamp_(min=0)
        v = v >> e
        parts.append(e.to(torch.uint8))
    bits = ((v[..., None] >> weights["down"]) & 1).to(torch.uint8)                  # [rows, n_prb, 24, W], MSB first
    parts.append((bits.reshape(bits.shape[0], bits.shape[1], 3 * W, 8) * weights["byte"]).sum(-1).to(torch.uint8))
    return torch.cat(parts, -1) if hdr else parts[0]


def main():
    ap = parser(__doc__, "fh_perf")
    ap.add_argument("--slots", type=int, default=256)
    args = ap.parse_args()
    B = args.slots
    lines = [f"tools/fh_perf.py: {N_PRB} PRB x {N_SYM} symbols x {N_PORTS} ports, {B} slots, scale 2^-11; {args.launches} launches x {args.repeats} repeats, "
             "alternating (a) (ca) (da) (b) (cb) (db)"]
    if args.rehearse:
        print("\n".join(lines + [describe(m, W, B)[2] + " -- not measured" for m, W in FORMATS]))
        return

    dev = gpu("fh_perf")
    lines[0] += f"; {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"
    g = torch.Generator(device=dev)
    g.manual_seed(16)
    n_sc = 12 * N_PRB
    src = torch.empty((B, N_PORTS, N_SYM, n_sc, 2), dtype=torch.float32, device=dev).normal_(generator=g).mul_(200.0 * SCALE)
    src[:, :, :, ::36] *= 40.0                                                # every 36th RE louder: several exponents
    grid_in = torch.view_as_complex(src).permute(0, 1, 3, 2)
    grid_out = torch.empty((B, N_PORTS, N_SYM, n_sc), dtype=torch.complex64, device=dev).permute(0, 1, 3, 2)
    grid_bytes = grid_out.permute(0, 1, 3, 2).reshape(-1).view(torch.uint8)
    for method, W in FORMATS:
        nb, rows, text = describe(method, W, B)
        hdr, pb = (1 if method == "bfp" else 0), nb // N_PRB
        fh = FH.PuschFronthaulDecompressor(N_PRB, N_SYM, method, W, SCALE, device=dev)
        comp = FH.PuschFronthaulCompressor.for_decompressor(fh)
        wire = torch.zeros((B, N_PORTS, N_SYM, (nb + 3) // 4 * 4), dtype=torch.uint8, device=dev)      # rows start on 4 bytes
        comp(grid_in, out=wire)
        rb, wb = rows * nb // 4 * 4, grid_bytes.numel()
        wire_out, wire_flat = torch.empty_like(wire), torch.zeros((rb,), dtype=torch.uint8, device=dev)
        offs = hdr * 8 + W * torch.arange(24, device=dev)
        idx = (offs >> 3).clamp(max=pb - 3)
        shift = (8 * (idx + 3) - offs - W).to(torch.int32)                      # the mantissa's distance from the low end of its three bytes
        weights = dict(down=torch.arange(W - 1, -1, -1, device=dev, dtype=torch.int32), byte=torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=dev))
        rows3, x3 = wire.view(rows, -1)[:, :nb].unflatten(1, (N_PRB, pb)), src.view(rows, N_PRB, 24)

        fns = {"a": lambda: fh(wire, out=grid_out), "ca": lambda: (grid_bytes[:rb].copy_(wire_flat), grid_bytes[rb:].fill_(0)),
               "da": lambda: torch_decompress(rows3, hdr, W, float(fh.scale), idx, shift),
               "b": lambda: comp(grid_in, out=wire_out), "cb": lambda: (wire_flat.copy_(grid_bytes[:rb]), grid_bytes[rb:].view(torch.int32).sum()),
               "db": lambda: torch_compress(x3, hdr, W, float(fh.inv_scale), weights)}
        # the compositions are the kernels' operators: by bits (before the twins overwrite the grid)
        fh(wire, out=grid_out)
        same_a = torch.equal(torch.view_as_real(grid_out.permute(0, 1, 3, 2)).reshape(rows, N_PRB, 24).view(torch.int32), fns["da"]().view(torch.int32))
        same_b = torch.equal(fns["db"]().view(rows, nb), wire.view(rows, -1)[:, :nb])
        for fn in fns.values():                                              # warm-up: code objects, allocator
            timed(fn, 2)
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.launches))
        m = {k: statistics.mean(ts) for k, ts in t.items()}
        ratio = lambda p, q: f"{m[p] / m[q]:.3f} ({min(u / w for u, w in zip(t[p], t[q])):.3f} .. {max(u / w for u, w in zip(t[p], t[q])):.3f})"   # noqa: E731
        per = lambda k: f"{(rb + wb) / m[k] / 1e6:8.1f} GB/s on {(rb + wb) / 1e9:.3f} GB"   # noqa: E731
        lines += [text,
                  f"  (a)  decompressor, one launch           {stats(t['a'])}   {per('a')}",
                  f"  (ca) twin: copy + fill                  {stats(t['ca'])}   {per('ca')}",
                  f"  (da) torch shift-and-mask composition   {stats(t['da'])}   {per('da')}",
                  f"  (b)  compressor, one launch             {stats(t['b'])}   {per('b')}",
                  f"  (cb) twin: copy + sum                   {stats(t['cb'])}   {per('cb')}",
                  f"  (db) torch composition                  {stats(t['db'])}   {per('db')}",
                  f"  (a)/(ca) = {ratio('a', 'ca')};  (a)/(da) = {ratio('a', 'da')};  (b)/(cb) = {ratio('b', 'cb')};  (b)/(db) = {ratio('b', 'db')}",
                  f"  composition == kernel by bits: decompress {same_a}, compress {same_b}"]
        del fh, comp, wire, wire_out, wire_flat, fns, rows3
        torch.cuda.empty_cache()
    finish(lines, args.out)


if __name__ == "__main__":
    main()
