"""A bounded, deterministic differential fuzz on the GPU of the OFDM modulator (csrc/ce_ofdm.hip `ce_ofdmtx_kernel` through
`PuschOfdmModulator`), the one PUSCH kernel the three earlier fuzzes leave at pinned cases: the 120 seeded draws of
tests/tx_fuzz_cases.py against the float64 operator ofdm_oracle.modulate under ofdm_tx_oracle.check with T = 4 C_TX_FUZZ, the
constant tests/test_tx_fuzz.py calibrates on these same cases with the float32 restatement (a sample of an all-zero symbol,
whose unit is 0, must be exactly 0: tx_fuzz_cases.tx_check).  Around the values: every cyclic prefix is bitwise its symbol's
tail; `out` lies in a sentinel-filled stream between guards and every element outside the first T samples of its rows -- gaps,
the surplus of a longer last dimension, lead, tail and guards -- is bitwise the sentinel afterwards; the grid, which lies in a
longer buffer of NaN, is bitwise unchanged, and no NaN reaches a sample; one (slot, port) of a batch equals its own call bit for
bit; a modulator built through `for_demodulator` gives the bits of one built directly, and the demodulator it was built from
returns |phi_l|^2 X from the samples, at its own window advance, under T_PAIR.  Nothing is skipped.

Every assertion message carries the case's dict: `realize_tx` of that dict replays the case on the CPU.  Every input is one the
oracle and the header define.

The file's name sorts it behind test_zzzzzzzzzzzzzz_hip_ofdm_tx.py: every earlier GPU test keeps its place in the run."""
import numpy as np
import pytest
import torch

import ofdm_oracle as OO
import tx_fuzz_cases as F
from srsran_ce_pytorch_amd import ofdm as OF

pytestmark = pytest.mark.gpu

# Cases a run flagged, kept exactly as they were drawn (the dicts of tx_fuzz_cases.draw_tx); they run after the seeded ones.
LOGGED_TX_CASES = []

GUARD = 64                                   # complex64 elements either side of a guarded buffer: keeps 16-byte alignment
FILL = np.complex64(complex(-5.0, 7.0))      # the sentinel
NAN = np.complex64(complex(np.nan, np.nan))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)      # one word per complex64 element: the shape stays


FILL_BITS = _bits(np.array([FILL]))[0]


def _grid(c, g):
    """(buffer, host copy, view): the grid g [B, R, n_sc, n_sym] as the permuted view of a dense [B, R, n_sym, n_sc] block that
    starts grid_lead elements into a buffer whose other elements are NaN -- 16-byte aligned, the only form the wrapper accepts."""
    B, R, n_sc, n_sym = g.shape
    n = B * R * n_sym * n_sc
    host = np.full(c["grid_lead"] + n + c["grid_tail"], NAN, np.complex64)
    host[c["grid_lead"]:c["grid_lead"] + n] = np.swapaxes(g, -1, -2).reshape(-1)
    buf = torch.as_tensor(host, device=_dev())
    view = buf[c["grid_lead"]:c["grid_lead"] + n].view(B, R, n_sym, n_sc).permute(0, 1, 3, 2)
    assert view.data_ptr() % 16 == 0, c
    return buf, host, view


def _out(c, T):
    """(stream, out): the case's `out` as a strided view into a sentinel-filled stream with a guard either side."""
    stream = torch.full((2 * GUARD + c["lead"] + F.tx_extent(c) + c["tail"],), complex(FILL), dtype=torch.complex64, device=_dev())
    out = stream.as_strided((c["B"], c["R"], c["row_len"]), (c["slot_stride"], c["port_stride"], 1), GUARD + c["lead"])
    assert out.data_ptr() % 16 == (8 if c["lead"] % 2 else 0), c
    return stream, out


@pytest.mark.parametrize("idx", range(F.N_TX + len(LOGGED_TX_CASES)))
def test_modulator_fuzz_case(idx):
    c = F.draw_tx(idx) if idx < F.N_TX else LOGGED_TX_CASES[idx - F.N_TX]
    what = f"tx {c}"
    d = F.realize_tx(c)
    dev, N, B, R, n_sym, T = _dev(), c["n_fft"], c["B"], c["R"], c["n_sym"], d.T
    direct = OF.PuschOfdmModulator(N, c["n_prb_grid"], c["cp_len"], n_sym=n_sym, sym_phasor=d.phi, device=dev)
    dem = None
    if c["via_dem"]:
        dem = OF.PuschOfdmDemodulator(N, c["n_prb_grid"], c["cp_len"], n_sym=n_sym, window_advance=c["advance"], sym_phasor=d.phi, device=dev)
    mod = OF.PuschOfdmModulator.for_demodulator(dem) if c["via_dem"] else direct
    assert mod.n_samples == T and mod.window_advance == 0, what
    buf, host, grid = _grid(c, d.grid)
    stream = out = None
    if c["layout"] != "dense":
        stream, out = _out(c, T)
    s = mod(grid, out=out)
    torch.cuda.synchronize()
    assert tuple(s.shape) == (B, R, T) and s.dtype == torch.complex64 and s.device == dev and (out is None or s.data_ptr() == out.data_ptr()), what
    got = s.cpu().numpy()
    # ---- values ----
    assert np.all(np.isfinite(got.view(np.float32))), f"{what}: non-finite samples (a read outside the grid reaches NaN)"
    F.tx_check(got, d.ref, d.rms, N, what, F.T_TX_FUZZ)
    # ---- the cyclic prefix: the symbol's tail stored a second time ----
    bits = _bits(got)
    for l, (t, cp) in enumerate(zip(d.starts, c["cp_len"])):
        assert np.array_equal(bits[..., t:t + cp], bits[..., t + N:t + N + cp]), f"{what}: the prefix of symbol {l} is not its tail"
    # ---- the write set ----
    if stream is not None:
        after = stream.cpu().numpy()
        body, rows = after[GUARD:len(after) - GUARD], F.tx_rows(c)
        assert len(body) == len(rows) and np.all(_bits(after[:GUARD]) == FILL_BITS) and np.all(_bits(after[len(after) - GUARD:]) == FILL_BITS), f"{what}: a guard was written"
        hit = ~rows & (_bits(body) != FILL_BITS)
        assert not hit.any(), f"{what}: written outside the rows, first at stream elements {np.flatnonzero(hit)[:4].tolist()}"
        for b in range(B):
            for r in range(R):
                o = c["lead"] + b * c["slot_stride"] + r * c["port_stride"]
                assert np.array_equal(_bits(body[o:o + T]), bits[b, r]), f"{what}: row ({b}, {r}) of the stream is not what was returned"
    # ---- the input ----
    assert np.array_equal(_bits(buf), _bits(host)), f"{what}: the grid's buffer was written"
    # ---- one (slot, port) alone ----
    if B * R > 1:
        b, r = c["slot"], c["port"]
        one = mod(_grid(c, d.grid[b:b + 1, r:r + 1])[2])
        torch.cuda.synchronize()
        assert np.array_equal(_bits(one)[0, 0], bits[b, r]), f"{what}: (slot, port) = ({b}, {r}) alone differs"
    # ---- the construction path and the way back ----
    if c["via_dem"]:
        plain = direct(grid)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(plain), bits), f"{what}: the directly constructed modulator differs"
        back = dem(s)                                     # the strided view of `out` where the case has one
        torch.cuda.synchronize()
        assert tuple(back.shape) == (B, R, d.n_sc, n_sym), what
        F.tx_check(back.cpu().numpy(), d.pair_ref, d.pair_rms, N, what + " round trip", F.T_PAIR, rule=OO.check)
