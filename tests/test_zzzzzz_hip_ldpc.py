"""GPU tests of the LDPC decoder extension (include/ce_ldpc.h): the kernel against the integer oracle of
tests/ldpc_oracle.py, by value (np.array_equal on hard, status and post -- no tolerance), on the smallest shapes at which
each path can go wrong: 2 x 4 at zc = 2, BG2-shaped 42 x 52 random graphs at zc = 7, 36, 64, 72, BG1-shaped 46 x 68 graphs
with 19-edge core rows at zc = 15, 208, 384 (the LDS maximum), a 12-row truncation and a graph without punctured columns.
The conditions these tests lean on (which inputs decode, where the mixed batch stops) are asserted from the oracle alone
in tests/test_ldpc.py.

The base-graph tables of TS 38.212 5.3.2 are not in this repository: every graph is a seeded random graph of the NR shape,
and nothing here is, or claims to be, a test against the real tables.

The file's name sorts it behind test_zzzzz_hip_tp.py: every earlier GPU test keeps its place in the run."""
import ctypes as C

import numpy as np
import pytest
import torch

import ldpc_oracle as O
from srsran_ce_pytorch_amd import _lib, ldpc as LD, ratematch as RM

pytestmark = pytest.mark.gpu

ALL = [c["name"] for c in O.CASES if c["name"] != "bg2_z8"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())      # a copy: the shared inputs are read-only


def _dec(name, **kw):
    g = O.graph(name)
    kw.setdefault("n_punctured_cols", g.n_punct)
    n_in, k_out = kw.pop("n_in", g.n_in), kw.pop("k_out", g.k_out)
    return g, LD.PuschLdpcDecoder(LD.LdpcGraph(g.rows, g.n_cols), g.zc, n_in, k_out, device=_dev(), **kw)


def _run(dec, llr, post=True):
    out = dec(_t(llr) if isinstance(llr, np.ndarray) else llr, return_post=post)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _ref(g, llr, max_iters, early, scale=1.0, k_out=None, n_punct=None):
    n_punct = g.n_punct if n_punct is None else n_punct
    L, status, _ = O.decode_ref(g.rows, g.n_cols, g.zc, O.channel(O.quantise(llr, scale), g.n_cols, g.zc, n_punct), max_iters, early)
    return O.pack(L, g.k_out if k_out is None else k_out), status, L


def _same(got, ref, what=""):
    hard, status, post = got
    rh, rs, rl = ref
    assert hard.dtype == np.uint8 and status.dtype == np.int32 and post.dtype == np.int16
    assert np.array_equal(status, rs), (what, status.tolist(), rs.tolist())
    assert np.array_equal(post, rl), (what, np.argwhere(post != rl)[:4].tolist())
    assert np.array_equal(hard, rh), what


@pytest.mark.parametrize("name", ALL)
def test_random_rows_against_the_oracle(name):
    """Not codewords, so most never converge: max_iters = 1, 2, 8 with early_stop on and off."""
    llr = O.random_inputs(name)
    for max_iters in (1, 2, 8):
        for early in (True, False):
            g, dec = _dec(name, max_iters=max_iters, early_stop=early)
            got = _run(dec, llr)
            assert got[0].shape == (3, dec.row_bytes) and got[1].shape == (3, 2) and got[2].shape == (3, g.n_bits)
            L, status, hard = O.reference(name, "random", max_iters, early)
            _same(got, (hard, status, L), f"{name} iters={max_iters} early={early}")


@pytest.mark.parametrize("name", O.CODEWORD_CASES)
def test_noisy_codewords_decode_to_the_bits_sent(name):
    info, llr = O.codeword_inputs(name)
    g, dec = _dec(name)
    got = _run(dec, llr)
    L, status, hard = O.reference(name, "codeword", 8, True)
    _same(got, (hard, status, L), name)
    assert np.array_equal(LD.unpack_bits(got[0], g.k_out), info) and np.all(got[1][:, 1] == 1)
    # [B, C, n_in] keeps its leading dimensions; without post the other two outputs are the same
    h3, s3 = _run(dec, _t(llr)[None], post=False)
    assert h3.shape == (1, 3, dec.row_bytes) and s3.shape == (1, 3, 2) and np.array_equal(h3[0], got[0]) and np.array_equal(s3[0], got[1])


@pytest.mark.parametrize("name", O.MIXED_CASES)
def test_mixed_batch_where_neighbours_stop_at_different_iterations(name):
    llr = O.mixed_inputs(name)
    g, dec = _dec(name)
    assert dec.blocks_per_workgroup >= 7
    got = _run(dec, llr)
    L, status, hard = O.reference(name, "mixed", 8, True)
    _same(got, (hard, status, L), name)
    for b in (0, 1, 4, 6, len(llr) - 1):                       # a block alone equals its place in the batch
        one = _run(dec, llr[b:b + 1])
        assert all(np.array_equal(o[0], w[b]) for o, w in zip(one, got)), b
    rev = _run(dec, llr[::-1])
    assert all(np.array_equal(r[::-1], w) for r, w in zip(rev, got))
    # without early_stop every block runs all 8 iterations and the parity is evaluated at the end
    g, dec = _dec(name, early_stop=False)
    L, status, hard = O.reference(name, "mixed", 8, False)
    assert np.all(status[:, 0] == 8) and 0 < status[:, 1].sum() < len(llr)
    _same(_run(dec, llr), (hard, status, L), name)


def test_more_workgroups_than_cus_at_zc_8():
    """zc = 8 packs 32 blocks into a workgroup, so 600 blocks would be 19 workgroups: 8790 blocks are 275, more than the 256
    CUs, the last one with 22 blocks.  Noisy codewords at four noise levels with every 32nd row random."""
    name, nb = "bg2_z8", 8790
    g, dec = _dec(name)
    assert dec.blocks_per_workgroup == 32 and -(-nb // 32) == 275 > torch.cuda.get_device_properties(_dev()).multi_processor_count
    rng = np.random.default_rng(99)
    info = rng.integers(0, 2, (nb, g.k_out))
    tx = O.encode(g.rows, g.n_sys, g.zc, info)[:, g.n_punct * g.zc:]
    llr = np.empty((nb, g.n_in), np.int8)
    for i, db in enumerate((3.0, 1.0, -1.0, -3.0)):
        llr[i::4] = O.noisy_llr(rng, tx[i::4], db, O.SCALE)
    llr[::32] = rng.integers(-128, 128, llr[::32].shape)      # one per workgroup runs all 8 iterations
    ref = _ref(g, llr, 8, True)
    assert len(set(ref[1][:, 0].tolist())) >= 4
    got = _run(dec, llr)
    _same(got, ref, name)
    for b in (0, 31, 32, 4391, nb - 23, nb - 1):
        one = _run(dec, llr[b:b + 1])
        assert all(np.array_equal(o[0], w[b]) for o, w in zip(one, got)), b
    one = _run(dec, llr[:600])                                  # 19 workgroups
    assert all(np.array_equal(o, w[:600]) for o, w in zip(one, got))


@pytest.mark.parametrize("name", ["bg2_z7", "bg1_z208"])
def test_float32_input_equals_int8_input_of_quantise(name):
    scale = 4.0                                                 # a power of two: the ties below are exact
    g, f32 = _dec(name, dtype=torch.float32, llr_scale=scale)
    _, i8 = _dec(name)
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((3, g.n_in)) * 20.0).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.5 / 4, -0.5 / 4, 1.5 / 4, 2.5 / 4, -2.5 / 4, 1e9, -1e9, 127.4 / 4, 127.6 / 4, -0.0, 3e38, -3e38,
                        42.5, -42.5, 1e-30], np.float32)
    x[1, 5:5 + len(special)] = special
    x[2, -len(special):] = special[::-1]
    q = O.quantise(x, scale)
    assert q.min() == -127 and q.max() == 127 and np.array_equal(O.quantise(special, scale)[:8], [0, 127, -127, 0, 0, 2, 2, -2])
    got = _run(f32, x)
    _same(got, _ref(g, x, 8, True, scale), name)
    assert all(np.array_equal(a, b) for a, b in zip(got, _run(i8, q.astype(np.int8))))


def test_int8_minus_128_is_minus_127_and_all_zero_stops_at_once():
    for name in ("bg2_z7", "bg2_z72"):
        g, dec = _dec(name)
        llr = np.array(O.random_inputs(name))
        llr[0, ::3] = -128
        llr[1] = -128
        twin = np.maximum(llr, -127).astype(np.int8)
        got = _run(dec, llr)
        _same(got, _ref(g, llr, 8, True), name)
        assert all(np.array_equal(a, b) for a, b in zip(got, _run(dec, twin)))
        hard, status, post = _run(dec, np.zeros((5, g.n_in), np.int8))
        assert not hard.any() and status.tolist() == [[1, 1]] * 5 and not post.any()


@pytest.mark.parametrize("n_in", [350, 349, 1])
def test_input_rows_that_start_unaligned(n_in):
    """N_cb = 350 in int8: row n starts at byte 350 n; 349 makes every other start odd; n_in = 1 leaves the rest at 0."""
    g, dec = _dec("bg2_z7", n_in=n_in)
    llr = np.array(O.codeword_inputs("bg2_z7")[1])[:, :n_in]
    llr = np.concatenate([llr, np.array(O.random_inputs("bg2_z7"))[:, :n_in]])
    _same(_run(dec, llr), _ref(g, llr, 8, True), n_in)
    f32 = _dec("bg2_z7", n_in=n_in, dtype=torch.float32, llr_scale=1.0)[1]
    _same(_run(f32, llr.astype(np.float32)), _ref(g, llr, 8, True), n_in)


@pytest.mark.parametrize("k_out", [1, 127, 128, 129, 360])
def test_padding_bits_of_hard_are_zero(k_out):
    g, dec = _dec("bg2_z36", k_out=k_out, max_iters=2)
    llr = np.array(O.random_inputs("bg2_z36"))
    llr[0] = -100
    got = _run(dec, llr)
    ref = _ref(g, llr, 2, True, k_out=k_out)
    _same(got, ref, k_out)
    assert got[0].shape[1] == 16 * -(-k_out // 128) and not np.unpackbits(got[0], axis=1)[:, k_out:].any()


@pytest.mark.parametrize("name", ["bg2_z7", "bg1_z384"])
def test_guard_regions_round_all_three_outputs(name):
    g, dec = _dec(name)
    llr = O.random_inputs(name)
    ref = _ref(g, llr, 8, True)
    dec._plan()
    nb, guard = 3, 64
    sizes = (nb * dec.row_bytes, nb * 8, nb * g.n_bits * 2)
    bufs = [torch.full((guard + -(-n // 16) * 16 + guard,), 0xA5, dtype=torch.uint8, device=_dev()) for n in sizes]
    src = _t(llr)
    ptr = [C.c_void_p(b.data_ptr() + guard) for b in bufs]
    assert all(p.value % 16 == 0 for p in ptr)
    dec._launch(C.c_void_p(src.data_ptr()), nb, *ptr)
    torch.cuda.synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for r, n in zip(raw, sizes):
        assert np.all(r[:guard] == 0xA5) and np.all(r[guard + n:] == 0xA5)
    hard = raw[0][guard:guard + sizes[0]].reshape(nb, -1)
    status = raw[1][guard:guard + sizes[1]].view(np.int32).reshape(nb, 2)
    post = raw[2][guard:guard + sizes[2]].view(np.int16).reshape(nb, -1)
    _same((hard, status, post), ref, name)
    assert np.array_equal(src.cpu().numpy(), llr)                 # the input is read only
    # post = NULL skips it
    for b in bufs:
        b.fill_(0xA5)
    dec._launch(C.c_void_p(src.data_ptr()), nb, ptr[0], ptr[1], None)
    torch.cuda.synchronize()
    assert np.all(bufs[2].cpu().numpy() == 0xA5) and np.array_equal(bufs[0].cpu().numpy()[guard:guard + sizes[0]].reshape(nb, -1), ref[0])


def test_empty_batch_and_argument_errors():
    g, dec = _dec("bg2_z7")
    hard, status, post = dec(torch.empty((0, g.n_in), dtype=torch.int8, device=_dev()), return_post=True)
    assert tuple(hard.shape) == (0, 16) and tuple(status.shape) == (0, 2) and tuple(post.shape) == (0, g.n_bits)
    hard, status = dec(torch.empty((0, 2, g.n_in), dtype=torch.int8, device=_dev()))
    assert tuple(hard.shape) == (0, 2, 16) and tuple(status.shape) == (0, 2, 2)
    good = _t(O.random_inputs("bg2_z7"))
    for bad in (good.float(), good[:, :-1], good[0], good[None, None], good.cpu(), _t(np.zeros((3, 2 * g.n_in), np.int8))[:, ::2], "x"):
        with pytest.raises(ValueError):
            dec(bad)
    lib, h = dec._lib, dec._handle
    buf = torch.zeros(4096, dtype=torch.uint8, device=_dev())
    p = buf.data_ptr()
    assert p % 16 == 0
    args = [C.c_void_p(good.data_ptr()), 3, C.c_void_p(p), C.c_void_p(p + 1024), C.c_void_p(p + 2048), None]
    for i in (0, 2, 3, 4):
        bad = list(args)
        bad[i] = C.c_void_p(bad[i].value + 4)
        assert lib.ce_ldpc_decode(h, *bad) == _lib.CE_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert lib.ce_ldpc_decode(h, args[0], -1, *args[2:]) == _lib.CE_ERR_INVALID
    assert lib.ce_ldpc_decode(h, None, 3, *args[2:]) == _lib.CE_ERR_INVALID
    assert lib.ce_ldpc_decode(h, args[0], 0, None, None, None, None) == 0          # n_blocks == 0 launches nothing
    info = _lib.LdpcInfo()
    assert lib.ce_ldpc_plan_get_info(h, C.byref(info)) == 0
    assert (info.n_edges, info.row_bytes, info.n_bits, info.blocks_per_workgroup, info.threads, info.lds_bytes) == \
        (dec.n_edges, 16, 364, dec.blocks_per_workgroup, dec.threads, dec.lds_bytes)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", sorted(O.CHAINS))
def test_chain_behind_rate_recovery(which):
    """K' bits -> random-graph codeword -> the transmitted positions of rm_oracle.slot_map -> noisy int8 LLRs ->
    PuschRateRecovery -> for_rate_recovery(rm, graph): hard equals the K' bits, for rv 0 and for rv 0 then rv 2 in place."""
    x = O.chain_inputs(which)
    c, d, g = x.c, x.d, x.g
    rm = RM.PuschRateRecovery(c["bg"], c["A"], c["qm"], c["L"], c["G"], device=_dev())
    dec = LD.PuschLdpcDecoder.for_rate_recovery(rm, LD.LdpcGraph(g.rows, g.n_cols))
    assert (dec.zc, dec.n_in, dec.k_out, rm.n_code_blocks) == (d.Zc, d.N_cb, d.Kp, d.C)
    soft = rm(_t(x.llr[0]), rv=0)
    for key, llr, rv in (((0,), None, None), ((0, 2), x.llr[2], 2)):
        if llr is not None:
            soft = rm(_t(llr), rv=rv, harq=soft, out=soft)
        hard, status, post = dec(soft, return_post=True)
        torch.cuda.synchronize()
        assert np.array_equal(soft.cpu().numpy(), x.soft[key])
        assert tuple(hard.shape) == (O.CHAIN_SLOTS, d.C, dec.row_bytes) and tuple(status.shape) == (O.CHAIN_SLOTS, d.C, 2)
        assert np.array_equal(LD.unpack_bits(hard, d.Kp).numpy(), x.bits), (which, key)
        ref = _ref(g, x.soft[key].reshape(-1, d.N_cb), 8, True, k_out=d.Kp, n_punct=2)
        _same((hard.cpu().numpy().reshape(-1, dec.row_bytes), status.cpu().numpy().reshape(-1, 2), post.cpu().numpy().reshape(-1, g.n_bits)), ref, (which, key))
        assert np.all(ref[1][:, 1] == 1)
