"""CPU-side checks of the LDPC decoder extension (include/ce_ldpc.h): the ABI, the host derivation, every refusal field by
field before any device call, the oracle against itself (vectorised against loops, the identity L = ch + sum R and the
int16 bound, encoder against syndrome), the kernel's 5-byte state packing restated, the Python helpers, and -- from the
oracle alone -- the conditions the GPU tests lean on.  No GPU.

The base-graph tables of TS 38.212 5.3.2 are not in this repository: every graph here is a seeded random graph of the NR
shape (tests/ldpc_oracle.py), and nothing is, or claims to be, a test against the real tables."""
import ctypes as C

import numpy as np
import pytest
import torch

import ldpc_oracle as O
import rm_oracle as R
import srsran_ce_pytorch_amd as PKG
from srsran_ce_pytorch_amd import _lib, ldpc as LD, ratematch as RM



@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _graph(name):
    g = O.graph(name)
    return g, LD.LdpcGraph(g.rows, g.n_cols)


def test_library_exports_every_declared_ldpc_symbol(lib):
    """The header against the binding: tests/test_abi_conformance.py.  Here: the sizes this stage's header implies, the
    relations between its constants and the oracle's, and the package's re-exports."""
    # LP64 sizes implied by the header: desc 12 * 4 + 3 * 8; info 6 * 4; view 18 * 4
    assert (C.sizeof(_lib.LdpcDesc), C.sizeof(_lib.LdpcInfo), C.sizeof(_lib.LdpcHostView)) == (72, 24, 72)
    assert _lib.CE_LDPC_L_BOUND == 127 + 95 * 46 == O.L_BOUND < 2 ** 15 and (3 * 127) >> 2 == 95
    assert (_lib.CE_LDPC_STATE_IDX_SHIFT, _lib.CE_LDPC_STATE_MAG_SHIFT) == (O.IDX_SHIFT, O.MAG_SHIFT)
    assert "ce_ldpc.hip" in _lib.SOURCES and "ce_ldpc.h" in _lib.REGISTRY
    assert PKG.PuschLdpcDecoder is LD.PuschLdpcDecoder and PKG.LdpcGraph is LD.LdpcGraph


def test_host_view_values(lib):
    for c in O.CASES:
        g, G = _graph(c["name"])
        for k_out in (1, 127, 128, 129, g.k_out):
            if k_out > g.k_out:
                continue
            v = LD.derive_host(G, g.zc, g.n_in, k_out, n_punctured_cols=g.n_punct)
            deg = [len(r) for r in g.rows]
            cols = np.bincount([c for r in g.rows for c, _ in r], minlength=g.n_cols)
            assert (v.n_sys, v.n_edges, v.max_row_degree, v.max_col_degree) == (g.n_sys, sum(deg), max(deg), cols.max())
            assert v.row_bytes == 16 * -(-k_out // 128) and v.n_bits == g.n_cols * g.zc and v.threads_per_block == g.zc
            per = -(-2 * v.n_bits // 16) * 16 + -(-4 * len(g.rows) * g.zc // 16) * 16 + -(-len(g.rows) * g.zc // 16) * 16
            assert v.lds_bytes_per_block == per == v.lds_l_bytes + v.lds_state32_bytes + v.lds_state8_bytes
            bpw = max(1, min(256 // g.zc, 80896 // per))
            assert v.blocks_per_workgroup == bpw and v.threads == bpw * g.zc <= 384
            assert v.lds_flag_bytes == -(-4 * (bpw + 1) // 16) * 16 and v.lds_bytes == bpw * per + v.lds_flag_bytes <= _lib.CE_LDPC_LDS_MAX
            assert bpw == 1 or 2 * v.lds_bytes <= _lib.CE_LDPC_LDS_MAX            # two workgroups of several blocks fit a CU
            assert v.schedule_bytes == 4 * (len(g.rows) + 1 + sum(deg))
    # what the GPU shapes exercise: several blocks per workgroup below zc = 128, one above; 19-edge rows in the BG1 shape
    assert {n: LD.derive_host(_graph(n)[1], O.graph(n).zc, O.graph(n).n_in, 1, n_punctured_cols=O.graph(n).n_punct).blocks_per_workgroup for n in
            ("tiny_z2", "bg2_z7", "bg2_z8", "bg2_z36", "bg2_z64", "bg2_z72", "bg1_z15", "bg1_z208", "bg1_z384")} == \
        {"tiny_z2": 128, "bg2_z7": 36, "bg2_z8": 32, "bg2_z36": 7, "bg2_z64": 4, "bg2_z72": 3, "bg1_z15": 14, "bg1_z208": 1, "bg1_z384": 1}
    assert LD.derive_host(_graph("bg1_z384")[1], 384, 25344, 8448).max_row_degree == 19


def test_the_largest_plan_is_accepted(lib):
    """46 x 68 with every row at 19 edges, zc = 384: 140 560 bytes of LDS, one workgroup per CU."""
    rows = [[((r + 3 * e) % 68, (7 * r + e) % 384) for e in range(19)] for r in range(46)]
    v = LD.derive_host(LD.LdpcGraph(rows, 68), 384, 68 * 384 - 2 * 384, 22 * 384, max_iters=255)
    assert (v.n_edges, v.max_row_degree, v.lds_bytes, v.threads, v.blocks_per_workgroup) == (874, 19, 140560, 384, 1)
    assert v.lds_bytes == 52224 + 5 * 46 * 384 + 16 <= _lib.CE_LDPC_LDS_MAX == 163840


def _desc(**over):
    g, G = _graph("bg2_z7")
    kw = dict(n_punctured_cols=2, dtype=torch.float32, llr_scale=2.0, max_iters=8, early_stop=True)
    desc, keep = LD.build_desc(G, 7, 350, 40, **kw)
    for k, v in over.items():
        setattr(desc, k, v)
    return desc, keep


@pytest.mark.parametrize("field,value", [
    ("abi_version", 4), ("zc", 1), ("zc", 385), ("n_rows", 0), ("n_rows", 47), ("n_cols", 42), ("n_cols", 69), ("n_punctured_cols", -1),
    ("n_punctured_cols", 11), ("n_in", 0), ("n_in", 351), ("k_out", 0), ("k_out", 71), ("in_format", 2), ("in_format", -1),
    ("llr_scale", 0.0), ("llr_scale", -1.0), ("llr_scale", float("inf")), ("llr_scale", float("nan")), ("max_iters", 0),
    ("max_iters", 256), ("early_stop", 2), ("early_stop", -1), ("row_start", None), ("col", None), ("shift", None)])
def test_every_refusal_names_its_field(lib, field, value):
    desc, keep = _desc()
    view, handle = _lib.LdpcHostView(), C.c_void_p()
    assert lib.ce_ldpc_derive_host(C.byref(desc), C.byref(view)) == 0
    if value is None:
        setattr(desc, field, C.POINTER(C.c_int32)())
    else:
        setattr(desc, field, value)
    assert lib.ce_ldpc_derive_host(C.byref(desc), C.byref(view)) == _lib.CE_ERR_INVALID
    text = _lib.last_error()
    assert (field in text) or (field == "abi_version" and "ABI" in text) or (value is None and "row_start, col and shift" in text), text
    assert lib.ce_ldpc_plan_create(C.byref(desc), C.byref(handle)) == _lib.CE_ERR_INVALID and not handle.value     # before any device call
    del keep


def test_graph_refusals_name_the_array(lib):
    def rc(rows, n_cols=52, zc=7, n_in=350, k_out=40):
        desc, keep = LD.build_desc(LD.LdpcGraph(rows, n_cols), zc, n_in, k_out)
        code = lib.ce_ldpc_derive_host(C.byref(desc), C.byref(_lib.LdpcHostView()))
        return code, _lib.last_error()
    g = O.graph("bg2_z7")
    good = [list(r) for r in g.rows]
    assert rc(good)[0] == 0
    for mutate, word in ((lambda r: r.__setitem__(5, r[5][:1]), "row_start"),                      # one edge
                         (lambda r: r.__setitem__(0, [(c, 0) for c in range(20)]), "row_start"),   # 20 edges
                         (lambda r: r.__setitem__(3, r[3][:-1] + [r[3][0]]), "col"),              # a column twice
                         (lambda r: r.__setitem__(7, [(52, 0)] + r[7][1:]), "col"),
                         (lambda r: r.__setitem__(7, [(-1, 0)] + r[7][1:]), "col"),
                         (lambda r: r.__setitem__(9, [(r[9][0][0], 7)] + r[9][1:]), "shift"),
                         (lambda r: r.__setitem__(9, [(r[9][0][0], -1)] + r[9][1:]), "shift")):
        rows = [list(r) for r in good]
        mutate(rows)
        code, text = rc(rows)
        assert code == _lib.CE_ERR_INVALID and word in text, (word, text)
    desc, keep = _desc()
    keep[0][0] = 1
    assert lib.ce_ldpc_derive_host(C.byref(desc), C.byref(_lib.LdpcHostView())) == _lib.CE_ERR_INVALID and "row_start[0]" in _lib.last_error()
    # int8 ignores llr_scale; columns no row touches and a prefix of rows are allowed
    desc, keep = _desc(in_format=_lib.CE_LDPC_I8, llr_scale=-1.0)
    assert lib.ce_ldpc_derive_host(C.byref(desc), C.byref(_lib.LdpcHostView())) == 0
    assert rc([[(0, 1), (3, 0)]], n_cols=5, zc=2, n_in=6, k_out=8)[0] == 0
    # the host entry points refuse null arguments
    assert lib.ce_ldpc_decode(None, None, 0, None, None, None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_ldpc_plan_get_info(None, None) == _lib.CE_ERR_INVALID and lib.ce_ldpc_derive_host(None, None) == _lib.CE_ERR_INVALID
    assert lib.ce_ldpc_plan_create(None, None) == _lib.CE_ERR_INVALID


def _ch(g, llr, scale=1.0):
    return O.channel(O.quantise(llr, scale), g.n_cols, g.zc, g.n_punct)


@pytest.mark.parametrize("name", O.SMALL_CASES)
def test_decode_ref_equals_decode_loop(name):
    g = O.graph(name)
    llr = np.concatenate([O.random_inputs(name), O.codeword_inputs(name)[1] if name != "tiny_z2" else O.random_inputs(name)[:1] // 4])
    ch = _ch(g, llr)
    for max_iters, early in ((1, True), (2, False), (3, True), (8, True)):
        L, status, _ = O.decode_ref(g.rows, g.n_cols, g.zc, ch, max_iters, early)
        for b in range(ch.shape[0]):
            Lb, sb = O.decode_loop(g.rows, g.n_cols, g.zc, ch[b], max_iters, early)
            assert np.array_equal(Lb, L[b]) and np.array_equal(sb, status[b]), (name, max_iters, early, b)


@pytest.mark.parametrize("name", [c["name"] for c in O.CASES])
def test_identity_and_the_int16_bound(name):
    """L = ch + the sum of R over the variable's edges at the end of any number of iterations, so |L| <= 127 + 95 * 46."""
    g = O.graph(name)
    llr = np.concatenate([O.random_inputs(name), np.full((1, g.n_in), 127, np.int8), np.full((1, g.n_in), -128, np.int8)])
    ch = _ch(g, llr)
    for max_iters in (1, 8):
        L, _, R_ = O.decode_ref(g.rows, g.n_cols, g.zc, ch, max_iters, False)
        acc = ch.copy()
        for v, r in zip(O._vars(g.rows, g.zc), R_):
            assert np.abs(r).max() <= 95
            np.add.at(acc, (np.arange(ch.shape[0])[:, None, None], v[None]), r)
        assert np.array_equal(acc, L)
        deg = np.bincount([c for r in g.rows for c, _ in r], minlength=g.n_cols).max()
        assert np.abs(L).max() <= 127 + 95 * deg <= O.L_BOUND


@pytest.mark.parametrize("name", O.CODEWORD_CASES)
def test_encoded_words_have_zero_syndrome(name):
    g = O.graph(name)
    info, _ = O.codeword_inputs(name)
    cw = O.encode(g.rows, g.n_sys, g.zc, info)
    assert cw.shape == (3, g.n_bits) and np.array_equal(cw[:, :g.k_out], info) and not O.syndrome(g.rows, g.zc, cw).any()
    cw[0, 5] ^= 1
    assert O.syndrome(g.rows, g.zc, cw)[0].any() and not O.syndrome(g.rows, g.zc, cw)[1:].any()


def test_state_packing_round_trips():
    """The kernel's 5 bytes per check (include/ce_ldpc.h) are four disjoint bit fields: every (idx, m1, m2) with three sign
    patterns, and every sign pattern with the extreme (idx, m1, m2), unpack to the R they stand for."""
    idx, m1, m2 = (a.ravel() for a in np.meshgrid(np.arange(19), np.arange(96), np.arange(96), indexing="ij"))
    e = np.arange(19)[:, None]
    for neg in (np.zeros_like(idx), np.full_like(idx, 2 ** 19 - 1), (idx * 2654435761 + m1 * 40503 + m2) % 2 ** 19):
        w, b = O.state_pack(neg, idx, m1, m2)
        assert w.dtype == np.uint32 and b.dtype == np.uint8 and int(w.max()) < 2 ** 31
        m = np.where(e == idx[None], m2[None], m1[None])
        assert np.array_equal(O.state_unpack(w, b, 19), np.where((neg[None] >> e) & 1, -m, m))
    neg = np.arange(2 ** 19)
    for i, a, c in ((0, 0, 0), (18, 95, 95), (18, 0, 95), (0, 95, 0), (31 & 18, 64, 1)):
        w, b = O.state_pack(neg, np.full_like(neg, i), np.full_like(neg, a), np.full_like(neg, c))
        m = np.where(e == i, c, a)
        assert np.array_equal(O.state_unpack(w, b, 19), np.where((neg[None] >> e) & 1, -m, m))
    assert 19 + 5 + 7 <= 32 and O.IDX_SHIFT == 19 and O.MAG_SHIFT == 19 + 5


def test_state_packing_holds_the_reference_messages():
    """The R of decode_ref, packed as the kernel packs them (sign bits, idx, the two scaled minima), unpack to themselves."""
    g = O.graph("bg1_z15")
    _, _, R_ = O.decode_ref(g.rows, g.n_cols, g.zc, _ch(g, O.random_inputs("bg1_z15")), 3, False)
    for r in R_:
        a = np.abs(r)
        idx = np.argmax(a, axis=1)
        neg = ((r < 0) << np.arange(r.shape[1])[None, :, None]).sum(1)
        w, b = O.state_pack(neg.ravel(), idx.ravel(), a.min(1).ravel(), a.max(1).ravel())
        assert np.array_equal(O.state_unpack(w, b, r.shape[1]).reshape(r.shape[1], *idx.shape).transpose(1, 0, 2), r)


def test_quantise():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 1e9, -1e9, np.inf, -np.inf, np.nan, -0.0, 63.49], np.float32)
    assert O.quantise(x).tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127, 127, -127, 0, 0, 63]
    assert O.quantise(x[:4], 3.0).tolist() == [2, 4, 8, -2] and O.quantise(np.array([-128, -127, 127, 0], np.int8)).tolist() == [-127, -127, 127, 0]
    assert O.quantise(np.array([3e38], np.float32), 3.0).tolist() == [127]            # the product overflows to +inf


# ---- the conditions the GPU tests lean on, from the oracle alone ----

@pytest.mark.parametrize("name", O.CODEWORD_CASES)
def test_reference_decodes_every_noisy_codeword(name):
    g = O.graph(name)
    info, llr = O.codeword_inputs(name)
    L, status, hard = O.reference(name, "codeword", 8, True)
    assert np.array_equal(LD.unpack_bits(hard, g.k_out), info) and np.all(status[:, 1] == 1) and np.all(status[:, 0] <= 6), status
    assert np.any((llr < 0) != (O.encode(g.rows, g.n_sys, g.zc, info)[:, g.n_punct * g.zc:] == 1))     # the channel made errors


@pytest.mark.parametrize("name", O.MIXED_CASES)
def test_mixed_batch_stops_at_one_inside_and_never(name):
    _, status, _ = O.reference(name, "mixed", 8, True)
    its = status[:, 0]
    assert np.any(its == 1) and np.any((its > 1) & (its < 8)) and np.any((its == 8) & (status[:, 1] == 0)), status.tolist()
    assert np.any(its[1:] != its[:-1]) and len(set(its.tolist())) >= 3
    assert status[0].tolist() == [1, 1]                                        # the all-zero row
    g = O.graph(name)
    assert LD.derive_host(LD.LdpcGraph(g.rows, g.n_cols), g.zc, g.n_in, g.k_out).blocks_per_workgroup >= 7     # they share workgroups


def test_random_rows_do_not_converge():
    for name in ("bg2_z7", "bg1_z208"):
        for max_iters in (1, 2, 8):
            for early in (True, False):
                _, status, _ = O.reference(name, "random", max_iters, early)
                assert status.tolist() == [[max_iters, 0]] * 3


@pytest.mark.parametrize("which", sorted(O.CHAINS))
def test_chain_reference_decodes_to_the_bits_sent(which):
    x = O.chain_inputs(which)
    g, d = x.g, x.d
    for key, soft in x.soft.items():
        assert soft.dtype == np.int8 and soft.shape == (O.CHAIN_SLOTS, d.C, d.N_cb) and np.all(soft[:, :, d.f0:d.f1] == 127)
        L, status, hard = O.decode_ref(g.rows, g.n_cols, g.zc, _ch(g, soft.reshape(-1, d.N_cb)), 8, True)[:2] + (None,)
        assert np.all(status[:, 1] == 1), (which, key, status.tolist())
        assert np.array_equal((L[:, :d.Kp] < 0).reshape(x.bits.shape), x.bits == 1), (which, key)


# ---- the Python helpers ----

def test_lifting_set_index_and_from_table():
    for zc in range(-1, 400):
        if zc in R.ZC_SET:
            a = zc
            while a % 2 == 0 and a > 2:
                a //= 2
            assert LD.lifting_set_index(zc) == (2, 3, 5, 7, 9, 11, 13, 15).index(a)
        else:
            with pytest.raises(ValueError):
                LD.lifting_set_index(zc)
    assert len(R.ZC_SET) == 51 and [LD.lifting_set_index(z) for z in (2, 3, 5, 7, 9, 11, 13, 15, 384, 208, 36)] == [0, 1, 2, 3, 4, 5, 6, 7, 1, 6, 4]
    G = LD.LdpcGraph.from_table([(1, 0, 250), (0, 2, 9), (0, 0, 307), (1, 3, 0), (1, 1, 76)], 36)
    assert G.rows == [[(0, 307 % 36), (2, 9)], [(0, 250 % 36), (1, 76 % 36), (3, 0)]] and (G.n_cols, G.n_rows, G.n_sys, G.n_edges) == (4, 2, 2, 5)
    with pytest.raises(ValueError):
        LD.LdpcGraph.from_table([(0, 0, 1), (2, 1, 1)], 4)
    rs, col, sh = G.csr()
    assert rs.tolist() == [0, 2, 5] and col.tolist() == [0, 2, 0, 1, 3] and sh.tolist() == [19, 9, 34, 4, 0] and rs.dtype == np.int32


def test_truncated_and_for_rate_recovery():
    g, G = _graph("bg1_z15")
    T12 = G.truncated(12)
    assert T12.rows == O.graph("bg1_z15_rows12").rows and (T12.n_cols, T12.n_sys) == (34, 22)
    for n in (0, 47):
        with pytest.raises(ValueError):
            G.truncated(n)
    with pytest.raises(ValueError):
        LD.LdpcGraph([[(0, 0), (3, 0)], [(1, 0), (2, 0)]], 4).truncated(1)
    x = O.chain_inputs("bg2")
    rm = RM.PuschRateRecovery(2, 24, "qpsk", 1, 480)
    g2, G2 = _graph("bg2_z7")
    dec = LD.PuschLdpcDecoder.for_rate_recovery(rm, G2, max_iters=5)
    assert (dec.zc, dec.n_in, dec.k_out, dec.dtype, dec.max_iters, dec.row_bytes, dec.device) == (7, 350, 40, torch.int8, 5, 16, None)
    for bad in (_graph("bg1_z15")[1],                                           # n_sys = 22 under base graph 2
                LD.LdpcGraph(g2.rows + [[(0, 0), (52, 0)]], 53),                # 53 columns
                LD.LdpcGraph(g2.rows[:8] + [[(0, 0), (19, 0)], [(0, 0), (18, 0)]], 20)):     # row 8 touches row 9's column
        with pytest.raises(ValueError):
            LD.PuschLdpcDecoder.for_rate_recovery(rm, bad)
    with pytest.raises(ValueError):                                             # N_cb = 350 does not fit 12 rows' 22 columns
        LD.PuschLdpcDecoder.for_rate_recovery(rm, G2.truncated(12))
    assert x.d.Zc == dec.zc and x.d.Kp == dec.k_out


def test_python_argument_checks_that_need_no_device():
    g, G = _graph("bg2_z7")
    with pytest.raises(ValueError):
        LD.PuschLdpcDecoder(G, 7, 350, 40, dtype=torch.float16)
    with pytest.raises(ValueError):
        LD.PuschLdpcDecoder(G, 7, 351, 40)
    with pytest.raises(ValueError):
        LD.PuschLdpcDecoder(G, 7, 350, 40, dtype=torch.float32, llr_scale=0.0)
    dec = LD.PuschLdpcDecoder(G, 7, 350, 40)
    assert dec.device is None and (dec.n_sys, dec.n_bits, dec.row_bytes, dec.early_stop) == (10, 364, 16, True)
    bits = np.array([[1, 0, 0, 0, 0, 0, 0, 1, 1]], np.int64)
    assert O.pack(-bits, 9).tolist() == [[0x81, 0x80] + [0] * 14] and LD.unpack_bits(O.pack(-bits, 9), 9).tolist() == bits.tolist()
    assert LD.unpack_bits(torch.from_numpy(O.pack(-bits, 9)), 9).tolist() == bits.tolist()
