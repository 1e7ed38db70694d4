"""Conv2d denoiser EXTENSION (include/ce_denoise.h) -- "parity unpinned": nothing in the reference corresponds to it,
so the HIP kernel is checked against the build's own numpy restatement (oracle/ce_denoise_oracle.py) only.
Tolerance: both sides round activations to fp16 at the same points; what differs is the accumulation order (and, rarely,
an fp16 rounding boundary), so the correction agrees to ~1e-3 of its own size; stated here as 2e-3 of max|h|."""

import numpy as np
import pytest

import ce_denoise_oracle as DO
from srsran_ce_pytorch_amd import _lib
from srsran_ce_pytorch_amd.denoiser import SHAPES, random_weights


def test_library_exports_the_denoiser_symbols():
    _lib.build()
    lib = _lib.load()
    # the header against the binding: tests/test_abi_conformance.py; here the list the entry point's build() looks for
    assert _lib.EXPORTS_DENOISE and _lib.EXPORTS_DENOISE == list(_lib.REGISTRY["ce_denoise.h"].signatures)
    for sym in _lib.EXPORTS_DENOISE:
        assert hasattr(lib, sym)


def test_oracle_identity_and_locality():
    w = random_weights(1)
    zero = {k: np.zeros_like(v) for k, v in w.items()}
    rng = np.random.default_rng(0)
    h = (rng.standard_normal((40, 14)) + 1j * rng.standard_normal((40, 14))).astype(np.complex64)
    assert np.array_equal(DO.denoise_plane(h, **zero), h)                      # zero weights: pure residual
    base = DO.denoise_plane(h, **w)
    h2 = h.copy()
    h2[20, 7] += 1.0
    changed = np.argwhere(DO.denoise_plane(h2, **w) != base)
    assert np.abs(changed - [20, 7]).max() <= 3                                 # receptive field of three 3x3 layers
    assert set(SHAPES) == set(w)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sc,n_layers,n_items", [(72, 1, 3), (32, 1, 1), (1, 1, 2), (33, 2, 2), (300, 1, 2), (100, 4, 1), (3276, 1, 1)])
def test_hip_denoiser_matches_its_oracle(n_sc, n_layers, n_items):
    import torch
    from srsran_ce_pytorch_amd.denoiser import Denoiser
    w = random_weights(7, gain=0.7)
    rng = np.random.default_rng(n_sc)
    h = (rng.standard_normal((n_items, n_sc, 14, n_layers)) + 1j * rng.standard_normal((n_items, n_sc, 14, n_layers))).astype(np.complex64)
    h *= np.float32(0.8)
    want = DO.denoise(h, w)
    dn = Denoiser(w, "cuda:0")
    t = torch.from_numpy(h.copy()).cuda()
    assert dn(t) is t
    got = t.cpu().numpy()
    corr = np.abs(want - h).max()
    assert corr > 0.05                                                          # the network really does something
    assert np.abs(got - want).max() <= 2e-3 * np.abs(h).max(), (np.abs(got - want).max(), corr)


@pytest.mark.gpu
def test_hip_denoiser_zero_weights_and_errors():
    import torch
    from srsran_ce_pytorch_amd.denoiser import Denoiser
    w = {k: np.zeros(s, np.float32) for k, s in SHAPES.items()}
    t = torch.randn(2, 50, 14, 1, dtype=torch.complex64, device="cuda:0")
    ref = t.clone()
    assert torch.equal(Denoiser(w)(t), ref)                                     # exact identity
    with pytest.raises(NotImplementedError):
        Denoiser(w)(torch.zeros(1, 50, 12, 1, dtype=torch.complex64, device="cuda:0"))
    with pytest.raises(ValueError):
        Denoiser(w)(torch.zeros(1, 50, 14, 1, dtype=torch.complex128, device="cuda:0"))
    with pytest.raises(ValueError):
        Denoiser(dict(w, w2=np.zeros((16, 8, 3, 3), np.float32)))
    Denoiser(w)(torch.zeros(0, 50, 14, 1, dtype=torch.complex64, device="cuda:0"))    # empty batch: no launch


@pytest.mark.gpu
def test_denoiser_through_estimate_config_attribute():
    """`config.Denoiser` (optional attribute, read like the reference reads CNNSmoothingAlpha): estimate() = estimation
    followed by the in-place denoiser; the shim inherits it."""
    import torch
    from srsran_ce_pytorch_amd import estimator as E, synth as S
    from srsran_ce_pytorch_amd.denoiser import Denoiser
    case = S.case_spec("dn", 25, [S.hop_spec([2, 11], 2, 20)], seed=11)
    b = S.build_case(case, 2)
    g = torch.as_tensor(b.grids, device="cuda:0")[None]
    p = torch.as_tensor(b.pilots, device="cuda:0")
    plain = E.estimate(g, p, b.beta, b.hop1, b.hop2, b.config)
    w = random_weights(2)
    b.config.Denoiser = Denoiser(w)
    den = E.estimate(g, p, b.beta, b.hop1, b.hop2, b.config)
    want = DO.denoise(plain[0].cpu().numpy(), w)
    assert np.abs(den[0].cpu().numpy() - want).max() <= 2e-3 * np.abs(want).max()
    for a, c in zip(plain[1:], den[1:]):
        assert torch.equal(a, c)                                                # scalars untouched
    one = E.srs_channel_estimator(g[0, 1], p, b.beta, b.hop1, b.hop2, b.config)
    assert torch.allclose(one[0], den[0][0, 1], atol=1e-6)


# ---- isolation and locality: what a plane holds outside an output's 3 x 3 x 3 receptive field cannot change it --------
# The kernel multiplies activations by weights that are zero by design (layer 1's K padding, the upper half of layer 2's
# last C fragment, layer 3's banded K-steps over 6 input rows for 4 output rows); 0 x Inf = NaN would carry one overflowing
# activation past the receptive field, so the activations saturate at the fp16 maximum (include/ce_denoise.h).
RF_N_SC = 100
RF_SC = (0, 1, 2, 3, *range(28, 36), 63, 64, RF_N_SC - 1)      # 28..35: the 32-row strip boundary (DN_T, csrc/ce_denoise.hip)
RF_SYM = (0, 6, 13)
RF_VALUES = {"nan": complex(np.nan, np.nan), "+inf": complex(np.inf, np.inf), "-inf": complex(-np.inf, -np.inf),
             "3e4": complex(3e4, 3e4), "1e5": complex(1e5, 1e5)}
HOT_W1_SCALE = 5.0     # layer-1 weights x5: a 3e4 RE drives layer-1 activations past 65504, a clean plane's stay below 32


def _rf_weights(name):
    w = random_weights(7, gain=0.7)
    if name == "hot":
        w["w1"] = w["w1"] * np.float32(HOT_W1_SCALE)
    return w


def _rf_plane():
    rng = np.random.default_rng(99)
    return (0.8 * (rng.standard_normal((RF_N_SC, 14)) + 1j * rng.standard_normal((RF_N_SC, 14)))).astype(np.complex64)


def _pre_activations(h, w):
    """The oracle's layer-1 and layer-2 inputs to ReLU (before fp16 rounding and saturation)."""
    x0 = DO._h(np.stack([h.real, h.imag]))
    a1 = DO.conv3x3(x0, DO._h(w["w1"]), w["b1"])
    a2 = DO.conv3x3(DO._h(np.clip(a1, 0.0, DO.FP16_MAX)), DO._h(w["w2"]), w["b2"])
    return a1, a2


def test_hot_weights_overflow_fp16_only_at_a_large_re():
    """The "hot" weight set does what the receptive-field test needs: every 3e4 RE it places drives a layer-1 activation
    past fp16 (65520 and up round to Inf), while a clean plane's activations stay far inside."""
    hot, plain = _rf_weights("hot"), _rf_weights("gain07")
    h = _rf_plane()
    for a in _pre_activations(h, hot):
        assert a.max() < 32.0
    for sc in RF_SC:
        for sym in RF_SYM:
            hp = h.copy()
            hp[sc, sym] = RF_VALUES["3e4"]
            a1, _ = _pre_activations(hp, hot)
            assert a1.max() >= 65520.0, (sc, sym, a1.max())
            assert max(a.max() for a in _pre_activations(hp, plain)) < 65504.0, (sc, sym)   # the plain set would not overflow


def test_oracle_saturates_activations():
    w = _rf_weights("hot")
    h = _rf_plane()
    h[50, 6] = RF_VALUES["3e4"]
    assert np.isfinite(DO.denoise_plane(h, **w)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", [1, 2, 4])
@pytest.mark.parametrize("n_sc", [1, 31, 32, 33, 64, 65, 3276])
def test_hip_denoiser_planes_are_isolated(n_sc, n_layers):
    """A plane of NaN and a plane of +Inf change no bit of any other (item, layer) plane."""
    import torch
    from srsran_ce_pytorch_amd.denoiser import Denoiser
    dn = Denoiser(random_weights(7, gain=0.7), "cuda:0")
    rng = np.random.default_rng(n_sc * 10 + n_layers)
    n_items = 4
    h = (0.8 * (rng.standard_normal((n_items, n_sc, 14, n_layers)) + 1j * rng.standard_normal((n_items, n_sc, 14, n_layers)))).astype(np.complex64)
    nan_plane, inf_plane = (1, 0), (2, n_layers - 1)
    hp = h.copy()
    hp[nan_plane[0], :, :, nan_plane[1]] = complex(np.nan, np.nan)
    hp[inf_plane[0], :, :, inf_plane[1]] = complex(np.inf, np.inf)
    outs = []
    for x in (h, hp):
        t = torch.from_numpy(x.copy()).cuda()
        dn(t)
        outs.append(t.cpu().numpy().view(np.int32).reshape(n_items, n_sc, 14, n_layers, 2))
    for i in range(n_items):
        for l in range(n_layers):
            if (i, l) not in (nan_plane, inf_plane):
                assert np.array_equal(outs[0][i, :, :, l], outs[1][i, :, :, l]), f"plane ({i}, {l}) changed"


@pytest.mark.gpu
@pytest.mark.parametrize("value", list(RF_VALUES), ids=list(RF_VALUES))
@pytest.mark.parametrize("weights", ["gain07", "hot"])
def test_hip_denoiser_receptive_field(weights, value):
    """One RE holds NaN, +-Inf, 3e4 or 1e5 (Inf once rounded to fp16): every output more than 3 subcarriers or 3 symbols
    away keeps the bits of the clean run.  One item per poisoned position (rows at both grid edges and around the strip
    boundaries, symbols at both slot edges and in the middle)."""
    import torch
    from srsran_ce_pytorch_amd.denoiser import Denoiser
    dn = Denoiser(_rf_weights(weights), "cuda:0")
    h = _rf_plane()
    pos = [(sc, sym) for sc in RF_SC for sym in RF_SYM]
    hp = np.repeat(h[None, :, :, None], len(pos) + 1, axis=0)                 # item 0: the clean plane
    for i, (sc, sym) in enumerate(pos, start=1):
        hp[i, sc, sym, 0] = RF_VALUES[value]
    t = torch.from_numpy(hp).cuda()
    dn(t)
    got = t.cpu().numpy()[..., 0].view(np.int32).reshape(len(pos) + 1, RF_N_SC, 14, 2)
    ysc, ysym = np.meshgrid(np.arange(RF_N_SC), np.arange(14), indexing="ij")
    for i, (sc, sym) in enumerate(pos, start=1):
        far = (np.abs(ysc - sc) > 3) | (np.abs(ysym - sym) > 3)
        bad = np.argwhere(far & (got[i] != got[0]).any(axis=-1))
        assert not len(bad), f"{weights}: {value} at ({sc}, {sym}) changed {len(bad)} outputs outside the receptive field, e.g. {bad[:4].tolist()}"
