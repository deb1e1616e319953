"""The oracle's NIF inference (o_nif_infer, oracle/ray_oracle.c) against a plain numpy restatement of the reference's model, written
from src/neural_networks/NifModel.cpp:
  * buildEncodeInput (:186-217): uvNorm = (uv - 1) * 2; phases uvNorm * 2^j (makeCoefficients, :467-473), cast to half before sin
    and cos in the fp16 model, the results cast back; features concatenated as [sin u | sin v | cos u | cos v];
  * buildInference (:300-327): per layer, when the activations' width differs from the kernel's row count the input features are
    appended to them (the concat); matMul, + bias where the layer has one, ReLU where its activation is "relu";
  * buildDecodeOutput (:219-240): x * max + mean, then exp when the model is log-tonemapped.
CPU only. In binary32 with sequential sums (the order a plain C loop over the kernel's rows takes) the restatement gives the oracle's
bits exactly, in all four combinations of binary16 features / binary16 weights and activations; in float64 it agrees to a stated
tolerance."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import nif_probe as npb
import oracle_lib as ol

GOLDEN = Path(__file__).resolve().parent / "golden" / "nif_tiny"
SINF, COSF, EXPF = npb.libm_sincos()
f32 = np.float32


def _h32(x):
    return np.asarray(x, f32).astype(np.float16).astype(f32)


def restated32(ks, bs, relu, embed, max_value, mean, log_tonemap, half_features, half_weights_acts, u, v):
    """NifModel.cpp in binary32, one rounding per operation, the dense sums taken over the kernel's rows in order. The sin / cos are
    libm's sinf / cosf (the oracle's choice of implementation; which implementation the IPU's popops uses is not this test's)."""
    un = (np.asarray(u, f32) - f32(1)) * f32(2)                          # :203-205
    vn = (np.asarray(v, f32) - f32(1)) * f32(2)
    coeff = np.array([2.0 ** j for j in range(embed)], f32)              # :467-473
    pu, pv = un[:, None] * coeff[None, :], vn[:, None] * coeff[None, :]  # :208-209
    if half_features:                                                    # :212, cast to half before sin / cos
        pu, pv = _h32(pu), _h32(pv)
    sc = [SINF(pu), SINF(pv), COSF(pu), COSF(pv)]
    if half_features:                                                    # :213-215, the half results cast back
        sc = [_h32(a) for a in sc]
    feats = np.concatenate(sc, axis=1).astype(f32)                       # :216, [sin u | sin v | cos u | cos v]
    x = feats
    for l, k in enumerate(ks):
        if x.shape[1] != k.shape[0]:                                     # :306-309, the concat
            x = np.concatenate([x, feats], axis=1)
        w = _h32(k) if half_weights_acts else np.asarray(k, f32)
        xin = _h32(x) if half_weights_acts else x
        y = np.zeros((x.shape[0], w.shape[1]), f32)
        for r in range(w.shape[0]):
            y += xin[:, r:r + 1] * w[r][None, :]
        if bs[l] is not None:                                            # :313-318
            y = y + np.asarray(bs[l], f32)[None, :]
        if relu[l]:                                                      # :320-322
            y = np.maximum(y, f32(0))
        x = y
    o = x * f32(max_value) + np.asarray(mean, f32)[None, :]              # :229-235
    return EXPF(o) if log_tonemap else o                                 # :237-239


def restated64(ks, bs, relu, embed, max_value, mean, log_tonemap, half_features, half_weights_acts, u, v):
    """The same model in float64 (binary16 roundings kept where the model makes them, nothing else rounded)."""
    x = npb.network64(ks, bs, relu, npb.features64(u, v, embed, half_features), round_acts=half_weights_acts,
                      half_weights=half_weights_acts)
    o = x * float(np.float32(max_value)) + np.asarray(mean, np.float32).astype(np.float64)[None, :]
    return np.exp(o) if log_tonemap else o


def oracle(ks, bs, relu, embed, max_value, mean, log_tonemap, half_features, half_weights_acts, u, v):
    nif, keep = ol.make_nif(ks, bs, relu, embed, max_value, mean, log_tonemap, half_features=half_features,
                            half_weights_acts=half_weights_acts)
    out = np.zeros((u.size, 3), f32)
    ol.lib().o_nif_infer(C.byref(nif), np.ascontiguousarray(u, f32).ctypes.data, np.ascontiguousarray(v, f32).ctypes.data, u.size,
                         out.ctypes.data)
    return out


def _rows(rng, n):
    u = rng.random(n).astype(f32); v = rng.random(n).astype(f32)
    eu, ev = npb.edge_coordinates()
    u[:16], v[:16] = eu, ev
    return u, v


# hidden 64, 4 hidden layers (the concat at hidden layer 2: 64 + 48 rows against a width of 64), ReLU everywhere but on hidden
# layer 1 and the last, no bias on hidden layer 3; the reference's decode constants
def _small_model(rng):
    ks, bs, relu = npb.random_weights(rng, hidden=64, layers=4)
    relu[1] = 0
    bs[3] = None
    mean = np.array([-2.3514461517333984, -2.2660605907440186, -1.9648972749710083], f32)
    return ks, bs, relu, 12, 3.4299468994140625, mean


# Float64 tolerance: |oracle - float64| / (|float64| + 0.05) on the decoded outputs (|outputs| ~ 0.1), stated and checked against a
# run. Everything in binary32: 1e-4 (measured 2.2e-5 at most). With binary16 features or activations: 2.5e-2 (measured 1.1e-2 at
# most): a binary16 rounding that goes the other way in binary32 and in float64 moves a value by a binary16 ulp, and the later
# layers carry that on. The bits are pinned by the binary32 restatement; this bounds how far the model's roundings take it.
def _tol64(half_features, half_weights_acts):
    return 2.5e-2 if (half_features or half_weights_acts) else 1e-4


@pytest.mark.parametrize("half_weights_acts", [False, True], ids=["f32_acts", "half_acts"])
@pytest.mark.parametrize("half_features", [False, True], ids=["f32_features", "half_features"])
@pytest.mark.parametrize("log_tonemap", [True, False], ids=["exp", "linear"])
def test_o_nif_infer_against_the_restated_model(half_features, half_weights_acts, log_tonemap):
    rng = np.random.default_rng(31)
    ks, bs, relu, embed, maxv, mean = _small_model(rng)
    u, v = _rows(rng, 400)
    args = (ks, bs, relu, embed, maxv, mean, log_tonemap, half_features, half_weights_acts, u, v)
    got = oracle(*args)
    want32 = restated32(*args)
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), np.argwhere(got != want32)[:3]
    want64 = restated64(*args)
    rel = np.abs(got - want64) / (np.abs(want64) + 0.05)
    assert rel.max() < _tol64(half_features, half_weights_acts), rel.max()


def test_restatement_pieces_on_probe_inputs():
    """The pieces of the model one at a time, on one-layer networks whose outputs are the features themselves: the normalisation,
    the 2^j coefficients, the half-rounded phase, the feature order (out[c] = feature f picks sin u, sin v, cos u, cos v at octaves
    0, 5 and 11) - against closed forms, not the restatement."""
    u = np.array([0.0, 1.0, 0.5, 0.25, 0.3], f32); v = np.array([1.0, 0.75, 0.5, 0.0, 0.7], f32)
    for feats in ((0, 12 + 5, 24 + 11), (36 + 0, 11, 24 + 5)):
        k = np.zeros((48, 3), f32)
        k[list(feats), [0, 1, 2]] = 1.0
        got = oracle([k], [None], [0], 12, 1.0, [0, 0, 0], False, True, True, u, v).astype(np.float64)
        for c, f in enumerate(feats):
            coord = (u, v)[(f // 12) % 2]
            j = f % 12
            phase = npb.half(((coord.astype(np.float64) - 1) * 2) * 2.0 ** j)
            want = npb.half((np.sin, np.cos)[f // 24](phase))
            assert np.array_equal(got[:, c], want), (f, got[:, c], want)
    # decode: x * max + mean, then exp (a bias-only network: x = bias)
    k = np.zeros((48, 3), f32)
    got = oracle([k], [np.array([0.5, -1.0, 0.0], f32)], [0], 12, 2.0, [0.25, 0.5, -1.0], True, True, True, u[:1], v[:1])
    assert np.allclose(got[0], np.exp([0.5 * 2 + 0.25, -1.0 * 2 + 0.5, -1.0]), rtol=1e-6)


@pytest.mark.skipif(not (irl.PKG_DIR / "libmi_nif_h5.so").exists(), reason="HDF5 plugin not built (no libhdf5 on this machine)")
@pytest.mark.parametrize("half_weights_acts", [False, True], ids=["f32_acts", "half_acts"])
@pytest.mark.parametrize("half_features", [False, True], ids=["f32_features", "half_features"])
def test_o_nif_infer_on_the_asset_fixture(half_features, half_weights_acts):
    """The committed Keras-H5 fixture (tests/golden/nif_tiny: widths 32 / 48 / 3, a bias-free layer) with its own decode constants."""
    a = irl.NifAssets(GOLDEN)
    u, v = _rows(np.random.default_rng(3), 300)
    args = (a.kernels, a.biases, a.relu, a.embedding_dimension, a.max_value, a.mean, a.log_tonemap, half_features, half_weights_acts, u, v)
    got = oracle(*args)
    want32 = restated32(*args)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), np.argwhere(got != want32)[:3]
    want64 = restated64(*args)
    rel = np.abs(got - want64) / (np.abs(want64) + 0.05)
    assert rel.max() < _tol64(half_features, half_weights_acts), rel.max()
