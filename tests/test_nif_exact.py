"""The NIF MLP kernels pinned exactly (pytest -m gpu): probe networks whose every product and sum is exact in binary16 and binary32
(tests/nif_probe.py), so each kernel's output must equal a float64 evaluation of the same network BIT FOR BIT; and the realistic
random network against float64, with the oracle's own error as the yardstick.

Every MLP kernel runs: a8 / b4 (K3a / K3b, nif_asm_kernel.hpp - checked to have run through mi_get_nif_clock, which only K3a / K3b
fill), w6 / t4 / t6 (nif_mlp_kernel) and r8 / r8s (K3r, the variants build). The probe networks keep K3a's exact shape and ReLU
pattern and vary only the weights."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import nif_probe as npb
import oracle_lib as ol

pytestmark = pytest.mark.gpu

KERNELS = ["a8", "b4", "w6", "t4", "t6", "r8", "r8s"]
K3A = ("a8", "b4")


class Mlp:
    """One scene whose NIF is replaced network by network; infer(u, v) -> [rows, 3] binary32, decoded as the identity."""

    def __init__(self, kernel):
        import torch
        self.torch = torch
        self.kernel = kernel
        self.scene = irl.HostScene.builtin("spheres")          # (owns what the desc points at)
        self.dev = irl.IpuScene(self.scene.desc, variants=kernel.startswith("r")).set_option("nif_shape", kernel)

    def set(self, ks, bs, relu):
        self.dev.setNif(ks, bs, relu, npb.EMBED, 1.0, np.zeros(3, np.float32), False)
        return self

    def infer(self, u, v):
        torch = self.torch
        n = u.size
        du, dv = torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda()
        out = torch.full((n, 3), float("nan"), device="cuda")
        self.dev.nif_infer_device(du.data_ptr(), dv.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if self.kernel in K3A:
            assert self.dev.nif_clock_ghz() is not None, f"{self.kernel}: the launch did not run K3a / K3b"
        return out.cpu().numpy()

    def close(self):
        self.dev.close()


@pytest.fixture(scope="module")
def rows():
    return npb.probe_rows(np.random.default_rng(2026))


def _bits_equal(got, want):
    return got.astype(np.float32).view(np.uint32) == np.asarray(want, np.float64).astype(np.float32).view(np.uint32)


def _oracle_features(u, v):
    """The oracle's features (o_nif_infer: libm sinf / cosf of the binary16 phases, rounded to binary16), read out through one-layer
    networks (out[c] = feature 3 g + c)."""
    out = np.zeros((u.size, npb.F), np.float32)
    for g in range(npb.F // 3):
        k = np.zeros((npb.F, 3), np.float32)
        k[3 * g + np.arange(3), np.arange(3)] = 1.0
        nif, keep = ol.make_nif([k], [None], [0], npb.EMBED, 1.0, [0, 0, 0], False, half_features=True, half_weights_acts=True)
        o = np.zeros((u.size, 3), np.float32)
        ol.lib().o_nif_infer(C.byref(nif), u.ctypes.data, v.ctypes.data, u.size, o.ctypes.data)
        out[:, 3 * g:3 * g + 3] = o
    return out


# ------------------------------------------------------------------------------------------------------
# A. exact probe networks
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", [0, npb.CONCAT], ids=["first_layer", "concat_layer"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_features_read_out_exactly(rows, kernel, via):
    """All 48 Fourier features of every row, read out through the first layer or through the concat layer's 48 appended rows (which
    also pins the offset the concat layer takes the features at): u, v reach every binary16 phase in [-4096, 0] that a binary32
    coordinate can give (26 625 phases; v a shuffled copy), a 40 000-row uniform sweep, and the edge pairs of
    nif_probe.edge_coordinates in the first rows, the last rows of the first 96- and 256-row passes and the ragged tail.

    Per row, no quantiles: the kernel's feature is RNE_half(sin / cos(phase)) of the float64 value, except that it may be one ulp
    away where that value lies within nif_probe.MIDPOINT_SLACK = 2^-22 (relative) of a binary16 midpoint. The slack is derived from
    the measured error of sincos_half_phase: 1.2e-7 relative at most over every finite binary16 phase on gfx950 (measured; the
    hardware v_sin / v_cos the kernels used before were 3.6e-7 ABSOLUTE, and put 19 of the 55 300 (phase, sin | cos) features of
    the phases in [-4096, 0] on another binary16 value, up to 4 ulps from the exact one - the bug this test was written for). The
    oracle's libm features obey the same rule, and the kernel's equal them bit for bit (measured: both are off the exact binary16
    value at the same few double-rounding midpoints only)."""
    u, v, _ = rows
    m = Mlp(kernel)
    got = np.zeros((u.size, npb.F), np.float32)
    for g in range(npb.F // 3):
        got[:, 3 * g:3 * g + 3] = m.set(*npb.feature_readout_network(g, via)).infer(u, v)
    m.close()
    pu, pv = npb.phases(u), npb.phases(v)
    raw = np.concatenate([np.sin(pu), np.sin(pv), np.cos(pu), np.cos(pv)], axis=1)
    want = npb.half(raw)
    assert np.isfinite(got).all()
    orc = _oracle_features(u, v)
    for name, feat in (("kernel", got), ("oracle", orc)):
        off = feat.astype(np.float64) != want
        bad = off & ~((npb.half_ulps_apart(feat, want) == 1) & npb.near_half_midpoint(raw))
        if bad.any():
            r, f = np.argwhere(bad)[0]
            raise AssertionError(f"{kernel}: {bad.sum()} {name} features differ from the float64 one beyond the midpoint rule; first row "
                                 f"{r} feature {f}: u {u[r]!r} v {v[r]!r} got {feat[r, f]!r} want {want[r, f]!r} (exact {raw[r, f]!r})")
        print(f"[{kernel}] {name}: {off.sum()} of {off.size} features one ulp off, all within the midpoint slack")
    assert np.array_equal(got.view(np.uint32), orc.view(np.uint32)), "kernel features differ from the oracle's"


def _checksum_network(layer):
    """Layer `layer` (0 .. LAYERS - 1) has bias c + 1 on column c and no other input; the later hidden layers carry the 320 columns;
    the last layer sums them with weights c + 1, (37 c mod 320) + 1 and (c < 160): sums of integers < 2^24, exact. A bias that is
    dropped, lands in another column or is added twice changes the sums."""
    ks, bs, relu = npb.zero_network()
    c = np.arange(npb.HIDDEN)
    bs[layer][:] = c + 1
    npb.carry(ks, layer + 1)
    ks[npb.LAYERS][c, 0] = c + 1
    ks[npb.LAYERS][c, 1] = (37 * c) % npb.HIDDEN + 1
    ks[npb.LAYERS][c, 2] = c < 160
    return ks, bs, relu


@pytest.mark.parametrize("kernel", KERNELS)
def test_biases_land_in_their_columns(rows, kernel):
    """Every bias of every layer in its own column: the checksum networks above for each hidden layer, and the last layer's three
    biases alone (2^-3, 3, -5: the final layer has no ReLU). Bit for bit against float64 on every row."""
    u, v, _ = rows
    u, v = u[:1000 + 13], v[:1000 + 13]
    m = Mlp(kernel)
    feats = npb.features64(u, v)
    nets = [_checksum_network(l) for l in range(npb.LAYERS)]
    last = npb.zero_network()
    last[1][npb.LAYERS][:] = [0.125, 3.0, -5.0]
    nets.append(last)
    for i, (ks, bs, relu) in enumerate(nets):
        got = m.set(ks, bs, relu).infer(u, v)
        want = npb.network64(ks, bs, relu, feats)
        ok = _bits_equal(got, want)
        assert ok.all(), (kernel, i, got[~ok.all(1)][:2], want[~ok.all(1)][:2])
    m.close()


# (layer, fp32 pre-activation, scale of the read-out) -> the binary16 activation RNE with gradual underflow gives, times the scale
ROUNDING_TARGETS = [
    (1 + 2.0 ** -11, 1.0),          # midpoint between 1 and 1 + 2^-10: to even, 1
    (1 + 3 * 2.0 ** -11, 1.0),      # midpoint between 1 + 2^-10 and 1 + 2^-9: to even, 1 + 2^-9
    (1 + 2.0 ** -11 + 2.0 ** -20, 1.0),   # just above the midpoint: up
    (2.0 ** -20, 1024.0),           # binary16 subnormal, scaled back up by a 2^10 weight in the next layer
    (3 * 2.0 ** -25, 1024.0),       # subnormal midpoint (1.5 x 2^-24): to even, 2^-23
    (2.0 ** -25, 1024.0),           # half the smallest subnormal: to even, 0
    (1.5 * 2.0 ** -25, 1024.0),     # above that: the smallest subnormal
    (65503.0, 1.0),                 # just below 65504: 65504
    (65487.0, 1.0),                 # just below the midpoint 65488 between 65472 and 65504: 65472
    (-3.0, 1.0),                    # negative: ReLU clamps to 0
    (-(2.0 ** -20), 1.0),           # negative subnormal: 0
    (2049.0, 1.0),                  # midpoint between 2048 and 2050: to even, 2048
]


def _rounding_network(layer, targets):
    """Hidden layer `layer` makes units 0 .. k-1 equal to the targets' pre-activations (bias only, exact in binary32); the next layer
    multiplies each by its scale (or the last layer does, when `layer` is the last hidden one), the rest carry; out[c] = unit c."""
    ks, bs, relu = npb.zero_network()
    k = len(targets)
    bs[layer][:k] = [t for t, _ in targets]
    idx = np.arange(k)
    scale = np.array([s for _, s in targets])
    for l in range(layer + 1, npb.LAYERS + 1):
        ks[l][idx, idx] = scale if l == layer + 1 else 1.0
    return ks, bs, relu


@pytest.mark.parametrize("kernel", KERNELS)
def test_binary16_rounding_edges(rows, kernel):
    """Hidden units whose exact binary32 pre-activation is a binary16 rounding midpoint, a subnormal (or the midpoint of two), a value
    just below 65504 or a negative one, in every hidden layer in turn, read out exactly. Expected: float64 with RNE and gradual
    underflow (what the oracle's round_through_half does); a flush-to-zero or truncating activation store fails here."""
    u, v, _ = rows
    u, v = u[:512 + 5], v[:512 + 5]
    m = Mlp(kernel)
    feats = npb.features64(u, v)
    for layer in range(npb.LAYERS):
        for g in range(0, len(ROUNDING_TARGETS), 3):
            tg = ROUNDING_TARGETS[g:g + 3]
            ks, bs, relu = _rounding_network(layer, tg)
            got = m.set(ks, bs, relu).infer(u, v)
            want = npb.network64(ks, bs, relu, feats, round_acts=True)
            assert (want == want[:1]).all()
            ok = _bits_equal(got, want)
            assert ok.all(), (kernel, layer, tg, got[~ok.all(1)][:1], want[:1])
    m.close()
    # the expectations themselves, spelled out
    assert npb.half([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 3 * 2.0 ** -25, 2.0 ** -25, 65503.0, 65487.0, 2049.0]).tolist() == \
        [1.0, 1 + 2.0 ** -9, 2.0 ** -23, 0.0, 65504.0, 65472.0, 2048.0]


@pytest.mark.parametrize("kernel", ["w6", "t4", "t6", "r8", "r8s"])
def test_linear_and_bias_free_hidden_layers(rows, kernel):
    """A hidden layer declared linear passes a negative value on, one declared without bias adds none (networks outside K3a's
    pattern, so nif_mlp_kernel and K3r only): the first layer's bias gives -3 and 5; layer 1 (linear, declared without bias) and
    layer 2 (linear) carry them; layer 3 splits them into relu(x), relu(-x); the last layer gives x. A ReLU applied where none is
    declared loses the -3."""
    u, v, _ = rows
    u, v = u[:300], v[:300]
    ks, bs, relu = npb.zero_network()
    bs[0][:2] = [-3.0, 5.0]
    relu[0] = 0
    bs[1] = None
    relu[1] = relu[2] = 0
    for l in (1, 2):
        ks[l][[0, 1], [0, 1]] = 1.0
    ks[3][[0, 1, 0, 1], [0, 1, 2, 3]] = [1.0, 1.0, -1.0, -1.0]
    npb.carry(ks, 4, 4)
    ks[npb.LAYERS][[0, 2, 1, 3], [0, 0, 1, 1]] = [1.0, -1.0, 1.0, -1.0]
    m = Mlp(kernel).set(ks, bs, relu)
    got = m.infer(u, v)
    m.close()
    assert (got == np.array([-3.0, 5.0, 0.0], np.float32)).all(), got[:2]


@pytest.mark.parametrize("shape", ["w6", "a8", "b4", "r8"])
def test_probe_render_skips_the_lists_holes_bit_exact(shape):
    """test_nif_render_with_every_mlp_kernel_skips_the_lists_holes (tests/test_gpu_parity.py) with a feature read-out network instead
    of random weights: the environment is exact, so the render's rgb must be the oracle's BIT FOR BIT - a row of the escaped list
    that is a hole (kNifHole) and got a result, or an escaped ray that got none or another's, shows.
    Hit records bit for bit everywhere; rgb bit for bit on all but at most 4 of the 12 288 rows, and those within 5 % (+ 0.05 absolute).
    Measured: 2 rows differ, by up to 2 % (0.0078 on 0.39 in the sin(16 v) channel, about one binary16 step of that phase). They are
    the same two with every kernel, so their difference enters before the MLP (whose features are pinned exactly above).
    It was not investigated further. The likely source is the escaped-ray coordinates: the device's acosf / atan2f against libm's."""
    ks, bs, relu = npb.zero_network()
    f = np.arange(npb.F)
    ks[0][f, 2 * f] = 1.0; ks[0][f, 2 * f + 1] = -1.0
    npb.carry(ks, 1, 2 * npb.F)
    for c, feat in enumerate((1, npb.EMBED + 4, 3 * npb.EMBED + 2)):      # sin u*2, sin v*16, cos v*4: more than a small bias
        ks[npb.LAYERS][2 * feat, c] = 1.0; ks[npb.LAYERS][2 * feat + 1, c] = -1.0
    s = irl.HostScene.builtin("monkey")
    d = s.desc
    d.set_image(128, 96); d.samples_per_pixel = 4
    dev = irl.IpuScene(d, variants=shape.startswith("r")).set_option("nif_shape", shape)
    dev.setNif(ks, bs, relu, npb.EMBED, 1.0, np.zeros(3, np.float32), False)
    got = s.init_ray_stream(); want = got.copy()
    dev.run(got, irl.MODE_PATH_TRACE)
    if shape in K3A:
        assert dev.nif_clock_ghz() is not None
    dev.close()
    nif, keep = ol.make_nif(ks, bs, relu, npb.EMBED, 1.0, [0, 0, 0], False, half_features=True, half_weights_acts=True)
    st = ol.Stats()
    ol.lib().o_path_trace_nif_pixel_rng(C.byref(d), C.byref(nif), 0.0, want.ctypes.data, want.size, 16, C.byref(st))
    assert (got["h"]["flags"] & irl.FLAG_ESCAPED).any()
    gh = np.ascontiguousarray(got["h"]).view(np.uint8).reshape(got.size, -1)
    wh = np.ascontiguousarray(want["h"]).view(np.uint8).reshape(want.size, -1)
    assert not (gh != wh).any(), shape
    g = np.stack([got["rgb"][k] for k in "xyz"], 1); w = np.stack([want["rgb"][k] for k in "xyz"], 1)
    bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).any(1))[0]
    print(f"[{shape}] rgb rows not bit exact: {bad.tolist()}")
    assert bad.size <= 4, (shape, bad.size)
    assert (np.abs(g[bad] - w[bad]) <= 0.05 * (np.abs(w[bad]) + 0.05)).all(), (g[bad], w[bad])


# ------------------------------------------------------------------------------------------------------
# B. the random network against float64
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_case():
    """The realistic random 6 x 320 network on 100 000 + 37 rows (the edge pairs placed as in part A), its float64 value (binary16
    features and weights, no activation rounding) and the oracle's (half_weights_acts), raw outputs (no decode)."""
    rng = np.random.default_rng(77)
    ks, bs, relu = npb.random_weights(rng)
    n = 100000 + 37
    u = rng.random(n).astype(np.float32); v = rng.random(n).astype(np.float32)
    eu, ev = npb.edge_coordinates()
    edges = np.concatenate([np.arange(16), np.arange(80, 96), np.arange(240, 256), np.arange(n - 16, n)])
    for k in range(4):
        u[edges[16 * k:16 * k + 16]], v[edges[16 * k:16 * k + 16]] = eu, ev
    f64 = npb.network64(ks, bs, relu, npb.features64(u, v), half_weights=True)
    nif, keep = ol.make_nif(ks, bs, relu, npb.EMBED, 1.0, [0, 0, 0], False, half_features=True, half_weights_acts=True)
    orc = np.zeros((n, 3), np.float32)
    ol.lib().o_nif_infer(C.byref(nif), u.ctypes.data, v.ctypes.data, n, orc.ctypes.data)
    return ks, bs, relu, u, v, edges, f64, orc.astype(np.float64)


@pytest.mark.parametrize("kernel", KERNELS)
def test_random_network_against_float64(random_case, kernel):
    """The kernel, the oracle (binary16 activations, sequential binary32 sums) and float64 (no activation rounding) on the same
    random network; errors are taken against float64 before any decode.
      * no systematic bias: per output channel the kernel's mean signed error is within 4 standard errors (of the per-row
        difference kernel - oracle) of the oracle's own - a round-toward-zero activation store shifts it by many;
        (measured, one run: |kernel - oracle| of the means at most 1.4e-6 against standard errors of 6e-7 - every kernel, every channel
        within 2.3 standard errors);
      * no extra error: the kernel's 50 %, 99 % and 100 % quantiles of |error| are at most 1.25 x the oracle's + 1e-5. The margins
        were MEASURED on one run, not derived: the largest kernel / oracle ratio was 1.0026 (the 100 % quantile; a8, b4, r8, r8s)
        and 1.0018 (w6, t4, t6), with the oracle's quantiles about 3.6e-4, 1.4e-3 and 2.6e-3;
      * the 64 edge rows one by one, not inside a quantile: |kernel - oracle| on each is at most 2 x the oracle's median |error| in
        that channel (measured: 3.2e-4 at most, against medians of 3.5e-4 - 3.7e-4)."""
    ks, bs, relu, u, v, edges, f64, orc = random_case
    m = Mlp(kernel).set(ks, bs, relu)
    got = m.infer(u, v).astype(np.float64)
    m.close()
    assert np.isfinite(got).all()
    ek, eo = got - f64, orc - f64
    d = ek - eo
    se = d.std(axis=0) / np.sqrt(d.shape[0])
    print(f"[{kernel}] mean signed error kernel {ek.mean(0)} oracle {eo.mean(0)} se {se}")
    assert (np.abs(ek.mean(0) - eo.mean(0)) <= 4 * se + 1e-12).all(), (ek.mean(0), eo.mean(0), se)
    qs = (0.5, 0.99, 1.0)
    qk = np.quantile(np.abs(ek), qs, axis=0); qo = np.quantile(np.abs(eo), qs, axis=0)
    print(f"[{kernel}] |error| quantiles 50/99/100 %: kernel {qk.tolist()} oracle {qo.tolist()} ratio {(qk / qo).tolist()}")
    assert (qk <= 1.25 * qo + 1e-5).all(), (qk, qo)
    dko = np.abs(got - orc)[edges]
    print(f"[{kernel}] edge rows: max |kernel - oracle| {dko.max(0)}, oracle median |error| {qo[0]}")
    assert (dko <= 2 * qo[0][None, :]).all(), (dko.max(0), qo[0])
