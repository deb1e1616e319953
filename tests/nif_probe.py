"""Probe networks and a float64 restatement of the NIF MLP, for tests/test_nif_exact.py and tests/test_oracle_nif.py.

A PROBE network has exactly the reference's shape (48 -> 320 -> 320 -> 320 -> (320 + 48) -> 320 -> 320 -> 3, ReLU on every layer but
the last: what K3a / K3b's generated body covers, nif_asm_covers) and weights that are 0, +-1 or powers of two with a few non-zero
terms per output, so every product and sum is exact in binary16 and binary32: the kernel's result then does not depend on the order
it accumulates in, and must equal the float64 evaluation bit for bit. Decoding is the identity (max 1, mean 0, no exp)."""
import ctypes as C

import numpy as np

EMBED = 12
F = 4 * EMBED                 # Fourier features: [sin u * 2^j | sin v * 2^j | cos u * 2^j | cos v * 2^j], j < EMBED
HIDDEN = 320
LAYERS = 6                    # hidden layers; the concat layer is hidden layer LAYERS // 2
CONCAT = LAYERS // 2
RELU = [1] * LAYERS + [0]

# Where a feature read-out may differ from the binary16 of the exact sin / cos by one ulp: where the exact value lies within this
# distance (relative) of a binary16 rounding midpoint. Both implementations under test compute sin / cos in binary32 and then round
# to binary16 - the kernel's sincos_half_phase (nif_kernels.hpp) to within 1.2e-7 relative (measured on gfx950 over every finite
# binary16 phase), the oracle's libm sinf / cosf to within one binary32 ulp (2^-23 relative) - so a binary32 result can land on the
# other side of a midpoint only when the exact value is closer than that to it. 2^-22 covers both with a factor of two to spare.
MIDPOINT_SLACK = 2.0 ** -22


def dims(hidden=HIDDEN, layers=LAYERS, embed=EMBED):
    f = 4 * embed
    d = [(f, hidden)]
    for l in range(1, layers):
        d.append((hidden + f if l == layers // 2 else hidden, hidden))
    d.append((hidden, 3))
    return d


def random_weights(rng, hidden=HIDDEN, embed=EMBED, layers=LAYERS):
    """The realistic random network of tests/test_gpu_parity.py (_nif_weights): binary16 kernels, He-scaled; binary32 biases."""
    ds = dims(hidden, layers, embed)
    ks = [(rng.normal(size=d) * np.sqrt(2.0 / d[0])).astype(np.float16).astype(np.float32) for d in ds]
    bs = [(rng.normal(size=d[1]) * 0.05).astype(np.float32) for d in ds]
    return ks, bs, [1] * (len(ds) - 1) + [0]


def zero_network():
    """All-zero kernels and biases of the probe shape (to be filled in by the caller)."""
    ds = dims()
    return [np.zeros(d, np.float32) for d in ds], [np.zeros(d[1], np.float32) for d in ds], list(RELU)


def carry(ks, first, unit_count=HIDDEN):
    """Hidden layers first .. LAYERS-1 pass units 0 .. unit_count-1 through unchanged (identity; ReLU keeps what is >= 0; the concat
    layer's 48 feature rows stay zero)."""
    for l in range(first, LAYERS):
        ks[l][np.arange(unit_count), np.arange(unit_count)] = 1.0


def feature_readout_network(group, via=0):
    """Layer `via` (0: the first layer, on the features; CONCAT: the concat layer, on its 48 appended feature rows) splits every
    feature f into h[2f] = relu(feat_f), h[2f+1] = relu(-feat_f); the later hidden layers carry them; the last layer gives
    out[c] = h[2f] - h[2f+1] = feat_f for f = 3 group + c. Sixteen groups read out the 48 features."""
    ks, bs, relu = zero_network()
    f = np.arange(F)
    row = f if via == 0 else HIDDEN + f
    ks[via][row, 2 * f] = 1.0
    ks[via][row, 2 * f + 1] = -1.0
    carry(ks, via + 1, 2 * F)
    for c in range(3):
        ks[LAYERS][2 * (3 * group + c), c] = 1.0
        ks[LAYERS][2 * (3 * group + c) + 1, c] = -1.0
    return ks, bs, relu


def half(x):
    """binary16 round-to-nearest-even with gradual underflow, back to float64 (numpy's conversion; the oracle's round_through_half is
    pinned against it in test_oracle_pins.py)."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def normalised(uv):
    """NifModel.cpp:203-205, uvNorm = 2 * (uv - 1), in binary32 as the reference computes it."""
    uv = np.asarray(uv, np.float32)
    return (uv - np.float32(1)) * np.float32(2)


def phases(uv, embed=EMBED):
    """[rows, embed] the binary16 phases 2^j * uvNorm (NifModel.cpp:208-212: the binary32 product, cast to half)."""
    n = normalised(uv).astype(np.float64)
    return half(n[:, None] * (2.0 ** np.arange(embed))[None, :])


def features64(u, v, embed=EMBED, half_features=True):
    """[rows, 4 embed] the features from float64 sin / cos (of the binary16 phases, rounded to binary16 when half_features)."""
    if half_features:
        pu, pv = phases(u, embed), phases(v, embed)
    else:
        c = (2.0 ** np.arange(embed))[None, :]
        pu, pv = (normalised(u).astype(np.float64)[:, None] * c), (normalised(v).astype(np.float64)[:, None] * c)
    f = np.concatenate([np.sin(pu), np.sin(pv), np.cos(pu), np.cos(pv)], axis=1)
    return half(f) if half_features else f


def near_half_midpoint(x):
    """True where float64 x lies within MIDPOINT_SLACK (relative) of a binary16 rounding midpoint."""
    x = np.asarray(x, np.float64)
    h = half(x)
    hb = h.astype(np.float16)
    up = np.nextafter(hb, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(hb, np.float16(-np.inf)).astype(np.float64)
    mid = np.where(x >= h, (h + up) / 2, (h + dn) / 2)
    return np.abs(x - mid) <= MIDPOINT_SLACK * np.abs(x)


def half_ulps_apart(a, b):
    """|a - b| in binary16 ulps (a, b: values that are binary16)."""
    def order(h):
        bits = np.asarray(h, np.float64).astype(np.float16).view(np.uint16).astype(np.int64)
        return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)
    return np.abs(order(a) - order(b))


def network64(ks, bs, relu, feats, round_acts=False, half_weights=False):
    """Float64 evaluation of the dense stack on given features [rows, F]: Dense(+bias)(+ReLU), the features appended to the
    activations when a layer's row count differs from the width (NifModel.cpp:300-327). round_acts: every layer's input rounded to
    binary16 (the fp16 model's activations); half_weights: the kernels rounded to binary16. Returns the raw [rows, 3] output."""
    x = np.asarray(feats, np.float64)
    for l, k in enumerate(ks):
        if x.shape[1] != k.shape[0]:
            x = np.concatenate([x, feats], axis=1)
        w = half(k) if half_weights else np.asarray(k, np.float64)
        xin = half(x) if round_acts else x
        y = xin @ w
        if bs[l] is not None:
            y = y + np.asarray(bs[l], np.float64)[None, :]
        if relu[l]:
            y = np.maximum(y, 0.0)
        x = y
    return x


def edge_coordinates():
    """Sixteen (u, v) pairs at the edges of [0, 1]: 0, 1, 0.5 and its neighbours, 1 - ulp, the smallest normal and subnormal
    binary32, -0.0, and a few more, each coordinate against a different partner."""
    e = np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), np.finfo(np.float32).tiny,
                  np.float32(2.0 ** -149), -0.0, 0.25, 0.75, 1 - 2.0 ** -11, 2.0 ** -24,
                  np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)),
                  np.float32(1 / 3), np.float32(2 / 3), 0.999], np.float32)
    return e, np.roll(e[::-1], 5)


def every_phase_coordinates():
    """Coordinates whose phases are every binary16 value in [-4096, 0] that some coordinate reaches exactly: phase t comes out of
    octave j for u = 1 + t / 2^(j+1) (exact in binary32 for the smallest j with |t| <= 2^(j+1), when that u is a binary32)."""
    t = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    t = -t[t <= 4096]
    j = np.maximum(np.ceil(np.log2(np.maximum(-t, 2.0 ** -30))) - 1, 0)
    u = 1 + t / 2.0 ** (j + 1)
    keep = (u.astype(np.float32).astype(np.float64) == u) & (j < EMBED)
    return u[keep].astype(np.float32)


def probe_rows(rng, sweep=40000, tail=37):
    """u, v for the exact probes: every reachable phase (u; a shuffled copy in v), a dense uniform sweep, and the sixteen edge pairs
    placed in the first rows, the last rows of the first 96-row and 256-row passes (nif_mlp_kernel w6 / K3a) and the ragged tail.
    Returns u, v and the row numbers of the edge pairs."""
    ph = every_phase_coordinates()
    sw = rng.random(sweep).astype(np.float32)
    u = np.concatenate([ph, sw])
    n = ((u.size + 255) // 256) * 256 + tail
    u = np.concatenate([u, rng.random(n - u.size).astype(np.float32)])
    v = rng.permutation(u)
    eu, ev = edge_coordinates()
    at = [np.arange(16), np.arange(80, 96), np.arange(240, 256), np.arange(n - 16, n)]
    for rows in at:
        u[rows], v[rows] = eu, ev
    return u, v, np.concatenate(at)


def libm_sincos():
    """libm's sinf / cosf / expf (what the oracle calls), vectorised over binary32 arrays."""
    m = C.CDLL("libm.so.6")
    for name in ("sinf", "cosf", "expf"):
        getattr(m, name).restype = C.c_float
        getattr(m, name).argtypes = [C.c_float]
    vec = lambda fn: np.vectorize(lambda x: fn(float(x)), otypes=[np.float32])
    return vec(m.sinf), vec(m.cosf), vec(m.expf)
