"""K1w's SHADE / GEN turn on its cheaper forms (pytest -m gpu): the shift-add output scrambler of rng_next (device only: inline
assembly), the two bounded-range sincos and the dielectric bounce on per-material constants staged in LDS (csrc/ray_math.h,
csrc/trace_wavefront.hpp). Every frame must be the oracle's, all 84 bytes of every
pixel: a wrong scrambler shows in every pixel of every case; the material cases put mirrors and dielectrics of ordinary and of
degenerate index (1, 0.5, 1e30) on both material paths - the staged one (up to 16 materials) and the global one (17)."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import nif_probe as npb
import oracle_lib as ol
import set_geometry_cases as sg
from test_gpu_parity import assert_streams_identical

pytestmark = pytest.mark.gpu


def _params(d, w, h, spp):
    d.set_image(w, h); d.samples_per_pixel = spp; d.path_trace = 1
    d.max_path_length, d.roulette_start_depth, d.rng_seed, d.device = 10, 3, 1442, 0
    return d


def _with_materials(hs, mats, mat_ids):
    """hs's geometry under other materials (the host builder sees the same primitives: the same tree)."""
    c = sg.Contents(hs.desc)
    g = irl.SceneDesc.from_buffer_copy(c.desc)
    mats, mat_ids = np.ascontiguousarray(mats, irl.MATERIAL), np.ascontiguousarray(mat_ids, np.uint32)
    assert mat_ids.size == g.num_mat_ids and int(mat_ids.max()) < mats.size
    g.materials, g.num_materials = mats.ctypes.data, mats.size
    g.mat_ids = mat_ids.ctypes.data
    g.fov_radians, g.anti_alias_scale = hs.desc.fov_radians, hs.desc.anti_alias_scale
    out = irl.HostScene.from_arrays(g)
    out._keep = [c, mats, mat_ids]
    assert out.desc.num_nodes == hs.desc.num_nodes
    return out


def seventeen_materials():
    """The spheres scene with its materials repeated up to 17, the repeats with other indices of refraction, and every second
    geometry on a repeat of its material: more materials than K1w stages, so every hit is shaded from the global array."""
    hs = irl.HostScene.builtin("spheres")
    c = sg.Contents(hs.desc)
    m0, ids0 = c.a["materials"], c.a["mat_ids"]
    n0 = m0.size
    assert 2 <= n0 <= 8 and (m0["type"] == 2).any() and (m0["type"] == 1).any()
    mats = np.resize(m0, 17)
    for k in range(n0, 17):
        mats[k]["ior"] = (1.33, 2.4, 1.1)[k % 3]
    ids = ids0 + n0 * np.minimum(np.arange(ids0.size, dtype=np.uint32) % 3, (16 - ids0) // n0)      # (material k is a repeat of k % n0)
    assert ids.max() >= n0 and (mats[ids]["type"] == m0[ids0]["type"]).all()
    return _with_materials(hs, mats, ids)


def odd_dielectrics():
    """The spheres scene with three of its spheres - the first diffuse one, the free glass one and the glass shell; the mirror stays -
    of glass of index 1 (no bend, r0 = 0), 0.5 (total reflection from outside) and 1e30 (1 / ior tiny, r0 rounds to 1), appended to
    its materials (still staged: at most 16)."""
    hs = irl.HostScene.builtin("spheres")
    c = sg.Contents(hs.desc)
    m0, ids = c.a["materials"], c.a["mat_ids"].copy()
    glass = m0[m0["type"] == 2][:1]
    mats = np.concatenate([m0, np.resize(glass, 3)])
    mats["ior"][m0.size:] = (1.0, 0.5, 1e30)
    assert mats.size <= 16
    balls = np.array([0, 2, 4])
    assert (c.a["geometry"]["type"][balls] == 1).all() and m0[ids[balls]]["type"].tolist() == [0, 2, 2] and (m0[ids]["type"] == 1).any()
    ids[balls] = m0.size + np.arange(3)
    return _with_materials(hs, mats, ids)


def _builtin(name, w, h, spp):
    hs = irl.HostScene.builtin(name)
    return hs, _params(hs.desc, w, h, spp)


CASES = {
    "box": lambda: _builtin("box", 48, 48, 32),
    "spheres": lambda: _builtin("spheres", 64, 64, 64),
    "17 materials": lambda: (lambda hs: (hs, _params(hs.desc, 40, 40, 16)))(seventeen_materials()),
    "ior 1, 0.5 and 1e30": lambda: (lambda hs: (hs, _params(hs.desc, 40, 40, 16)))(odd_dielectrics()),
    "instrumented build": lambda: _builtin("box", 32, 32, 8),
    "nested-loop kernel": lambda: _builtin("spheres", 32, 32, 8),
    "NIF slots": lambda: _builtin("monkey", 32, 32, 8),
}


@pytest.fixture(scope="module")
def oracle_frames():
    """Every case's scene, its fresh ray stream and the oracle's frame, computed once."""
    out = {}
    for name, make in CASES.items():
        hs, d = make()
        first = hs.init_ray_stream()
        want = first.copy()
        ol.path_trace_pixel_rng(d, want, 16)
        out[name] = (hs, d, first, want)
    return out


@pytest.mark.parametrize("name", ["box", "spheres", "17 materials", "ior 1, 0.5 and 1e30"])
def test_frame_is_the_oracles(oracle_frames, name):
    hs, d, first, want = oracle_frames[name]
    if name != "box":
        # the bounces the case is about happen: paths end on glass and on the mirror (the last hit's geometry), and refract
        mats = sg.Contents(d).a
        last = mats["materials"][mats["mat_ids"][want["h"]["geomID"][want["h"]["geomID"] != 0xFFFF]]]["type"]
        assert (last == 2).any() and (last == 1).any(), name
    dev = irl.IpuScene(d)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
    assert_streams_identical(got, want, name)


def test_instrumented_build(oracle_frames):
    hs, d, first, want = oracle_frames["instrumented build"]
    dev = irl.IpuScene(d).set_option("full_stats", 1)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
    c = dev.counters(); dev.close()
    assert c["nodes_visited"] > 0, "not the instrumented build"
    assert_streams_identical(got, want, "box, full_stats")


def test_nested_loop_kernel(oracle_frames):
    hs, d, first, want = oracle_frames["nested-loop kernel"]
    dev = irl.IpuScene(d).set_option("kernel", 0)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
    assert_streams_identical(got, want, "spheres, kernel 0")


def test_nif_slot_render(oracle_frames):
    """A NIF render runs K1w's slot build. Its environment is the all-zero network here (exactly 0 for every escaped ray, decoded as
    the identity), so the frame - rgb included - is the plain oracle's."""
    hs, d, first, want = oracle_frames["NIF slots"]
    ks, bs, relu = npb.zero_network()
    dev = irl.IpuScene(d)
    dev.setNif(ks, bs, relu, npb.EMBED, 1.0, np.zeros(3, np.float32), False)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
    assert (got["h"]["flags"] & irl.FLAG_ESCAPED).any()
    assert_streams_identical(got, want, "monkey, NIF slots")
