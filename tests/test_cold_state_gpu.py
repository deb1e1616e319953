"""The hit record of a pixel's LAST sample, written through by the HOT builds of the default kernel (pytest -m gpu).

Those builds (K1wHotRot, K1wHotBary: plain renders with option hot_nodes on, which `auto` is for the built-in scenes) no longer carry the
last hit's leaf and distance and the bounce's normal in LDS for every sample (18 cold words, not 23: trace_wavefront.hpp LAST_THROUGH,
DESIGN.md section 33). A lane on its pixel's last sample writes t_max, prim_id, geom_id and the normal
of the record as they arise - GEN the empty record's, a SHADE with a hit the hit's, a SHADE without a hit t_max alone - and the end of the
pixel writes the rest. The same builds count casts and paths in two LDS words per wave. Every case compares the whole TraceResult stream
byte for byte, and casts and paths, with oracle_lib.path_trace_pixel_rng. Images are 16 x 8 (one whole row of 8 x 8 tiles) and 40 x 24
(whole tiles and a ragged rest); every case takes well under a second on the GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import set_geometry_cases as sg
from test_gpu_parity import _desc_restored, assert_streams_identical

pytestmark = pytest.mark.gpu

SIZES = ((16, 8), (40, 24))


def _segment_samples(spp):
    """ray_math.h segment_samples: spp / 16 rounded up, then up to a power of two, no shorter than 4 and no longer than 64."""
    want = (spp + 15) // 16
    shift = 0 if want <= 1 else (want - 1).bit_length()
    return 1 << min(max(shift, 2), 6)


@pytest.fixture(scope="module")
def scenes():
    return {name: irl.HostScene.builtin(name) for name in ("box", "spheres")}


def _check(desc, stream, what, options=(), frames=1, scribble=False):
    """`frames` renders of `stream` on one scene against as many of the oracle's; returns the oracle's stream. scribble: before the last
    render the record of every pixel is overwritten with bytes no render leaves (the stream the oracle continues keeps its own)."""
    got, want = stream.copy(), stream.copy()
    dev = irl.IpuScene(desc)
    for key, value in options:
        dev.set_option(key, value)
    casts = paths = 0
    for f in range(frames):
        if scribble and f == frames - 1:
            got.view(np.uint8).reshape(got.size, -1)[:, irl.TRACE_RESULT.fields["h"][1]:] = 0xA5
        dev.run(got, irl.MODE_PATH_TRACE)
        st = ol.path_trace_pixel_rng(desc, want, 16)
        casts += st.casts; paths += st.paths
    c = dev.counters(); dev.close()
    assert_streams_identical(got, want, what)
    assert (c["casts"], c["paths"]) == (casts, paths), what
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("spp", [1, 2, 5, 65, 70])
def test_sample_counts_where_the_last_sample_stands_alone_or_ends_a_segment(scenes, size, spp):
    """spp 1: the only sample is the last. 5 and 65: segments of 4 and 8 samples, so the last segment holds one sample - the lane that
    fetches it is on the last sample from its first GEN. 70: a last segment of six."""
    assert (_segment_samples(5), 5 % 4, _segment_samples(65), 65 % 8, _segment_samples(70)) == (4, 1, 8, 1, 8)
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(*size); d.samples_per_pixel = spp; d.path_trace = 1
        _check(d, s.init_ray_stream(), f"box {size}, {spp} spp")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("maxlen,roulette", [(1, 3), (2, 0), (10, 0)])
def test_path_length_limits(scenes, size, maxlen, roulette):
    """max_path_length 1: the last path ends at its first SHADE, hit or not. 2 and 10 with the roulette from the first bounce on."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(*size); d.samples_per_pixel = 5; d.path_trace = 1
        d.max_path_length, d.roulette_start_depth = maxlen, roulette
        want = _check(d, s.init_ray_stream(), f"box {size}, max_path_length {maxlen}, roulette from {roulette}")
        if maxlen == 1:
            hit = want["h"]["primID"] != irl.INVALID_PRIM
            assert hit.any() and np.all(np.isfinite(want["h"]["r"]["tMax"][hit]))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spheres_scene_normal_computed_at_the_hit(scenes, size):
    s = scenes["spheres"]
    with _desc_restored(s.desc) as d:
        d.set_image(*size); d.samples_per_pixel = 6; d.path_trace = 1
        want = _check(d, s.init_ray_stream(), f"spheres {size}, hot_nodes 96", options=(("hot_nodes", 96),))
        geom = s.geometry
        on_sphere = (want["h"]["geomID"] != irl.INVALID_GEOM) & (geom["type"][np.minimum(want["h"]["geomID"], geom.size - 1)] == 1)
        assert on_sphere.any(), "no pixel's last hit is a sphere"


def test_box_scene_cropped_to_the_light(scenes):
    """The 40 x 24 window of a 160 x 120 image round the pixels whose camera rays hit an emitter (found with the oracle at one sample,
    one bounce), and a 16 x 8 window inside it."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(160, 120); d.samples_per_pixel = 1; d.path_trace = 1; d.max_path_length = 1
        first = s.init_ray_stream(); ol.path_trace_pixel_rng(d, first, 16)
        emissive = s.materials["emissive"][s.mat_ids] != 0
        g = first["h"]["geomID"]
        lit = (g != irl.INVALID_GEOM) & emissive[np.minimum(g, emissive.size - 1)]
        assert lit.any(), "no camera ray of the box scene hits an emitter"
        row, col = int(np.median(first["u"][lit])), int(np.median(first["v"][lit]))
        d.max_path_length = 10
        for w, h in ((40, 24), (16, 8)):
            c0, r0 = min(max(col - w // 2, 0), 160 - w), min(max(row - h // 2, 0), 120 - h)
            for spp in (1, 5):
                d.samples_per_pixel = spp
                d.set_image(160, 120, (w, h, c0, r0))
                want = _check(d, s.init_ray_stream(), f"box cropped to the light, {w} x {h} at ({c0}, {r0}), {spp} spp")
                assert max(float(want["rgb"][k].max()) for k in "xyz") > 0.0


def _one_triangle(size, spp):
    """One emissive diffuse triangle at z = -10 that covers part of the view: a camera ray either escapes at once or hits it, bounces
    into the half space in front of it and escapes there (nothing else to hit; no roulette before bounce 3)."""
    c = sg.hand([("mesh", 1)], size=32, spp=spp)
    v = c.a["mesh_verts"]
    v["x"][:] = (-1.0, 2.0, -1.0, 30.0, 31.0, 30.0); v["y"][:] = (-1.0, -1.0, 2.0, 30.0, 30.0, 31.0); v["z"][:] = (-10.0, -10.0, -10.0, 50.0, 50.0, 50.0)
    d = irl.SceneDesc.from_buffer_copy(c.twin()[0])
    d.set_image(*size)
    return c, d


def _frame_of(desc):
    import ctypes as C
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    return rays


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("spp", [1, 5])
def test_one_triangle_last_path_escapes_at_once_or_after_its_hit(size, spp):
    c, d = _one_triangle(size, spp)
    want = _check(d, _frame_of(d), f"one triangle {size}, {spp} spp, hot_nodes 96", options=(("hot_nodes", 96),))
    _check(d, _frame_of(d), f"one triangle {size}, {spp} spp, hot_nodes 0", options=(("hot_nodes", 0),))
    h = want["h"]
    assert np.all(h["flags"] == irl.FLAG_ESCAPED) and np.all(np.isinf(h["r"]["tMax"]))
    missed = h["primID"] == irl.INVALID_PRIM
    # escaped at the primary ray: the empty record; hit, then escaped: the ids and the normal of the hit stay, t_max is inf
    assert missed.any() and np.all(h["geomID"][missed] == irl.INVALID_GEOM)
    assert np.all((h["normal"]["x"][missed] == 0) & (h["normal"]["y"][missed] == 0) & (h["normal"]["z"][missed] == 1))
    assert (~missed).any() and np.all(h["primID"][~missed] == 0) and np.all(h["geomID"][~missed] == 0)
    assert np.all(np.abs(h["normal"]["z"][~missed]) == 1)


@pytest.mark.parametrize("hot", [0, 96, "auto"])
def test_hot_node_counts(scenes, hot):
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.path_trace = 1
        for size, spp in ((SIZES[0], 5), (SIZES[1], 70)):
            d.set_image(*size); d.samples_per_pixel = spp
            _check(d, s.init_ray_stream(), f"box {size}, {spp} spp, hot_nodes={hot}", options=(("hot_nodes", hot),))


@pytest.mark.parametrize("normals", [False, True], ids=["face normals", "vertex normals"])
def test_collada_scene_crop_with_and_without_vertex_normals(normals, capfd):
    """hot_nodes 96: `auto` declines this scene, and the build under test is the HOT one - with vertex normals the barycentric build,
    whose normal is interpolated at the hit. The launch names its build."""
    s = irl.HostScene.import_file(Path(irl.REPO_ROOT) / "assets" / "test_scene.dae", load_normals=normals)
    d = s.desc
    d.path_trace = 1
    for (w, h), spp in ((SIZES[0], 5), (SIZES[1], 9)):
        d.samples_per_pixel = spp
        d.set_image(160, 160, (w, h, 64, 72))
        capfd.readouterr()
        want = _check(d, s.init_ray_stream(), f"test_scene.dae normals={normals}, {w} x {h}, {spp} spp, hot_nodes 96", options=(("hot_nodes", 96), ("say_grid", 1)))
        assert re.findall(r"96 hot nodes of \d+ that fit, build (\w+)", capfd.readouterr().err) == ["K1wHotBary" if normals else "K1wHotRot"]
        assert (want["h"]["primID"] != irl.INVALID_PRIM).any()
        _check(d, s.init_ray_stream(), f"test_scene.dae normals={normals}, {w} x {h}, {spp} spp, hot_nodes auto")


def test_second_frame_on_one_stream_overwrites_the_record(scenes):
    """Two frames accumulated on one stream; before the second, every byte of every record is overwritten with a pattern: each field
    must be written again by that launch."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.path_trace = 1
        for size, spp in ((SIZES[0], 1), (SIZES[1], 5), (SIZES[1], 70)):
            d.set_image(*size); d.samples_per_pixel = spp
            _check(d, s.init_ray_stream(), f"box {size}, {spp} spp, two frames", frames=2, scribble=True)


def test_render_cut_into_launches_by_the_partial_sum_budget(scenes):
    """seg_budget_kb 1: 256 floats hold no whole segment of these frames, so every launch takes one segment - nine launches at 70 spp,
    the last sample in the last of them; 10 KB holds segments of the smaller frame two at a time."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.path_trace = 1; d.samples_per_pixel = 70
        for size in SIZES:
            d.set_image(*size)
            for kb in (1, 10):
                _check(d, s.init_ray_stream(), f"box {size}, 70 spp, {kb} KB of partial sums", options=(("seg_budget_kb", kb),))


def test_headline_build_stages_more_nodes_in_two_resident_workgroups(scenes, capfd):
    """hot_nodes = auto on the box scene: K1wHotRot, 768 threads, room for more than the 316 nodes that 23 cold words left, and still two
    workgroups per compute unit (a device of 4 units: 8 workgroups, where the frame has work for 12)."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(*SIZES[1]); d.samples_per_pixel = 70; d.path_trace = 1
        capfd.readouterr()
        _check(d, s.init_ray_stream(), "box, say_grid", options=(("hot_nodes", "auto"), ("say_grid", 1), ("cus", 4)))
        said = re.findall(r"grid (\d+) workgroups of (\d+) threads, (\d+) hot nodes of (\d+) that fit, build (\w+)", capfd.readouterr().err)
        assert said, "the launch did not name its hot nodes"
        for wgs, threads, count, fit, build in said:
            assert (int(wgs), int(threads), build) == (8, 768, "K1wHotRot") and int(fit) > 316 and 0 < int(count) <= int(fit), said
