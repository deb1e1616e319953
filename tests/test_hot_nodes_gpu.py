"""Scene option "hot_nodes" on the GPU (pytest -m gpu): plain renders of the default kernel walk a private, hot-first copy of the
BVH arrays with the layout-free protocol and run the box-test runs whose lanes all stand in the staged prefix from LDS
(trace_wavefront.hpp HOT). Every TraceResult byte and every instrumented counter must stay the oracle's, whatever the count:
0 (off), 1, 2, odd and round counts, more than fits; trees that are hot as a whole, of one node and of none; the barycentric
build; the literal box test; live scenes, whose updates retire the copy; NIF renders, which keep the shared arrays; two streams."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import refit_cases as rc
import set_geometry_cases as sg
from test_gpu_parity import _desc_restored, _nif_weights, _soup_scene, assert_streams_identical

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 31, 96, 60000)          # 60000: more than a workgroup has room for, and than these trees have nodes


@pytest.fixture(scope="module")
def scenes():
    return {name: irl.HostScene.builtin(name) for name in ("box", "spheres")}


def _render(dev, s):
    got = s.init_ray_stream()
    dev.run(got, irl.MODE_PATH_TRACE)
    return got


def _frame_of(desc):
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    return rays


def _lds_steps(desc, hot, stream_of):
    """LDS box-test steps the instrumented build counts for one render of desc with hot_nodes = hot."""
    dev = irl.IpuScene(desc).set_option("full_stats", 1).set_option("hot_nodes", hot)
    dev.run(stream_of(), irl.MODE_PATH_TRACE)
    st = dev.hot_stats(); dev.close()
    return st["lds_steps"]


CROP = (131, 77, 7, 3)


@pytest.fixture(scope="module")
def box_frames(scenes):
    """The oracle's frames of the box scene at 70 spp (a segmented sample count): the whole 200 x 120 window and a ragged crop."""
    s = scenes["box"]
    out = {}
    with _desc_restored(s.desc) as d:
        d.path_trace = 1; d.samples_per_pixel = 70
        for crop in (None, CROP):
            d.set_image(200, 120) if crop is None else d.set_image(150, 90, crop)
            want = s.init_ray_stream(); ol.path_trace_pixel_rng(d, want, 16)
            out[crop] = want
    return out


def test_box_scene_every_count_and_a_ragged_crop(scenes, box_frames, capfd):
    """... and the plain build itself must have been what rendered: with say_grid the launch names the hot nodes it staged - as many
    as asked for, never more than fit -, and says nothing of them with the option off."""
    import re
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.path_trace = 1; d.samples_per_pixel = 70
        for crop in (None, CROP):
            d.set_image(200, 120) if crop is None else d.set_image(150, 90, crop)
            for hot in COUNTS + ("auto",):
                dev = irl.IpuScene(d).set_option("hot_nodes", hot).set_option("say_grid", 1)
                capfd.readouterr()
                got = _render(dev, s); dev.close()
                said = re.findall(r"workgroups of (\d+) threads, (\d+) hot nodes of (\d+) that fit", capfd.readouterr().err)
                assert_streams_identical(got, box_frames[crop], f"box, hot_nodes={hot}, crop={crop}")
                if hot == 0:
                    assert not said
                else:      # (70 spp: one launch of a few segments)
                    assert said and all(int(t) == 768 for t, _, _ in said), (hot, said)
                    fit = int(said[0][2])
                    assert fit >= 96 and all(int(c) == (fit if hot in (60000, "auto") else hot) for _, c, _ in said), (hot, said)


def test_instrumented_build_sees_lds_runs_only_with_the_option(scenes):
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.path_trace = 1; d.samples_per_pixel = 8; d.set_image(200, 120)
        assert _lds_steps(d, 96, s.init_ray_stream) > 0 and _lds_steps(d, 0, s.init_ray_stream) == 0
        with pytest.raises(irl.RaylibError):
            irl.IpuScene(d).set_option("hot_nodes", 70000)
        with pytest.raises(irl.RaylibError):
            irl.IpuScene(d).set_option("hot_nodes", "many")


def test_whole_tree_hot_one_primitive_and_empty_scene(scenes):
    s = scenes["spheres"]
    with _desc_restored(s.desc) as d:
        d.set_image(96, 64); d.samples_per_pixel = 20; d.path_trace = 1
        want = s.init_ray_stream(); ol.path_trace_pixel_rng(d, want, 16)
        assert d.num_nodes < 96
        for hot in COUNTS:
            dev = irl.IpuScene(d).set_option("hot_nodes", hot)
            got = _render(dev, s); dev.close()
            assert_streams_identical(got, want, f"spheres (the whole tree hot), hot_nodes={hot}")
    one = rc.edge_scene("one")                                 # one node: the root is a leaf (rootInterior = 0)
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(one.desc), 48, 20)
    assert d.num_nodes == 1
    want = _frame_of(d); ol.path_trace_pixel_rng(d, want, 16)
    for hot in (1, 96):
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        got = _frame_of(d); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert_streams_identical(got, want, f"one primitive, hot_nodes={hot}")
    # no node at all. The oracle, like the reference, reads node 0 of any tree, so it cannot render this one: the frame is the
    # nested-loop kernel's and today's default kernel's, in which every path escapes at once
    empty = sg.hand([])
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(empty.twin()[0]), 48, 20)
    assert d.num_nodes == 0
    frames = []
    for hot, kernel in ((0, 0), (0, 1), (96, 1)):
        dev = irl.IpuScene(d).set_option("hot_nodes", hot).set_option("kernel", kernel)
        got = _frame_of(d); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        frames.append(got)
    assert np.all(frames[0]["h"]["flags"] == irl.FLAG_ESCAPED) and np.all(frames[0]["h"]["geomID"] == irl.INVALID_GEOM)
    assert_streams_identical(frames[1], frames[0], "empty scene, default kernel")
    assert_streams_identical(frames[2], frames[0], "empty scene, hot_nodes=96")


def test_vertex_normal_scenes_run_the_barycentric_build():
    s = irl.HostScene.import_file(Path(irl.REPO_ROOT) / "assets" / "test_scene.dae", load_normals=True)
    d = s.desc
    d.set_image(160, 160); d.samples_per_pixel = 8; d.path_trace = 1
    want = s.init_ray_stream(); ol.path_trace_pixel_rng(d, want, 16)
    for hot in (1, 31, 96):
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        got = _render(dev, s); dev.close()
        assert_streams_identical(got, want, f"test_scene.dae with normals, hot_nodes={hot}")
    assert _lds_steps(d, 96, s.init_ray_stream) > 0
    s = _soup_scene(np.random.default_rng(1235), 600, True)
    d = s.desc
    d.set_image(160, 120); d.samples_per_pixel = 6; d.path_trace = 1
    want = s.init_ray_stream(); ol.path_trace_pixel_rng(d, want, 16)
    for hot in (2, 96):
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        got = _render(dev, s); dev.close()
        assert_streams_identical(got, want, f"soup with normals, hot_nodes={hot}")


def test_instrumented_build_counts_the_reference_visits(scenes):
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(256, 256); d.samples_per_pixel = 3; d.path_trace = 1
        want = s.init_ray_stream(); st = ol.path_trace_pixel_rng(d, want, 16)
        seen = {}
        for hot in (0, 96):
            dev = irl.IpuScene(d).set_option("full_stats", 1).set_option("hot_nodes", hot)
            got = _render(dev, s)
            c = dev.counters(); seen[hot] = c; h = dev.hot_stats(); dev.close()
            assert_streams_identical(got, want, f"instrumented path trace, hot_nodes={hot}")
            assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (st.casts, st.nodesVisited, st.leafTests, st.paths), hot
            if hot:
                assert h["lds_steps"] > 0 and h["global_steps"] > 0 and 0 < h["hot_visits"] <= c["nodes_visited"]
                assert h["lds_lanes"] + h["global_lanes"] <= c["nodes_visited"]
            else:
                assert not any(h.values())
        assert seen[0] == seen[96]


def test_literal_box_test_lane(scenes):
    """A cast with a zero direction component takes the literal compare / select box test (exactSlab), and a burst with such a
    lane keeps the global form, test by test, on the private copy's leaf-at-itself protocol. With anti_alias_scale 0 the camera
    ray of pixel (row h / 2, col w / 2) of an EVEN-sized image points straight down the axis - the camera maps a pixel to
    (col / w - 0.5, row / h - 0.5), which no pixel of an odd-sized image makes zero -, and the stream itself says so: the
    un-jittered direction of that record has two zero components."""
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(64, 48); d.samples_per_pixel = 20; d.path_trace = 1; d.anti_alias_scale = 0.0
        first = s.init_ray_stream()
        centre = first[24 * 64 + 32]
        assert int(centre["u"]) == 24 and int(centre["v"]) == 32
        dirn = centre["h"]["r"]["direction"]
        assert float(dirn["x"]) == 0.0 and float(dirn["y"]) == 0.0 and float(dirn["z"]) != 0.0, dirn
        want = first.copy(); ol.path_trace_pixel_rng(d, want, 16)
        for hot in (0, 96, "auto"):
            dev = irl.IpuScene(d).set_option("hot_nodes", hot)
            got = _render(dev, s); dev.close()
            assert_streams_identical(got, want, f"anti_alias_scale 0 at 64 x 48, hot_nodes={hot}")


def test_live_scene_updates_retire_the_private_copy():
    hs = rc.scene("box")
    base = sg.render_params(irl.SceneDesc.from_buffer_copy(hs.desc), 48, 12)
    dev = irl.IpuScene(base).set_option("hot_nodes", 96).set_option("full_stats", 1)

    def check(desc, what, lds):
        dev.reset_counters()
        want = _frame_of(desc); ol.path_trace_pixel_rng(desc, want, 16)
        got = _frame_of(desc); dev.run(got, irl.MODE_PATH_TRACE)
        assert_streams_identical(got, want, what)
        assert (dev.hot_stats()["lds_steps"] > 0) == lds, what

    check(base, "as created", True)
    v, sp, di = rc.jitter(hs, 21, 3.0)
    dev.update_geometry(vertices=v, spheres=sp, discs=di)
    m = rc.Moved(hs, verts=v, spheres=sp, discs=di).refit()
    check(sg.render_params(m.desc, 48, 12), "after mi_scene_update", False)
    dev.rebuild_bvh()
    nodes = dev.bvh_nodes()
    m.set_nodes(nodes); m.desc.num_nodes = len(nodes); m.desc.max_leaf_depth = dev.live_stats()["max_leaf_depth"]
    check(sg.render_params(m.desc, 48, 12), "after mi_scene_rebuild", False)
    c = sg.named("soup", size=48, spp=12)
    dev.set_geometry(c.desc)
    check(c.twin()[0], "after mi_scene_set_geometry", False)
    dev.close()
    # a scene that is only rebuilt, and one that only gets new contents
    dev = irl.IpuScene(base).set_option("hot_nodes", 96).set_option("full_stats", 1)
    dev.rebuild_bvh()
    nodes = dev.bvh_nodes()
    m = rc.Moved(hs).set_nodes(nodes); m.desc.num_nodes = len(nodes); m.desc.max_leaf_depth = dev.live_stats()["max_leaf_depth"]
    check(sg.render_params(m.desc, 48, 12), "rebuilt without an update", False)
    dev.close()
    dev = irl.IpuScene(base).set_option("hot_nodes", 96).set_option("full_stats", 1)
    dev.set_geometry(c.desc)
    check(c.twin()[0], "new contents without an update", False)
    dev.close()


def test_nif_renders_keep_the_shared_arrays(scenes):
    sp = scenes["spheres"]
    with _desc_restored(sp.desc) as d:
        rng = np.random.default_rng(6)
        ks, bs, relu = _nif_weights(rng, hidden=64, embed=12, layers=4)
        d.set_image(96, 64); d.samples_per_pixel = 20; d.path_trace = 1
        frames = []
        for hot in (0, 96):
            dev = irl.IpuScene(d).set_option("hot_nodes", hot)
            dev.setNif(ks, bs, relu, 12, 3.43, np.array([-2.35, -2.26, -1.96], np.float32), True)
            frames.append(_render(dev, sp)); dev.close()
        assert_streams_identical(frames[1], frames[0], "NIF render, hot_nodes on against off")


def test_one_scene_on_two_streams(scenes):
    import torch
    s = scenes["box"]
    with _desc_restored(s.desc) as d:
        d.set_image(200, 120); d.samples_per_pixel = 100; d.path_trace = 1
        dev = irl.IpuScene(d).set_option("hot_nodes", 96)
        host = s.init_ray_stream(); want = host.copy()
        ol.path_trace_pixel_rng(d, want, 16)
        raw = torch.from_numpy(host.view(np.uint8).reshape(host.size, -1).copy())
        bufs = [raw.cuda(), raw.cuda()]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for b, st in zip(bufs, streams):
            dev.run_device(b.data_ptr(), host.size, irl.MODE_PATH_TRACE, st.cuda_stream)
        torch.cuda.synchronize()
        for b in bufs:
            got = np.frombuffer(b.cpu().numpy().tobytes(), dtype=irl.TRACE_RESULT)
            assert_streams_identical(got, want, "two streams of one scene, hot_nodes on")
        dev.close()
