"""Scene option leaf_frame on the GPU (pytest -m gpu): K1w's SHADE turn loads the tangent frame of a diffuse bounce off a triangle or
disc from a per-leaf record (csrc/leaf_frame.hpp) instead of computing it per hit. Every byte of every TraceResult is the oracle's
either way: on a hand-made flat scene that holds the frame's special normals, after the record was rewritten on the device by a
refit, a rebuild and new contents, on the box scene (plain; as a NIF-slot render the settings agree with each other), on a scene
with vertex normals (which never sees a record), and against the build that carries barycentrics (lean_hit 0), whose frames are
all computed."""
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
from test_gpu_parity import assert_streams_identical, _nif_weights
from test_leaf_frame import flat_contents

pytestmark = pytest.mark.gpu

SIZE, SPP = 32, 16
HOT_ON = 32          # the private copy with that many nodes staged (clamped to the tree); 0 = the shared arrays


def _stream(desc):
    import ctypes as C
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    return rays


def _oracle(desc):
    want = _stream(desc)
    ol.path_trace_pixel_rng(desc, want, 16)
    return want


def _render(dev, desc, **options):
    for k, v in options.items():
        dev.set_option(k, v)
    got = _stream(desc)
    dev.run(got, irl.MODE_PATH_TRACE)
    return got


def _all_settings(dev, desc, want, what):
    for frame in (0, 1):
        for hot in (0, HOT_ON):
            got = _render(dev, desc, leaf_frame=frame, hot_nodes=hot)
            assert_streams_identical(got, want, f"{what}: leaf_frame={frame}, hot_nodes={hot}")


def _diffuse_hits(want):
    """Paths of the oracle's frame whose last recorded hit is on a primitive (a smoke check that the scene is not looked past)."""
    return int((want["h"]["primID"] != 0xFFFFFFFF).sum())


def test_hand_made_flat_scene_either_way_shared_and_private_arrays():
    c = flat_contents(SIZE, SPP)
    desc = c.twin()[0]
    want = _oracle(desc)
    assert _diffuse_hits(want) > want.size // 2
    dev = irl.IpuScene(desc)
    _all_settings(dev, desc, want, "flat scene")
    dev.close()


def test_the_record_follows_the_geometry_through_update_rebuild_and_new_contents():
    a, b = flat_contents(SIZE, SPP), flat_contents(SIZE, SPP, moved=True)
    desc, topo, depth = a.twin()
    dev = irl.IpuScene(desc)
    dev.set_option("leaf_frame", 1)
    first = _render(dev, desc)            # (the records as uploaded have been read once before anything rewrites them)
    assert_streams_identical(first, _oracle(desc), "flat scene as created")
    # a refit: every vertex, the sphere and the disc moved, the topology kept - refit_write_kernel rewrites normals and frames
    dev.update_geometry(**b.update_args())
    moved = irl.SceneDesc.from_buffer_copy(b.desc)
    nodes = np.ascontiguousarray(topo)
    moved.bvh_nodes, moved.num_nodes, moved.max_leaf_depth = nodes.ctypes.data, len(nodes), depth
    refit = np.ascontiguousarray(irl.refit_compact_bvh(moved))
    moved.bvh_nodes = refit.ctypes.data
    want = _oracle(moved)
    assert not np.array_equal(want.view(np.uint8), first.view(np.uint8))
    _all_settings(dev, moved, want, "after mi_scene_update")
    # a rebuild of the moved arrays: rebuild_scatter_kernel writes every record at its new place
    dev.rebuild_bvh()
    _all_settings(dev, b.twin()[0], _oracle(b.twin()[0]), "after mi_scene_rebuild")
    # new contents of other counts (a second disc, a second sphere): the record array is allocated anew and written by the same kernel
    c = flat_contents(SIZE, SPP, extra=True)
    dev.set_geometry(c.desc)
    _all_settings(dev, c.twin()[0], _oracle(c.twin()[0]), "after mi_scene_set_geometry")
    # ... and back, through an update of the new contents
    j = c.jittered(3)
    dev.update_geometry(**j.update_args())
    moved = irl.SceneDesc.from_buffer_copy(j.desc)
    nodes = np.ascontiguousarray(c.twin()[1])
    moved.bvh_nodes, moved.num_nodes, moved.max_leaf_depth = nodes.ctypes.data, len(nodes), c.twin()[2]
    refit = np.ascontiguousarray(irl.refit_compact_bvh(moved))
    moved.bvh_nodes = refit.ctypes.data
    _all_settings(dev, moved, _oracle(moved), "update after mi_scene_set_geometry")
    dev.close()


def test_box_scene_plain_and_nif_slot_render():
    s = irl.HostScene.builtin("box")
    d = s.desc
    d.set_image(SIZE, SIZE); d.samples_per_pixel = 64; d.path_trace = 1
    want = _oracle(d)
    dev = irl.IpuScene(d)
    _all_settings(dev, d, want, "box scene")
    dev.close()
    # one NIF-slot render (the slot instantiations of the same turn; they compute every frame, in ray_math.h's select form, and must
    # not mind the option or the records the scene holds): the settings agree byte for byte
    rng = np.random.default_rng(21)
    ks, bs, relu = _nif_weights(rng, hidden=64, embed=12, layers=3)
    frames = []
    for options in ({"leaf_frame": 1}, {"leaf_frame": 0}, {"lean_hit": 0}):
        dev = irl.IpuScene(d)
        dev.setNif(ks, bs, relu, 12, 3.43, np.array([-2.35, -2.26, -1.96], np.float32), True)
        frames.append(_render(dev, d, **options))
        dev.close()
    assert_streams_identical(frames[1], frames[0], "NIF render, leaf_frame off")
    assert_streams_identical(frames[2], frames[0], "NIF render, the build with barycentrics")


def test_scene_with_vertex_normals_takes_the_computed_form():
    s = irl.HostScene.import_file(Path(irl.REPO_ROOT) / "assets" / "test_scene.dae", load_normals=True)
    d = s.desc
    d.set_image(16, 16); d.samples_per_pixel = 16; d.path_trace = 1
    want = _oracle(d)
    dev = irl.IpuScene(d)
    _all_settings(dev, d, want, "test_scene.dae with normals")
    dev.close()


def test_loaded_frames_against_the_build_with_barycentrics():
    """lean_hit 0 sends a flat scene through the build whose frames are all computed: a second, independent computed form."""
    flat, box = flat_contents(SIZE, SPP), irl.HostScene.builtin("box")      # (kept: the descs point into them)
    box.desc.set_image(SIZE, SIZE); box.desc.samples_per_pixel = SPP; box.desc.path_trace = 1
    for name, desc in (("flat scene", flat.twin()[0]), ("box", box.desc)):
        for hot in (0, HOT_ON):
            dev = irl.IpuScene(desc)
            loaded = _render(dev, desc, leaf_frame=1, lean_hit=1, hot_nodes=hot)
            computed = _render(dev, desc, leaf_frame=1, lean_hit=0, hot_nodes=hot)
            dev.close()
            assert_streams_identical(loaded, computed, f"{name}, hot_nodes={hot}: leaf_frame 1 against lean_hit 0")
