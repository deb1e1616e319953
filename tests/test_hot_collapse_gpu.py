"""The collapsed private copy on the GPU (pytest -m gpu): with scene option "hot_nodes" on, plain renders of the default kernel walk
a copy of the BVH arrays from which the interior nodes whose box test decides nothing have been taken (csrc/hot_order.hpp). Every
TraceResult byte must stay the oracle's with the option off, at 96 and at auto: on the box scene, a tree that collapses to its root
and its leaves, one primitive, no primitive, and a camera ray with zero direction components (the literal box test), alone and from
the plane of a flat leaf on a face of a deleted node - the case in which the literal test hits a box and misses the box around it,
for which such casts walk a region of every node. The
instrumented build keeps the copy of every node and reports the reference's visits; a refit retires both copies."""
import re

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import refit_cases as rc
import set_geometry_cases as sg
from test_gpu_parity import _desc_restored, assert_streams_identical
from test_hot_nodes_gpu import _frame_of

pytestmark = pytest.mark.gpu

HOT = (0, 96, "auto")
SIZE, SPP = 32, 16


def _renders(d, want, what, **options):
    for hot in HOT:
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        for k, v in options.items():
            dev.set_option(k, v)
        got = _frame_of(d); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert_streams_identical(got, want, f"{what}, hot_nodes={hot}")


@pytest.fixture(scope="module")
def box():
    return irl.HostScene.builtin("box")


def test_box_scene(box):
    with _desc_restored(box.desc) as d:
        d.set_image(SIZE, SIZE); d.samples_per_pixel = SPP; d.path_trace = 1
        c = irl.hot_collapse(np.array(box.nodes))
        assert 96 < c["hot"].size < d.num_nodes          # nodes do leave, and more stay than the prefix stages
        want = _frame_of(d); ol.path_trace_pixel_rng(d, want, 16)
        _renders(d, want, "box")


def test_tree_that_collapses_to_root_and_leaves():
    """Six triangles that each span the same cube: every box of the tree is that cube, so every interior node but the root leaves."""
    lo, hi = np.array([-5, -5, -45], np.float32), np.array([5, 5, -35], np.float32)
    corner = lambda *bits: np.where(bits, hi, lo)
    tris = [[corner(0, 0, 0), corner(1, 1, 1), corner(1, 0, 1)], [corner(0, 0, 0), corner(1, 1, 1), corner(0, 1, 0)],
            [corner(1, 0, 0), corner(0, 1, 1), corner(0, 0, 1)], [corner(1, 0, 0), corner(0, 1, 1), corner(1, 1, 0)],
            [corner(0, 1, 0), corner(1, 0, 1), corner(0, 0, 1)], [corner(0, 0, 1), corner(1, 1, 0), corner(1, 0, 0)]]
    hs = rc.triangles(tris)
    c = irl.hot_collapse(np.array(hs.nodes))
    assert hs.nodes.size == 11 and c["hot"].size == 7 and c["keep"].tolist() == [1] + [int(x) for x in (c["preorder"]["hit"][1:] & 0x80000000) != 0]
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(hs.desc), SIZE, SPP)
    want = _frame_of(d); ol.path_trace_pixel_rng(d, want, 16)
    assert np.any(want["h"]["geomID"] != irl.INVALID_GEOM)          # (the camera does see them)
    _renders(d, want, "six triangles in one cube")


def test_one_primitive_and_no_primitive():
    one = rc.edge_scene("one")
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(one.desc), SIZE, SPP)
    assert d.num_nodes == 1
    want = _frame_of(d); ol.path_trace_pixel_rng(d, want, 16)
    _renders(d, want, "one primitive")
    # no node at all: the oracle, like the reference, reads node 0 of any tree; the frame to meet is the nested-loop kernel's
    empty = sg.hand([])
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(empty.twin()[0]), SIZE, SPP)
    assert d.num_nodes == 0
    dev = irl.IpuScene(d).set_option("hot_nodes", 0).set_option("kernel", 0)
    want = _frame_of(d); dev.run(want, irl.MODE_PATH_TRACE); dev.close()
    assert np.all(want["h"]["flags"] == irl.FLAG_ESCAPED)
    _renders(d, want, "empty scene")


def test_zero_direction_components_take_the_literal_box_test(box):
    """anti_alias_scale 0: the camera ray of pixel (row h / 2, col w / 2) of an even-sized image points straight down the axis, and
    its casts walk the collapsed copy with the reference's compare / select sequence."""
    with _desc_restored(box.desc) as d:
        d.set_image(SIZE, SIZE); d.samples_per_pixel = SPP; d.path_trace = 1; d.anti_alias_scale = 0.0
        first = _frame_of(d)
        dirn = first[(SIZE // 2) * SIZE + SIZE // 2]["h"]["r"]["direction"]
        assert float(dirn["x"]) == 0.0 and float(dirn["y"]) == 0.0 and float(dirn["z"]) != 0.0, dirn
        want = first.copy(); ol.path_trace_pixel_rng(d, want, 16)
        _renders(d, want, "anti_alias_scale 0")


def test_literal_cast_from_the_plane_of_a_flat_leaf_on_a_face():
    """Three triangles, one flat in the plane y = 0 through the camera and on the upper face of the node the collapse takes out. With
    anti_alias_scale 0 the centre pixel's camera ray is (+0, -0, -1): the literal box test misses that node (products +inf and NaN) and
    would hit the flat leaf (NaN and NaN), so the collapsed tree on its own tests a primitive the reference never reaches. The plain
    builds start such a cast in the region of every node: the frame is the oracle's."""
    tris = [[[-1, 0, -10], [1, 0, -10], [0, 0, -12]], [[-1, -0.5, -10], [1, -0.125, -10], [0, -0.25, -12]], [[-1, 0, -10], [1, 1, -12], [0, 0.5, -10]]]
    hs = rc.triangles(tris)
    nodes = np.array(hs.nodes)
    c = irl.hot_collapse(nodes)
    assert c["keep"].tolist() == [1, 0, 1, 1, 1]
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(hs.desc), SIZE, SPP)
    d.anti_alias_scale = 0.0
    first = _frame_of(d)
    r = first[(SIZE // 2) * SIZE + SIZE // 2]["h"]["r"]
    o = [float(r["origin"][k]) for k in "xyz"]; dirn = np.array([r["direction"][k] for k in "xyz"], np.float32)
    assert o == [0.0, 0.0, 0.0] and dirn[1] == 0.0 and np.signbit(dirn[1]) and irl.hot_cast_is_literal(o, dirn)
    leaf = np.uint32(0x80000000)
    ref, _ = irl.hot_walk_count(c["preorder"], o, dirn, None)
    alone, _ = irl.hot_walk_count(c["hot"], o, dirn, c["leaf_link"])
    assert not np.any(ref & leaf) and np.any(alone & leaf)          # (the case is the one described)
    want = first.copy(); ol.path_trace_pixel_rng(d, want, 16)
    _renders(d, want, "flat leaf on a face, -0 direction component")


def test_instrumented_renders_report_the_reference_visits(box):
    with _desc_restored(box.desc) as d:
        d.set_image(SIZE, SIZE); d.samples_per_pixel = SPP; d.path_trace = 1
        want = _frame_of(d); st = ol.path_trace_pixel_rng(d, want, 16)
        for hot in HOT:
            dev = irl.IpuScene(d).set_option("full_stats", 1).set_option("hot_nodes", hot)
            got = _frame_of(d); dev.run(got, irl.MODE_PATH_TRACE)
            c = dev.counters(); dev.close()
            assert_streams_identical(got, want, f"instrumented, hot_nodes={hot}")
            assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (st.casts, st.nodesVisited, st.leafTests, st.paths), hot


def test_refit_retires_the_collapsed_copy(capfd):
    hs = rc.scene("box")
    base = sg.render_params(irl.SceneDesc.from_buffer_copy(hs.desc), SIZE, SPP)
    dev = irl.IpuScene(base).set_option("hot_nodes", 96).set_option("say_grid", 1)

    def check(desc, what, staged):
        want = _frame_of(desc); ol.path_trace_pixel_rng(desc, want, 16)
        capfd.readouterr()
        got = _frame_of(desc); dev.run(got, irl.MODE_PATH_TRACE)
        said = re.findall(r"(\d+) hot nodes of \d+ that fit", capfd.readouterr().err)
        assert_streams_identical(got, want, what)
        assert (said == ["96"] * len(said) and bool(said)) if staged else not said, (what, said)

    check(base, "as created", True)
    v, sp, di = rc.jitter(hs, 21, 3.0)
    dev.update_geometry(vertices=v, spheres=sp, discs=di)
    m = rc.Moved(hs, verts=v, spheres=sp, discs=di).refit()
    check(sg.render_params(m.desc, SIZE, SPP), "after a refit", False)
    dev.close()
