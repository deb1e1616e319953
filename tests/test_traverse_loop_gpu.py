"""K1w's TRAVERSE loop (pytest -m gpu): a lane's phase is read off its `node` word - walking, stopped at a primitive (the leaf flag
rides in the register up to the LEAF turn), walk complete, and three values above every byte offset for GEN, FETCH and DONE - and a
run of box tests takes its length once. Wherever that can go wrong the frame must stay the oracle's, all 84 bytes of every
TraceResult, with the oracle's casts and paths, and the instrumented build must count the oracle's box tests and primitive tests:
one wave with every walking population that changes the length of a run, trees of 0, 1 and 3 nodes and one whose last node is a
leaf (its link is the array's end, next to the first parked value), streams of 1 and 65 pixels (lanes parked in FETCH and DONE are
voted on while others walk), the literal box test beside spelled-out runs, and each default-path build once."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import set_geometry_cases as sg
from test_gpu_parity import _nif_weights, assert_streams_identical, rows_differing
from test_leaf_turn_gpu import _case, _params

pytestmark = pytest.mark.gpu

HOT = (0, 96)          # off, and forced on (96 nodes staged whatever the tree's size)


def _oracle(d, first):
    want = first.copy()
    st = ol.path_trace_pixel_rng(d, want, 16)
    return want, st


def _check(d, first, want, st, what, hots=HOT, instrumented=True, variants=False, options=()):
    """The plain build's frame and counts, then the instrumented build's, against the oracle's - for every hot_nodes value."""
    for hot in hots:
        for stats in ((0, 1) if instrumented else (0,)):
            dev = irl.IpuScene(d, variants=variants).set_option("hot_nodes", hot).set_option("full_stats", stats)
            for k, v in options:
                dev.set_option(k, v)
            got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
            c = dev.counters(); dev.close()
            tag = f"{what}, hot_nodes={hot}, full_stats={stats}"
            assert_streams_identical(got, want, tag)
            assert (c["casts"], c["paths"]) == (st.casts, st.paths), tag
            if stats:
                assert (c["nodes_visited"], c["leaf_tests"]) == (st.nodesVisited, st.leafTests), tag


# ---- run lengths ---------------------------------------------------------------------------------------------------
LANES = (1, 3, 4, 7, 8, 23, 24, 25, 64)      # a run is 1 + min(lanes / 4, 6) box tests: 1, 1, 2, 2, 3, 6, 7, 7 and 7 - both sides of the full-length run's entry


@pytest.fixture(scope="module")
def tile():
    """The 8 x 8 pixels in the middle of a 64 x 64 view into the box scene: one wave's tile, every camera ray ends on a wall of the box."""
    s = irl.HostScene.builtin("box")
    d = _params(s.desc, 64, 64, 6)
    d.set_image(64, 64, (8, 8, 28, 28))
    first = s.init_ray_stream()
    assert first.size == 64
    return s, d, first


@pytest.mark.parametrize("lanes", LANES)
def test_one_wave_with_this_many_walking_lanes(tile, lanes):
    s, d, first = tile
    sub = np.ascontiguousarray(first[:lanes])
    want, st = _oracle(d, sub)
    # every cast walks eight nodes or more: all lanes of the stream are still walking when the first run of a burst ends, so that run
    # has the length its population asks for
    assert st.nodesVisited >= 8 * st.casts and st.casts > st.paths == lanes * 6
    _check(d, sub, want, st, f"{lanes} walking lanes")


# ---- the phase in the node word --------------------------------------------------------------------------------------
TREES = [("one node", False), ("three nodes", False), ("last leaf", False), ("one node", True), ("last leaf", True)]


@pytest.mark.parametrize("name,normals", TREES)
def test_small_trees_and_a_last_leaf(name, normals):
    """One node: the root is a leaf, every cast stops at a primitive on its first box test and the node behind it is the array's end.
    Three nodes: a root and two leaves. Last leaf: most walks end at the array's final node, whose link is numNodes << 5."""
    hs, d = _case(name, normals)
    if name == "last leaf":
        d.set_image(40, 24); d.samples_per_pixel = 4
        assert int(hs.nodes[-1]["link"]) == 60 and int(hs.nodes[-1]["geomID"]) != 0xFFFF
    first = hs.init_ray_stream()
    want, st = _oracle(d, first)
    assert st.leafTests > 0
    _check(d, first, want, st, f"{name}, normals={normals}")


def test_no_node_at_all():
    """node = 0 of an empty tree is already its end: every path escapes at once (the oracle, like the reference, reads node 0 of
    any tree and cannot render this one: the frame is the nested-loop kernel's)."""
    empty = sg.hand([])
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(empty.twin()[0]), 16, 4)
    assert d.num_nodes == 0

    def frame(kernel, hot=0, stats=0):
        dev = irl.IpuScene(d).set_option("kernel", kernel).set_option("hot_nodes", hot).set_option("full_stats", stats)
        got = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
        irl.host_lib().mi_init_ray_stream(C.byref(d), got.ctypes.data, got.size)
        dev.run(got, irl.MODE_PATH_TRACE)
        c = dev.counters(); dev.close()
        return got, c

    want, _ = frame(0)
    assert np.all(want["h"]["flags"] == irl.FLAG_ESCAPED)
    for hot in HOT:
        for stats in (0, 1):
            got, c = frame(1, hot, stats)
            assert_streams_identical(got, want, f"empty scene, hot_nodes={hot}, full_stats={stats}")
            assert c["casts"] == c["paths"] == 16 * 16 * 4 and (c["nodes_visited"], c["leaf_tests"]) == (0, 0)


@pytest.mark.parametrize("pixels", (1, 65))
def test_streams_of_1_and_65_pixels(pixels):
    """One pixel: 63 lanes of the wave are DONE from the first FETCH on. 65: a second wave (or a second service of the first) holds one
    pixel; lanes finish their four samples at different times and sit in FETCH, then DONE, while the others walk."""
    s = irl.HostScene.builtin("box")
    d = _params(s.desc, 64, 64, 4)
    first = np.ascontiguousarray(s.init_ray_stream()[64 * 30 + 10:64 * 30 + 10 + pixels])      # (a stretch of a row across the box, wrapping into the next)
    want, st = _oracle(d, first)
    assert st.paths == pixels * 4 and st.leafTests > 0
    _check(d, first, want, st, f"{pixels} pixels at 4 spp")


# ---- the literal box test beside spelled-out runs -----------------------------------------------------------------------
def test_zero_and_denormal_direction_components_beside_ordinary_rays():
    """anti_alias_scale 0 in an even-sized image: the camera rays of the centre row and column have a component that is exactly zero,
    the other pixels of the same 8 x 8 tile are ordinary - a burst with such a camera ray takes the literal test, test by test, the
    same wave's other bursts run spelled out. With a field of view of 1e-38 rad every camera ray's x and y are denormal or zero, and
    they share their waves with the ordinary rays of the second and later bounces."""
    for fov, size in ((None, (16, 16)), (1e-38, (16, 8))):
        s = irl.HostScene.builtin("box")
        d = _params(s.desc, size[0], size[1], 8)
        d.anti_alias_scale = 0.0
        if fov is not None:
            d.fov_radians = fov
        first = s.init_ray_stream()
        dx, dy = first["h"]["r"]["direction"]["x"], first["h"]["r"]["direction"]["y"]
        tiny = np.float32(1.1754944e-38)
        assert np.any(dx == 0) and np.any(dy == 0) and np.any(dx != 0) and np.any(dy != 0)
        if fov is None:
            assert np.sum((np.abs(dx) > tiny) & (np.abs(dy) > tiny)) > first.size // 2
        else:
            assert np.all(np.abs(dx) < tiny) and np.all(np.abs(dy) < tiny)
        want, st = _oracle(d, first)
        assert st.casts > st.paths          # (bounce rays, all ordinary, beside the camera rays)
        _check(d, first, want, st, f"anti_alias_scale 0, fov {fov}")


# ---- each default-path build once -----------------------------------------------------------------------------------------
def test_vertex_normal_scene_runs_the_barycentric_builds():
    hs, d = _case("box", True)
    d.set_image(40, 40); d.samples_per_pixel = 4
    first = hs.init_ray_stream()
    want, st = _oracle(d, first)
    _check(d, first, want, st, "box with vertex normals")


def test_shared_arrays_without_the_rotated_records():
    """leaf_rot 0: the plain records of the shared arrays (the 256-thread builds without ROT)."""
    s = irl.HostScene.builtin("box")
    d = _params(s.desc, 40, 40, 4)
    first = s.init_ray_stream()
    want, st = _oracle(d, first)
    _check(d, first, want, st, "leaf_rot 0", hots=(0,), instrumented=False, options=(("leaf_rot", 0),))


def test_nif_slot_render():
    """The slot build (NIF renders), with and without the first box test in the set-up turn: hit records are the oracle's byte for
    byte; rgb carries the MLP's stated tolerance (test_gpu_parity.py::test_config5_monkey_with_nif_environment)."""
    rng = np.random.default_rng(8)
    ks, bs, relu = _nif_weights(rng, hidden=64, embed=12, layers=4)
    mean = np.array([-2.35, -2.26, -1.96], np.float32)
    s = irl.HostScene.builtin("monkey")
    d = _params(s.desc, 48, 48, 4)
    nif, keep = ol.make_nif(ks, bs, relu, 12, 3.43, mean, True, half_features=True, half_weights_acts=True)
    first = s.init_ray_stream(); want = first.copy()
    st = ol.Stats()
    ol.lib().o_path_trace_nif_pixel_rng(C.byref(d), C.byref(nif), 0.0, want.ctypes.data, want.size, 16, C.byref(st))
    w = np.stack([want["rgb"][k] for k in "xyz"], 1)
    for first_test in (0, 1):
        dev = irl.IpuScene(d).set_option("nif_first_test", first_test)
        dev.setNif(ks, bs, relu, 12, 3.43, mean, True)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
        c = dev.counters(); dev.close()
        assert rows_differing(np.ascontiguousarray(got["h"]), np.ascontiguousarray(want["h"])).size == 0, f"hit records, nif_first_test={first_test}"
        assert (c["casts"], c["paths"]) == (st.casts, st.paths)
        g = np.stack([got["rgb"][k] for k in "xyz"], 1)
        err = np.abs(g - w) / (np.abs(w) + 0.05)
        assert np.quantile(err, 0.995) < 0.03 and err.max() < 0.3, (first_test, np.quantile(err, 0.995), err.max())


def test_tolerance_tier_first_hits():
    """Scene option "fast" against its stated tolerance for first hits (test_gpu_parity.py::test_fast_tier_within_its_stated_tolerance):
    the same primitive in every pixel, the hit distance within 1e-6 relative."""
    s = irl.HostScene.builtin("box")
    d = _params(s.desc, 96, 96, 1)
    d.max_path_length = 1
    first = s.init_ray_stream()
    want, st = _oracle(d, first)
    dev = irl.IpuScene(d).set_option("fast", 1)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
    c = dev.counters(); dev.close()
    assert (c["casts"], c["paths"]) == (st.casts, st.paths)
    for k in ("primID", "geomID", "flags"):
        assert np.array_equal(got["h"][k], want["h"][k]), k
    hit = want["h"]["primID"] != irl.INVALID_PRIM
    assert hit.mean() > 0.6
    ta, tb = want["h"]["r"]["tMax"][hit], got["h"]["r"]["tMax"][hit]
    assert np.all(np.abs(ta - tb) <= 1e-6 * np.abs(ta))


@pytest.mark.parametrize("options", [(("spec", 1),), (("merge", 0),), (("waves", 4),), (("merge", 0), ("spec", 1), ("waves", 4)),
                                     (("tune", "8,16,24,48,3,2,7"),), (("tune", "8,16,24,48,3,64,0"),)],
                         ids=lambda o: " ".join(f"{k}={v}" for k, v in o))
def test_variants_library(options):
    """The forms kept in the variants build: the speculative walk (which keeps a phase word of its own), the two-turn form, the
    four-wave build, and run-time weights with the longest runs the ladder spells out (eight tests) and with none beyond the first."""
    s = irl.HostScene.builtin("box")
    d = _params(s.desc, 40, 40, 4)
    first = s.init_ray_stream()
    want, st = _oracle(d, first)
    _check(d, first, want, st, f"variants build, {options}", hots=(0,), variants=True, options=options)
