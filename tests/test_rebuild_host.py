"""The host twin of the BVH rebuild, mi_build_lbvh_compact, without a GPU: the node format on the standard scenes, independence
from the desc's own nodes, the oracle's walk on the twin's nodes against every primitive without a BVH, degenerate inputs,
refusals, and a numpy / Python restatement of the whole LBVH that pins the twin itself."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import refit_cases as rc
import rebuild_cases as bc

SCENES = ["box", "spheres", "test_scene.dae", "soup", "soup-normals"]


@pytest.mark.parametrize("name", SCENES)
def test_format_contract(name):
    hs = rc.scene(name)
    nodes, depth = bc.twin(hs.desc)
    assert len(nodes) == hs.desc.num_nodes
    bc.assert_format(hs.desc, nodes, depth, name)
    # what mi_scene_create itself checks on a node array, restated: finite minima and extents
    assert np.isfinite(nodes["min_x"]).all() and np.isfinite(nodes["min_y"]).all() and np.isfinite(nodes["min_z"]).all()
    for f in ("dx", "dy", "dz"):
        assert ((nodes[f] & 0x7C00) != 0x7C00).all()


@pytest.mark.parametrize("name", ["soup", "box"])
def test_moved_geometry_keeps_the_format(name):
    hs = rc.scene(name)
    v, s, d = rc.jitter(hs, 5, 6.0)
    m = bc.rebuilt(hs, verts=v, spheres=s, discs=d)
    bc.assert_format(m.desc, m.nodes, m.desc.max_leaf_depth, f"{name} jittered")
    assert not np.array_equal(rc.node_bytes(m.nodes), rc.node_bytes(bc.twin(hs.desc)[0]))


@pytest.mark.parametrize("shape,seed", [("caterpillar", None), ("caterpillar", 3), ("balanced", None), ("comb", 9)])
def test_prior_topology_does_not_matter(shape, seed):
    hs = rc.edge_scene("comb")
    want, depth = bc.twin(hs.desc)
    nodes, d = rc.retopologise(hs, shape, seed=seed)
    m = rc.with_topology(hs, nodes, d)
    got, got_depth = bc.twin(m.desc)
    rc.assert_nodes_equal(got, want, f"twin under a {shape} tree")
    assert got_depth == depth


@pytest.mark.parametrize("name,seed", [("soup", 41), ("spheres", 42), ("box-simple", 43)])
def test_oracle_walk_on_twin_nodes_against_brute_force(name, seed):
    hs = rc.scene(name)
    m = bc.rebuilt(hs)
    rays = bc.seeded_rays(m.nodes, 300, seed)
    t, prim, geom, occ = bc.oracle_closest(m.desc, rays)
    want = rc.brute_force_closest(m.desc, rays)
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), f"{name}: {(t != want).sum()} rays differ in t"
    assert np.array_equal(occ, np.isfinite(want)), f"{name}: any hit"
    assert np.isfinite(want).sum() > 30


def _tri_scene(points):
    hs = rc.triangles(points)
    nodes, depth = bc.twin(hs.desc)
    bc.assert_format(hs.desc, nodes, depth, f"{len(points)} triangles")
    return hs, nodes, depth


def test_zero_one_two_three_primitives():
    empty = irl.SceneDesc()
    nodes, depth = irl.build_lbvh(empty)
    assert len(nodes) == 0 and depth == 0
    tri = np.array([[0, 0, -5], [1, 0, -5], [0, 1, -6]], np.float32)
    hs, nodes, depth = _tri_scene([tri])
    assert len(nodes) == 1 and depth == 1 and nodes["geomID"][0] == 0 and nodes["link"][0] == 0
    hs, nodes, depth = _tri_scene([tri, tri + 3])
    assert len(nodes) == 3 and depth == 2 and nodes["geomID"][0] == irl.INVALID_GEOM and nodes["link"][0] == 2
    hs, nodes, depth = _tri_scene([tri, tri + 3, tri - 4])
    assert len(nodes) == 5 and depth == 3


@pytest.mark.parametrize("count", [2, 64, 100, 1000])
def test_coincident_primitives_give_a_balanced_tree(count):
    tri = np.array([[0, 0, -5], [1, 0, -5], [0, 1, -6]], np.float32)
    hs, nodes, depth = _tri_scene([tri] * count)
    assert depth == 1 + int(np.ceil(np.log2(count))), f"{count} coincident triangles: depth {depth}"


def test_zero_extent_axes():
    rng = np.random.default_rng(12)
    base = np.array([[-.5, -.5, 0], [.5, -.5, 0], [0, .5, 0]], np.float32)
    plane = [base + np.array([x, y, -20], np.float32) for x, y in rng.integers(-40, 40, (200, 2))]       # all centroids at z = -20
    line = [base + np.array([x, 0, -20], np.float32) for x in rng.integers(-400, 400, 200)]             # ... and at y = -1/6 too
    point = [base * np.float32(s) + np.array([0, 0, -20], np.float32) for s in (1, 3, 5, 7)]            # nested: the same centroid on x and z
    for what, pts in (("plane", plane), ("line", line), ("nested", point)):
        hs, nodes, depth = _tri_scene(pts)
        got, d2 = bc.numpy_lbvh(hs.desc)
        rc.assert_nodes_equal(nodes, got, f"zero-extent axes ({what}): twin against numpy")
        assert depth == d2 and depth <= 63 + 32 + 1


def test_mixed_primitives_and_subnormal_coordinates():
    for name in ("spheres", "soup"):                         # spheres + discs + triangles
        hs = rc.scene(name)
        nodes, depth = bc.twin(hs.desc)
        got, d2 = bc.numpy_lbvh(hs.desc)
        rc.assert_nodes_equal(nodes, got, f"{name}: twin against numpy")
        assert depth == d2
    rng = np.random.default_rng(2)
    tiny = (rng.integers(-2000, 2000, (60, 3, 3)).astype(np.float32) * np.float32(1e-42)).astype(np.float32)   # binary32 subnormals
    assert (np.abs(tiny[tiny != 0]) < np.finfo(np.float32).tiny).all()
    hs, nodes, depth = _tri_scene(list(tiny))
    got, d2 = bc.numpy_lbvh(hs.desc)
    rc.assert_nodes_equal(nodes, got, "subnormal coordinates: twin against numpy")
    assert depth == d2 and len({int(k) for k in bc.numpy_keys(*bc.canonical_prims(hs.desc)[:2])}) > 30     # the keys still tell them apart


@pytest.mark.parametrize("name", ["box-simple", "soup-normals"])
def test_numpy_restatement_agrees_with_the_twin(name):
    hs = rc.scene(name)
    v, s, d = rc.jitter(hs, 8, 2.0)
    for m in (rc.Moved(hs), rc.Moved(hs, verts=v, spheres=s, discs=d)):
        nodes, depth = bc.twin(m.desc)
        got, d2 = bc.numpy_lbvh(m.desc)
        rc.assert_nodes_equal(nodes, got, f"{name}: twin against numpy")
        assert depth == d2


def test_twin_ignores_the_descs_nodes_and_rebuild_is_idempotent():
    hs = rc.scene("box")
    m = bc.rebuilt(hs)
    again, depth = bc.twin(m.desc)                            # the desc now carries the twin's own nodes
    rc.assert_nodes_equal(again, m.nodes, "twin of a twin-built desc")
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    d.bvh_nodes, d.num_nodes = None, 0
    rc.assert_nodes_equal(irl.build_lbvh(d)[0], m.nodes, "twin without nodes")


def test_refusals_carry_the_refits_messages():
    hs = rc.scene("soup")
    lib = irl.host_lib()
    out = np.zeros(hs.desc.num_nodes, irl.BVH_NODE)
    n, depth = C.c_uint32(), C.c_uint32()
    v = hs.verts.copy(); v["x"][0:3] = np.nan                       # a triangle with no finite x: its box is empty
    m = rc.Moved(hs, verts=v)
    assert lib.mi_build_lbvh_compact(C.byref(m.desc), out.ctypes.data, C.byref(n), C.byref(depth)) == 1
    assert b"a node box is not finite" in lib.mi_host_last_error()
    assert lib.mi_refit_compact_bvh(C.byref(m.desc), out.ctypes.data) == 1 and b"a node box is not finite" in lib.mi_host_last_error()
    v = hs.verts.copy(); v["x"][4] += np.float32(70000.0)           # an extent above 65504
    m = rc.Moved(hs, verts=v)
    assert lib.mi_build_lbvh_compact(C.byref(m.desc), out.ctypes.data, C.byref(n), C.byref(depth)) == 4
    assert b"Cannot compress BVH bounds into fp16 (half)" in lib.mi_host_last_error()
    v = hs.verts.copy(); v["y"][7] = np.nan                         # one NaN coordinate is ignored, as the refit ignores it
    m = rc.Moved(hs, verts=v)
    assert lib.mi_build_lbvh_compact(C.byref(m.desc), out.ctypes.data, C.byref(n), C.byref(depth)) == 0 and n.value == hs.desc.num_nodes
