"""The BVH rebuild on the GPU (pytest -m gpu): mi_scene_rebuild gives a live scene a new topology from its current geometry.
After a rebuild the device nodes equal the host twin (mi_build_lbvh_compact) byte for byte, whatever tree the scene had, and
every query and render equals - bit for bit - a scene freshly created from the current arrays and the twin's nodes, and the CPU
oracle on them. Every twin depth is checked against the oracle's 128-entry stack (rebuild_cases.twin)."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import refit_cases as rc
import rebuild_cases as bc
import test_refit_gpu as tg

pytestmark = pytest.mark.gpu

SCENES = ["box", "spheres", "test_scene.dae", "soup", "soup-normals"]


def _assert_rebuilt(dev, m, depth, what):
    rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, f"{what}: device nodes against the twin")
    assert depth == m.desc.max_leaf_depth, f"{what}: depth {depth}, the twin's {m.desc.max_leaf_depth}"


@pytest.mark.parametrize("name", SCENES)
def test_rebuild_equals_twin_fresh_scene_and_oracle(name):
    hs = rc.scene(name)
    m = bc.rebuilt(hs)
    dev = irl.IpuScene(tg._frame(hs.desc))
    _assert_rebuilt(dev, m, dev.rebuild_bvh(), name)
    assert not np.array_equal(rc.node_bytes(m.nodes), rc.node_bytes(hs.nodes))
    _assert_rebuilt(dev, m, dev.rebuild_bvh(), f"{name}, rebuilt twice")
    fresh = irl.IpuScene(tg._frame(m.desc))
    rc.assert_nodes_equal(fresh.bvh_nodes(), m.nodes, f"{name}: fresh scene's nodes")
    tg._check_queries(dev, fresh, m.desc, tg._rays(m.nodes, 50000, 3), name, oracle_n=3000)
    tg._check_renders(dev, fresh, m.desc, name, oracle=True)
    dev.close(); fresh.close()


def test_rebuild_variants_build_kernels_and_blob_scene():
    hs = rc.scene("box")
    m = bc.rebuilt(hs)
    dev = irl.IpuScene(tg._frame(hs.desc), variants=True)
    _assert_rebuilt(dev, m, dev.rebuild_bvh(), "variants build")
    fresh = irl.IpuScene(tg._frame(m.desc), variants=True)
    tg._check_renders(dev, fresh, m.desc, "variants build", kernels=(0, 1, 2, 3), oracle=False)
    blob_scene = irl.IpuScene.from_blob(irl.serialise_scene(hs.desc), hs.desc)
    _assert_rebuilt(blob_scene, m, blob_scene.rebuild_bvh(), "blob scene")
    rays = tg._rays(m.nodes, 20000, 4)
    tg.assert_bytes_equal(blob_scene.intersect(rays), fresh.intersect(rays), "blob scene: closest hit")
    assert np.array_equal(blob_scene.occluded(rays), fresh.occluded(rays))


@pytest.mark.parametrize("seed", [None, 11])
def test_prior_topology_does_not_matter(seed):
    shape = "caterpillar"                           # every leaf of the scene, one node per height, in the builder's or a shuffled order
    hs = rc.edge_scene("balanced")
    nodes, depth = rc.retopologise(hs, shape, seed=seed)
    src = rc.with_topology(hs, nodes, depth)
    dev = irl.IpuScene(src.desc)
    rc.assert_nodes_equal(dev.bvh_nodes(), nodes, "the hand-made tree")
    m = bc.rebuilt(hs)
    _assert_rebuilt(dev, m, dev.rebuild_bvh(), f"{shape} tree rebuilt")
    fresh = irl.IpuScene(m.desc)
    rays = tg._rays(m.nodes, 20000, 6)
    tg.assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), f"{shape}: closest hit")


def _device_update(torch, dev, stream, verts=None, spheres=None):
    with torch.cuda.stream(stream):
        kw = {}
        if verts is not None:
            kw["vertices"] = torch.from_numpy(np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float32)).cuda()
        if spheres is not None:
            kw["spheres"] = torch.from_numpy(np.stack([spheres[k] for k in ("x", "y", "z", "radius")], 1).astype(np.float32)).cuda()
        dev.update_geometry_device(**kw)
        stream.synchronize()


def test_sequence_update_rebuild_update_rebuild_and_back():
    """update -> rebuild -> update -> (refused update) -> rebuild -> the original arrays -> rebuild, both update entries, the rebuilds
    on a side stream. After each step the nodes equal the host reference - the refit of the PREVIOUS step's topology for an update,
    the twin for a rebuild - and the queries equal a fresh scene's. (A rebuild of a live scene cannot be refused in the middle of a
    sequence: its geometry passed the same box checks when it came in, and every box of any tree over it lies inside the same
    root box. The refused rebuild is test_refused_rebuild_leaves_the_scene_unchanged; the refusal here is an update's.)"""
    torch = pytest.importorskip("torch")
    hs = rc.scene("soup-normals")
    dev = irl.IpuScene(hs.desc)
    side = torch.cuda.Stream()

    def check(m, what):
        rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, what)
        fresh = irl.IpuScene(m.desc)
        r = tg._rays(m.nodes, 8000, 31)
        tg.assert_bytes_equal(dev.intersect(r), fresh.intersect(r), f"{what}: closest hit")
        assert np.array_equal(dev.occluded(r), fresh.occluded(r)), f"{what}: any hit"
        d = tg._frame(m.desc, 32, 32, 4)
        tg.assert_bytes_equal(tg._render(dev, d, irl.MODE_PATH_TRACE), tg._render(fresh, d, irl.MODE_PATH_TRACE), f"{what}: path trace")
        fresh.close()

    def under(prev, **arrays):                                # the host refit of `arrays` under prev's topology
        m = rc.Moved(hs, **arrays)
        m.desc.num_nodes, m.desc.max_leaf_depth = len(prev.nodes), prev.desc.max_leaf_depth
        return m.set_nodes(prev.nodes.copy()).refit()

    v1, s1, d1 = rc.jitter(hs, 61, 3.0)
    dev.update_geometry(vertices=v1, spheres=s1, discs=d1)                                    # host entry
    a = under(rc.Moved(hs, nodes=hs.nodes.copy()), verts=v1, spheres=s1, discs=d1)
    check(a, "update")
    b = bc.rebuilt(hs, verts=v1, spheres=s1, discs=d1)
    assert dev.rebuild_bvh(side.cuda_stream) == b.desc.max_leaf_depth
    check(b, "update, rebuild")
    v2 = bc.thrown_apart(hs, 62, 25.0)
    s2 = s1.copy(); s2["y"] += 20.0
    _device_update(torch, dev, side, verts=v2, spheres=s2)                                    # device entry
    c = under(b, verts=v2, spheres=s2, discs=d1)
    check(c, "update, rebuild, update")
    bad = v2.copy(); bad["x"][4] += np.float32(70000.0)
    with pytest.raises(irl.RaylibError):
        dev.update_geometry(vertices=bad)
    check(c, "after a refused update")
    e = bc.rebuilt(hs, verts=v2, spheres=s2, discs=d1)
    assert dev.rebuild_bvh(side.cuda_stream) == e.desc.max_leaf_depth
    check(e, "update, rebuild, update, rebuild")
    dev.update_geometry(vertices=hs.verts.copy(), spheres=hs.spheres.copy(), discs=hs.discs.copy())
    check(under(e), "back to the original arrays")
    f = bc.rebuilt(hs)
    assert dev.rebuild_bvh() == f.desc.max_leaf_depth
    check(f, "the original arrays, rebuilt")


def test_refused_rebuild_leaves_the_scene_unchanged():
    """A scene created from arrays its nodes do not bound (mi_scene_create checks the nodes, not the geometry against them): the
    rebuild computes boxes from the geometry and refuses, and nothing of the scene changes."""
    hs = rc.scene("soup")
    for change, word in ((("x", slice(0, 3), np.nan), "not finite"), (("x", 4, np.float32(70000.0)), "65504")):
        v = hs.verts.copy()
        v[change[0]][change[1]] = change[2]
        m = rc.Moved(hs, verts=v, nodes=hs.nodes.copy())
        dev = irl.IpuScene(m.desc)
        rays = tg._rays(hs.nodes, 10000, 9)
        before, occ = dev.intersect(rays), dev.occluded(rays)
        nodes = dev.bvh_nodes()
        with pytest.raises(irl.RaylibError) as err:
            dev.rebuild_bvh()
        assert "failed (1)" in str(err.value) and word in str(err.value), str(err.value)       # MI_ERR_INVALID_ARG
        with pytest.raises(irl.RaylibError):
            irl.build_lbvh(m.desc)                                                            # the twin refuses too
        rc.assert_nodes_equal(dev.bvh_nodes(), nodes, f"after a refused rebuild ({word})")
        tg.assert_bytes_equal(dev.intersect(rays), before, f"after a refused rebuild ({word}): closest hit")
        assert np.array_equal(dev.occluded(rays), occ)
        dev.update_geometry(vertices=hs.verts.copy())                                         # good geometry: now it rebuilds
        good = bc.rebuilt(hs)
        _assert_rebuilt(dev, good, dev.rebuild_bvh(), "after the refusal")
        dev.close()


def test_rebuild_waits_for_enqueued_render():
    torch = pytest.importorskip("torch")
    hs = rc.scene("box")
    d = tg._frame(hs.desc, 256, 256, 64)
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    want = rays.copy()
    ref = irl.IpuScene(d)
    ref.run(want, irl.MODE_PATH_TRACE)
    dev = irl.IpuScene(d)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    dev.run_device(buf.data_ptr(), rays.size, irl.MODE_PATH_TRACE, side.cuda_stream)      # enqueued, not waited for
    depth = dev.rebuild_bvh(other.cuda_stream)
    side.synchronize()
    got = buf.cpu().numpy().view(irl.TRACE_RESULT)
    tg.assert_bytes_equal(got, want, "render enqueued before the rebuild")
    _assert_rebuilt(dev, bc.rebuilt(hs), depth, "after the rebuild")


def test_counters_options_and_timing_survive():
    hs = rc.scene("box")
    d = tg._frame(hs.desc, 32, 32, 4)
    dev = irl.IpuScene(d)
    dev.set_option("rebuild_timing", 1).set_option("kernel", 0)
    tg._render(dev, d, irl.MODE_PATH_TRACE)
    before = dev.counters()
    dev.rebuild_bvh()
    assert dev.counters() == before
    ms = dev.rebuild_timing()
    assert len(ms) == 6 and all(x >= 0 for x in ms) and sum(ms) > 0
    m = bc.rebuilt(hs)
    fresh = irl.IpuScene(tg._frame(m.desc, 32, 32, 4))
    fresh.set_option("kernel", 0)
    tg.assert_bytes_equal(tg._render(dev, d, irl.MODE_PATH_TRACE), tg._render(fresh, tg._frame(m.desc, 32, 32, 4), irl.MODE_PATH_TRACE), "kernel 0 kept")


def test_one_and_two_primitives_and_an_empty_scene():
    tri = np.array([[0, 0, -5], [1, 0, -5], [0, 1, -6]], np.float32)
    for pts, n, depth in (([tri], 1, 1), ([tri, tri + 3], 3, 2)):
        hs = rc.triangles(pts)
        dev = irl.IpuScene(hs.desc)
        m = bc.rebuilt(hs)
        assert len(m.nodes) == n
        _assert_rebuilt(dev, m, dev.rebuild_bvh(), f"{len(pts)} primitives")
        assert dev.rebuild_bvh() == depth
        fresh = irl.IpuScene(m.desc)
        rays = tg._rays(m.nodes, 5000, 2)
        tg.assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), f"{len(pts)} primitives: closest hit")
        assert np.isfinite(dev.intersect(rays)["t"]).sum() > 0
    hs = rc.triangles([tri])
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = 0
    dev = irl.IpuScene(empty)
    assert dev.rebuild_bvh() == 0 and len(dev.bvh_nodes()) == 0


@pytest.mark.parametrize("name,seed", [("soup", 51), ("box-simple", 52)])
def test_geometry_level_meaning(name, seed):
    """Closest-hit t after a rebuild equals the closest hit over every primitive without a BVH; any-hit answers do not change;
    primIDs equal the pre-rebuild ones wherever the brute-force runner-up is not equal in t. Excluded by that rule for these
    seeds: 0 of 400 rays in either scene (measured on the CPU with the twin and the oracle); the cap is 1 %."""
    hs = rc.scene(name)
    v, s, d = rc.jitter(hs, 6, 1.0)
    dev = irl.IpuScene(hs.desc)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    m = bc.rebuilt(hs, verts=v, spheres=s, discs=d)
    rays = bc.seeded_rays(m.nodes, 400, seed)
    before, occ = dev.intersect(rays), dev.occluded(rays)
    dev.rebuild_bvh()
    after, occ2 = dev.intersect(rays), dev.occluded(rays)
    best, second = bc.brute_force_two(m.desc, rays)
    tg.assert_bytes_equal(best, rc.brute_force_closest(m.desc, rays), "the two brute-force closest hits")
    t = np.where(after["flags"] & irl.FLAG_ESCAPED, np.float32(np.inf), after["t"]).astype(np.float32)
    assert np.array_equal(t.view(np.uint32), best.view(np.uint32)), f"{(t != best).sum()} rays differ from brute force in t"
    assert np.array_equal(before["t"].view(np.uint32), after["t"].view(np.uint32))
    assert np.array_equal(occ, occ2), "any hit changed"
    tied = np.isfinite(best) & (best == second)
    share = tied.sum() / rays.size
    print(f"{name}: {tied.sum()} of {rays.size} rays excluded by the tie rule")
    assert share <= 0.01
    for f in ("primID", "geomID"):
        assert np.array_equal(before[f][~tied], after[f][~tied]), f"{f} changed without a tie"
    assert np.isfinite(best).sum() > 100


def test_purpose_rebuilt_tree_is_cheaper_than_refitted_tree_after_large_motion():
    """Eight interleaved meshes of a soup thrown apart (refit_cases.rigid per mesh): the refitted tree's boxes span the gaps. The
    oracle's box tests per cast (48 x 48 x 4 path trace, CPU) on the device's own nodes: 2100.7 on the refitted tree, 83.2 on the
    rebuilt one for this seed (the direction is what is asserted)."""
    hs = rc.soup(77, False, n_tris=2000, n_meshes=8)
    v = bc.thrown_apart(hs, 1, 30.0)
    dev = irl.IpuScene(hs.desc)
    dev.update_geometry(vertices=v)
    refit = rc.Moved(hs, verts=v).set_nodes(dev.bvh_nodes())
    cost_refit = bc.nodes_visited_per_cast(refit.desc)
    depth = dev.rebuild_bvh()
    m = bc.rebuilt(hs, verts=v)
    _assert_rebuilt(dev, m, depth, "thrown apart")
    reb = rc.Moved(hs, verts=v).set_nodes(dev.bvh_nodes())
    reb.desc.max_leaf_depth = depth
    cost_rebuilt = bc.nodes_visited_per_cast(reb.desc)
    print(f"box tests per cast: refitted {cost_refit:.1f}, rebuilt {cost_rebuilt:.1f}")
    assert cost_rebuilt < cost_refit


def test_large_soup_rebuild():
    import os
    old = os.environ.get("MI_BVH_REINSERT")
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the fixture builds in seconds
    try:
        hs = rc.soup(7, False, n_tris=1 << 20, n_meshes=64, spread=200.0)
    finally:
        if old is None:
            del os.environ["MI_BVH_REINSERT"]
        else:
            os.environ["MI_BVH_REINSERT"] = old
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, 13, 0.5)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    m = bc.rebuilt(hs, verts=v, spheres=s, discs=d)
    _assert_rebuilt(dev, m, dev.rebuild_bvh(), "1 M-triangle soup")
    fresh = irl.IpuScene(m.desc)
    rays = tg._rays(m.nodes, 20000, 10)
    tg.assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), "1 M-triangle soup: closest hit")
    assert np.array_equal(dev.occluded(rays), fresh.occluded(rays))
    v2, s2, d2 = rc.jitter(hs, 14, 0.5)                      # and the refit after it, on the rebuilt topology
    dev.update_geometry(vertices=v2, spheres=s2, discs=d2)
    m2 = rc.Moved(hs, verts=v2, spheres=s2, discs=d2)
    m2.desc.num_nodes, m2.desc.max_leaf_depth = len(m.nodes), m.desc.max_leaf_depth
    rc.assert_nodes_equal(dev.bvh_nodes(), m2.set_nodes(m.nodes.copy()).refit().nodes, "1 M-triangle soup: update after the rebuild")


def test_group_replicas_rebuild():
    hs = rc.scene("box")
    d = tg._frame(hs.desc, 64, 64, 8)
    g = irl.IpuGroup(d, [0, 0])
    for sc in g.scenes():
        sc.rebuild_bvh()
    m = bc.rebuilt(hs)
    single = irl.IpuScene(tg._frame(m.desc, 64, 64, 8))
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    want = rays.copy()
    g.run(rays, irl.MODE_PATH_TRACE)
    single.run(want, irl.MODE_PATH_TRACE)
    tg.assert_bytes_equal(rays, want, "group of two rebuilt replicas")
    g.close()
