"""New contents for a live scene on the GPU (pytest -m gpu): mi_scene_set_geometry / mi_scene_set_geometry_device replace a scene's
geometry list, meshes, primitives and materials - every count may change - and build the BVH of the new contents on the device.
Afterwards the device nodes equal the host twin's (mi_build_lbvh_compact) byte for byte and every query and render equals - bit for
bit - a scene freshly created from the new arrays and those nodes, while options, counters, the NIF environment and the render
parameters stay. Every scene here is created with set_geometry_cases.render_params: a live scene keeps its own."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import rebuild_cases as bc
import refit_cases as rc
import set_geometry_cases as sg
import test_refit_gpu as tg

pytestmark = pytest.mark.gpu

FRAME = (32, 32, 4)


def _query_rays(nodes, n, seed):
    if len(nodes):
        return tg._rays(nodes, n, seed)
    rng = np.random.default_rng(seed)                     # an empty scene has no root box: rays round the origin, all of them miss
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return qb.make_rays(rng.uniform(-5, 5, (n, 3)).astype(np.float32), d.astype(np.float32))


def _nodes_equal(got, want, what):
    if len(want) == 0:                                    # (refit_cases.assert_nodes_equal compares rows: it needs one)
        assert len(got) == 0, f"{what}: {len(got)} nodes, want none"
    else:
        rc.assert_nodes_equal(got, want, what)


def _check(dev, c, got_depth, what, rays=20000, oracle=False, renders=True, variants=False, kernels=(1,)):
    """dev holds contents c: nodes and depth are the twin's; queries and frames equal a fresh scene's from the twin's nodes.
    Returns the casts this made on dev (counters go on counting)."""
    desc, nodes, depth = c.twin()
    _nodes_equal(dev.bvh_nodes(), nodes, f"{what}: device nodes against the host twin")
    assert got_depth == depth == dev.live_stats()["max_leaf_depth"], f"{what}: depth {got_depth}, twin {depth}"
    assert len(nodes) == (2 * c.num_prims - 1 if c.num_prims else 0)
    before = dev.counters()["casts"]
    fresh = irl.IpuScene(desc, variants=variants)
    tg._check_queries(dev, fresh, desc, _query_rays(nodes, rays, 3), what, oracle_n=3000 if oracle else 0)
    if renders:
        tg._check_renders(dev, fresh, desc, what, kernels=kernels, oracle=False, frame=FRAME)
    fresh.close()
    return dev.counters()["casts"] - before


# ------------------------------------------------------------------------------------------------------
# 1  equality, pair by pair
# ------------------------------------------------------------------------------------------------------
PAIRS = [("box-simple", "soup-normals", False),           # small to large, no normals to normals
         ("soup-normals", "box-simple", False),           # large to small, normals to none
         ("box-simple", "spheres", False),                # meshes only to a sphere and disc mix
         ("spheres", "test_scene.dae", False),
         ("soup", "test_scene.dae", True),                # against the oracle too
         ("test_scene.dae", "soup", False)]


@pytest.mark.parametrize("first,second,oracle", PAIRS)
def test_set_geometry_equals_fresh_scene(first, second, oracle):
    a, b = sg.named(first), sg.named(second)
    assert a.num_prims != b.num_prims
    dev = irl.IpuScene(a.twin()[0])
    depth = dev.set_geometry(b.desc)
    _check(dev, b, depth, f"{first} -> {second}", oracle=oracle)
    st = dev.live_stats()
    assert st["geometry_sets"] == 1 and st["host_derivations"] == 0
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 2  the hand-made tables through the device entry
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", [k for k in sg.HAND_MADE if k not in ("empty scene", "one sphere", "one triangle")])
def test_hand_made_tables_from_torch_tensors(label):
    pytest.importorskip("torch")
    c = sg.hand(sg.HAND_MADE[label])
    a = sg.named("box-simple")                            # (kept: its desc points into it)
    dev = irl.IpuScene(a.twin()[0])
    depth = dev.set_geometry_device(c.desc, **c.tensors())
    _check(dev, c, depth, label, rays=8000, renders=False)
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3  one scene through a sequence
# ------------------------------------------------------------------------------------------------------
def test_one_scene_through_a_sequence():
    torch = pytest.importorskip("torch")
    steps = [sg.named("box"), sg.named("soup-normals"), sg.hand([]), sg.hand(sg.HAND_MADE["one sphere"]), sg.named("test_scene.dae"),
             sg.named("box")]
    start = sg.hand(sg.HAND_MADE["one triangle"])
    dev = irl.IpuScene.from_geometry(start.desc)
    side = torch.cuda.Stream()
    casts = dev.counters()["casts"]
    assert casts == 0
    for k, c in enumerate(steps):
        what = f"step {k} ({c.name})"
        if k % 2:
            t = c.tensors()
            depth = dev.set_geometry_device(c.desc, stream=side.cuda_stream, **t)      # (renders and queries below: the null stream)
        else:
            depth = dev.set_geometry(c.desc)
        casts += _check(dev, c, depth, what, rays=6000)
        st = dev.live_stats()
        assert st["geometry_sets"] == k + 2 and st["host_derivations"] == 0, (what, st)
        assert st["max_leaf_depth"] == c.twin()[2]
        # a refit from the device-made tables, at the new size
        j = c.jittered(100 + k)
        dev.update_geometry(**j.update_args())
        moved = irl.SceneDesc.from_buffer_copy(j.desc)
        topo = np.ascontiguousarray(c.twin()[1])
        moved.bvh_nodes, moved.num_nodes = (topo.ctypes.data if topo.size else None), len(topo)
        want = irl.refit_compact_bvh(moved) if topo.size else topo
        _nodes_equal(dev.bvh_nodes(), want, f"{what}: update after set_geometry against the host refit")
        assert dev.live_stats()["host_derivations"] == 0
        # ... and the rebuild of the moved arrays is the twin of the moved arrays; again: the identity
        d2 = dev.rebuild_bvh()
        _nodes_equal(dev.bvh_nodes(), j.twin()[1], f"{what}: rebuild after the update")
        assert d2 == j.twin()[2]
        dev.rebuild_bvh()
        _nodes_equal(dev.bvh_nodes(), j.twin()[1], f"{what}: rebuild twice")
    # set_geometry right before a rebuild: the identity
    last = steps[-1]
    dev.set_geometry(last.desc)
    dev.rebuild_bvh()
    _nodes_equal(dev.bvh_nodes(), last.twin()[1], "rebuild right after set_geometry")
    assert dev.counters()["casts"] == casts, "the counters go on counting across set_geometry"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4  a scene without a host BVH; the blob path; the variants build
# ------------------------------------------------------------------------------------------------------
def test_from_geometry_blob_scene_and_variants_build():
    c = sg.named("box")
    desc, nodes, depth = c.twin()
    dev = irl.IpuScene.from_geometry(c.desc)
    _check(dev, c, dev.live_stats()["max_leaf_depth"], "from_geometry")
    assert dev.live_stats()["host_derivations"] == 0
    dev.close()
    # a scene made from the serialised blob takes new contents the same way
    a = sg.named("box-simple")
    blob_scene = irl.IpuScene.from_blob(irl.serialise_scene(a.twin()[0]), a.twin()[0])
    _check(blob_scene, c, blob_scene.set_geometry(c.desc), "blob scene", renders=False)
    blob_scene.close()
    # the variants build: every kernel family on the new contents
    dev = irl.IpuScene(a.twin()[0], variants=True)
    _check(dev, c, dev.set_geometry(c.desc), "variants build", rays=4000, variants=True, kernels=(0, 1, 2, 3))
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 5  what stays
# ------------------------------------------------------------------------------------------------------
def test_options_and_auto_rebuild_baseline_stay():
    import live_cases as lc
    hs, thrown = lc.purpose()                                 # the soup of eight meshes, and its meshes thrown apart
    c = sg.Contents(hs.desc, "purpose")
    nodes = np.ascontiguousarray(c.twin()[1])
    t = sg.Contents(hs.desc, "purpose, thrown"); t.a["mesh_verts"][...] = thrown
    degraded = irl.SceneDesc.from_buffer_copy(t.desc)          # the thrown arrays under the tree of the unthrown ones
    degraded.bvh_nodes, degraded.num_nodes, degraded.max_leaf_depth = nodes.ctypes.data, len(nodes), c.twin()[2]
    refit = irl.refit_compact_bvh(degraded)
    degraded.bvh_nodes = refit.ctypes.data
    est_new, est_degraded = irl.bvh_cost(nodes)["estimate"], irl.bvh_cost(refit)["estimate"]
    assert est_degraded > lc.RATIO * est_new                   # host twins: 12 158 against 1 819 - the throw passes 3 x the new tree's baseline
    dev = irl.IpuScene(degraded)
    dev.set_option("full_stats", 1).set_option("auto_rebuild", lc.RATIO)
    dev.update_geometry(vertices=thrown)                       # the old baseline: the degraded tree's own estimate - against it nothing fires
    assert dev.live_stats()["auto_rebuilds"] == 0
    dev.set_geometry(c.desc)
    dev.intersect(tg._rays(nodes, 4000, 5))
    cnt = dev.counters()
    assert cnt["nodes_visited"] > 0 and cnt["leaf_tests"] > 0, cnt          # full_stats still holds
    dev.update_geometry(vertices=thrown)                       # the same arrays again: against the NEW tree's baseline they are a throw
    st = dev.live_stats()
    assert st["auto_rebuilds"] == 1 and st["updates_applied"] == 2 and st["geometry_sets"] == 1, st
    _nodes_equal(dev.bvh_nodes(), t.twin()[1], "the automatic rebuild's nodes")
    dev.close()


def test_nif_environment_stays():
    import nif_probe as npb
    ks, bs, relu = npb.random_weights(np.random.default_rng(9))
    a, b = sg.named("box-simple", size=48), sg.named("spheres", size=48)
    desc = b.twin()[0]

    def nif_frame(sc):
        rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
        irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
        sc.run(rays, irl.MODE_PATH_TRACE)
        return rays

    dev = irl.IpuScene(a.twin()[0])
    dev.setNif(ks, bs, relu, npb.EMBED, 1.0, np.zeros(3, np.float32), False)
    nif_frame(dev)
    dev.set_geometry(b.desc)
    got = nif_frame(dev)
    fresh = irl.IpuScene(desc)
    fresh.setNif(ks, bs, relu, npb.EMBED, 1.0, np.zeros(3, np.float32), False)
    want = nif_frame(fresh)
    assert (got["h"]["flags"] & irl.FLAG_ESCAPED).any(), "no ray reached the environment"
    # (two scenes, one network, one kernel, the same launches: the same bits - as test_nif_render_sample_batching_is_order_exact asserts)
    tg.assert_bytes_equal(got, want, "NIF render after set_geometry against a fresh scene with the same NIF")
    dev.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------
# 6  ordering
# ------------------------------------------------------------------------------------------------------
def test_set_geometry_waits_for_enqueued_render():
    torch = pytest.importorskip("torch")
    a, b = sg.named("box", size=64, spp=16), sg.named("soup-normals", size=64, spp=16)
    da, db = a.twin()[0], b.twin()[0]
    rays = np.zeros(da.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(da), rays.ctypes.data, rays.size)
    want_old, want_new = rays.copy(), rays.copy()
    ref = irl.IpuScene(da); ref.run(want_old, irl.MODE_PATH_TRACE); ref.close()
    ref = irl.IpuScene(db); ref.run(want_new, irl.MODE_PATH_TRACE); ref.close()
    dev = irl.IpuScene(da)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    buf2 = buf.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev.run_device(buf.data_ptr(), rays.size, irl.MODE_PATH_TRACE, side.cuda_stream)      # enqueued, not waited for
    dev.set_geometry(b.desc)
    side.synchronize()
    tg.assert_bytes_equal(buf.cpu().numpy().view(irl.TRACE_RESULT), want_old, "render enqueued before set_geometry")
    dev.run_device(buf2.data_ptr(), rays.size, irl.MODE_PATH_TRACE, side.cuda_stream)
    side.synchronize()
    tg.assert_bytes_equal(buf2.cpu().numpy().view(irl.TRACE_RESULT), want_new, "render after set_geometry")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 7  refusals leave the scene unchanged
# ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_unchanged():
    pytest.importorskip("torch")
    a = sg.named("soup")
    dev = irl.IpuScene(a.twin()[0])
    nodes = a.twin()[1]
    rays = tg._rays(nodes, 10000, 9)
    before, occ = dev.intersect(rays), dev.occluded(rays)
    stats = dev.live_stats()

    def refused(call, words, what):
        with pytest.raises(irl.RaylibError) as e:
            call()
        assert "failed (1)" in str(e.value) and words in str(e.value), (what, str(e.value))          # MI_ERR_INVALID_ARG
        _nodes_equal(dev.bvh_nodes(), nodes, f"after refusing {what}")
        tg.assert_bytes_equal(dev.intersect(rays), before, f"after refusing {what}: closest hit")
        assert np.array_equal(dev.occluded(rays), occ), what
        st = dev.live_stats()
        assert (st["updates_applied"], st["geometry_sets"]) == (stats["updates_applied"], stats["geometry_sets"]), (what, st)

    def fresh_refuses(c, words):                              # ... exactly what create refuses, in its words
        with pytest.raises(irl.RaylibError) as e:
            d = irl.SceneDesc.from_buffer_copy(c.desc)
            filler = np.zeros(max(2 * c.num_prims - 1, 1), irl.BVH_NODE)
            d.bvh_nodes, d.num_nodes = filler.ctypes.data, (2 * c.num_prims - 1)
            irl.IpuScene(d)
        assert words in str(e.value), str(e.value)

    b = sg.named("test_scene.dae")
    m = 0
    b.a["mesh_tris"][3 * (int(b.a["mesh_info"][m]["firstIndex"]) + 1) + 2] = b.a["mesh_info"][m]["numVertices"]
    refused(lambda: dev.set_geometry_device(b.desc, **b.tensors()), "triangle vertex index out of range", "a triangle index (device entry)")
    fresh_refuses(b, "triangle vertex index out of range")
    def twin_refuses(c, words):                               # ... and what the host twin of the build refuses, in its words
        with pytest.raises(irl.RaylibError) as e:
            irl.build_lbvh(c.desc)
        assert words in str(e.value), str(e.value)

    # (a vertex at +inf makes its box's extent +inf: above 65504, the builder's check - the twin's and the device's alike; "not finite"
    # is what a NaN box is called, test_rebuild_gpu)
    half = "Cannot compress BVH bounds into fp16 (half)"
    b = sg.named("test_scene.dae"); b.a["mesh_verts"]["y"][7] = np.inf
    refused(lambda: dev.set_geometry(b.desc), half, "a vertex at +inf")
    twin_refuses(b, half)
    b = sg.named("test_scene.dae"); b.a["mesh_verts"]["x"][4] += np.float32(70000.0)
    refused(lambda: dev.set_geometry(b.desc), "65504", "an extent above 65504")
    twin_refuses(b, half)
    b = sg.named("soup-normals"); b.desc.num_normals -= 1
    refused(lambda: dev.set_geometry(b.desc), "normals must be absent or one per vertex", "num_normals != num_verts")
    fresh_refuses(b, "normals must be absent or one per vertex")
    b = sg.named("test_scene.dae"); b.a["mat_ids"][0] = b.desc.num_materials
    refused(lambda: dev.set_geometry(b.desc), "material index out of range", "a material index")
    fresh_refuses(b, "material index out of range")
    b = sg.named("test_scene.dae"); b.desc.mesh_verts = None
    refused(lambda: dev.set_geometry(b.desc), "mesh arrays are null", "a null mesh_verts with a count")
    fresh_refuses(b, "mesh arrays are null")
    # a correct call after the refusals lands
    b = sg.named("test_scene.dae")
    _check(dev, b, dev.set_geometry(b.desc), "after the refusals", rays=6000, renders=False)
    dev.close()
