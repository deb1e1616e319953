"""Point queries on the GPU (pytest -m gpu): mi_point_query / mi_point_query_device against the host twin mi_point_query_host,
byte for byte, for both kinds - mixed point sets, the launch-shape edges, the counters, live scenes (update, rebuild, new
contents), torch tensors on a stream, destruction behind an enqueued query, host batches, the variants build."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc

pytestmark = pytest.mark.gpu

CLOSEST, WITHIN = irl.POINT_CLOSEST, irl.POINT_WITHIN
SCENES = ["box", "spheres", "soup", "soup-normals"]
N = 20000

_cases = {}


def _surface_points(hs):
    """Hit points of the scene's camera rays: positions on surfaces."""
    dev = irl.IpuScene(hs.desc)
    rays = qb.primary_rays(hs)
    _, p, _ = qb.hit_points(rays, dev.intersect(rays))
    dev.close()
    return p


def _case(name):
    """(scene, points, the twin's CLOSEST result, its WITHIN result, its visits for CLOSEST and for WITHIN), computed once."""
    if name not in _cases:
        hs = pc.scene(name)
        pts = pc.mixed_points(hs, N, seed=SCENES.index(name) + 11, surface=_surface_points(hs))
        # a few queries that are written without a walk
        pts["x"][7] = np.nan; pts["z"][8] = np.inf; pts["radius"][9] = np.nan; pts["radius"][10] = -1.0
        want, vc = irl.point_query_host(hs.desc, CLOSEST, pts)
        inside, vw = irl.point_query_host(hs.desc, WITHIN, pts)
        _cases[name] = (hs, pts, want, inside, vc, vw)
    return _cases[name]


def _device_closest(dev, pts):
    """CLOSEST through the device entry on torch memory (the host entry is checked against it in the batch test)."""
    import torch
    t_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    out = torch.zeros(pts.size * 32, dtype=torch.uint8, device="cuda")
    dev.point_query_device(CLOSEST, t_pts.data_ptr(), out.data_ptr(), pts.size)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(irl.POINT_HIT)


@pytest.mark.parametrize("name", SCENES)
def test_device_equals_twin_byte_for_byte(name):
    hs, pts, want, inside, vc, vw = _case(name)
    found = want["primID"] != irl.INVALID_PRIM
    assert 0.2 < found.mean() < 0.95 and np.array_equal(inside, found)
    assert (want["dist"][found] == 0).sum() > N // 100           # points exactly on vertices / disc centres
    dev = irl.IpuScene(hs.desc)
    pc.assert_bytes_equal(dev.closest_points(pts), want, f"{name}: CLOSEST, host entry")
    pc.assert_bytes_equal(_device_closest(dev, pts), want, f"{name}: CLOSEST, device entry")
    got = dev.within(pts)
    assert np.array_equal(got, inside), f"{name}: WITHIN: {(got != inside).sum()} points differ"
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    dev.close()


def test_launch_shape_edges():
    hs, pts, want, inside, _, _ = _case("soup")
    dev = irl.IpuScene(hs.desc)
    assert dev.closest_points(pts[:0]).size == 0 and dev.within(pts[:0]).size == 0
    for n in (1, 63, 64, 65, 255, 256, 257):
        for first in (0, 4099):
            sl = slice(first, first + n)
            pc.assert_bytes_equal(dev.closest_points(pts[sl]), want[sl], f"CLOSEST, n = {n} from {first}")
            assert np.array_equal(dev.within(pts[sl]), inside[sl]), f"WITHIN, n = {n} from {first}"
    dev.close()


@pytest.mark.parametrize("name", ["box", "soup-normals"])
def test_full_stats_counts_box_tests_and_primitive_evaluations(name):
    hs, pts, want, inside, vc, vw = _case(name)
    dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    dev.reset_counters()
    pc.assert_bytes_equal(dev.closest_points(pts), want, f"{name}: instrumented CLOSEST")
    c = dev.counters()
    assert (c["casts"], c["paths"]) == (0, 0)
    assert (c["nodes_visited"], c["leaf_tests"]) == (vc["box_tests"], vc["prim_evals"])
    dev.reset_counters()
    assert np.array_equal(dev.within(pts), inside)
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (0, vw["box_tests"], vw["prim_evals"], 0)
    assert vw["box_tests"] < vc["box_tests"]                      # WITHIN stops at the first accept
    dev.close()


def test_live_scene_update_rebuild_and_new_contents():
    import torch
    hs, pts, want, inside, _, _ = _case("soup")
    dev = irl.IpuScene(hs.desc)
    rng = np.random.default_rng(3)
    moved = hs.verts.copy()
    for c in "xyz":
        moved[c] += rng.normal(scale=0.4, size=moved.size).astype(np.float32)
    sph = hs.spheres.copy(); sph["x"] += 2.5; sph["radius"] = 2.0
    dsc = hs.discs.copy(); dsc["cy"] += 1.0

    # a query enqueued before the update sees the old geometry
    many = np.tile(pts, 8)
    t_pts = torch.from_numpy(many.view(np.uint8).copy()).cuda()
    out = torch.zeros(many.size * 32, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    dev.point_query_device(CLOSEST, t_pts.data_ptr(), out.data_ptr(), many.size, st.cuda_stream)
    dev.update_geometry(vertices=moved, spheres=sph, discs=dsc)
    st.synchronize()
    pc.assert_bytes_equal(out.cpu().numpy().view(irl.POINT_HIT), np.tile(want, 8), "enqueued before the update: the old geometry")

    def check(desc, what):
        w, _ = irl.point_query_host(desc, CLOSEST, pts)
        pc.assert_bytes_equal(dev.closest_points(pts), w, f"{what}: CLOSEST")
        wi, _ = irl.point_query_host(desc, WITHIN, pts)
        assert np.array_equal(dev.within(pts), wi), f"{what}: WITHIN"
        return w

    after = check(pc.with_nodes(hs.desc, dev.bvh_nodes(), mesh_verts=moved, spheres=sph, discs=dsc), "after update_geometry")
    assert (after["dist"] != want["dist"]).mean() > 0.3            # (the update moved something)
    refit_nodes = dev.bvh_nodes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != refit_nodes.tobytes()
    check(pc.with_nodes(hs.desc, dev.bvh_nodes(), mesh_verts=moved, spheres=sph, discs=dsc), "after rebuild_bvh")
    other = pc.soup(77, True, n_tris=250)                           # other counts, vertex normals appear
    dev.set_geometry(other.desc)
    assert len(dev.bvh_nodes()) == 2 * 252 - 1
    check(pc.with_nodes(other.desc, dev.bvh_nodes()), "after set_geometry")
    dev.close()


def test_torch_nearest_on_a_non_default_stream():
    import torch
    hs, pts, want, inside, _, _ = _case("soup-normals")
    dev = irl.IpuScene(hs.desc)
    host = dev.closest_points(pts)
    pc.assert_bytes_equal(host, want, "host entry")
    p = torch.from_numpy(np.stack([pts[c] for c in "xyz"], 1).copy()).cuda()
    r = torch.from_numpy(pts["radius"].copy()).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        res = dev.nearest(p, r)
        w = dev.nearest(p, r, within=True)
    st.synchronize()
    assert np.array_equal(res["dist"].cpu().numpy().view(np.uint32), host["dist"].view(np.uint32))
    assert np.array_equal(res["prim_id"].cpu().numpy().view(np.uint32), host["primID"])
    assert np.array_equal(res["geom_id"].cpu().numpy(), host["geomID"].astype(np.int16).astype(np.int32))
    q = np.stack([host["point"][c] for c in "xyz"], 1)
    assert np.array_equal(res["point"].cpu().numpy().view(np.uint32), q.view(np.uint32))
    assert np.array_equal(res["bary"].cpu().numpy().view(np.uint32), np.stack([host["b1"], host["b2"]], 1).view(np.uint32))
    assert np.array_equal(w["within"].cpu().numpy(), inside)
    # a scalar radius (the default: +inf)
    res2 = dev.nearest(p[:1000])
    torch.cuda.synchronize()
    plain = pts[:1000].copy(); plain["radius"] = np.inf
    assert np.array_equal(res2["prim_id"].cpu().numpy().view(np.uint32), dev.closest_points(plain)["primID"])
    dev.close()


def test_destroy_waits_for_an_enqueued_point_query():
    """A scene destroyed right after mi_point_query_device enqueued a large batch: destroy waits for it (the slot's lastWork
    event), and the batch's results are complete."""
    import torch
    hs, pts, want, _, _, _ = _case("box")
    many = np.tile(pts, 50)                                         # a million points
    t_pts = torch.from_numpy(many.view(np.uint8).copy()).cuda()
    out = torch.zeros(many.size * 32, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    dev = irl.IpuScene(hs.desc)
    dev.point_query_device(CLOSEST, t_pts.data_ptr(), out.data_ptr(), many.size, st.cuda_stream)
    dev.close()
    st.synchronize()
    pc.assert_bytes_equal(out.cpu().numpy().view(irl.POINT_HIT), np.tile(want, 50), "destroyed behind its point query")


def test_host_batches_give_the_same_bytes():
    hs, pts, want, inside, _, _ = _case("soup")
    dev = irl.IpuScene(hs.desc)
    for batch in (1000, 4096, 7):
        dev.setRayBatch(batch)
        m = N if batch != 7 else 300
        pc.assert_bytes_equal(dev.closest_points(pts[:m]), want[:m], f"host batches of {batch}")
        assert np.array_equal(dev.within(pts[:m]), inside[:m]), f"host batches of {batch}, WITHIN"
    dev.close()


def test_variants_build_gives_the_same_bytes():
    hs, pts, want, inside, vc, _ = _case("soup-normals")
    dev = irl.IpuScene(hs.desc, variants=True)
    pc.assert_bytes_equal(dev.closest_points(pts), want, "variants build: CLOSEST")
    assert np.array_equal(dev.within(pts), inside)
    dev.set_option("full_stats", 1)
    dev.reset_counters()
    pc.assert_bytes_equal(dev.closest_points(pts), want, "variants build: instrumented CLOSEST")
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (0, vc["box_tests"], vc["prim_evals"])
    dev.close()
