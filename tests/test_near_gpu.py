"""Neighbour lists on the GPU (pytest -m gpu): mi_near_offsets* / mi_near_fill* against the host twins mi_near_offsets_host /
mi_near_fill_host, byte for byte - the full lists and the K nearest, the counters, the prefix sum at its tile edges, host batches,
the capacity guard, live scenes (rebuild, new tree, update), the variants build, torch tensors on a stream, and ordering against
an update."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import near_cases as nc
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


def _device_offsets(dev, pts, stream=0):
    import torch
    t_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    t_off = torch.full((pts.size + 1,), -1, dtype=torch.int64, device="cuda")
    dev.near_offsets_device(t_pts.data_ptr(), t_off.data_ptr(), pts.size, stream)
    torch.cuda.synchronize()
    return t_off.cpu().numpy().view(np.uint64)


def _device_fill(dev, pts, offsets, total, capacity=None):
    """The device entry into a sentinel buffer of `total` (+ 64) records; returns the whole buffer."""
    import torch
    t_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    t_off = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
    t_buf = torch.from_numpy(nc.sentinel_buffer(total).view(np.uint8).copy()).cuda()
    dev.near_fill_device(t_pts.data_ptr(), t_off.data_ptr(), t_buf.data_ptr(), total if capacity is None else capacity, pts.size)
    torch.cuda.synchronize()
    return t_buf.cpu().numpy().view(irl.NEIGHBOUR)


def _sentinels(buf, first):
    return np.all(buf[first:] == np.array(nc.SENTINEL, irl.NEIGHBOUR))


# ------------------------------------------------------------------------------------------------------
# 1. the device against the twin
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.CASES)
def test_device_equals_twin_byte_for_byte(name):
    hs, pts, offsets, recs, _, _ = nc.twin(name)
    dev = irl.IpuScene(hs.desc)
    got = dev.neighbours(pts)
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.NEIGHBOUR and got[0][0] == 0 and got[0][-1] == got[1].size
    nc.assert_same(got, (offsets, recs), f"{name}: host entries")
    assert np.array_equal(_device_offsets(dev, pts), offsets), f"{name}: offsets, device entry"
    buf = _device_fill(dev, pts, offsets, recs.size)
    pc.assert_bytes_equal(buf[:recs.size], recs, f"{name}: fill, device entry")
    assert _sentinels(buf, recs.size)
    for k in nc.KS:
        want, _ = nc.twin_k(name, k)
        pc.assert_bytes_equal(dev.k_nearest(pts, k), want, f"{name}: the {k} nearest, host entry")
        buf = _device_fill(dev, pts, nc.k_offsets(pts.size, k), pts.size * k)
        pc.assert_bytes_equal(buf[:pts.size * k], want.reshape(-1), f"{name}: the {k} nearest, device entry")
        assert _sentinels(buf, pts.size * k)
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    dev.close()


def test_k_nearest_with_an_infinite_radius_and_an_empty_scene():
    hs, pts = nc.scene("soup"), nc.points_of("soup").copy()
    pts["radius"] = np.inf
    dev = irl.IpuScene(hs.desc)
    for k in nc.KS:
        want, _ = nc.twin_k("soup", k, np.inf)
        pc.assert_bytes_equal(dev.k_nearest(pts, k), want, f"soup, radius inf: the {k} nearest")
    dev.close()
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = empty.num_spheres = empty.num_discs = 0
    dev = irl.IpuScene(empty)
    offsets, recs = dev.neighbours(pts)
    assert not offsets.any() and recs.size == 0
    pc.assert_bytes_equal(dev.k_nearest(pts[:50], 2).reshape(-1), np.concatenate([nc.records([], i, 2) for i in range(50)]), "an empty scene pads")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 2. counters
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "box"])
def test_full_stats_counts_box_tests_and_primitive_evaluations(name):
    hs, pts, offsets, recs, vo, vf = nc.twin(name)
    want4, v4 = nc.twin_k(name, 4)
    dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    for call, v in ((lambda: dev.near_offsets(pts), vo), (lambda: dev.near_fill(pts, offsets, nc.sentinel_buffer(recs.size), recs.size), vf),
                    (lambda: dev.k_nearest(pts, 4), v4)):
        dev.reset_counters()
        call()
        c = dev.counters()
        assert (c["casts"], c["paths"]) == (0, 0)
        assert (c["nodes_visited"], c["leaf_tests"]) == (v["box_tests"], v["prim_evals"])
    pc.assert_bytes_equal(dev.k_nearest(pts, 4), want4, f"{name}: the instrumented build's 4 nearest")
    nc.assert_same(dev.neighbours(pts), (offsets, recs), f"{name}: the instrumented build's lists")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. the prefix sum's tiles, host batches
# ------------------------------------------------------------------------------------------------------
_tiled = {}


def _tiled_case():
    """The soup's points six times over (2400: more than one tile of the prefix sum), with the twin's lists."""
    if not _tiled:
        hs = nc.scene("soup")
        pts = np.tile(nc.points_of("soup"), 6)
        offsets, _ = irl.near_offsets_host(hs.desc, pts)
        recs, _ = irl.near_fill_host(hs.desc, pts, offsets)
        _tiled["case"] = (hs, pts, offsets, recs)
    return _tiled["case"]


def test_scan_wiring_at_the_tile_edges():
    hs, pts, offsets, recs = _tiled_case()
    dev = irl.IpuScene(hs.desc)
    for n in (1, 2047, 2048, 2049):
        want = offsets[:n + 1]
        assert np.array_equal(dev.near_offsets(pts[:n]), want), f"host entry, n = {n}"
        assert np.array_equal(_device_offsets(dev, pts[:n]), want), f"device entry, n = {n}"
    nc.assert_same(dev.neighbours(pts[:2049]), (offsets[:2050], recs[:int(offsets[2049])]), "2049 points")
    dev.close()


def test_host_batches_give_the_same_bytes_and_global_point_indices():
    hs, pts, offsets, recs = _tiled_case()
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(1000)
    got = dev.neighbours(pts)
    nc.assert_same(got, (offsets, recs), "batches of 1000")
    assert np.array_equal(got[1]["point"], np.repeat(np.arange(pts.size, dtype=np.uint32), np.diff(offsets).astype(np.int64)))
    want4, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(pts.size, 4))
    got4 = dev.k_nearest(pts, 4)
    pc.assert_bytes_equal(got4.reshape(-1), want4, "the 4 nearest in batches of 1000")
    assert np.array_equal(got4["point"], np.repeat(np.arange(pts.size, dtype=np.uint32), 4).reshape(-1, 4))
    dev.setRayBatch(7)
    nc.assert_same(dev.neighbours(pts[:300]), (offsets[:301], recs[:int(offsets[300])]), "batches of 7")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. bounds
# ------------------------------------------------------------------------------------------------------
def test_nothing_is_written_outside_a_segment_or_past_capacity():
    hs, pts, offsets, recs, _, _ = nc.twin("soup")
    total = recs.size
    dev = irl.IpuScene(hs.desc)
    for capacity in (total, total - 1, total // 2, 0):
        want, _ = irl.near_fill_host(hs.desc, pts, offsets, capacity=capacity, hits=nc.sentinel_buffer(total))
        assert _sentinels(want, capacity)
        buf = nc.sentinel_buffer(total)
        dev.near_fill(pts, offsets, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, capacity {capacity}"
        assert _device_fill(dev, pts, offsets, total, capacity).tobytes() == want.tobytes(), f"device entry, capacity {capacity}"
    # offsets that do not ascend: the segments of tests/test_near_host.py - a K far above the count cut at capacity, decreasing
    # pairs, len 0 and 1, the 25 and the 3 nearest of more
    counts = np.diff(offsets).astype(np.int64)
    many, few, none = np.nonzero(counts > 25)[0], np.nonzero((counts >= 3) & (counts < 25))[0], np.nonzero(counts == 0)[0]
    some = pts[[few[0], many[1], many[2], many[3], few[1], many[0], many[4], none[0]]]
    odd = np.array([70, 2 ** 40, 30, 31, 31, 0, 25, 28, 27], np.uint64)
    for capacity in (100, 85, 20, 0):
        want, _ = irl.near_fill_host(hs.desc, some, odd, capacity=capacity, hits=nc.sentinel_buffer(100))
        assert _sentinels(want, capacity) and (capacity == 0 or not _sentinels(want, 0))
        buf = nc.sentinel_buffer(100)
        dev.near_fill(some, odd, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, offsets that do not ascend, capacity {capacity}"
        assert _device_fill(dev, some, odd, 100, capacity).tobytes() == want.tobytes(), f"device entry, offsets that do not ascend, capacity {capacity}"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. live scenes
# ------------------------------------------------------------------------------------------------------
def _margin_lists(offsets, recs, margin):
    return [recs[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in np.nonzero(margin)[0]]


def test_the_bytes_do_not_depend_on_the_tree_on_points_with_margin():
    hs, pts, offsets, recs, _, _ = nc.twin("soup")
    _, _, _, margin = nc.soup_margin()
    want = _margin_lists(offsets, recs, margin)
    far = pts.copy(); far["radius"] = np.inf
    want4 = nc.twin_k("soup", 4, np.inf)[0][margin]
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    assert _margin_lists(*dev.neighbours(pts), margin) == want, "after rebuild_bvh"
    pc.assert_bytes_equal(dev.k_nearest(far, 4)[margin], want4, "the 4 nearest after rebuild_bvh")
    # and all points, exactly, against the twin on the rebuilt nodes
    desc = pc.with_nodes(hs.desc, dev.bvh_nodes())
    o2, _ = irl.near_offsets_host(desc, pts)
    r2, _ = irl.near_fill_host(desc, pts, o2)
    nc.assert_same(dev.neighbours(pts), (o2, r2), "after rebuild_bvh, against the twin on the new nodes")
    dev.close()
    built = irl.IpuScene.from_geometry(hs.desc)
    assert _margin_lists(*built.neighbours(pts), margin) == want, "from_geometry"
    pc.assert_bytes_equal(built.k_nearest(far, 4)[margin], want4, "the 4 nearest from_geometry")
    built.close()


def test_update_geometry_equals_a_fresh_scene_and_orders_behind_enqueued_queries():
    import torch
    hs, pts, offsets, recs, _, _ = nc.twin("soup")
    want4, _ = nc.twin_k("soup", 4)
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    # a fill enqueued before the update sees the old geometry
    many = np.tile(pts, 8)
    t_pts = torch.from_numpy(many.view(np.uint8).copy()).cuda()
    t_off = torch.arange(many.size + 1, dtype=torch.int64, device="cuda") * 4
    out = torch.zeros((many.size * 4, 4), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    dev.near_fill_device(t_pts.data_ptr(), t_off.data_ptr(), out.data_ptr(), many.size * 4, many.size, st.cuda_stream)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    st.synchronize()
    old = out.cpu().numpy().view(irl.NEIGHBOUR).reshape(8, pts.size, 4)
    for rep in range(8):
        assert np.array_equal(old[rep]["point"], np.repeat(np.arange(pts.size, dtype=np.uint32) + rep * pts.size, 4).reshape(-1, 4))
        for f in ("dist2", "primID", "geomID", "flags"):
            assert old[rep][f].tobytes() == want4[f].tobytes(), f"enqueued before the update: the old geometry ({f}, copy {rep})"
    moved = dev.neighbours(pts)
    moved4 = dev.k_nearest(pts, 4)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    fresh = irl.IpuScene(m.desc)
    nc.assert_same(moved, fresh.neighbours(pts), "after update_geometry: a fresh scene of the moved arrays")
    pc.assert_bytes_equal(moved4, fresh.k_nearest(pts, 4), "the 4 nearest after update_geometry")
    fresh.close()
    o2, _ = irl.near_offsets_host(m.desc, pts)
    r2, _ = irl.near_fill_host(m.desc, pts, o2)
    nc.assert_same(moved, (o2, r2), "after update_geometry: the twin on the moved arrays")
    assert moved[1].tobytes() != recs.tobytes()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 6. the variants build, torch
# ------------------------------------------------------------------------------------------------------
def test_variants_build_gives_the_same_bytes():
    hs, pts, offsets, recs, vo, _ = nc.twin("soup")
    var = irl.IpuScene(hs.desc, variants=True)
    nc.assert_same(var.neighbours(pts), (offsets, recs), "variants build")
    for k in nc.KS:
        pc.assert_bytes_equal(var.k_nearest(pts, k), nc.twin_k("soup", k)[0], f"variants build: the {k} nearest")
    var.set_option("full_stats", 1)
    var.reset_counters()
    assert np.array_equal(var.near_offsets(pts), offsets)
    c = var.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (0, vo["box_tests"], vo["prim_evals"])
    var.close()


def test_torch_forms_on_a_non_default_stream():
    import torch
    hs, pts, offsets, recs, _, _ = nc.twin("soup")
    want4, _ = nc.twin_k("soup", 4)
    want_inf, _ = nc.twin_k("soup", 4, np.inf)
    dev = irl.IpuScene(hs.desc)
    p = torch.from_numpy(np.stack([pts[c] for c in "xyz"], 1).copy()).cuda()
    r = torch.from_numpy(pts["radius"].copy()).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ball = dev.ball_query(p, r)
        near = dev.knn(p, 4, r)
        near_inf = dev.knn(p, 4)
    st.synchronize()
    assert ball["offsets"].dtype == torch.int64 and np.array_equal(ball["offsets"].cpu().numpy().astype(np.uint64), offsets)
    assert np.array_equal(near["offsets"].cpu().numpy(), np.arange(pts.size + 1) * 4)
    for got, want in ((ball, recs), (near, want4), (near_inf, want_inf)):
        assert np.array_equal(got["dist2"].cpu().numpy().view(np.uint32), want["dist2"].view(np.uint32))
        assert np.array_equal(got["prim_id"].cpu().numpy().view(np.uint32), want["primID"])
        assert np.array_equal(got["geom_id"].cpu().numpy(), want["geomID"].astype(np.int16).astype(np.int32))
        assert np.array_equal(got["point_ids"].cpu().numpy(), want["point"].astype(np.int64))
    assert near["dist2"].shape == (pts.size, 4) and ball["dist2"].shape == (recs.size,)
    dev.close()
