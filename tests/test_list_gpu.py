"""Crossing lists on the GPU (mi_list_offsets*, mi_list_fill*): the device's offsets and record bytes against the checker of
tests/list_cases.py, exactly; offsets against the device's own counts; the same bytes on any tree over the same geometry; the first K
crossings; the capacity guard; offsets from another state of the scene; the prefix sum and the launch at their edges; batches, the
variants build, torch streams and counters."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import count_cases as cc
import list_cases as lc
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = (F(-7.5), 0xABCD1234, 0x5A5A, 0xA5A5, 0xDEADBEEF)


def assert_same(got, want, what):
    """(offsets, hits) pairs, exactly."""
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at rays {np.nonzero(got[0][1:] != want[0][1:])[0][:4]}"
    if got[1].tobytes() != want[1].tobytes():
        bad = np.nonzero((got[1].view(np.uint32).reshape(-1, 4) != want[1].view(np.uint32).reshape(-1, 4)).any(1))[0]
        raise AssertionError(f"{what}: {bad.size}/{want[1].size} records differ, first {bad[:4]}: got {got[1][bad[:4]]} want {want[1][bad[:4]]}")


def sentinel_buffer(records):
    """A 16-byte aligned CROSSING array of `records` + 64 records, every one the sentinel."""
    buf = irl.aligned_bytes((records + 64) * irl.CROSSING.itemsize).view(irl.CROSSING)
    buf[:] = SENTINEL
    return buf


def empty_desc(hs):
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = empty.num_spheres = empty.num_discs = 0
    return empty


# ------------------------------------------------------------------------------------------------------
# 1. lists against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layers", "soup", "mixed", "box", "spheres"])
def test_lists_equal_the_checkers(name):
    hs, rays, lists = lc.case(name)
    dev = irl.IpuScene(hs.desc)
    got = dev.list_crossings(rays)
    dev.close()
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.CROSSING and got[0][0] == 0 and got[0][-1] == got[1].size
    assert_same(got, lc.packed(lists), name)


def test_double_fallback_lists_on_grazing_rays():
    differing = 0
    for seed in range(4):
        hs = cc.grazing_scene(np.random.default_rng(900 + seed), 48)
        rays = cc.grazing_rays(seed)
        res = {}
        for df in (0, 1):
            if df:
                with ol.double_fallback():
                    want = lc.ListChecker(hs).lists(rays)
            else:
                want = lc.ListChecker(hs).lists(rays)
            dev = irl.IpuScene(hs.desc).set_option("double_fallback", df)
            got = dev.list_crossings(rays)
            dev.close()
            assert_same(got, lc.packed(want), f"grazing rays, double_fallback {df}, seed {seed}")
            res[df] = want
        differing += sum(1 for a, b in zip(res[0], res[1]) if a != b)
    assert differing > 0, "the constructed rays never took the binary64 branch to a different list"


# ------------------------------------------------------------------------------------------------------
# 2. offsets against counts, device against device
# ------------------------------------------------------------------------------------------------------
def test_offsets_are_the_running_total_of_the_counts():
    hs = cc.scene("box")
    rays = cc.mixed_rays(hs, 50000, seed=77)
    dev = irl.IpuScene(hs.desc)
    offsets, counts = dev.list_offsets(rays), dev.count_crossings(rays)
    dev.close()
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets), counts.astype(np.uint64)) and counts.max() >= 2


# ------------------------------------------------------------------------------------------------------
# 3. canonical across trees and updates
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layers", "soup"])
def test_the_bytes_do_not_depend_on_the_tree(name):
    hs, rays, lists = lc.case(name)
    want = lc.packed(lists)
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    assert_same(dev.list_crossings(rays), want, f"{name} after rebuild_bvh")
    # moved geometry, the tree refitted: what a fresh scene of the moved geometry (its own refitted tree) lists, and the LBVH's too
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    moved = dev.list_crossings(rays)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    fresh = irl.IpuScene(m.desc)
    assert_same(moved, fresh.list_crossings(rays), f"{name} after update_geometry")
    fresh.close()
    dev.rebuild_bvh()
    assert_same(dev.list_crossings(rays), moved, f"{name} after update_geometry and rebuild_bvh")
    assert moved[1].tobytes() != want[1].tobytes()
    dev.close()
    built = irl.IpuScene.from_geometry(hs.desc)
    assert_same(built.list_crossings(rays), want, f"{name} from_geometry")
    built.close()


# ------------------------------------------------------------------------------------------------------
# 4. the first K
# ------------------------------------------------------------------------------------------------------
def test_first_crossings_on_layers():
    hs, rays, lists = lc.case("layers")
    longest = max(len(x) for x in lists)
    assert 8 < longest < 80
    dev = irl.IpuScene(hs.desc)
    for k in (1, 3, 8, 80):
        got = dev.first_crossings(rays, k)
        want = lc.first_k(lists, k)
        assert got.shape == (rays.size, k)
        assert_same((np.zeros(1), got.reshape(-1)), (np.zeros(1), want.reshape(-1)), f"first_crossings k = {k}")
    dev.close()


@pytest.mark.parametrize("name", ["soup-tris", "cube", "box-simple"])
def test_the_first_crossing_is_the_closest_hit(name):
    hs = cc.scene(name)
    rays = cc.mixed_rays(hs, 4000, 5)
    dev = irl.IpuScene(hs.desc)
    first, hit = dev.first_crossings(rays, 1)[:, 0], dev.intersect(rays)
    dev.close()
    found = hit["primID"] != irl.INVALID_PRIM
    assert found.sum() > 400 and (~found).sum() > 400
    assert np.array_equal(first["primID"] != irl.INVALID_PRIM, found)
    for a, b in (("t", "t"), ("primID", "primID"), ("geomID", "geomID")):
        assert first[a][found].tobytes() == hit[b][found].tobytes(), (name, a)
    assert np.all(np.isposinf(first["t"][~found])) and np.all(first["flags"][~found] == irl.FLAG_ESCAPED) and np.all(first["flags"][found] == 0)
    assert np.array_equal(first["ray"], np.arange(rays.size, dtype=np.uint32))


# ------------------------------------------------------------------------------------------------------
# 5. bounds
# ------------------------------------------------------------------------------------------------------
def test_nothing_is_written_at_or_past_capacity():
    import torch
    hs, rays, lists = lc.case("layers")
    offsets, full = lc.packed(lists)
    total = full.size
    dev = irl.IpuScene(hs.desc)
    t_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    t_off = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
    for capacity in (total, total - 1, total // 2, 0):
        # the host entry
        buf = sentinel_buffer(total)
        dev.list_fill(rays, offsets, buf, capacity)
        assert buf[:capacity].tobytes() == full[:capacity].tobytes(), f"host entry, capacity {capacity}"
        assert np.all(buf[capacity:] == np.array(SENTINEL, irl.CROSSING)), f"host entry, capacity {capacity}: a record at or past capacity was written"
        # the device entry
        t_buf = torch.from_numpy(sentinel_buffer(total).view(np.uint8).copy()).cuda()
        dev.list_fill_device(t_rays.data_ptr(), t_off.data_ptr(), t_buf.data_ptr(), capacity, rays.size)
        torch.cuda.synchronize()
        out = t_buf.cpu().numpy().view(irl.CROSSING)
        assert out[:capacity].tobytes() == full[:capacity].tobytes(), f"device entry, capacity {capacity}"
        assert np.all(out[capacity:] == np.array(SENTINEL, irl.CROSSING)), f"device entry, capacity {capacity}: a record at or past capacity was written"
    # offsets that do not ascend (and whose segments do not overlap): a decreasing pair is an empty segment, the others are filled
    # where they say, the one that runs past capacity cut there. Segments: ray 0 [13, 16), ray 2 [8, 11), ray 4 [3, 6), ray 6 [6, 8)
    odd = np.array([13, 2 ** 40, 8, 11, 3, 6, 6, 8], np.uint64)
    want = sentinel_buffer(16)
    for ray, lo, hi in ((0, 13, 16), (2, 8, 11), (4, 3, 6), (6, 6, 8)):
        want[lo:hi] = lc.records(lists[ray], ray, hi - lo)
    buf = sentinel_buffer(16)
    dev.list_fill(rays[:7], odd, buf, 16)
    assert buf.tobytes() == want.tobytes(), "host entry, offsets that do not ascend"
    t_buf = torch.from_numpy(sentinel_buffer(16).view(np.uint8).copy()).cuda()
    t_odd = torch.from_numpy(odd.view(np.int64).copy()).cuda()
    dev.list_fill_device(t_rays.data_ptr(), t_odd.data_ptr(), t_buf.data_ptr(), 16, 7)
    torch.cuda.synchronize()
    assert t_buf.cpu().numpy().tobytes() == want.tobytes(), "device entry, offsets that do not ascend"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 6. offsets from another state of the scene
# ------------------------------------------------------------------------------------------------------
def test_offsets_from_another_state_of_the_scene():
    hs, rays, lists = lc.case("layers")
    dev = irl.IpuScene(hs.desc)
    offsets = dev.list_offsets(rays)
    total = int(offsets[-1])
    assert total > 20 * rays.size
    # everything moved clear of the rays: every segment is padding
    v, s, d = hs.verts.copy(), hs.spheres.copy(), hs.discs.copy()
    v["x"] += F(1000); s["x"] += F(1000); d["cx"] += F(1000)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    assert not dev.count_crossings(rays).any()
    buf = sentinel_buffer(total)
    dev.list_fill(rays, offsets, buf, total)
    owner = np.repeat(np.arange(rays.size, dtype=np.uint32), np.diff(offsets).astype(np.int64))
    pad = np.zeros(total, irl.CROSSING)
    pad["t"], pad["primID"], pad["geomID"], pad["flags"], pad["ray"] = np.inf, irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, owner
    assert buf[:total].tobytes() == pad.tobytes()
    assert np.all(buf[total:] == np.array(SENTINEL, irl.CROSSING))
    dev.close()
    # offsets of an empty scene, filled once the scene has its geometry: nothing is written, and it is no error
    dev = irl.IpuScene(empty_desc(hs))
    zero = dev.list_offsets(rays)
    assert zero.size == rays.size + 1 and not zero.any()
    assert dev.first_crossings(rays[:300], 2).tobytes() == lc.first_k([[]] * 300, 2).tobytes()      # an empty scene pads
    dev.set_geometry(hs.desc)
    buf = sentinel_buffer(0)
    dev.list_fill(rays, zero, buf, buf.size)
    assert np.all(buf == np.array(SENTINEL, irl.CROSSING))
    assert_same(dev.list_crossings(rays), lc.packed(lists), "layers, set on an empty scene")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 7. the prefix sum and the launch at their edges
# ------------------------------------------------------------------------------------------------------
def test_scan_and_launch_edges():
    hs = cc.scene("cube")
    n_max = 1000003
    o = np.zeros((n_max, 3), F)
    o[:, 0] = np.where(np.arange(n_max) % 2 == 0, 0.3, 5.0)          # through the cube | past it
    o[:, 1] = 0.2
    o[:, 2] = -4.0
    rays = qb.make_rays(o, np.tile(np.array([0.013, 0.021, 1.0], F), (n_max, 1)))
    dev = irl.IpuScene(hs.desc)
    counts = dev.count_crossings(rays)
    assert counts[0] == 2 and counts[1] == 0 and np.array_equal(counts[:2], counts[-3:-1])
    for n in (1, 2, 255, 256, 257, 65535, 65536, 65537, n_max):
        offsets = dev.list_offsets(rays[:n])
        want = np.concatenate([[0], np.cumsum(counts[:n], dtype=np.uint64)]).astype(np.uint64)
        assert np.array_equal(offsets, want), n
        assert isinstance(int(offsets[-1]), int) and int(offsets[-1]) == int(counts[:n].sum(dtype=np.uint64)) == 2 * ((n + 1) // 2)
        # a slice that is not 16-byte aligned goes through the aligned copy
        odd = irl.aligned_bytes(n * 32 + 16)[8:8 + n * 32].view(irl.RAY)
        odd[:] = rays[:n]
        assert odd.ctypes.data % 16 == 8
        assert np.array_equal(dev.list_offsets(odd), want), n
        if n <= 65537:
            offs, hits = dev.list_crossings(odd)
            assert hits.size == want[-1] and np.array_equal(hits["ray"], np.repeat(np.arange(n, dtype=np.uint32), counts[:n]))
            assert np.all(hits["t"][0::2] < hits["t"][1::2])
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 8. batches, variants, streams, counters
# ------------------------------------------------------------------------------------------------------
def test_host_batches_and_the_variants_build():
    hs, rays, lists = lc.case("layers")
    want = lc.packed(lists)
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(700)
    got = dev.list_crossings(rays)
    assert_same(got, want, "batches of 700")
    assert np.array_equal(got[1]["ray"], np.repeat(np.arange(rays.size, dtype=np.uint32), np.diff(want[0]).astype(np.int64)))
    assert dev.first_crossings(rays, 3).tobytes() == lc.first_k(lists, 3).tobytes()
    dev.close()
    var = irl.IpuScene(hs.desc, variants=True)
    assert_same(var.list_crossings(rays), want, "variants build")
    var.setRayBatch(700)
    assert_same(var.list_crossings(rays), want, "variants build, batches of 700")
    assert var.first_crossings(rays, 8).tobytes() == lc.first_k(lists, 8).tobytes()
    var.close()


def test_torch_entries_on_a_non_default_stream():
    import torch
    hs, rays, lists = lc.case("layers")
    dev = irl.IpuScene(hs.desc)
    offsets, hits = dev.list_crossings(rays)
    first = dev.first_crossings(rays, 4)
    o = np.stack([rays["origin"][c] for c in "xyz"], 1)
    d = np.stack([rays["direction"][c] for c in "xyz"], 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t_o, t_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        t_min, t_max = torch.from_numpy(rays["tMin"].copy()).cuda(), torch.from_numpy(rays["tMax"].copy()).cuda()
        r = dev.cast_all(t_o, t_d, t_min, t_max)
        f = dev.cast_first(t_o, t_d, 4, t_min, t_max)
    st.synchronize()
    assert r["ray_splits"].dtype == torch.int64 and np.array_equal(r["ray_splits"].cpu().numpy().astype(np.uint64), offsets)
    for got, want in ((r, hits), (f, first)):
        assert np.array_equal(got["t"].cpu().numpy().view(np.uint32), want["t"].view(np.uint32))
        assert np.array_equal(got["prim_id"].cpu().numpy().view(np.uint32), want["primID"])
        assert np.array_equal(got["geom_id"].cpu().numpy(), want["geomID"].astype(np.int16).astype(np.int32))
        assert np.array_equal(got["far"].cpu().numpy(), (want["flags"] & irl.CROSS_FAR) != 0)
        assert np.array_equal(got["ray_ids"].cpu().numpy(), want["ray"].astype(np.int64))
    assert r["far"].any() and f["t"].shape == (rays.size, 4)
    dev.close()


def test_counters():
    hs, rays, lists = lc.case("soup")
    sub = rays[:1024]
    _, boxes, tests = cc.Checker(hs).counts(sub)
    dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    dev.count_crossings(sub)
    c0 = dev.counters()
    assert (c0["casts"], c0["nodes_visited"], c0["leaf_tests"]) == (1024, boxes, tests)
    for call in (lambda: dev.list_offsets(sub), lambda: dev.first_crossings(sub, 2), lambda: dev.first_crossings(sub, 0)):
        dev.reset_counters()
        call()
        c = dev.counters()
        assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (1024, boxes, tests, 0)
    dev.reset_counters()
    dev.list_crossings(sub)          # offsets + fill
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (2048, 2 * boxes, 2 * tests)
    dev.close()
    dev = irl.IpuScene(hs.desc)
    dev.list_crossings(sub)
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (2048, 0, 0)
    dev.close()


def test_destroy_waits_for_an_enqueued_fill():
    import torch
    hs, rays, lists = lc.case("layers")
    want = lc.first_k(lists, 8)
    t_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    t_off = (torch.arange(rays.size + 1, dtype=torch.int64, device="cuda") * 8)
    out = torch.zeros((rays.size * 8, 4), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    dev = irl.IpuScene(hs.desc)
    dev.list_fill_device(t_rays.data_ptr(), t_off.data_ptr(), out.data_ptr(), rays.size * 8, rays.size, st.cuda_stream)
    dev.close()
    st.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
