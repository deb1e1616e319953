"""Triangle queries on the GPU (pytest -m gpu): mi_tri_query* / mi_tri_offsets* / mi_tri_fill* against the host twins
mi_tri_query_host / mi_tri_offsets_host / mi_tri_fill_host, byte for byte - any, count, offsets and fill with their visit totals,
the workgroup's and the prefix sum's edges, host batches of 36-byte items with offsets that do not ascend, the heap's sift paths,
canaries, live scenes, the options, the tensor entries on a stream and mesh against scene."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc
import tri_cases as tc
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _device_query(dev, kind, tq, stream=0):
    import torch
    t_tq = _cuda(tq)
    t_out = torch.full((tq.size,), 0x7F, dtype=torch.uint8 if kind == tc.ANY else torch.int32, device="cuda")
    dev.tri_query_device(kind, t_tq.data_ptr(), t_out.data_ptr(), tq.size, stream)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    return out.view(np.bool_) if kind == tc.ANY else out.view(np.uint32)


def _device_offsets(dev, tq, stream=0):
    import torch
    t_tq = _cuda(tq)
    t_off = torch.full((tq.size + 1,), -1, dtype=torch.int64, device="cuda")
    dev.tri_offsets_device(t_tq.data_ptr(), t_off.data_ptr(), tq.size, stream)
    torch.cuda.synchronize()
    return t_off.cpu().numpy().view(np.uint64)


def _device_fill(dev, tq, offsets, total, capacity=None):
    """The device entry into a sentinel buffer of `total` (+ 64) records; returns the whole buffer."""
    import torch
    t_tq, t_off, t_buf = _cuda(tq), _cuda(offsets.astype(np.uint64)), _cuda(tc.sentinel_buffer(total))
    dev.tri_fill_device(t_tq.data_ptr(), t_off.data_ptr(), t_buf.data_ptr(), total if capacity is None else capacity, tq.size)
    torch.cuda.synchronize()
    return t_buf.cpu().numpy().view(irl.CONTACT)


class _OwnStream:
    """A non-default stream made for one test and destroyed behind it, as a torch stream. torch.cuda.Stream() would hand out one
    of torch's pooled streams, which stay bound to a hardware queue for the rest of the process: how many of those a process holds
    decides which queue a stream created later shares, and tests that run after this file (the launch-progress probe of
    test_gpu_parity.py needs a queue of its own beside the render's) must find the process as they would without it."""

    def __enter__(self):
        import ctypes
        import torch
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)      # the runtime torch has loaded
        self.hip = ctypes.CDLL(path)
        self.handle = ctypes.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(ctypes.byref(self.handle), 1) == 0                       # hipStreamNonBlocking
        self.stream = torch.cuda.ExternalStream(self.handle.value)
        self.stream.wait_stream(torch.cuda.current_stream())
        return self.stream

    def __exit__(self, *exc):
        assert self.hip.hipStreamSynchronize(self.handle) == 0 and self.hip.hipStreamDestroy(self.handle) == 0
        return False


def _gapped(lens, gap):
    """Offsets that give every item of a batch TWICE - first its own segment of lens[j] records, then an empty, decreasing one -
    with the segments laid out back to front and `gap` records that nobody owns behind each: (offsets [2 n + 1], total)."""
    lens = np.asarray(lens, np.int64)
    starts = (np.cumsum((lens + gap)[::-1])[::-1] - (lens + gap)).astype(np.uint64)
    off = np.zeros(2 * len(lens) + 1, np.uint64)
    off[0:-1:2] = starts
    off[1::2] = starts + lens.astype(np.uint64)
    return off, int((lens + gap).sum())


def _whole_scene_query(hs):
    """One query whose products overflow: nothing separates, so it lists every primitive of the scene."""
    return tc.tris([((-1e30, -1e30, -1e30), (1e30, 1e30, -1e30), (0, 1e30, 1e30))])


# ------------------------------------------------------------------------------------------------------
# 1. the device against the twin, both libraries
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
@pytest.mark.parametrize("name", ["box", "spheres", "soup"])
def test_device_equals_twin_byte_for_byte(name, variants):
    hs, tq, offsets, recs, counts, anys, v = tc.twin(name)
    dev = irl.IpuScene(hs.desc, variants=variants)
    assert np.array_equal(dev.tri_touches(tq), anys) and np.array_equal(_device_query(dev, tc.ANY, tq), anys), f"{name}: any"
    assert np.array_equal(dev.count_contacts(tq), counts) and np.array_equal(_device_query(dev, tc.COUNT, tq), counts), f"{name}: count"
    got = dev.list_contacts(tq)
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.CONTACT and got[0][0] == 0 and got[0][-1] == got[1].size
    tc.assert_same(got, (offsets, recs), f"{name}: host entries")
    assert np.array_equal(_device_offsets(dev, tq), offsets), f"{name}: offsets, device entry"
    buf = _device_fill(dev, tq, offsets, recs.size)
    pc.assert_bytes_equal(buf[:recs.size], recs, f"{name}: fill, device entry")
    assert tc.is_sentinel(buf[recs.size:]).all()
    for k in (1, 4):
        want, _ = irl.tri_fill_host(hs.desc, tq, tc.k_offsets(tq.size, k))
        pc.assert_bytes_equal(dev.first_contacts(tq, k).reshape(-1), want, f"{name}: the first {k}, host entry")
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    # the instrumented build: the same bytes and the twin's visit totals
    dev.set_option("full_stats", 1)
    calls = (("any", lambda: dev.tri_touches(tq), anys), ("count", lambda: dev.count_contacts(tq), counts),
             ("offsets", lambda: dev.tri_offsets(tq), offsets),
             ("fill", lambda: dev.tri_fill(tq, offsets, tc.sentinel_buffer(recs.size), recs.size)[:recs.size], recs))
    for what, call, want in calls:
        dev.reset_counters()
        out = call()
        assert out.tobytes() == want.tobytes(), f"{name}: {what} under full_stats"
        c = dev.counters()
        assert (c["casts"], c["paths"]) == (0, 0)
        assert (c["nodes_visited"], c["leaf_tests"]) == (v[what]["box_tests"], v[what]["prim_evals"]), f"{name}: the visits of {what}"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 2. a workgroup's edge, the prefix sum's tiles, host batches
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_workgroup_edges(n):
    hs, tq, offsets, recs, counts, anys, _ = tc.twin("soup", 257)
    dev = irl.IpuScene(hs.desc)
    sub = tq[:n]
    assert np.array_equal(_device_query(dev, tc.ANY, sub), anys[:n]) and np.array_equal(_device_query(dev, tc.COUNT, sub), counts[:n])
    assert np.array_equal(_device_offsets(dev, sub), offsets[:n + 1])
    total = int(offsets[n])
    buf = _device_fill(dev, sub, offsets[:n + 1], total)
    assert buf[:total].tobytes() == recs[:total].tobytes(), f"fill, n = {n}"
    assert tc.is_sentinel(buf[total:]).all()
    dev.close()


def test_scan_tile_edge():
    """One triangle more than a tile of the prefix sum (2048), every one touching nothing but the last: its count crosses the
    tile's edge."""
    hs = tc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    n = 2049
    far = np.tile((hi + F(100)).astype(F), (n, 1))
    tq = qb.make_tris(far, far + F(1), far + np.array([0, 1, 0], F))
    tq[-1] = _whole_scene_query(hs)[0]
    want = np.zeros(n + 1, np.uint64)
    want[-1] = 602
    assert np.array_equal(irl.tri_offsets_host(hs.desc, tq)[0], want)
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(_device_offsets(dev, tq), want) and np.array_equal(dev.tri_offsets(tq), want)
    dev.close()


@pytest.mark.parametrize("batch", [1, 7, 300])
def test_host_batches_and_offsets_that_do_not_ascend(batch):
    """36-byte items through the two-slot pipeline: batches of 1, 7 and the whole set (300: the 150 queries given twice)."""
    hs, tq, offsets, recs, counts, anys, _ = tc.twin("soup")
    assert tq.size == 150
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(batch)
    assert np.array_equal(dev.tri_touches(tq), anys) and np.array_equal(dev.count_contacts(tq), counts)
    got = dev.list_contacts(tq)
    tc.assert_same(got, (offsets, recs), f"batches of {batch}")
    assert np.array_equal(got[1]["tri"], np.repeat(np.arange(tq.size, dtype=np.uint32), counts.astype(np.int64))), "triangle indices are global"
    want4, _ = irl.tri_fill_host(hs.desc, tq, tc.k_offsets(tq.size, 4))
    pc.assert_bytes_equal(dev.first_contacts(tq, 4).reshape(-1), want4, f"the first 4 in batches of {batch}")
    # offsets that do not ascend - the segments laid out back to front, one untouched record behind each, every item followed by
    # an empty decreasing pair -: the pipeline copies such a batch item by item
    pairs = np.repeat(tq, 2)
    pair_off, total = _gapped(counts, 1)
    want = tc.sentinel_buffer(total)
    irl.tri_fill_host(hs.desc, pairs, pair_off, capacity=total, hits=want)
    assert tc.is_sentinel(want).sum() == tq.size + 64, "the gaps and the tail keep their canaries"
    buf = tc.sentinel_buffer(total)
    dev.tri_fill(pairs, pair_off, buf, total)
    assert buf.tobytes() == want.tobytes(), f"host entry in batches of {batch}"
    if batch == 7:
        assert _device_fill(dev, pairs, pair_off, total).tobytes() == want.tobytes(), "device entry"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. the heap, canaries
# ------------------------------------------------------------------------------------------------------
def test_heap_sift_paths():
    """One query touching the whole soup: segments of 1, 2, 3, 7, 8 and count - 1 records receive the head of the full list."""
    hs = tc.scene("soup")
    tq = _whole_scene_query(hs)
    offsets, _ = irl.tri_offsets_host(hs.desc, tq)
    full, _ = irl.tri_fill_host(hs.desc, tq, offsets)
    count = int(offsets[1])
    assert count == 602
    lens = [1, 2, 3, 7, 8, count - 1, count, count + 5]
    pair_tq = np.repeat(tq, 2 * len(lens))
    pair_off, total = _gapped(lens, 2)                                                   # two canaries behind every segment
    offs = pair_off[0::2]
    dev = irl.IpuScene(hs.desc)
    buf = _device_fill(dev, pair_tq, pair_off, total)
    for j, ln in enumerate(lens):
        seg = buf[int(offs[j]):int(offs[j]) + ln]
        want = np.concatenate([full[:ln], tc.records([], 0, max(ln - count, 0))]).copy()
        want["tri"] = 2 * j
        pc.assert_bytes_equal(seg, want, f"len = {ln}: the head of the full list")
        assert tc.is_sentinel(buf[int(offs[j]) + ln:int(offs[j]) + ln + 2]).all(), f"len = {ln}: the canaries behind the segment"
    assert tc.is_sentinel(buf[total:]).all()
    want = tc.sentinel_buffer(total)
    irl.tri_fill_host(hs.desc, pair_tq, pair_off, capacity=total, hits=want)
    assert buf.tobytes() == want.tobytes(), "the twin"
    dev.close()


def test_nothing_is_written_past_capacity():
    hs, tq, offsets, recs, _, _, _ = tc.twin("soup")
    total = recs.size
    dev = irl.IpuScene(hs.desc)
    for capacity in (total - 1, total // 2, 0):
        want, _ = irl.tri_fill_host(hs.desc, tq, offsets, capacity=capacity, hits=tc.sentinel_buffer(total))
        assert tc.is_sentinel(want[capacity:]).all()
        buf = tc.sentinel_buffer(total)
        dev.tri_fill(tq, offsets, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, capacity {capacity}"
        assert _device_fill(dev, tq, offsets, total, capacity).tobytes() == want.tobytes(), f"device entry, capacity {capacity}"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. live scenes, options
# ------------------------------------------------------------------------------------------------------
def _twin_lists(desc, tq):
    offsets, _ = irl.tri_offsets_host(desc, tq)
    return offsets, irl.tri_fill_host(desc, tq, offsets)[0]


def test_rebuild_and_set_geometry_give_the_same_lists():
    hs, tq, offsets, recs, _, _, _ = tc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    got = dev.list_contacts(tq)
    tc.assert_same(got, (offsets, recs), "after rebuild_bvh: the bytes do not depend on the tree")
    tc.assert_same(got, _twin_lists(pc.with_nodes(hs.desc, dev.bvh_nodes()), tq), "after rebuild_bvh: the twin on the new nodes")
    other = tc.scene("spheres")
    dev.set_geometry(other.desc)
    otq = tc.tris_of("spheres")
    tc.assert_same(dev.list_contacts(otq), _twin_lists(pc.with_nodes(other.desc, dev.bvh_nodes()), otq), "after set_geometry: the twin on the new description")
    dev.set_geometry(hs.desc)
    tc.assert_same(dev.list_contacts(tq), (offsets, recs), "after set_geometry of the first contents")
    dev.close()


def test_update_geometry_equals_a_fresh_scene_and_a_refit_keeps_the_bytes():
    hs, tq, offsets, recs, _, _, _ = tc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    moved = dev.list_contacts(tq)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    tc.assert_same(moved, _twin_lists(m.desc, tq), "after update_geometry: the twin on the moved arrays")
    assert moved[1].tobytes() != recs.tobytes()
    fresh = irl.IpuScene(m.desc)
    tc.assert_same(fresh.list_contacts(tq), moved, "a fresh scene of the moved contents")
    fresh.close()
    # the same contents again, by a refit: the first lists, byte for byte
    dev.update_geometry(vertices=hs.verts.copy(), spheres=hs.spheres.copy(), discs=hs.discs.copy())
    tc.assert_same(dev.list_contacts(tq), (offsets, recs), "a refit back to the first contents")
    dev.close()


def test_options_change_nothing():
    hs, tq, offsets, recs, counts, anys, _ = tc.twin("soup")
    for option, value in (("double_fallback", 1), ("fast", 1), ("query_kernel", 1), ("hot_nodes", 64)):
        dev = irl.IpuScene(hs.desc)
        dev.set_option(option, value)
        assert np.array_equal(dev.tri_touches(tq), anys) and np.array_equal(dev.count_contacts(tq), counts), option
        tc.assert_same(dev.list_contacts(tq), (offsets, recs), option)
        dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. torch
# ------------------------------------------------------------------------------------------------------
def test_tensor_entries_on_a_non_default_stream():
    import torch
    hs, tq, offsets, recs, counts, anys, _ = tc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    t = torch.from_numpy(np.stack([tq["a"], tq["b"], tq["c"]], 1).copy()).cuda()
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            t_any = dev.tri_any(t)
            t_count = dev.tri_count(t)
            t_off, t_recs = dev.tri_list(t)
        st.synchronize()
        got = (t_any.cpu(), t_count.cpu(), t_off.cpu(), t_recs.cpu())
        del t_any, t_count, t_off, t_recs
    t_any, t_count, t_off, t_recs = got
    assert t_any.dtype == torch.bool and np.array_equal(t_any.numpy(), anys)
    assert t_count.dtype == torch.int32 and np.array_equal(t_count.numpy().view(np.uint32), counts)
    assert t_off.dtype == torch.int64 and np.array_equal(t_off.numpy().view(np.uint64), offsets)
    assert t_recs.shape == (recs.size, 4) and t_recs.numpy().tobytes() == recs.tobytes()
    dev.close()


def test_mesh_contacts_of_a_displaced_copy_of_the_soup():
    import torch
    hs = tc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    own = tc.scene_tris32(hs)
    shift = ((hi - lo) * F(0.1)).astype(F)
    verts = (own.reshape(-1, 3) + shift).astype(F)                       # an indexed mesh: three vertices per face, displaced
    faces = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
    dev = irl.IpuScene(hs.desc)
    offsets, recs = dev.list_contacts(qb.make_tris(verts, faces))
    which = np.repeat(np.arange(len(faces)), np.diff(offsets).astype(np.int64))
    want = np.stack([which, recs["geomID"].astype(np.int64), recs["primID"].astype(np.int64)], 1)
    assert len(want) > 100
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            t_v, t_f = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
            rows = dev.mesh_contacts(t_v, t_f)
            hit = dev.collides(t_v, t_f)
            far = dev.collides(t_v + 1000.0, t_f)
            any_face = dev.tri_any(t_v[t_f])
        st.synchronize()
        rows, any_face = rows.cpu(), any_face.cpu()
        del t_v, t_f
    assert rows.dtype == torch.int64 and np.array_equal(rows.numpy(), want), "mesh_contacts is the composition of list_contacts"
    assert hit is True and far is False and hit == bool(any_face.any())
    assert np.array_equal(any_face.numpy(), np.diff(offsets) > 0)
    dev.close()
