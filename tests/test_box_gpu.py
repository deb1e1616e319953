"""Box queries on the GPU (pytest -m gpu): mi_box_query* / mi_box_offsets* / mi_box_fill* against the host twins mi_box_query_host
/ mi_box_offsets_host / mi_box_fill_host, byte for byte - any, count, offsets and fill with their visit totals, the workgroup's and
the prefix sum's edges, host batches with offsets that do not ascend, the heap's sift paths, canaries, live scenes, the tensor
entries on a stream and the voxelisation."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc
import box_cases as bc
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _device_query(dev, kind, bx, stream=0):
    import torch
    t_bx = _cuda(bx)
    t_out = torch.full((bx.size,), 0x7F, dtype=torch.uint8 if kind == bc.ANY else torch.int32, device="cuda")
    dev.box_query_device(kind, t_bx.data_ptr(), t_out.data_ptr(), bx.size, stream)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    return out.view(np.bool_) if kind == bc.ANY else out.view(np.uint32)


def _device_offsets(dev, bx, stream=0):
    import torch
    t_bx = _cuda(bx)
    t_off = torch.full((bx.size + 1,), -1, dtype=torch.int64, device="cuda")
    dev.box_offsets_device(t_bx.data_ptr(), t_off.data_ptr(), bx.size, stream)
    torch.cuda.synchronize()
    return t_off.cpu().numpy().view(np.uint64)


def _device_fill(dev, bx, offsets, total, capacity=None):
    """The device entry into a sentinel buffer of `total` (+ 64) records; returns the whole buffer."""
    import torch
    t_bx, t_off, t_buf = _cuda(bx), _cuda(offsets.astype(np.uint64)), _cuda(bc.sentinel_buffer(total))
    dev.box_fill_device(t_bx.data_ptr(), t_off.data_ptr(), t_buf.data_ptr(), total if capacity is None else capacity, bx.size)
    torch.cuda.synchronize()
    return t_buf.cpu().numpy().view(irl.OVERLAP)


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


# ------------------------------------------------------------------------------------------------------
# 1. the device against the twin, both libraries
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
@pytest.mark.parametrize("name", ["box", "spheres", "soup"])
def test_device_equals_twin_byte_for_byte(name, variants):
    hs, bx, offsets, recs, counts, anys, v = bc.twin(name)
    dev = irl.IpuScene(hs.desc, variants=variants)
    assert np.array_equal(dev.touches(bx), anys) and np.array_equal(_device_query(dev, bc.ANY, bx), anys), f"{name}: any"
    assert np.array_equal(dev.count_overlaps(bx), counts) and np.array_equal(_device_query(dev, bc.COUNT, bx), counts), f"{name}: count"
    got = dev.list_overlaps(bx)
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.OVERLAP and got[0][0] == 0 and got[0][-1] == got[1].size
    bc.assert_same(got, (offsets, recs), f"{name}: host entries")
    assert np.array_equal(_device_offsets(dev, bx), offsets), f"{name}: offsets, device entry"
    buf = _device_fill(dev, bx, offsets, recs.size)
    pc.assert_bytes_equal(buf[:recs.size], recs, f"{name}: fill, device entry")
    assert bc.is_sentinel(buf[recs.size:]).all()
    for k in (1, 4):
        want, _ = irl.box_fill_host(hs.desc, bx, bc.k_offsets(bx.size, k))
        pc.assert_bytes_equal(dev.first_overlaps(bx, k).reshape(-1), want, f"{name}: the first {k}, host entry")
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    # the instrumented build: the same bytes and the twin's visit totals
    dev.set_option("full_stats", 1)
    calls = (("any", lambda: dev.touches(bx), anys), ("count", lambda: dev.count_overlaps(bx), counts),
             ("offsets", lambda: dev.box_offsets(bx), offsets),
             ("fill", lambda: dev.box_fill(bx, offsets, bc.sentinel_buffer(recs.size), recs.size)[:recs.size], recs))
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
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_workgroup_edges(n):
    hs, bx, offsets, recs, counts, anys, _ = bc.twin("soup", 513)
    dev = irl.IpuScene(hs.desc)
    sub = bx[:n]
    assert np.array_equal(_device_query(dev, bc.ANY, sub), anys[:n]) and np.array_equal(_device_query(dev, bc.COUNT, sub), counts[:n])
    assert np.array_equal(_device_offsets(dev, sub), offsets[:n + 1])
    total = int(offsets[n])
    buf = _device_fill(dev, sub, offsets[:n + 1], total)
    pc.assert_bytes_equal(buf[:total], recs[:total], f"fill, n = {n}")
    assert bc.is_sentinel(buf[total:]).all()
    dev.close()


def test_scan_tile_edge():
    """One box more than a tile of the prefix sum (2048), every box empty but the last: its count crosses the tile's edge."""
    hs = bc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    n = 2049
    far = (hi + F(100)).astype(F)
    bx = qb.make_boxes(np.tile(far, (n, 1)), np.tile(far + F(1), (n, 1)))
    bx["lo"][-1], bx["hi"][-1] = lo, hi
    want = np.zeros(n + 1, np.uint64)
    want[-1] = 602
    assert np.array_equal(irl.box_offsets_host(hs.desc, bx)[0], want)
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(_device_offsets(dev, bx), want) and np.array_equal(dev.box_offsets(bx), want)
    dev.close()


def test_host_batches_and_offsets_that_do_not_ascend():
    hs, bx, offsets, recs, counts, anys, _ = bc.twin("soup", 513)
    bx, offsets, counts, anys = bx[:257], offsets[:258], counts[:257], anys[:257]
    recs = recs[:int(offsets[257])]
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(100)
    assert np.array_equal(dev.touches(bx), anys) and np.array_equal(dev.count_overlaps(bx), counts)
    got = dev.list_overlaps(bx)
    bc.assert_same(got, (offsets, recs), "batches of 100")
    assert np.array_equal(got[1]["box"], np.repeat(np.arange(257, dtype=np.uint32), counts.astype(np.int64))), "box indices are global"
    want4, _ = irl.box_fill_host(hs.desc, bx, bc.k_offsets(257, 4))
    pc.assert_bytes_equal(dev.first_overlaps(bx, 4).reshape(-1), want4, "the first 4 in batches of 100")
    # offsets that do not ascend - the segments laid out back to front, one untouched record behind each -: the pipeline copies
    # such a batch item by item
    pairs_bx = np.repeat(bx, 2)
    pair_off, total = _gapped(counts, 1)
    want = bc.sentinel_buffer(total)
    irl.box_fill_host(hs.desc, pairs_bx, pair_off, capacity=total, hits=want)
    assert bc.is_sentinel(want).sum() == 257 + 64, "the gaps and the tail keep their canaries"
    buf = bc.sentinel_buffer(total)
    dev.box_fill(pairs_bx, pair_off, buf, total)
    assert buf.tobytes() == want.tobytes(), "host entry in batches of 100"
    assert _device_fill(dev, pairs_bx, pair_off, total).tobytes() == want.tobytes(), "device entry"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. the heap, canaries
# ------------------------------------------------------------------------------------------------------
def test_heap_sift_paths():
    """One box over the whole soup: segments of 1, 2, 3, 7, 8 and count - 1 records receive the head of the full list."""
    hs = bc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    bx = qb.make_boxes(lo[None], hi[None])
    offsets, _ = irl.box_offsets_host(hs.desc, bx)
    full, _ = irl.box_fill_host(hs.desc, bx, offsets)
    count = int(offsets[1])
    assert count == 602
    lens = [1, 2, 3, 7, 8, count - 1, count, count + 5]
    pair_bx = np.repeat(bx, 2 * len(lens))
    pair_off, total = _gapped(lens, 2)                                                   # two canaries behind every segment
    offs = pair_off[0::2]
    dev = irl.IpuScene(hs.desc)
    buf = _device_fill(dev, pair_bx, pair_off, total)
    for j, ln in enumerate(lens):
        seg = buf[int(offs[j]):int(offs[j]) + ln]
        want = np.concatenate([full[:ln], bc.records([], 0, max(ln - count, 0))]).copy()
        want["box"] = 2 * j
        pc.assert_bytes_equal(seg, want, f"len = {ln}: the head of the full list")
        assert bc.is_sentinel(buf[int(offs[j]) + ln:int(offs[j]) + ln + 2]).all(), f"len = {ln}: the canaries behind the segment"
    assert bc.is_sentinel(buf[total:]).all()
    want = bc.sentinel_buffer(total)
    irl.box_fill_host(hs.desc, pair_bx, pair_off, capacity=total, hits=want)
    assert buf.tobytes() == want.tobytes(), "the twin"
    dev.close()


def test_nothing_is_written_past_capacity():
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    total = recs.size
    dev = irl.IpuScene(hs.desc)
    for capacity in (total - 1, total // 2, 0):
        want, _ = irl.box_fill_host(hs.desc, bx, offsets, capacity=capacity, hits=bc.sentinel_buffer(total))
        assert bc.is_sentinel(want[capacity:]).all()
        buf = bc.sentinel_buffer(total)
        dev.box_fill(bx, offsets, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, capacity {capacity}"
        assert _device_fill(dev, bx, offsets, total, capacity).tobytes() == want.tobytes(), f"device entry, capacity {capacity}"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. live scenes
# ------------------------------------------------------------------------------------------------------
def _twin_lists(desc, bx):
    offsets, _ = irl.box_offsets_host(desc, bx)
    return offsets, irl.box_fill_host(desc, bx, offsets)[0]


def test_rebuild_and_set_geometry_give_the_same_lists():
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    got = dev.list_overlaps(bx)
    bc.assert_same(got, (offsets, recs), "after rebuild_bvh: the bytes do not depend on the tree")
    bc.assert_same(got, _twin_lists(pc.with_nodes(hs.desc, dev.bvh_nodes()), bx), "after rebuild_bvh: the twin on the new nodes")
    # other contents, then the first ones again
    other = bc.scene("spheres")
    dev.set_geometry(other.desc)
    obx = bc.boxes_of("spheres")
    bc.assert_same(dev.list_overlaps(obx), _twin_lists(pc.with_nodes(other.desc, dev.bvh_nodes()), obx), "after set_geometry: the twin on the new description")
    dev.set_geometry(hs.desc)
    bc.assert_same(dev.list_overlaps(bx), (offsets, recs), "after set_geometry of the first contents")
    dev.close()


def test_update_geometry_equals_the_twin_and_orders_behind_enqueued_queries():
    import torch
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    want4, _ = irl.box_fill_host(hs.desc, bx, bc.k_offsets(bx.size, 4))
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    # a fill enqueued before the update sees the old geometry
    many = np.tile(bx, 8)
    t_bx = _cuda(many)
    t_off = torch.arange(many.size + 1, dtype=torch.int64, device="cuda") * 4
    out = torch.zeros((many.size * 4, 4), dtype=torch.int32, device="cuda")
    with _OwnStream() as st:
        dev.box_fill_device(t_bx.data_ptr(), t_off.data_ptr(), out.data_ptr(), many.size * 4, many.size, st.cuda_stream)
        dev.update_geometry(vertices=v, spheres=s, discs=d)
        st.synchronize()
    old = out.cpu().numpy().view(irl.OVERLAP).reshape(8, bx.size, 4)
    want4 = want4.reshape(bx.size, 4)
    for rep in range(8):
        assert np.array_equal(old[rep]["box"], np.repeat(np.arange(bx.size, dtype=np.uint32) + rep * bx.size, 4).reshape(-1, 4))
        for f in ("primID", "geomID", "flags", "reserved"):
            assert old[rep][f].tobytes() == want4[f].tobytes(), f"enqueued before the update: the old geometry ({f}, copy {rep})"
    moved = dev.list_overlaps(bx)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    bc.assert_same(moved, _twin_lists(m.desc, bx), "after update_geometry: the twin on the moved arrays")
    assert moved[1].tobytes() != recs.tobytes()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. torch
# ------------------------------------------------------------------------------------------------------
def test_tensor_entries_on_a_non_default_stream():
    import torch
    hs, bx, offsets, recs, counts, anys, _ = bc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    lo, hi = torch.from_numpy(bx["lo"].copy()).cuda(), torch.from_numpy(bx["hi"].copy()).cuda()
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            t_any = dev.box_any(lo, hi)
            t_count = dev.box_count(lo, hi)
            t_off, t_recs = dev.box_list(lo, hi)
        st.synchronize()
        got = (t_any.cpu(), t_count.cpu(), t_off.cpu(), t_recs.cpu())
        del t_any, t_count, t_off, t_recs
    t_any, t_count, t_off, t_recs = got
    assert t_any.dtype == torch.bool and np.array_equal(t_any.cpu().numpy(), anys)
    assert t_count.dtype == torch.int32 and np.array_equal(t_count.cpu().numpy().view(np.uint32), counts)
    assert t_off.dtype == torch.int64 and np.array_equal(t_off.cpu().numpy().view(np.uint64), offsets)
    assert t_recs.shape == (recs.size, 4) and t_recs.cpu().numpy().tobytes() == recs.tobytes()
    dev.close()


def test_voxelize_equals_the_twin_on_the_same_cells():
    import torch
    hs = bc.scene("box")
    lo, hi = pc.root_box(hs.nodes)
    # a grid of 8^3 cells whose planes are exact in binary32 and which holds the scene: origin and cell are powers of two times integers
    cell = F(2.0 ** np.ceil(np.log2(float((hi - lo).max()) / 6.0)))
    origin = (np.floor(lo / cell) * cell - cell).astype(F)
    assert np.all(origin + 8 * cell > hi)
    dev = irl.IpuScene(hs.desc)
    grid = dev.voxelize(tuple(float(x) for x in origin), float(cell), (8, 8, 8))
    assert grid.dtype == torch.bool and tuple(grid.shape) == (8, 8, 8)
    idx = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3).astype(F)
    cells = qb.make_boxes((origin + idx * cell).astype(F), (origin + (idx + F(1)) * cell).astype(F))
    want, _ = irl.box_query_host(hs.desc, bc.ANY, cells)
    got = grid.cpu().numpy()
    assert np.array_equal(got.reshape(-1), want)
    assert 0 < got.sum() < 512
    # neighbouring cells share their faces bit for bit: a wall lying in a grid plane sets the cells on both sides of it
    wall = pc.hand_scene(tris=[((0.0, 0.0, 4.0), (8.0, 0.0, 4.0), (0.0, 8.0, 4.0)), ((8.0, 8.0, 4.0), (8.0, 0.0, 4.0), (0.0, 8.0, 4.0))])
    flat = irl.IpuScene(wall.desc)
    g = flat.voxelize((0.0, 0.0, 0.0), 1.0, (8, 8, 8)).cpu().numpy()
    assert g[:, :, 3].all() and g[:, :, 4].all() and not g[:, :, :3].any() and not g[:, :, 5:].any()
    flat.close()
    dev.close()
