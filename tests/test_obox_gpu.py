"""Oriented-box queries on the GPU (pytest -m gpu): mi_obox_query* / mi_obox_offsets* / mi_obox_fill* against the host twins
mi_obox_query_host / mi_obox_offsets_host / mi_obox_fill_host, byte for byte - any, count, offsets and fill with their visit totals,
the workgroup's and the prefix sum's edges, host batches of 48-byte items with offsets that do not ascend, the heap's sift paths,
canaries, the 24 exact rotations against the box queries, live scenes, options, the tensor entries on a stream, and the other
families' lists before and after (the pipeline's input slots grew)."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc
import box_cases as bc
import obox_cases as oc
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


FRONT = 64      # bytes of canary in front of every output the helpers below hand to an entry (a multiple of 16: the hits' alignment)
CANARY = 0x7F


def _guarded(nbytes, on_device):
    """A buffer of FRONT + nbytes + FRONT canary bytes (a torch device tensor or a 16-byte aligned numpy array) and the address of
    its interior: what an entry is handed, so that a write in front of an output shows as well as one behind it."""
    import torch
    if on_device:
        whole = torch.full((FRONT + nbytes + FRONT,), CANARY, dtype=torch.uint8, device="cuda")
        return whole, whole.data_ptr() + FRONT
    whole = irl.aligned_bytes(FRONT + nbytes + FRONT)
    whole[:] = CANARY
    return whole, whole.ctypes.data + FRONT


def _interior(whole, nbytes, dtype, what):
    """The interior of a _guarded buffer as `dtype`, once both margins are seen intact."""
    raw = whole.cpu().numpy() if hasattr(whole, "cpu") else whole
    assert (raw[:FRONT] == CANARY).all(), f"{what}: something was written in front of the output"
    assert (raw[FRONT + nbytes:] == CANARY).all(), f"{what}: something was written behind the output"
    return raw[FRONT:FRONT + nbytes].copy().view(dtype)


def _device_query(dev, kind, bx, stream=0):
    import torch
    t_bx = _cuda(bx)
    nbytes = bx.size * (1 if kind == oc.ANY else 4)
    whole, ptr = _guarded(nbytes, True)
    dev.obox_query_device(kind, t_bx.data_ptr(), ptr, bx.size, stream)
    torch.cuda.synchronize()
    return _interior(whole, nbytes, np.bool_ if kind == oc.ANY else np.uint32, "any / count, device entry")


def _device_offsets(dev, bx, stream=0):
    import torch
    t_bx = _cuda(bx)
    whole, ptr = _guarded((bx.size + 1) * 8, True)
    dev.obox_offsets_device(t_bx.data_ptr(), ptr, bx.size, stream)
    torch.cuda.synchronize()
    return _interior(whole, (bx.size + 1) * 8, np.uint64, "offsets, device entry")


FRONT_RECS = FRONT // 16


def _device_fill(dev, bx, offsets, total, capacity=None):
    """The device entry into a sentinel buffer of FRONT_RECS + `total` (+ 64) records, handed over from record FRONT_RECS on; returns
    the buffer from there on, once the records in front are seen to be sentinels still."""
    import torch
    t_bx, t_off, t_buf = _cuda(bx), _cuda(offsets.astype(np.uint64)), _cuda(bc.sentinel_buffer(total + FRONT_RECS))
    dev.obox_fill_device(t_bx.data_ptr(), t_off.data_ptr(), t_buf.data_ptr() + FRONT, total if capacity is None else capacity, bx.size)
    torch.cuda.synchronize()
    buf = t_buf.cpu().numpy().view(irl.OVERLAP)
    assert bc.is_sentinel(buf[:FRONT_RECS]).all(), "fill, device entry: something was written in front of the hits"
    return buf[FRONT_RECS:]


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
    hs, bx, offsets, recs, counts, anys, v = oc.twin(name)
    dev = irl.IpuScene(hs.desc, variants=variants)
    assert np.array_equal(dev.obox_touches(bx), anys) and np.array_equal(_device_query(dev, oc.ANY, bx), anys), f"{name}: any"
    assert np.array_equal(dev.count_obox_overlaps(bx), counts) and np.array_equal(_device_query(dev, oc.COUNT, bx), counts), f"{name}: count"
    got = dev.list_obox_overlaps(bx)
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.OVERLAP and got[0][0] == 0 and got[0][-1] == got[1].size
    bc.assert_same(got, (offsets, recs), f"{name}: host entries")
    assert np.array_equal(_device_offsets(dev, bx), offsets), f"{name}: offsets, device entry"
    buf = _device_fill(dev, bx, offsets, recs.size)
    pc.assert_bytes_equal(buf[:recs.size], recs, f"{name}: fill, device entry")
    assert bc.is_sentinel(buf[recs.size:]).all()
    for k in (1, 4):
        want, _ = irl.obox_fill_host(hs.desc, bx, bc.k_offsets(bx.size, k))
        pc.assert_bytes_equal(dev.first_obox_overlaps(bx, k).reshape(-1), want, f"{name}: the first {k}, host entry")
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    # the instrumented build: the same bytes and the twin's visit totals
    dev.set_option("full_stats", 1)
    calls = (("any", lambda: dev.obox_touches(bx), anys), ("count", lambda: dev.count_obox_overlaps(bx), counts),
             ("offsets", lambda: dev.obox_offsets(bx), offsets),
             ("fill", lambda: dev.obox_fill(bx, offsets, bc.sentinel_buffer(recs.size), recs.size)[:recs.size], recs))
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
    hs, bx, offsets, recs, counts, anys, _ = oc.twin("soup", 257)
    dev = irl.IpuScene(hs.desc)
    sub = bx[:n]
    assert np.array_equal(_device_query(dev, oc.ANY, sub), anys[:n]) and np.array_equal(_device_query(dev, oc.COUNT, sub), counts[:n])
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
    bx = qb.make_oboxes(np.tile(far, (n, 1)), np.ones((n, 3), F), quat=oc.random_quats(np.random.default_rng(3), n))
    bx["centre"][-1], bx["half"][-1] = (lo + hi) * F(0.5), (hi - lo)
    want = np.zeros(n + 1, np.uint64)
    want[-1] = 602
    assert np.array_equal(irl.obox_offsets_host(hs.desc, bx)[0], want)
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(_device_offsets(dev, bx), want) and np.array_equal(dev.obox_offsets(bx), want)
    dev.close()


@pytest.mark.parametrize("batch", [1, 7, 300])
def test_host_batches_and_offsets_that_do_not_ascend(batch):
    """48-byte items through the two-slot pipeline: batches of 1, 7 and the whole set (300: the 150 queries given twice)."""
    hs, bx, offsets, recs, counts, anys, _ = oc.twin("soup")
    assert bx.size == 150
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(batch)
    assert np.array_equal(dev.obox_touches(bx), anys) and np.array_equal(dev.count_obox_overlaps(bx), counts)
    got = dev.list_obox_overlaps(bx)
    oc.assert_same(got, (offsets, recs), f"batches of {batch}")
    assert np.array_equal(got[1]["box"], np.repeat(np.arange(bx.size, dtype=np.uint32), counts.astype(np.int64))), "box indices are global"
    want4, _ = irl.obox_fill_host(hs.desc, bx, oc.k_offsets(bx.size, 4))
    pc.assert_bytes_equal(dev.first_obox_overlaps(bx, 4).reshape(-1), want4, f"the first 4 in batches of {batch}")
    # offsets that do not ascend - the segments laid out back to front, one untouched record behind each, every item followed by
    # an empty decreasing pair -: the pipeline copies such a batch item by item
    pairs = np.repeat(bx, 2)
    pair_off, total = _gapped(counts, 1)
    want = oc.sentinel_buffer(total)
    irl.obox_fill_host(hs.desc, pairs, pair_off, capacity=total, hits=want)
    assert oc.is_sentinel(want).sum() == bx.size + 64, "the gaps and the tail keep their canaries"
    buf = oc.sentinel_buffer(total)
    dev.obox_fill(pairs, pair_off, buf, total)
    assert buf.tobytes() == want.tobytes(), f"host entry in batches of {batch}"
    if batch == 7:
        assert _device_fill(dev, pairs, pair_off, total).tobytes() == want.tobytes(), "device entry"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. the heap, canaries
# ------------------------------------------------------------------------------------------------------
def test_heap_sift_paths():
    """One turned box over the whole soup: segments of 1, 2, 3, 7, 8, count - 1, count and count + 5 records receive the head of the
    full list, padded."""
    hs = bc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    bx = qb.make_oboxes(((lo + hi) * F(0.5))[None], (hi - lo)[None], quat=np.array([[0.3, -0.5, 0.2, 0.8]], F))
    offsets, _ = irl.obox_offsets_host(hs.desc, bx)
    full, _ = irl.obox_fill_host(hs.desc, bx, offsets)
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
    irl.obox_fill_host(hs.desc, pair_bx, pair_off, capacity=total, hits=want)
    assert buf.tobytes() == want.tobytes(), "the twin"
    dev.close()


def test_nothing_is_written_past_capacity():
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    total = recs.size
    dev = irl.IpuScene(hs.desc)
    for capacity in (total - 1, total // 2, 0):
        want, _ = irl.obox_fill_host(hs.desc, bx, offsets, capacity=capacity, hits=bc.sentinel_buffer(total))
        assert bc.is_sentinel(want[capacity:]).all()
        buf = bc.sentinel_buffer(total)
        dev.obox_fill(bx, offsets, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, capacity {capacity}"
        assert _device_fill(dev, bx, offsets, total, capacity).tobytes() == want.tobytes(), f"device entry, capacity {capacity}"
    dev.close()


def test_canaries_on_both_sides_of_every_output():
    """any, count, offsets and hits of the HOST entries written into the interior of canary buffers (the device entries go through
    _device_query / _device_offsets / _device_fill, which do the same on device memory in every test above): nothing in front,
    nothing behind, the twin's bytes between - whole, in batches of 7, and with a capacity that cuts the fill."""
    hs, bx, offsets, recs, counts, anys, _ = oc.twin("soup")
    n, total = bx.size, recs.size
    dev = irl.IpuScene(hs.desc)
    lib, h = dev._lib, dev._h
    src = irl.IpuScene._source(bx, irl.OBOX)
    for batch in (0, 7):
        if batch:
            dev.setRayBatch(batch)
        for kind, want, dtype in ((oc.ANY, anys, np.bool_), (oc.COUNT, counts, np.uint32)):
            whole, ptr = _guarded(want.nbytes, False)
            dev._check(lib.mi_obox_query(h, kind, src.ctypes.data, ptr, n))
            assert np.array_equal(_interior(whole, want.nbytes, dtype, f"host entry, kind {kind}, batch {batch}"), want)
        whole, ptr = _guarded(offsets.nbytes, False)
        dev._check(lib.mi_obox_offsets(h, src.ctypes.data, ptr, n))
        assert np.array_equal(_interior(whole, offsets.nbytes, np.uint64, f"host offsets, batch {batch}"), offsets)
        for capacity in (total, total // 2):
            whole, ptr = _guarded(total * 16, False)
            dev._check(lib.mi_obox_fill(h, src.ctypes.data, offsets.ctypes.data, ptr, capacity, n))
            got = _interior(whole, total * 16, irl.OVERLAP, f"host fill, capacity {capacity}, batch {batch}")
            want, _ = irl.obox_fill_host(hs.desc, bx, offsets, capacity=capacity, hits=oc.sentinel_buffer(total)[:total])
            cut = np.frombuffer(bytes([CANARY]) * (16 * (total - capacity)), irl.OVERLAP)
            pc.assert_bytes_equal(got[:capacity], want[:capacity], f"host fill, capacity {capacity}, batch {batch}")
            assert got[capacity:].tobytes() == cut.tobytes(), "nothing at or past capacity"
        # the device entries once more, explicitly: the same margins on device memory
        assert np.array_equal(_device_query(dev, oc.ANY, bx), anys) and np.array_equal(_device_query(dev, oc.COUNT, bx), counts)
        assert np.array_equal(_device_offsets(dev, bx), offsets)
        pc.assert_bytes_equal(_device_fill(dev, bx, offsets, total)[:total], recs, "device fill between canaries")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. live scenes
# ------------------------------------------------------------------------------------------------------
def _twin_lists(desc, bx):
    return oc.full(desc, bx)


def test_rebuild_and_set_geometry_give_the_same_lists():
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    got = dev.list_obox_overlaps(bx)
    bc.assert_same(got, (offsets, recs), "after rebuild_bvh: the bytes do not depend on the tree")
    bc.assert_same(got, _twin_lists(pc.with_nodes(hs.desc, dev.bvh_nodes()), bx), "after rebuild_bvh: the twin on the new nodes")
    # other contents, then the first ones again
    other = bc.scene("spheres")
    dev.set_geometry(other.desc)
    obx = oc.oboxes_of("spheres")
    bc.assert_same(dev.list_obox_overlaps(obx), _twin_lists(pc.with_nodes(other.desc, dev.bvh_nodes()), obx), "after set_geometry: the twin on the new description")
    dev.set_geometry(hs.desc)
    bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), "after set_geometry of the first contents")
    dev.close()


def test_update_geometry_equals_the_twin_and_orders_behind_enqueued_queries():
    import torch
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    want4, _ = irl.obox_fill_host(hs.desc, bx, bc.k_offsets(bx.size, 4))
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    # a fill enqueued before the update sees the old geometry
    many = np.tile(bx, 8)
    t_bx = _cuda(many)
    t_off = torch.arange(many.size + 1, dtype=torch.int64, device="cuda") * 4
    out = torch.zeros((many.size * 4, 4), dtype=torch.int32, device="cuda")
    with _OwnStream() as st:
        dev.obox_fill_device(t_bx.data_ptr(), t_off.data_ptr(), out.data_ptr(), many.size * 4, many.size, st.cuda_stream)
        dev.update_geometry(vertices=v, spheres=s, discs=d)
        st.synchronize()
    old = out.cpu().numpy().view(irl.OVERLAP).reshape(8, bx.size, 4)
    want4 = want4.reshape(bx.size, 4)
    for rep in range(8):
        assert np.array_equal(old[rep]["box"], np.repeat(np.arange(bx.size, dtype=np.uint32) + rep * bx.size, 4).reshape(-1, 4))
        for f in ("primID", "geomID", "flags", "reserved"):
            assert old[rep][f].tobytes() == want4[f].tobytes(), f"enqueued before the update: the old geometry ({f}, copy {rep})"
    moved = dev.list_obox_overlaps(bx)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    bc.assert_same(moved, _twin_lists(m.desc, bx), "after update_geometry: the twin on the moved arrays")
    assert moved[1].tobytes() != recs.tobytes()
    fresh = irl.IpuScene(m.desc)
    bc.assert_same(fresh.list_obox_overlaps(bx), moved, "a fresh scene of the moved contents")
    fresh.close()
    # the same contents again, by a refit: the first lists, byte for byte
    dev.update_geometry(vertices=hs.verts.copy(), spheres=hs.spheres.copy(), discs=hs.discs.copy())
    bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), "a refit back to the first contents")
    dev.close()


def test_options_change_nothing():
    hs, bx, offsets, recs, counts, anys, _ = oc.twin("soup")
    for option, value in (("double_fallback", 1), ("fast", 1), ("query_kernel", 1), ("hot_nodes", 64)):
        dev = irl.IpuScene(hs.desc)
        dev.set_option(option, value)
        assert np.array_equal(dev.obox_touches(bx), anys) and np.array_equal(dev.count_obox_overlaps(bx), counts), option
        bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), option)
        dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. the exact rotations on the device, and the other families beside this one
# ------------------------------------------------------------------------------------------------------
def test_the_24_cube_rotations_equal_the_box_queries_on_the_device():
    hs = oc.dyadic_scene()
    rng = np.random.default_rng(72)
    rows_o, rows_b = [], []
    for q, absR in oc.cube_rotations():
        centre = (rng.integers(-12, 13, (12, 3)) * 0.5).astype(F)
        half = (rng.integers(0, 13, (12, 3)) * 0.5).astype(F)
        world = (half.astype(np.float64) @ absR.T).astype(F)
        rows_o += list(zip(centre, half, [q] * 12))
        rows_b += list(zip(centre - world, centre + world))
    ob, ab = oc.oboxes(rows_o), bc.boxes(rows_b)
    dev = irl.IpuScene(hs.desc)
    got, want = dev.list_obox_overlaps(ob), dev.list_overlaps(ab)
    bc.assert_same(got, want, "the 24 rotations: list_overlaps of the permuted axis-aligned boxes")
    assert np.array_equal(dev.count_obox_overlaps(ob), dev.count_overlaps(ab)) and np.array_equal(dev.obox_touches(ob), dev.touches(ab))
    assert got[1].size > 1000 and 0 < (got[1]["flags"] == irl.OVERLAP_CONTAINED).sum() < got[1].size
    dev.set_option("full_stats", 1)
    visits = []
    for call in (lambda: dev.obox_offsets(ob), lambda: dev.box_offsets(ab)):
        dev.reset_counters()
        call()
        c = dev.counters()
        visits.append((c["nodes_visited"], c["leaf_tests"]))
    assert visits[0] == visits[1] and visits[0][0] > 0, "the slabs pass exactly what the six compares pass"
    dev.close()


def test_the_other_families_lists_are_what_they_were():
    """The pipeline's input slots grew from 36 to 48 bytes an item: a box list and a contact list through the host entries before
    and after a batch of oriented-box queries, in batches of 7, are the same bytes (and the twins')."""
    import tri_cases as tc
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    _, ab, b_off, b_recs, _, _, _ = bc.twin("soup")
    _, tq, t_off, t_recs, _, _, _ = tc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(7)
    before = (dev.list_overlaps(ab[:60]), dev.list_contacts(tq[:60]))
    bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), "the oriented boxes between them")
    after = (dev.list_overlaps(ab[:60]), dev.list_contacts(tq[:60]))
    for what, x, y in (("list_overlaps", before[0], after[0]), ("list_contacts", before[1], after[1])):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes(), what
    assert before[0][0].tobytes() == b_off[:61].tobytes() and before[0][1].tobytes() == b_recs[:int(b_off[60])].tobytes()
    assert before[1][0].tobytes() == t_off[:61].tobytes() and before[1][1].tobytes() == t_recs[:int(t_off[60])].tobytes()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 6. torch
# ------------------------------------------------------------------------------------------------------
def test_tensor_entries_on_a_non_default_stream():
    import torch
    hs, bx, offsets, recs, counts, anys, _ = oc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    c, h, q = (torch.from_numpy(bx[f].copy()).cuda() for f in ("centre", "half", "quat"))
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            t_any = dev.obox_any(c, h, q)
            t_count = dev.obox_count(c, h, q)
            t_off, t_recs = dev.obox_list(c, h, q)
        st.synchronize()
        got = (t_any.cpu(), t_count.cpu(), t_off.cpu(), t_recs.cpu())
        del t_any, t_count, t_off, t_recs
    t_any, t_count, t_off, t_recs = got
    assert t_any.dtype == torch.bool and np.array_equal(t_any.cpu().numpy(), anys)
    assert t_count.dtype == torch.int32 and np.array_equal(t_count.cpu().numpy().view(np.uint32), counts)
    assert t_off.dtype == torch.int64 and np.array_equal(t_off.cpu().numpy().view(np.uint64), offsets)
    assert t_recs.shape == (recs.size, 4) and t_recs.cpu().numpy().tobytes() == recs.tobytes()
    dev.close()
