"""Frustum queries on the GPU (pytest -m gpu): mi_frustum_query* / mi_frustum_offsets* / mi_frustum_fill* against the host twins
mi_frustum_query_host / mi_frustum_offsets_host / mi_frustum_fill_host, byte for byte - any, count, offsets and fill with their visit
totals, the workgroup's and the prefix sum's edges, host batches of 96-byte items with offsets that do not ascend, the heap's sift
paths, canaries, live scenes (update, poses, rebuild, set-geometry, a refit back), options, the tensor entries on a stream, cull, and
the other families' lists before and after."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc
import box_cases as bc
import frustum_cases as fc
import refit_cases as rc
import pose_cases as po

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


def _device_query(dev, kind, fr, stream=0):
    import torch
    t_fr = _cuda(fr)
    nbytes = fr.size * (1 if kind == fc.ANY else 4)
    whole, ptr = _guarded(nbytes, True)
    dev.frustum_query_device(kind, t_fr.data_ptr(), ptr, fr.size, stream)
    torch.cuda.synchronize()
    return _interior(whole, nbytes, np.bool_ if kind == fc.ANY else np.uint32, "any / count, device entry")


def _device_offsets(dev, fr, stream=0):
    import torch
    t_fr = _cuda(fr)
    whole, ptr = _guarded((fr.size + 1) * 8, True)
    dev.frustum_offsets_device(t_fr.data_ptr(), ptr, fr.size, stream)
    torch.cuda.synchronize()
    return _interior(whole, (fr.size + 1) * 8, np.uint64, "offsets, device entry")


FRONT_RECS = FRONT // 16


def _device_fill(dev, fr, offsets, total, capacity=None):
    """The device entry into a sentinel buffer of FRONT_RECS + `total` (+ 64) records, handed over from record FRONT_RECS on; returns
    the buffer from there on, once the records in front are seen to be sentinels still."""
    import torch
    t_fr, t_off, t_buf = _cuda(fr), _cuda(offsets.astype(np.uint64)), _cuda(bc.sentinel_buffer(total + FRONT_RECS))
    dev.frustum_fill_device(t_fr.data_ptr(), t_off.data_ptr(), t_buf.data_ptr() + FRONT, total if capacity is None else capacity, fr.size)
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
    hs, fr, offsets, recs, counts, anys, v = fc.twin(name)
    dev = irl.IpuScene(hs.desc, variants=variants)
    assert np.array_equal(dev.frustum_touches(fr), anys) and np.array_equal(_device_query(dev, fc.ANY, fr), anys), f"{name}: any"
    assert np.array_equal(dev.count_frustum_overlaps(fr), counts) and np.array_equal(_device_query(dev, fc.COUNT, fr), counts), f"{name}: count"
    got = dev.list_frustum_overlaps(fr)
    assert got[0].dtype == np.uint64 and got[1].dtype == irl.OVERLAP and got[0][0] == 0 and got[0][-1] == got[1].size
    bc.assert_same(got, (offsets, recs), f"{name}: host entries")
    assert np.array_equal(_device_offsets(dev, fr), offsets), f"{name}: offsets, device entry"
    buf = _device_fill(dev, fr, offsets, recs.size)
    pc.assert_bytes_equal(buf[:recs.size], recs, f"{name}: fill, device entry")
    assert bc.is_sentinel(buf[recs.size:]).all()
    for k in (1, 4):
        want, _ = irl.frustum_fill_host(hs.desc, fr, bc.k_offsets(fr.size, k))
        pc.assert_bytes_equal(dev.first_frustum_overlaps(fr, k).reshape(-1), want, f"{name}: the first {k}, host entry")
    c = dev.counters()
    assert c["casts"] == 0 and c["paths"] == 0 and c["nodes_visited"] == 0 and c["leaf_tests"] == 0
    # the instrumented build: the same bytes and the twin's visit totals
    dev.set_option("full_stats", 1)
    calls = (("any", lambda: dev.frustum_touches(fr), anys), ("count", lambda: dev.count_frustum_overlaps(fr), counts),
             ("offsets", lambda: dev.frustum_offsets(fr), offsets),
             ("fill", lambda: dev.frustum_fill(fr, offsets, bc.sentinel_buffer(recs.size), recs.size)[:recs.size], recs))
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
    hs, fr, _, _, counts, _, _ = fc.twin("soup", 257)
    sub = np.roll(fr, -int(np.nonzero(counts)[0][0]))[:n]          # (from the first frustum that lists something: n = 1 has a list)
    offsets, recs = fc.full(hs.desc, sub)
    total = int(offsets[n])
    assert total > 0
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(_device_query(dev, fc.ANY, sub), irl.frustum_query_host(hs.desc, fc.ANY, sub)[0])
    assert np.array_equal(_device_query(dev, fc.COUNT, sub), np.diff(offsets).astype(np.uint32))
    assert np.array_equal(_device_offsets(dev, sub), offsets)
    buf = _device_fill(dev, sub, offsets, total)
    pc.assert_bytes_equal(buf[:total], recs, f"fill, n = {n}")
    assert bc.is_sentinel(buf[total:]).all()
    dev.close()


def test_scan_tile_edge():
    """One frustum more than a tile of the prefix sum (2048), every frustum empty but the last: its count crosses the tile's edge."""
    hs = bc.scene("soup")
    lo, hi = pc.root_box(hs.nodes)
    n = 2049
    far = (hi + F(100)).astype(F)
    fr = np.repeat(fc.frusta([fc.cube(far, far + F(1))]), n)
    fr["planes"][-1] = 0.0                                         # six absent planes: the whole scene
    want = np.zeros(n + 1, np.uint64)
    want[-1] = 602
    assert np.array_equal(irl.frustum_offsets_host(hs.desc, fr)[0], want)
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(_device_offsets(dev, fr), want) and np.array_equal(dev.frustum_offsets(fr), want)
    assert np.array_equal(_device_query(dev, fc.COUNT, fr), np.diff(want).astype(np.uint32)) and _device_query(dev, fc.ANY, fr).sum() == 1
    dev.close()


@pytest.mark.parametrize("batch", [1, 7, 300])
def test_host_batches_and_offsets_that_do_not_ascend(batch):
    """96-byte items - the largest there are, the ones that size the slots - through the two-slot pipeline: any, count, lists and the first 4 of the 150 queries in batches of 1, 7 and 300 (one
    batch, larger than the set); the gapped fill gives every query twice, 300 items, so that there 300 is exactly the whole set."""
    hs, fr, offsets, recs, counts, anys, _ = fc.twin("soup")
    assert fr.size == 150
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(batch)
    assert np.array_equal(dev.frustum_touches(fr), anys) and np.array_equal(dev.count_frustum_overlaps(fr), counts)
    got = dev.list_frustum_overlaps(fr)
    fc.assert_same(got, (offsets, recs), f"batches of {batch}")
    assert np.array_equal(got[1]["box"], np.repeat(np.arange(fr.size, dtype=np.uint32), counts.astype(np.int64))), "box indices are global"
    want4, _ = irl.frustum_fill_host(hs.desc, fr, fc.k_offsets(fr.size, 4))
    pc.assert_bytes_equal(dev.first_frustum_overlaps(fr, 4).reshape(-1), want4, f"the first 4 in batches of {batch}")
    # offsets that do not ascend - the segments laid out back to front, one untouched record behind each, every item followed by
    # an empty decreasing pair -: the pipeline copies such a batch item by item
    pairs = np.repeat(fr, 2)
    pair_off, total = _gapped(counts, 1)
    want = fc.sentinel_buffer(total)
    irl.frustum_fill_host(hs.desc, pairs, pair_off, capacity=total, hits=want)
    assert fc.is_sentinel(want).sum() == fr.size + 64, "the gaps and the tail keep their canaries"
    buf = fc.sentinel_buffer(total)
    dev.frustum_fill(pairs, pair_off, buf, total)
    assert buf.tobytes() == want.tobytes(), f"host entry in batches of {batch}"
    if batch == 7:
        assert _device_fill(dev, pairs, pair_off, total).tobytes() == want.tobytes(), "device entry"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. the heap, canaries
# ------------------------------------------------------------------------------------------------------
def test_heap_sift_paths():
    """One frustum of six absent planes over the whole soup: segments of 1, 2, 3, 7, 8, count - 1, count and count + 5 records receive the head of the
    full list, padded."""
    hs = bc.scene("soup")
    fr = fc.frusta([[]])                                           # six absent planes
    offsets, _ = irl.frustum_offsets_host(hs.desc, fr)
    full, _ = irl.frustum_fill_host(hs.desc, fr, offsets)
    count = int(offsets[1])
    assert count == 602
    lens = [1, 2, 3, 7, 8, count - 1, count, count + 5]
    pair_fr = np.repeat(fr, 2 * len(lens))
    pair_off, total = _gapped(lens, 2)                                                   # two canaries behind every segment
    offs = pair_off[0::2]
    dev = irl.IpuScene(hs.desc)
    buf = _device_fill(dev, pair_fr, pair_off, total)
    for j, ln in enumerate(lens):
        seg = buf[int(offs[j]):int(offs[j]) + ln]
        want = np.concatenate([full[:ln], bc.records([], 0, max(ln - count, 0))]).copy()
        want["box"] = 2 * j
        pc.assert_bytes_equal(seg, want, f"len = {ln}: the head of the full list")
        assert bc.is_sentinel(buf[int(offs[j]) + ln:int(offs[j]) + ln + 2]).all(), f"len = {ln}: the canaries behind the segment"
    assert bc.is_sentinel(buf[total:]).all()
    want = bc.sentinel_buffer(total)
    irl.frustum_fill_host(hs.desc, pair_fr, pair_off, capacity=total, hits=want)
    assert buf.tobytes() == want.tobytes(), "the twin"
    dev.close()


def test_nothing_is_written_past_capacity():
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    total = recs.size
    dev = irl.IpuScene(hs.desc)
    for capacity in (total - 1, total // 2, 0):
        want, _ = irl.frustum_fill_host(hs.desc, fr, offsets, capacity=capacity, hits=bc.sentinel_buffer(total))
        assert bc.is_sentinel(want[capacity:]).all()
        buf = bc.sentinel_buffer(total)
        dev.frustum_fill(fr, offsets, buf, capacity)
        assert buf.tobytes() == want.tobytes(), f"host entry, capacity {capacity}"
        assert _device_fill(dev, fr, offsets, total, capacity).tobytes() == want.tobytes(), f"device entry, capacity {capacity}"
    dev.close()


def test_canaries_on_both_sides_of_every_output():
    """any, count, offsets and hits of the HOST entries written into the interior of canary buffers (the device entries go through
    _device_query / _device_offsets / _device_fill, which do the same on device memory in every test above): nothing in front,
    nothing behind, the twin's bytes between - whole, in batches of 7, and with a capacity that cuts the fill."""
    hs, fr, offsets, recs, counts, anys, _ = fc.twin("soup")
    n, total = fr.size, recs.size
    dev = irl.IpuScene(hs.desc)
    lib, h = dev._lib, dev._h
    src = irl.IpuScene._source(fr, irl.FRUSTUM)
    for batch in (0, 7):
        if batch:
            dev.setRayBatch(batch)
        for kind, want, dtype in ((fc.ANY, anys, np.bool_), (fc.COUNT, counts, np.uint32)):
            whole, ptr = _guarded(want.nbytes, False)
            dev._check(lib.mi_frustum_query(h, kind, src.ctypes.data, ptr, n))
            assert np.array_equal(_interior(whole, want.nbytes, dtype, f"host entry, kind {kind}, batch {batch}"), want)
        whole, ptr = _guarded(offsets.nbytes, False)
        dev._check(lib.mi_frustum_offsets(h, src.ctypes.data, ptr, n))
        assert np.array_equal(_interior(whole, offsets.nbytes, np.uint64, f"host offsets, batch {batch}"), offsets)
        for capacity in (total, total // 2):
            whole, ptr = _guarded(total * 16, False)
            dev._check(lib.mi_frustum_fill(h, src.ctypes.data, offsets.ctypes.data, ptr, capacity, n))
            got = _interior(whole, total * 16, irl.OVERLAP, f"host fill, capacity {capacity}, batch {batch}")
            want, _ = irl.frustum_fill_host(hs.desc, fr, offsets, capacity=capacity, hits=fc.sentinel_buffer(total)[:total])
            cut = np.frombuffer(bytes([CANARY]) * (16 * (total - capacity)), irl.OVERLAP)
            pc.assert_bytes_equal(got[:capacity], want[:capacity], f"host fill, capacity {capacity}, batch {batch}")
            assert got[capacity:].tobytes() == cut.tobytes(), "nothing at or past capacity"
        # the device entries once more, explicitly: the same margins on device memory
        assert np.array_equal(_device_query(dev, fc.ANY, fr), anys) and np.array_equal(_device_query(dev, fc.COUNT, fr), counts)
        assert np.array_equal(_device_offsets(dev, fr), offsets)
        pc.assert_bytes_equal(_device_fill(dev, fr, offsets, total)[:total], recs, "device fill between canaries")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. live scenes
# ------------------------------------------------------------------------------------------------------
def _twin_lists(desc, fr):
    return fc.full(desc, fr)


def test_rebuild_and_set_geometry_give_the_same_lists():
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    before = dev.bvh_nodes().tobytes()
    dev.rebuild_bvh()
    assert dev.bvh_nodes().tobytes() != before, "the rebuild left the tree as it was"
    got = dev.list_frustum_overlaps(fr)
    bc.assert_same(got, (offsets, recs), "after rebuild_bvh: the bytes do not depend on the tree")
    bc.assert_same(got, _twin_lists(pc.with_nodes(hs.desc, dev.bvh_nodes()), fr), "after rebuild_bvh: the twin on the new nodes")
    # other contents, then the first ones again
    other = bc.scene("spheres")
    dev.set_geometry(other.desc)
    ofr = fc.frusta_of("spheres")
    bc.assert_same(dev.list_frustum_overlaps(ofr), _twin_lists(pc.with_nodes(other.desc, dev.bvh_nodes()), ofr), "after set_geometry: the twin on the new description")
    dev.set_geometry(hs.desc)
    bc.assert_same(dev.list_frustum_overlaps(fr), (offsets, recs), "after set_geometry of the first contents")
    dev.close()


def test_set_poses_equals_the_twin_on_the_posed_arrays():
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    p = po.seeded_poses(hs, 7)
    p["translation"] *= F(0.25)
    dev.set_poses(p)
    want = po.posed(hs, p)
    got = dev.list_frustum_overlaps(fr)
    bc.assert_same(got, _twin_lists(want.desc, fr), "after set_poses: the twin on the posed arrays")
    assert got[1].tobytes() != recs.tobytes()
    dev.set_poses(qb.make_poses(p.size))
    bc.assert_same(dev.list_frustum_overlaps(fr), (offsets, recs), "the identity poses bring the rest scene's lists back")
    dev.close()


def test_update_geometry_equals_the_twin_and_orders_behind_enqueued_queries():
    import torch
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    want4, _ = irl.frustum_fill_host(hs.desc, fr, bc.k_offsets(fr.size, 4))
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, seed=5, scale=0.25)
    # a fill enqueued before the update sees the old geometry
    many = np.tile(fr, 8)
    t_fr = _cuda(many)
    t_off = torch.arange(many.size + 1, dtype=torch.int64, device="cuda") * 4
    out = torch.zeros((many.size * 4, 4), dtype=torch.int32, device="cuda")
    with _OwnStream() as st:
        dev.frustum_fill_device(t_fr.data_ptr(), t_off.data_ptr(), out.data_ptr(), many.size * 4, many.size, st.cuda_stream)
        dev.update_geometry(vertices=v, spheres=s, discs=d)
        st.synchronize()
    old = out.cpu().numpy().view(irl.OVERLAP).reshape(8, fr.size, 4)
    want4 = want4.reshape(fr.size, 4)
    for rep in range(8):
        assert np.array_equal(old[rep]["box"], np.repeat(np.arange(fr.size, dtype=np.uint32) + rep * fr.size, 4).reshape(-1, 4))
        for f in ("primID", "geomID", "flags", "reserved"):
            assert old[rep][f].tobytes() == want4[f].tobytes(), f"enqueued before the update: the old geometry ({f}, copy {rep})"
    moved = dev.list_frustum_overlaps(fr)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()          # (kept: its desc points into its arrays)
    bc.assert_same(moved, _twin_lists(m.desc, fr), "after update_geometry: the twin on the moved arrays")
    assert moved[1].tobytes() != recs.tobytes()
    fresh = irl.IpuScene(m.desc)
    bc.assert_same(fresh.list_frustum_overlaps(fr), moved, "a fresh scene of the moved contents")
    fresh.close()
    # the same contents again, by a refit: the first lists, byte for byte
    dev.update_geometry(vertices=hs.verts.copy(), spheres=hs.spheres.copy(), discs=hs.discs.copy())
    bc.assert_same(dev.list_frustum_overlaps(fr), (offsets, recs), "a refit back to the first contents")
    dev.close()


def test_options_change_nothing():
    hs, fr, offsets, recs, counts, anys, _ = fc.twin("soup")
    for option, value in (("double_fallback", 1), ("fast", 1), ("query_kernel", 1), ("hot_nodes", 64)):
        dev = irl.IpuScene(hs.desc)
        dev.set_option(option, value)
        assert np.array_equal(dev.frustum_touches(fr), anys) and np.array_equal(dev.count_frustum_overlaps(fr), counts), option
        bc.assert_same(dev.list_frustum_overlaps(fr), (offsets, recs), option)
        dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. the other families beside this one
# ------------------------------------------------------------------------------------------------------
def test_the_other_families_lists_are_what_they_were():
    """Box, triangle, oriented-box, capsule and neighbour lists of fixed batches through the host entries, in batches of 7, before and after
    frustum calls on the same scene: the same bytes (and the twins')."""
    import tri_cases as tc
    import obox_cases as oc
    import near_cases as nc
    import capsule_cases as cc
    hs, fr, offsets, recs, counts, anys, _ = fc.twin("soup")
    _, ab, b_off, b_recs, _, _, _ = bc.twin("soup")
    _, tq, t_off, t_recs, _, _, _ = tc.twin("soup")
    _, ob, o_off, o_recs, _, _, _ = oc.twin("soup")
    _, cq, c_off, c_recs, _, _, _ = cc.twin("soup")
    _, pts, n_off, n_recs, _, _ = nc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    dev.setRayBatch(7)

    def others():
        return (dev.list_overlaps(ab[:60]), dev.list_contacts(tq[:60]), dev.list_obox_overlaps(ob[:60]), dev.list_capsule_overlaps(cq[:60]),
                dev.neighbours(pts[:60]))

    before = others()
    bc.assert_same(dev.list_frustum_overlaps(fr), (offsets, recs), "the frusta between them")
    assert np.array_equal(dev.frustum_touches(fr), anys) and np.array_equal(dev.count_frustum_overlaps(fr), counts)
    pc.assert_bytes_equal(_device_fill(dev, fr, offsets, recs.size)[:recs.size], recs, "and through the device entry")
    after = others()
    names = ("list_overlaps", "list_contacts", "list_obox_overlaps", "list_capsule_overlaps", "neighbours")
    for what, x, y in zip(names, before, after):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes(), what
    for what, x, (off, rec) in zip(names, before, ((b_off, b_recs), (t_off, t_recs), (o_off, o_recs), (c_off, c_recs), (n_off, n_recs))):
        assert x[0].tobytes() == off[:61].tobytes() and x[1].tobytes() == rec[:int(off[60])].tobytes(), f"{what}: the twin"
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 6. torch
# ------------------------------------------------------------------------------------------------------
def test_tensor_entries_on_a_non_default_stream():
    import torch
    hs, fr, offsets, recs, counts, anys, _ = fc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    planes = torch.from_numpy(fr["planes"].copy()).cuda()
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            t_any = dev.frustum_any(planes)
            t_count = dev.frustum_count(planes)
            t_off, t_recs = dev.frustum_list(planes)
        st.synchronize()
        got = (t_any.cpu(), t_count.cpu(), t_off.cpu(), t_recs.cpu())
        del t_any, t_count, t_off, t_recs
    t_any, t_count, t_off, t_recs = got
    assert t_any.dtype == torch.bool and np.array_equal(t_any.cpu().numpy(), anys)
    assert t_count.dtype == torch.int32 and np.array_equal(t_count.cpu().numpy().view(np.uint32), counts)
    assert t_off.dtype == torch.int64 and np.array_equal(t_off.cpu().numpy().view(np.uint64), offsets)
    assert t_recs.shape == (recs.size, 4) and t_recs.cpu().numpy().tobytes() == recs.tobytes()
    with pytest.raises(ValueError, match="planes must be"):
        dev.frustum_any(planes[:, :5])
    dev.close()


def test_cull_is_one_frustums_list():
    """cull(view_proj) against list_frustum_overlaps on the frustum make_frusta makes of the same matrix, for both depth conventions, and
    against the twin."""
    hs = bc.scene("box")
    lo, hi = pc.root_box(hs.nodes)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    dev = irl.IpuScene(hs.desc)
    for depth in ("zo", "no"):
        m = qb.camera_view_proj(eye=0.5 * (lo64 + hi64) + (0.3, 0.1, 0.2) * (hi64 - lo64), forward=(-0.6, -0.2, -1.0), up=(0, 1, 0), fovy=np.radians(40.0),
                                aspect=1.5, near=0.01 * float((hi64 - lo64).max()), far=10.0 * float((hi64 - lo64).max()), depth=depth)
        fr = qb.make_frusta(view_proj=m, depth=depth)
        offsets, recs = dev.list_frustum_overlaps(fr)
        rows = dev.cull(m, depth=depth)
        assert rows.dtype == np.int64 and rows.shape == (recs.size, 2) and 0 < recs.size < 0.9 * len([1 for lf in fc.FrustumChecker(hs).leaf if lf is not None])
        assert np.array_equal(rows[:, 0], recs["geomID"]) and np.array_equal(rows[:, 1], recs["primID"])
        bc.assert_same((offsets, recs), fc.full(hs.desc, fr), f"cull, depth {depth}: the twin")
    dev.close()
