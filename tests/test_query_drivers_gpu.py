"""The host side the five query families share (csrc/query_drivers.hpp), on the GPU: every host entry through one pipeline check
(four batches, a slot reused, a ragged tail), one scene's slot buffers and staging shared by records of different sizes and
regrown, the per-batch limit of the host entries, a refit right behind every device entry's launch, and which build
double_fallback + full_stats picks. Everything is compared with the same call made another way - one batch, a fresh scene, an
untouched scene, double_fallback alone -, bytes for bytes."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import count_cases as cc
import point_cases as pc

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = (F(-7.5), 0xABCD1234, 0x5A5A, 0xA5A5, 0xDEADBEEF)
_cache = {}


def _case():
    """The builtin box scene, 8192 rays, 4096 points of mixed radii, and the same points with one finite radius (neighbour lists)."""
    if not _cache:
        hs = cc.scene("box")
        lo, hi = cc.root_box(hs)
        rays = cc.mixed_rays(hs, 8192, seed=31)
        pts = pc.mixed_points(hs, 4096, seed=32)
        near = pts.copy()
        near["radius"] = F(0.01) * F(np.linalg.norm(hi - lo))          # (lists of a few records, some of a hundred)
        _cache["case"] = (hs, rays, pts, near)
    return _cache["case"]


def _records(n, dtype):
    buf = irl.aligned_bytes(max(n, 1) * dtype.itemsize).view(dtype)
    buf[:] = SENTINEL
    return buf


def _lists(offsets_of, fill, src, dtype):
    offsets = offsets_of(src)
    total = int(offsets[-1])
    hits = _records(total, dtype)
    fill(src, offsets, hits, total)
    return offsets, hits


def _descending_offsets(n, k):
    """n + 1 offsets that do not ascend: even entries i hold a segment of k records, the later the entry the lower its place;
    every odd entry's pair decreases, which is an empty segment. Returns (offsets, records the segments span)."""
    m = n // 2 + 1
    i = np.arange(n + 1)
    return (k * np.where(i % 2 == 0, m - 1 - i // 2, m - i // 2)).astype(np.uint64), k * m


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        if g.tobytes() != w.tobytes():
            gb, wb = g.reshape(-1).view(np.uint8).reshape(g.size, -1), w.reshape(-1).view(np.uint8).reshape(w.size, -1)
            bad = np.nonzero((gb != wb).any(1))[0]
            raise AssertionError(f"{what}: {bad.size}/{g.size} records differ, first {bad[:4]}")


def _host_calls(rays, pts, near):
    """Every host entry by name: dev -> its result (an array or a tuple of arrays)."""
    odd, span = _descending_offsets(rays.size, 3)

    def fill_descending(fill, src, dtype):
        return fill(src, odd, _records(span, dtype), span)

    return {
        "intersect": lambda d: d.intersect(rays),
        "occluded": lambda d: d.occluded(rays),
        "closest_points": lambda d: d.closest_points(pts),
        "within": lambda d: d.within(pts),
        "count_crossings": lambda d: d.count_crossings(rays),
        "inside": lambda d: d.inside(pts),
        "signed_distance": lambda d: d.signed_distance(pts),
        "list_offsets + list_fill": lambda d: _lists(d.list_offsets, d.list_fill, rays, irl.CROSSING),
        "near_offsets + near_fill": lambda d: _lists(d.near_offsets, d.near_fill, near, irl.NEIGHBOUR),
        "first_crossings": lambda d: d.first_crossings(rays, 3),
        "k_nearest": lambda d: d.k_nearest(near, 3),
        "list_fill, descending offsets": lambda d: fill_descending(d.list_fill, rays, irl.CROSSING),
        "near_fill, descending offsets": lambda d: fill_descending(d.near_fill, near, irl.NEIGHBOUR),
    }


# ------------------------------------------------------------------------------------------------------
# 1. the pipeline: four batches, the tail of another length, both slots used twice
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
def test_four_batches_with_a_ragged_tail_equal_one_batch(variants):
    hs, rays, pts, near = _case()
    n = 1000
    calls = _host_calls(rays[:n], pts[:n], near[:n])
    dev = irl.IpuScene(hs.desc, variants=variants)
    dev.setRayBatch(0)
    want = {name: call(dev) for name, call in calls.items()}
    dev.setRayBatch(301)          # 301 + 301 + 301 + 97
    for name, call in calls.items():
        _same(call(dev), want[name], f"{name}: batches of 301 against one batch")
    dev.close()
    # the descending fills put ray 2 j's first three records where the offsets say, and write nowhere else
    odd, span = _descending_offsets(n, 3)
    for name, first in (("list_fill, descending offsets", "first_crossings"), ("near_fill, descending offsets", "k_nearest")):
        buf = want[name]
        for i in (0, 2, 300, 302, 600, 998):
            assert buf[int(odd[i]):int(odd[i]) + 3].tobytes() == want[first][i].tobytes(), (name, i)
        assert np.all(buf[:3] == np.array(SENTINEL, buf.dtype)) and not np.any(buf[3:] == np.array(SENTINEL, buf.dtype)), name
    for name in ("list_offsets + list_fill", "near_offsets + near_fill"):          # (every batch has lists to place)
        assert np.all(np.diff(want[name][0][[0, 301, 602, 903, 1000]].astype(np.int64)) > 0), name


# ------------------------------------------------------------------------------------------------------
# 2. one scene's buffers under records of different sizes, growing
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
def test_families_share_one_scenes_buffers_and_regrow_them(variants):
    hs, rays, pts, near = _case()
    sequence = [
        ("intersect of 256 rays", lambda d: d.intersect(rays[:256])),
        ("closest_points of 1024 points", lambda d: d.closest_points(pts[:1024])),
        ("list_crossings of 4096 rays", lambda d: d.list_crossings(rays[:4096])),
        ("neighbours of 512 points", lambda d: d.neighbours(near[:512])),
        ("count_crossings of 8192 rays", lambda d: d.count_crossings(rays)),
        ("signed_distance of 300 points", lambda d: d.signed_distance(pts[:300])),
    ]
    dev = irl.IpuScene(hs.desc, variants=variants)
    got = [call(dev) for _, call in sequence]
    dev.close()
    for (what, call), g in zip(sequence, got):
        fresh = irl.IpuScene(hs.desc, variants=variants)
        _same(g, call(fresh), f"{what}: after the calls before it against a fresh scene")
        fresh.close()


# ------------------------------------------------------------------------------------------------------
# 3. the per-batch limit of the host entries
# ------------------------------------------------------------------------------------------------------
def test_host_entries_refuse_a_batch_one_launch_cannot_index():
    hs, rays, pts, near = _case()
    dev = irl.IpuScene(hs.desc)
    want = dev.intersect(rays[:256])
    dev.setRayBatch(0)
    lib, h = dev._lib, dev._h
    src_rays, src_pts = irl.aligned_bytes(64 * 32), irl.aligned_bytes(64 * 16)
    r, p = src_rays.ctypes.data, src_pts.ctypes.data
    out = irl.aligned_bytes(64 * 32)
    hits = irl.aligned_bytes(64 * 16)
    o, x = out.ctypes.data, hits.ctypes.data
    n = 0xFFBFFFFF + 1
    refused = {
        "mi_query": (lambda: lib.mi_query(h, 0, r, o, n), b"rays"),
        "mi_point_query": (lambda: lib.mi_point_query(h, 0, p, o, n), b"points"),
        "mi_count_query": (lambda: lib.mi_count_query(h, r, o, n), b"rays"),
        "mi_point_sign": (lambda: lib.mi_point_sign(h, 1, p, o, None, n), b"points"),
        "mi_list_offsets": (lambda: lib.mi_list_offsets(h, r, o, n), b"rays"),
        "mi_list_fill": (lambda: lib.mi_list_fill(h, r, o, x, 64, n), b"rays"),
        "mi_near_offsets": (lambda: lib.mi_near_offsets(h, p, o, n), b"points"),
        "mi_near_fill": (lambda: lib.mi_near_fill(h, p, o, x, 64, n), b"points"),
    }
    for name, (call, noun) in refused.items():
        assert call() == 1, name          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert err.startswith(name.encode() + b": more " + noun + b" per batch than one launch indexes"), (name, err)
        assert not out.any() and not hits.any(), f"{name}: a refused call wrote to its buffers"
    _same(dev.intersect(rays[:256]), want, "a query after the refused calls")
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 4. a refit right behind every device entry's launch
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
def test_update_geometry_waits_for_every_device_entrys_launch(variants):
    import torch
    hs, rays, pts, near = _case()
    n, k = 4096, 3
    rays, pts, near = rays[:n], pts[:n], near[:n]
    ref = irl.IpuScene(hs.desc, variants=variants)          # never updated
    l_off, n_off = ref.list_offsets(rays), ref.near_offsets(near)
    k_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(k)).astype(np.uint64)
    want = {
        "closest": ref.intersect(rays), "any": ref.occluded(rays).view(np.uint8), "point closest": ref.closest_points(pts),
        "point within": ref.within(pts).view(np.uint8), "count": ref.count_crossings(rays), "inside": ref.inside(pts),
        "distance": ref.signed_distance(pts), "list offsets": l_off, "near offsets": n_off,
        "list fill": ref.first_crossings(rays, k).reshape(-1), "near fill": ref.k_nearest(near, k).reshape(-1),
    }
    ref.close()

    def gpu(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    t_rays, t_pts, t_near, t_koff = gpu(rays), gpu(pts), gpu(near), gpu(k_off)
    R, P, O = t_rays.data_ptr(), t_pts.data_ptr(), t_koff.data_ptr()
    entries = [      # (name, query_kernel, bytes out, (dev, out pointer, stream) -> the call)
        ("closest", 0, n * 32, lambda d, o, s: d.query_device(irl.QUERY_CLOSEST, R, o, n, s)),
        ("any", 0, n, lambda d, o, s: d.query_device(irl.QUERY_ANY, R, o, n, s)),
        ("closest", 1, n * 32, lambda d, o, s: d.query_device(irl.QUERY_CLOSEST, R, o, n, s)),
        ("any", 1, n, lambda d, o, s: d.query_device(irl.QUERY_ANY, R, o, n, s)),
        ("point closest", 0, n * 32, lambda d, o, s: d.point_query_device(irl.POINT_CLOSEST, P, o, n, s)),
        ("point within", 0, n, lambda d, o, s: d.point_query_device(irl.POINT_WITHIN, P, o, n, s)),
        ("count", 0, n * 4, lambda d, o, s: d.count_query_device(R, o, n, s)),
        ("inside", 0, n, lambda d, o, s: d.point_sign_device(irl.SIGN_INSIDE, P, o, n, None, s)),
        ("distance", 0, n * 32, lambda d, o, s: d.point_sign_device(irl.SIGN_DISTANCE, P, o, n, None, s)),
        ("list offsets", 0, (n + 1) * 8, lambda d, o, s: d.list_offsets_device(R, o, n, s)),
        ("near offsets", 0, (n + 1) * 8, lambda d, o, s: d.near_offsets_device(t_near.data_ptr(), o, n, s)),
        ("list fill", 0, n * k * 16, lambda d, o, s: d.list_fill_device(R, O, o, n * k, n, s)),
        ("near fill", 0, n * k * 16, lambda d, o, s: d.near_fill_device(t_near.data_ptr(), O, o, n * k, n, s)),
    ]
    same = {a: getattr(hs, a) for a in ("verts", "spheres", "discs") if getattr(hs, a).size}
    assert "verts" in same
    st = torch.cuda.Stream()
    for name, kernel, size, call in entries:
        dev = irl.IpuScene(hs.desc, variants=variants).set_option("query_kernel", kernel)
        out = torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        call(dev, out.data_ptr(), st.cuda_stream)
        dev.update_geometry(vertices=same["verts"], spheres=same.get("spheres"), discs=same.get("discs"))
        st.synchronize()
        got = out.cpu().numpy()
        dev.close()
        assert got.tobytes() == want[name].tobytes(), f"{name}, query_kernel {kernel}: a launch with an unchanged refit behind it against an untouched scene"


# ------------------------------------------------------------------------------------------------------
# 5. double_fallback before full_stats: that build has no instrumented twin
# ------------------------------------------------------------------------------------------------------
def test_double_fallback_takes_precedence_over_full_stats():
    hs = cc.grazing_scene(np.random.default_rng(900), 48)
    rays = cc.grazing_rays(0)
    pts = cc.points_of(np.stack([rays["origin"][c] for c in "xyz"], 1) + F(0.25))
    k_off = (np.arange(rays.size + 1, dtype=np.uint64) * np.uint64(4)).astype(np.uint64)
    calls = {
        "count": lambda d: d.count_crossings(rays),
        "list offsets": lambda d: d.list_offsets(rays),
        "list fill": lambda d: d.list_fill(rays, k_off, _records(rays.size * 4, irl.CROSSING), rays.size * 4),
        "inside": lambda d: d.inside(pts),
    }
    alone = irl.IpuScene(hs.desc).set_option("double_fallback", 1)
    both = irl.IpuScene(hs.desc).set_option("double_fallback", 1).set_option("full_stats", 1)
    plain = irl.IpuScene(hs.desc)
    differs = False
    for name, call in calls.items():
        both.reset_counters()
        want = call(alone)
        _same(call(both), want, f"{name}: double_fallback + full_stats against double_fallback alone")
        c = both.counters()
        assert c["casts"] == rays.size and c["nodes_visited"] == 0 and c["leaf_tests"] == 0, (name, c)
        differs = differs or call(plain).tobytes() != want.tobytes()
    assert differs, "the grazing rays never took the binary64 branch to another answer"
    # signed distance: the walk as above behind the point query, which has an instrumented build and no binary64 one
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stats.closest_points(pts)
    p = stats.counters()
    assert p["nodes_visited"] > 0 and p["leaf_tests"] > 0
    both.reset_counters()
    _same(both.signed_distance(pts), alone.signed_distance(pts), "signed distance: double_fallback + full_stats against double_fallback alone")
    c = both.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (pts.size, p["nodes_visited"], p["leaf_tests"]), c
    for d in (alone, both, plain, stats):
        d.close()
