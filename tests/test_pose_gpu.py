"""Rigid poses on the GPU (mi_scene_set_poses*, both libraries): after a pose call the scene is what mi_scene_update with the host
twin's arrays leaves - nodes, queries and a render, byte for byte -, at the sizes where the pose pass can go wrong, through every
sequence the contract names (absolute poses, identity, update, bake, rebuild, new contents, auto_rebuild), with its refusals, its
ordering behind enqueued work and the torch entry."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc
import pose_cases as po
import refit_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


def _scene(name, size=16, spp=4):
    hs = rc.scene(name)
    hs.desc.set_image(size, size)
    hs.desc.samples_per_pixel = spp
    return hs


def _poses(hs, seed):
    """Seeded poses with translations of a quarter of the root box: the bodies stay within the fp16 extents."""
    p = po.seeded_poses(hs, seed)
    p["translation"] *= F(0.25)
    return p


def _probes(nodes, seed=11, n=4000):
    """(rays, points, boxes) about the root box of `nodes`: what the scenes of one test are all asked."""
    rng = np.random.default_rng(seed)
    lo, hi = pc.root_box(nodes)
    size = np.maximum(hi - lo, F(1.0))
    o = rng.uniform(lo - size, hi + size, (n, 3)).astype(F)
    target = rng.uniform(lo, hi, (n, 3)).astype(F)
    rays = qb.make_rays(o, (target - o).astype(F))
    points = qb.make_points(rng.uniform(lo - size / 2, hi + size / 2, (n // 4, 3)).astype(F))
    c = rng.uniform(lo, hi, (n // 8, 3)).astype(F)
    h = rng.uniform(0.02, 0.2, (n // 8, 3)).astype(F) * size
    return rays, points, qb.make_boxes(c - h, c + h)


def _answers(dev, probes):
    rays, points, boxes = probes
    offsets, recs = dev.list_overlaps(boxes)
    return {"closest hits": dev.intersect(rays).tobytes(), "closest points": dev.closest_points(points).tobytes(),
            "overlap offsets": offsets.tobytes(), "overlaps": recs.tobytes()}


def _assert_same_answers(got, want, what):
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differ"


def _render(dev, desc):
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    dev.run(rays, irl.MODE_PATH_TRACE)
    return rays.tobytes()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class _OwnStream:
    """A non-default stream made for one test and destroyed behind it, as a torch stream (torch.cuda.Stream() would hand out one of
    torch's pooled streams, which stay bound to a hardware queue for the rest of the process)."""

    def __enter__(self):
        import torch
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)      # the runtime torch has loaded
        self.hip = C.CDLL(path)
        self.handle = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(self.handle), 1) == 0                            # hipStreamNonBlocking
        self.stream = torch.cuda.ExternalStream(self.handle.value)
        self.stream.wait_stream(torch.cuda.current_stream())
        return self.stream

    def __exit__(self, *exc):
        assert self.hip.hipStreamSynchronize(self.handle) == 0 and self.hip.hipStreamDestroy(self.handle) == 0
        return False


# ------------------------------------------------------------------------------------------------------
# 1. a posed scene is the updated scene
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [False, True])
@pytest.mark.parametrize("name", ["soup-normals", "spheres"])
def test_posed_scene_equals_an_update(name, variants):
    hs = _scene(name)
    p = _poses(hs, 3)
    dev = irl.IpuScene(hs.desc, variants=variants)
    assert dev.poses().tobytes() == qb.make_poses(p.size).tobytes(), "identities before the first pose call"
    dev.set_poses(p)
    want = po.posed(hs, p)
    rc.assert_nodes_equal(dev.bvh_nodes(), want.nodes, f"{name}: nodes after set_poses")
    assert dev.poses().tobytes() == p.tobytes()
    fresh = irl.IpuScene(want.desc, variants=variants)
    probes = _probes(want.nodes)
    _assert_same_answers(_answers(dev, probes), _answers(fresh, probes), f"{name}: a fresh scene of the twin's arrays")
    assert _render(dev, hs.desc) == _render(fresh, want.desc), f"{name}: the 16 x 16 render"
    # and the same scene through the update it stands for
    upd = irl.IpuScene(hs.desc, variants=variants)
    upd.update_geometry(**po.update_args(irl.pose_geometry_host(hs.desc, p)))
    rc.assert_nodes_equal(upd.bvh_nodes(), want.nodes, f"{name}: nodes after update_geometry")
    _assert_same_answers(_answers(upd, probes), _answers(dev, probes), f"{name}: update_geometry with the twin's arrays")
    assert upd.live_stats() == dev.live_stats()
    for s in (dev, fresh, upd):
        s.close()


# ------------------------------------------------------------------------------------------------------
# 2. sizes at the edges
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(po.EDGES))
def test_sizes_at_the_edges(name):
    e = po.edge(name)
    dev = irl.IpuScene(e.desc)
    probes = _probes(e.nodes, n=800)
    for seed in (1, 2):
        p = _poses(e, seed)
        dev.set_poses(p)
        want = po.posed(e, p)
        rc.assert_nodes_equal(dev.bvh_nodes(), want.nodes, f"{name}, seed {seed}")
        fresh = irl.IpuScene(want.desc)
        _assert_same_answers(_answers(dev, probes), _answers(fresh, probes), f"{name}, seed {seed}")
        fresh.close()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 3. sequences
# ------------------------------------------------------------------------------------------------------
def test_poses_are_absolute_and_identity_returns_the_rest_scene():
    hs = _scene("soup-normals")
    a, b = _poses(hs, 1), _poses(hs, 2)
    rest = po.with_arrays(hs, po.arrays_of(hs.desc))
    probes = _probes(rest.nodes)
    ref = irl.IpuScene(hs.desc)
    at_rest = _answers(ref, probes)
    dev = irl.IpuScene(hs.desc)
    dev.set_poses(a)
    dev.set_poses(b)
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, b).nodes, "A then B is B alone")
    dev.set_poses(qb.make_poses(a.size))
    rc.assert_nodes_equal(dev.bvh_nodes(), rest.nodes, "pose, then the identity: the rest scene's nodes")
    _assert_same_answers(_answers(dev, probes), at_rest, "pose, then the identity")
    # the vertex bytes are the rest bytes: baked, they pose like the scene as created
    dev.bake_poses()
    dev.set_poses(a)
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, a).nodes, "identity, bake, A")
    for s in (ref, dev):
        s.close()


def test_update_and_bake_set_a_new_rest():
    hs = _scene("soup")
    p = _poses(hs, 4)
    dev = irl.IpuScene(hs.desc)
    dev.set_poses(_poses(hs, 5))
    v, s, d = rc.jitter(hs, seed=6)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    assert dev.poses().tobytes() == qb.make_poses(p.size).tobytes(), "an update resets the poses"
    moved = po.with_arrays(hs, {"vertices": v, "normals": np.zeros(0, irl.VEC3), "spheres": s, "discs": d})
    dev.set_poses(p)
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(moved, p).nodes, "update_geometry, then a pose: the updated geometry is the rest")
    # bake: the posed geometry becomes the rest, the same pose composes
    once = po.posed(moved, p)
    before = dev.bvh_nodes().tobytes()
    dev.bake_poses()
    assert dev.bvh_nodes().tobytes() == before, "a bake moves nothing"
    assert dev.poses().tobytes() == qb.make_poses(p.size).tobytes(), "a bake resets the poses"
    dev.set_poses(p)
    twice = po.posed(once, p)
    rc.assert_nodes_equal(dev.bvh_nodes(), twice.nodes, "bake, then the same pose: composed")
    probes = _probes(twice.nodes)
    fresh = irl.IpuScene(twice.desc)
    _assert_same_answers(_answers(dev, probes), _answers(fresh, probes), "bake, then the same pose")
    for sc in (dev, fresh):
        sc.close()


def test_rebuild_and_set_geometry_then_pose():
    hs = _scene("soup")
    a, b = _poses(hs, 7), _poses(hs, 8)
    dev = irl.IpuScene(hs.desc)
    dev.set_poses(a)
    dev.rebuild_bvh()
    assert dev.poses().tobytes() == a.tobytes(), "a rebuild keeps the poses"
    topology = dev.bvh_nodes()
    dev.set_poses(b)
    want = po.posed(hs, b, topology)
    rc.assert_nodes_equal(dev.bvh_nodes(), want.nodes, "rebuild, then a pose: the rest snapshot is kept, B is absolute")
    # new contents: another geometry list, other counts; the snapshot and the poses go
    other = _scene("spheres")
    dev.set_geometry(other.desc)
    assert dev.poses().tobytes() == qb.make_poses(other.desc.num_geometry).tobytes(), "new contents reset the poses"
    with pytest.raises(irl.RaylibError, match="num_geometry differs"):
        dev.set_poses(b)
    topology = dev.bvh_nodes()
    p = _poses(other, 9)
    dev.set_poses(p)
    want = po.posed(other, p, topology)
    want.desc.max_leaf_depth = dev.live_stats()["max_leaf_depth"]
    rc.assert_nodes_equal(dev.bvh_nodes(), want.nodes, "set_geometry, then a pose")
    probes = _probes(want.nodes, n=800)
    fresh = irl.IpuScene(want.desc)
    _assert_same_answers(_answers(dev, probes), _answers(fresh, probes), "set_geometry, then a pose")
    for s in (dev, fresh):
        s.close()


def test_auto_rebuild_fires_as_for_the_update():
    hs = _scene("soup")
    G = hs.desc.num_geometry
    ratio = 1.2      # (geometry 0 shifted by 0.5 / 5 / 20 / 200 raises the refitted tree's estimate to 1.001 / 1.07 / 1.28 / 1.49 of the first)
    dev = irl.IpuScene(hs.desc).set_option("auto_rebuild", ratio)
    upd = irl.IpuScene(hs.desc).set_option("auto_rebuild", ratio)
    fired = []
    for shift in (0.5, 5.0, 20.0, 200.0):
        p = qb.make_poses(G)
        p["translation"][0] = (shift, 0, 0)
        dev.set_poses(p)
        upd.update_geometry(**po.update_args(irl.pose_geometry_host(hs.desc, p)))
        a, b = dev.live_stats(), upd.live_stats()
        assert a == b, f"shift {shift}: {a} against {b}"
        rc.assert_nodes_equal(dev.bvh_nodes(), upd.bvh_nodes(), f"shift {shift}")
        fired.append(a["auto_rebuilds"])
    assert fired[0] == 0 and fired[1] == 0 and fired[-1] >= 1, fired
    assert dev.poses()["translation"][0].tolist() == [200.0, 0.0, 0.0]
    for s in (dev, upd):
        s.close()


# ------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------
BAD = {"NaN": po.HAND["NaN"][0], "scale 0": po.HAND["scale 0"][0], "too far": po.TOO_FAR}
WORDS = {"NaN": "pose 2 is not valid", "scale 0": "pose 2 is not valid", "too far": "65504"}


@pytest.mark.parametrize("device_entry", [False, True])
@pytest.mark.parametrize("posed_before", [False, True])
def test_refusals_leave_everything_as_it_was(posed_before, device_entry):
    import torch
    hs = _scene("soup")
    G = hs.desc.num_geometry
    dev = irl.IpuScene(hs.desc)
    a, b = _poses(hs, 12), _poses(hs, 13)
    if posed_before:
        dev.set_poses(a)
    nodes, stored = dev.bvh_nodes(), dev.poses()
    probes = _probes(nodes, n=1500)
    before = _answers(dev, probes)
    entry = "mi_scene_set_poses_device" if device_entry else "mi_scene_set_poses:"
    for what, row in BAD.items():
        p = po.with_pose(G, 2, row)
        with pytest.raises(irl.RaylibError) as e:
            if device_entry:
                dev.pose(*(torch.from_numpy(p[f].copy()).cuda() for f in ("quat", "translation", "scale")))
            else:
                dev.set_poses(p)
        msg = str(e.value)
        assert "failed (1)" in msg and entry in msg and WORDS[what] in msg and "unchanged" in msg, msg
        rc.assert_nodes_equal(dev.bvh_nodes(), nodes, f"after refusing {what}")
        _assert_same_answers(_answers(dev, probes), before, f"after refusing {what}")
        assert dev.poses().tobytes() == stored.tobytes(), f"after refusing {what}: the stored poses"
    for bad_n in (G - 1, G + 1):
        with pytest.raises(irl.RaylibError, match="num_geometry differs"):
            dev.set_poses(qb.make_poses(bad_n))
    dev.set_poses(b)
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, b).nodes, "the next valid pose: from the rest geometry")
    assert dev.poses().tobytes() == b.tobytes()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# 5. ordering, 6. the torch entry, 7. the other families
# ------------------------------------------------------------------------------------------------------
def test_pose_waits_for_an_enqueued_list_fill():
    import torch
    hs = _scene("soup")
    rays, _, _ = _probes(hs.nodes, n=3000)
    many = np.tile(rays, 8)
    t_rays = _cuda(many)
    t_off = torch.arange(many.size + 1, dtype=torch.int64, device="cuda") * 4
    ref = irl.IpuScene(hs.desc)
    want = torch.zeros((many.size * 4, 4), dtype=torch.int32, device="cuda")
    ref.list_fill_device(t_rays.data_ptr(), t_off.data_ptr(), want.data_ptr(), many.size * 4, many.size)
    torch.cuda.synchronize()
    dev = irl.IpuScene(hs.desc)
    out = torch.zeros_like(want)
    p = _poses(hs, 14)
    with _OwnStream() as st:
        dev.list_fill_device(t_rays.data_ptr(), t_off.data_ptr(), out.data_ptr(), many.size * 4, many.size, st.cuda_stream)      # enqueued, not waited for
        dev.set_poses(p)
        st.synchronize()
    assert out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), "a fill enqueued before the pose sees the old geometry"
    assert (want.cpu().numpy().view(irl.CROSSING)["primID"] != irl.INVALID_PRIM).sum() > 1000, "the rays cross something"
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, p).nodes, "after the pose")
    posed_out = torch.zeros_like(want)
    dev.list_fill_device(t_rays.data_ptr(), t_off.data_ptr(), posed_out.data_ptr(), many.size * 4, many.size)
    torch.cuda.synchronize()
    assert posed_out.cpu().numpy().tobytes() != want.cpu().numpy().tobytes(), "a fill enqueued after it sees the posed geometry"
    for s in (ref, dev):
        s.close()


def test_torch_entry_on_a_stream_of_its_own():
    import torch
    hs = _scene("soup-normals")
    p = _poses(hs, 15)
    dev = irl.IpuScene(hs.desc)
    q, t, s = (torch.from_numpy(p[f].copy()).cuda() for f in ("quat", "translation", "scale"))
    with _OwnStream() as st:
        with torch.cuda.stream(st):
            dev.pose(q, t, s)
        st.synchronize()
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, p).nodes, "pose() on tensors")
    assert dev.poses().tobytes() == p.tobytes()
    # scale None is 1
    dev.pose(q, t)
    p1 = p.copy(); p1["scale"] = 1
    rc.assert_nodes_equal(dev.bvh_nodes(), po.posed(hs, p1).nodes, "pose() without a scale")
    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        dev.pose(q.cpu(), t)
    dev.set_option("refit_timing", 1)
    dev.pose(q, t, s)
    ms = dev.pose_timing()
    assert ms[0] > 0 and ms[1] > 0, ms
    dev.close()


def test_the_other_families_of_an_unposed_scene_are_what_they_were():
    import box_cases as bc
    import obox_cases as oc
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    _, ab, b_off, b_recs, _, _, _ = bc.twin("soup")
    dev = irl.IpuScene(hs.desc)
    bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), "oriented boxes, an unposed scene")
    bc.assert_same(dev.list_overlaps(ab), (b_off, b_recs), "boxes, an unposed scene")
    # posed and brought back by the identity, the lists are the first ones; another scene's poses do not reach this one
    other = irl.IpuScene(hs.desc)
    other.set_poses(_poses(hs, 16))
    dev.set_poses(_poses(hs, 17))
    assert dev.list_obox_overlaps(bx)[1].tobytes() != recs.tobytes()
    dev.set_poses(qb.make_poses(hs.desc.num_geometry))
    bc.assert_same(dev.list_obox_overlaps(bx), (offsets, recs), "oriented boxes, posed and brought back")
    bc.assert_same(dev.list_overlaps(ab), (b_off, b_recs), "boxes, posed and brought back")
    for s in (dev, other):
        s.close()
