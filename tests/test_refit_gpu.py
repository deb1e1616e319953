"""Geometry updates on the GPU (pytest -m gpu): mi_scene_update / mi_scene_update_device refit the BVH and rewrite the scene's
records in place. After an update the device nodes equal the host refit (mi_refit_compact_bvh) byte for byte, and every query and
render equals - bit for bit - a scene freshly created from the moved arrays and those nodes, and the CPU oracle on them."""
import ctypes as C
import os

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import refit_cases as rc

pytestmark = pytest.mark.gpu


def assert_bytes_equal(got, want, what):
    gb, wb = got.view(np.uint8).reshape(got.size, -1), want.view(np.uint8).reshape(want.size, -1)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} records differ; first at {i}:\n got  {got[i]}\n want {want[i]}")


def _root_box(nodes):
    n = nodes[0]
    lo = np.array([n["min_x"], n["min_y"], n["min_z"]], np.float32)
    ext = np.array([n["dx"], n["dy"], n["dz"]], np.uint16).view(np.float16).astype(np.float32)
    return lo, lo + ext


def _rays(nodes, n, seed):
    """Origins inside and around the root box, random directions (some with zero components), some finite t_max / positive t_min."""
    rng = np.random.default_rng(seed)
    lo, hi = _root_box(nodes)
    size = hi - lo
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    out = rng.random(n) < 0.3
    o[out] = rng.uniform(lo - size, hi + size, (out.sum(), 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(3):
        d[k * n // 30:(k + 1) * n // 30, k] = 0.0
    rays = qb.make_rays(o, d.astype(np.float32))
    diag = float(np.linalg.norm(size))
    sel = rng.random(n) < 0.1
    rays["tMax"][sel] = rng.uniform(0, diag, sel.sum())
    sel = rng.random(n) < 0.1
    rays["tMin"][sel] = rng.uniform(0, diag / 4, sel.sum())
    return rays


def _oracle_closest(desc, rays):
    o = ol.lib()
    want = np.zeros(rays.size, irl.QUERY_HIT)
    occ = np.zeros(rays.size, bool)
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    for i in range(rays.size):
        x = o.o_bvh_intersect(C.byref(desc), C.byref(buf[i]), None)
        want["t"][i] = x.t
        if x.hit:
            want["primID"][i], want["geomID"][i] = x.primID, x.geomID
            want["normal"][i] = (x.normal.x, x.normal.y, x.normal.z)
        else:
            want["primID"][i], want["geomID"][i], want["flags"][i] = irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED
        occ[i] = bool(o.o_bvh_occluded(C.byref(desc), C.byref(buf[i]), None))
    return want, occ


def _check_queries(dev, fresh, desc, rays, what, oracle_n=4000):
    """dev's closest / any hits equal fresh's byte for byte, under both query kernels and double_fallback; the first oracle_n
    rays equal the oracle's (t, primID, geomID, flags, normal: the oracle has no barycentrics here)."""
    got = {}
    for opts in ({"query_kernel": 0}, {"query_kernel": 1}, {"query_kernel": 0, "double_fallback": 1}):
        for sc in (dev, fresh):
            for k, v in opts.items():
                sc.set_option(k, v)
        a, b = dev.intersect(rays), fresh.intersect(rays)
        assert_bytes_equal(a, b, f"{what}: closest hit {opts}")
        oa, ob = dev.occluded(rays), fresh.occluded(rays)
        assert np.array_equal(oa, ob), f"{what}: any hit {opts}: {(oa != ob).sum()} rays differ"
        got[tuple(opts.items())] = (a, oa)
        for sc in (dev, fresh):
            sc.set_option("double_fallback", 0).set_option("query_kernel", 0)
    if oracle_n:
        a, oa = got[(("query_kernel", 0),)]
        want, occ = _oracle_closest(desc, rays[:oracle_n])
        for f in ("t", "primID", "geomID", "flags", "normal"):
            assert_bytes_equal(np.ascontiguousarray(a[f][:oracle_n]), np.ascontiguousarray(want[f]), f"{what}: oracle {f}")
        assert np.array_equal(oa[:oracle_n], occ), f"{what}: oracle any hit"


def _frame(desc, w=64, h=64, spp=16):
    d = irl.SceneDesc.from_buffer_copy(desc)
    d.set_image(w, h)
    d.samples_per_pixel = spp
    return d


def _render(sc, desc, mode):
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    sc.run(rays, mode)
    return rays


def _check_renders(dev, fresh, desc, what, kernels=(0, 1), oracle=True, frame=(64, 64, 16)):
    """Path-trace and shadow-trace frames of dev equal fresh's (and the oracle's) bit for bit."""
    d = _frame(desc, *frame)
    for k in kernels:
        dev.set_option("kernel", k); fresh.set_option("kernel", k)
        a, b = _render(dev, d, irl.MODE_PATH_TRACE), _render(fresh, d, irl.MODE_PATH_TRACE)
        assert_bytes_equal(a, b, f"{what}: path trace, kernel {k}")
    dev.set_option("kernel", 1); fresh.set_option("kernel", 1)
    s_a, s_b = _render(dev, d, irl.MODE_SHADOW_TRACE), _render(fresh, d, irl.MODE_SHADOW_TRACE)
    assert_bytes_equal(s_a, s_b, f"{what}: shadow trace")
    if oracle:
        want = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
        irl.host_lib().mi_init_ray_stream(C.byref(d), want.ctypes.data, want.size)
        shadow = want.copy()
        ol.path_trace_pixel_rng(d, want, 16)
        assert_bytes_equal(a, want, f"{what}: path trace against the oracle")
        ol.shadow_trace(d, shadow, 16)
        assert_bytes_equal(s_a, shadow, f"{what}: shadow trace against the oracle")


# ------------------------------------------------------------------------------------------------------
# parity after an update
# ------------------------------------------------------------------------------------------------------
def _moves(name, hs):
    """(label, Moved) updates for scene `name`."""
    v, s, d = rc.jitter(hs, 11, 0.4 if name not in ("box", "box-simple") else 4.0)
    out = [("jitter", rc.Moved(hs, verts=v, spheres=s, discs=d))]
    if name == "box":
        out.append(("rigid monkey", rc.Moved(hs, verts=rc.rigid(hs, 6, 0.6, (25.0, 10.0, -15.0)))))
    if name == "spheres":
        s2 = hs.spheres.copy(); s2["y"] += 30.0; s2["radius"] *= 1.3
        out.append(("spheres moved", rc.Moved(hs, spheres=s2)))
    if name in ("soup-normals", "test_scene.dae"):
        rng = np.random.default_rng(5)
        n = rng.normal(size=(hs.desc.num_normals, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
        nn = np.zeros(hs.desc.num_normals, irl.VEC3); nn["x"], nn["y"], nn["z"] = n.astype(np.float32).T
        out.append(("new normals", rc.Moved(hs, verts=v, normals=nn)))
    return out


def _update_args(m, hs, label):
    kw = {}
    if label in ("jitter", "rigid monkey", "new normals") and hs.desc.num_verts:
        kw["vertices"] = m.verts
    if label in ("jitter", "spheres moved") and hs.desc.num_spheres:
        kw["spheres"] = m.spheres
    if label == "jitter" and hs.desc.num_discs:
        kw["discs"] = m.discs
    if label == "new normals":
        kw["normals"] = m.normals
    return kw


SCENES = ["box-simple", "box", "spheres", "soup", "soup-normals", "test_scene.dae"]


@pytest.mark.parametrize("name", SCENES)
def test_update_equals_fresh_scene_and_oracle(name):
    hs = rc.scene(name)
    for label, m in _moves(name, hs):
        m.refit()
        dev = irl.IpuScene(_frame(hs.desc))                   # (the frame's image size: the camera rays are the oracle's)
        dev.update_geometry(**_update_args(m, hs, label))
        rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, f"{name} {label}: device nodes against the host refit")
        assert not np.array_equal(rc.node_bytes(m.nodes), rc.node_bytes(hs.nodes))
        fresh = irl.IpuScene(_frame(m.desc))
        rc.assert_nodes_equal(fresh.bvh_nodes(), m.nodes, f"{name} {label}: fresh scene's nodes")
        _check_queries(dev, fresh, m.desc, _rays(m.nodes, 50000, 3), f"{name} {label}")
        _check_renders(dev, fresh, m.desc, f"{name} {label}", oracle=(label == "jitter"))
        dev.close(); fresh.close()


def test_update_variants_build_kernels_and_blob_scene():
    hs = rc.scene("box")
    v, s, d = rc.jitter(hs, 21, 3.0)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()
    dev = irl.IpuScene(_frame(hs.desc), variants=True)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    fresh = irl.IpuScene(_frame(m.desc), variants=True)
    _check_renders(dev, fresh, m.desc, "variants build", kernels=(0, 1, 2, 3), oracle=False)
    # a scene made from the serialised blob updates the same way
    blob_scene = irl.IpuScene.from_blob(irl.serialise_scene(hs.desc), hs.desc)
    blob_scene.update_geometry(vertices=v, spheres=s, discs=d)
    rc.assert_nodes_equal(blob_scene.bvh_nodes(), m.nodes, "blob scene")
    rays = _rays(m.nodes, 20000, 4)
    assert_bytes_equal(blob_scene.intersect(rays), fresh.intersect(rays), "blob scene: closest hit")


def test_identity_update_changes_nothing():
    hs = rc.scene("box")
    dev = irl.IpuScene(hs.desc)
    rays = _rays(hs.nodes, 30000, 8)
    before, occ = dev.intersect(rays), dev.occluded(rays)
    d = _frame(hs.desc, 48, 48, 8)
    frame = _render(dev, d, irl.MODE_PATH_TRACE)
    dev.update_geometry(vertices=hs.verts.copy(), spheres=hs.spheres.copy(), discs=hs.discs.copy())
    rc.assert_nodes_equal(dev.bvh_nodes(), hs.nodes, "identity update")
    assert_bytes_equal(dev.intersect(rays), before, "identity update: closest hit")
    assert np.array_equal(dev.occluded(rays), occ)
    assert_bytes_equal(_render(dev, d, irl.MODE_PATH_TRACE), frame, "identity update: path trace")
    dev.update_geometry()                                   # nothing given: nothing changes
    assert_bytes_equal(dev.intersect(rays), before, "empty update: closest hit")


def test_animation_from_torch_tensors_on_a_side_stream():
    torch = pytest.importorskip("torch")
    hs = rc.scene("soup-normals")
    dev = irl.IpuScene(hs.desc)
    base = np.stack([hs.verts["x"], hs.verts["y"], hs.verts["z"]], 1).astype(np.float32)
    side = torch.cuda.Stream()
    for f in range(10):
        t = np.float32(0.3 * (f + 1))
        moved = base.copy()
        moved[:, 0] += np.float32(2.0) * np.sin(moved[:, 1] * np.float32(0.1) + t).astype(np.float32)
        moved[:, 2] += np.float32(0.5) * t
        sph = np.array([[0.0, 0.5 * f, -40.0, 3.0]], np.float32)
        with torch.cuda.stream(side):
            tv = torch.from_numpy(moved).cuda()
            ts = torch.from_numpy(sph).cuda()
            dev.update_geometry_device(vertices=tv, spheres=ts)
        v = np.zeros(len(moved), irl.VEC3); v["x"], v["y"], v["z"] = moved.T
        s = hs.spheres.copy(); s[0] = tuple(sph[0])
        m = rc.Moved(hs, verts=v, spheres=s).refit()
        rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, f"frame {f}")
        fresh = irl.IpuScene(m.desc)
        rays = _rays(m.nodes, 4000, 100 + f)
        assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), f"frame {f}: closest hit")
        fresh.close()


def test_update_waits_for_enqueued_render():
    torch = pytest.importorskip("torch")
    hs = rc.scene("box")
    d = _frame(hs.desc, 256, 256, 64)
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    want = rays.copy()
    ref = irl.IpuScene(d)
    ref.run(want, irl.MODE_PATH_TRACE)
    dev = irl.IpuScene(d)
    buf = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev.run_device(buf.data_ptr(), rays.size, irl.MODE_PATH_TRACE, side.cuda_stream)      # enqueued, not waited for
    v = rc.rigid(hs, 6, 1.2, (60.0, 40.0, 0.0))
    dev.update_geometry(vertices=v)
    side.synchronize()
    got = buf.cpu().numpy().view(irl.TRACE_RESULT)
    assert_bytes_equal(got, want, "render enqueued before the update")
    m = rc.Moved(hs, verts=v).refit()
    rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, "after the update")


def test_refusals_leave_the_scene_unchanged():
    hs = rc.scene("soup")
    dev = irl.IpuScene(hs.desc)
    rays = _rays(hs.nodes, 20000, 9)
    before, occ = dev.intersect(rays), dev.occluded(rays)
    nodes = dev.bvh_nodes()

    def refused(**kw):
        with pytest.raises(irl.RaylibError) as e:
            dev.update_geometry(**kw)
        assert "failed (1)" in str(e.value), str(e.value)          # MI_ERR_INVALID_ARG
        rc.assert_nodes_equal(dev.bvh_nodes(), nodes, f"after refusing {list(kw)}")
        assert_bytes_equal(dev.intersect(rays), before, f"after refusing {list(kw)}: closest hit")
        assert np.array_equal(dev.occluded(rays), occ)
        return str(e.value)

    v = hs.verts.copy(); v["x"][0:3] = np.nan                         # a triangle with no finite x: its box is empty
    assert "not finite" in refused(vertices=v)
    v = hs.verts.copy(); v["x"][4] += np.float32(70000.0)             # an extent above 65504
    assert "65504" in refused(vertices=v)
    assert "num_verts" in refused(vertices=hs.verts[:-1].copy())
    assert "num_spheres" in refused(spheres=np.zeros(2, irl.SPHERE))
    assert "without normals" in refused(normals=hs.verts.copy())
    # a good update after the refusals still lands
    v, s, d = rc.jitter(hs, 3, 0.2)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    rc.assert_nodes_equal(dev.bvh_nodes(), rc.Moved(hs, verts=v, spheres=s, discs=d).refit().nodes, "after the refusals")


def test_large_soup():
    old = os.environ.get("MI_BVH_REINSERT")
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the 1 M-triangle fixture builds in seconds
    try:
        hs = rc.soup(7, False, n_tris=1 << 20, n_meshes=64, spread=200.0)
    finally:
        if old is None:
            del os.environ["MI_BVH_REINSERT"]
        else:
            os.environ["MI_BVH_REINSERT"] = old
    dev = irl.IpuScene(hs.desc)
    v, s, d = rc.jitter(hs, 13, 0.5)
    dev.update_geometry(vertices=v, spheres=s, discs=d)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()
    rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, "1 M-triangle soup")
    fresh = irl.IpuScene(m.desc)
    rays = _rays(m.nodes, 20000, 10)
    assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), "1 M-triangle soup: closest hit")
    assert np.array_equal(dev.occluded(rays), fresh.occluded(rays))


def test_group_replicas_update():
    hs = rc.scene("box")
    d = _frame(hs.desc, 64, 64, 8)
    v, s, dd = rc.jitter(hs, 17, 3.0)
    g = irl.IpuGroup(d, [0, 0])
    for sc in g.scenes():
        sc.update_geometry(vertices=v, spheres=s, discs=dd)
    single = irl.IpuScene(d)
    single.update_geometry(vertices=v, spheres=s, discs=dd)
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    want = rays.copy()
    g.run(rays, irl.MODE_PATH_TRACE)
    single.run(want, irl.MODE_PATH_TRACE)
    assert_bytes_equal(rays, want, "group of two updated replicas")
    g.close()
