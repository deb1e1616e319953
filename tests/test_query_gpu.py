"""Ray queries on the GPU (pytest -m gpu): mi_query / mi_query_device against the CPU oracle's o_bvh_intersect / o_bvh_occluded
(CompactBvh::intersect / ::occluded), bit for bit, under both query kernels (option query_kernel: 0 = one thread per ray,
1 = K4). Barycentrics are checked against o_ray_shear + o_intersect_triangle on the hit triangle."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol

pytestmark = pytest.mark.gpu

KERNELS = (0, 1)


# ------------------------------------------------------------------------------------------------------
# scenes and rays
# ------------------------------------------------------------------------------------------------------
def _soup(seed, with_normals, n_tris=600):
    """Random triangle soup in two meshes + a sphere + a disc (as tests/test_gpu_parity.py builds it)."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10, 10, (n_tris, 3)).astype(np.float32); centers[:, 2] -= 40
    verts = (centers.repeat(3, 0) + rng.normal(scale=1.5, size=(3 * n_tris, 3))).astype(np.float32)
    half = n_tris // 2
    tris = np.concatenate([np.arange(3 * half), np.arange(3 * (n_tris - half))]).astype(np.uint16).reshape(-1, 3)
    v = np.zeros(len(verts), dtype=irl.VEC3); v["x"], v["y"], v["z"] = verts.T
    nrm = np.zeros(len(verts) if with_normals else 0, dtype=irl.VEC3)
    if with_normals:
        nn = rng.normal(size=(len(verts), 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nrm["x"], nrm["y"], nrm["z"] = nn.T
    info = np.zeros(2, dtype=irl.MESH_INFO)
    info[0] = (0, 0, half, 3 * half); info[1] = (half, 3 * half, n_tris - half, 3 * (n_tris - half))
    sph = np.zeros(1, dtype=irl.SPHERE); sph[0] = (0, 0, -40, 3)
    dsc = np.zeros(1, dtype=irl.DISC); dsc[0] = (0, 1, 0, 30, 0, -12, -40)
    mats = np.zeros(4, dtype=irl.MATERIAL); mats["albedo"]["x"] = .5; mats["ior"] = 1.5
    mat_ids = np.arange(4, dtype=np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = info.ctypes.data, 2
    g.mesh_tris, g.num_tris = tris.ctypes.data, n_tris
    g.mesh_verts, g.num_verts = v.ctypes.data, len(v)
    g.mesh_normals, g.num_normals = (nrm.ctypes.data if with_normals else None), len(nrm)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, 4
    g.materials, g.num_materials = mats.ctypes.data, 4
    g.spheres, g.num_spheres = sph.ctypes.data, 1
    g.discs, g.num_discs = dsc.ctypes.data, 1
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, nrm, tris, info, sph, dsc, mats, mat_ids]
    return hs


def _scene(name):
    if name == "soup":
        return _soup(1234, False)
    if name == "soup-normals":
        return _soup(1235, True)
    if name == "test_scene.dae":
        return irl.HostScene.import_file(Path(irl.REPO_ROOT) / "assets" / "test_scene.dae", load_normals=True)
    return irl.HostScene.builtin(name)


SCENES = ["box-simple", "box", "spheres", "soup", "soup-normals", "test_scene.dae"]


@pytest.fixture(scope="module")
def scene_cache():
    cache = {}

    def get(name):
        if name not in cache:
            hs = _scene(name)
            hs.desc.set_image(64, 64)
            cache[name] = hs
        return cache[name]
    return get


def _root_box(hs):
    n = hs.nodes[0]
    lo = np.array([n["min_x"], n["min_y"], n["min_z"]], np.float32)
    ext = np.array([n["dx"], n["dy"], n["dz"]], np.uint16).view(np.float16).astype(np.float32)
    return lo, lo + ext


def _mixed_rays(hs, n, seed):
    """Origins inside and outside the scene's box, random directions with some zero components (infinite inverses), finite
    t_max and positive t_min on some, rays leaving surfaces (offset_origin), and a few NaN rays."""
    rng = np.random.default_rng(seed)
    lo, hi = _root_box(hs)
    size = hi - lo
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    out = rng.random(n) < 0.35
    o[out] = rng.uniform(lo - size, hi + size, (out.sum(), 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(3):
        d[k * n // 40:(k + 1) * n // 40, k] = 0.0                      # one zero component
    d[3 * n // 40:3 * n // 40 + 30] = [0, 0, -1]                         # two zero components
    d[3 * n // 40 + 30:3 * n // 40 + 60] = [1, 0, 0]
    rays = qb.make_rays(o, d.astype(np.float32))
    diag = float(np.linalg.norm(size))
    sel = rng.random(n) < 0.1
    rays["tMax"][sel] = rng.uniform(0, diag, sel.sum())
    sel = rng.random(n) < 0.1
    rays["tMin"][sel] = rng.uniform(0, diag / 4, sel.sum())
    # rays starting on surfaces: the first hits of some of these rays, offset as offset_origin does, in new directions
    k = n // 5
    first = np.zeros(k, irl.QUERY_HIT)
    for i in range(k):
        first[i] = _oracle_closest_one(hs.desc, rays[i])
    surf = qb.bounce_rays(rays[:k], first, 1, seed + 1)
    rays[n - len(surf):] = surf
    # NaN rays
    nan = np.float32("nan")
    rays["origin"]["x"][100] = nan; rays["direction"]["y"][101] = nan; rays["tMin"][102] = nan; rays["tMax"][103] = nan
    rays["direction"]["x"][104] = np.inf; rays["origin"]["z"][105] = -np.inf
    return rays


# ------------------------------------------------------------------------------------------------------
# the oracle's answers, in the entry points' result format
# ------------------------------------------------------------------------------------------------------
def _oracle_closest_one(desc, ray, st=None):
    o = ol.lib()
    r = ol.Ray.from_buffer_copy(ray.tobytes())
    x = o.o_bvh_intersect(C.byref(desc), C.byref(r), C.byref(st) if st is not None else None)
    h = np.zeros((), irl.QUERY_HIT)
    h["t"] = x.t
    if x.hit:
        h["primID"] = x.primID; h["geomID"] = x.geomID; h["flags"] = 0
        h["normal"] = (x.normal.x, x.normal.y, x.normal.z)
    else:
        h["primID"] = irl.INVALID_PRIM; h["geomID"] = irl.INVALID_GEOM; h["flags"] = irl.FLAG_ESCAPED
    return h


def _triangle(hs, geom, prim):
    g = hs.geometry[geom]
    if g["type"] != 0:
        return None
    info = hs.mesh_info[g["index"]]
    tri = hs.tris.reshape(-1, 3)[info["firstIndex"] + prim]
    v = hs.verts[info["firstVertex"] + tri.astype(np.int64)]
    return [ol.Vec3(float(p["x"]), float(p["y"]), float(p["z"])) for p in v]


def oracle_query(hs, rays):
    """(closest QUERY_HIT array with the barycentrics of triangle hits, occluded bool array, closest Stats, any-hit Stats)"""
    o = ol.lib()
    desc = hs.desc
    want = np.zeros(rays.size, irl.QUERY_HIT)
    occ = np.zeros(rays.size, bool)
    sc, sa = ol.Stats(), ol.Stats()
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    bary = (C.c_float * 3)()
    for i in range(rays.size):
        want[i] = _oracle_closest_one(desc, rays[i], sc)
        occ[i] = bool(o.o_bvh_occluded(C.byref(desc), C.byref(buf[i]), C.byref(sa)))
        if want["primID"][i] != irl.INVALID_PRIM:
            tri = _triangle(hs, int(want["geomID"][i]), int(want["primID"][i]))
            if tri is not None:
                sh = ol.Shear()
                o.o_ray_shear(C.byref(buf[i]), C.byref(sh))
                o.o_intersect_triangle(tri[0], tri[1], tri[2], C.byref(sh), np.float32(np.inf), bary)
                want["b1"][i], want["b2"][i] = bary[1], bary[2]
    return want, occ, sc, sa


def assert_bytes_equal(got, want, what):
    gb, wb = got.view(np.uint8).reshape(got.size, -1), want.view(np.uint8).reshape(want.size, -1)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} records differ; first at {i}:\n got  {got[i]}\n want {want[i]}")


_oracle_cache = {}


def _case(scene_cache, name, n=50000):
    if name not in _oracle_cache:
        hs = scene_cache(name)
        rays = _mixed_rays(hs, n, seed=SCENES.index(name) + 7)
        _oracle_cache[name] = (rays,) + oracle_query(hs, rays)
    return scene_cache(name), _oracle_cache[name]


# ------------------------------------------------------------------------------------------------------
# 1 - 3: closest hit, any hit, counters
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_closest_and_any_hit_bit_exact(scene_cache, name):
    hs, (rays, want, occ, sc, sa) = _case(scene_cache, name)
    assert (want["primID"] != irl.INVALID_PRIM).mean() > 0.1 and (want["primID"] == irl.INVALID_PRIM).any()
    for k in KERNELS:
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k)
        got = dev.intersect(rays)
        assert_bytes_equal(got, want, f"{name}: closest hit, query_kernel {k}")
        miss = got["primID"] == irl.INVALID_PRIM
        assert np.all(got["geomID"][miss] == irl.INVALID_GEOM) and np.all(got["flags"][miss] == irl.FLAG_ESCAPED)
        assert np.all(got["flags"][~miss] == 0)
        c = dev.counters()
        assert c["casts"] == sc.casts == rays.size and c["nodes_visited"] == 0 and c["paths"] == 0
        got_occ = dev.occluded(rays)
        assert np.array_equal(got_occ, occ), f"{name}: any hit, query_kernel {k}: {(got_occ != occ).sum()} rays differ"
        assert dev.counters()["casts"] == sc.casts + sa.casts
        dev.close()


@pytest.mark.parametrize("name", ["box", "soup-normals"])
def test_full_stats_counters_equal_the_oracles(scene_cache, name):
    hs, (rays, want, occ, sc, sa) = _case(scene_cache, name)
    for k in KERNELS:
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k).set_option("full_stats", 1)
        assert_bytes_equal(dev.intersect(rays), want, f"{name}: instrumented closest hit, query_kernel {k}")
        c = dev.counters()
        assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (sc.casts, sc.nodesVisited, sc.leafTests)
        dev.reset_counters()
        assert np.array_equal(dev.occluded(rays), occ)
        c = dev.counters()
        assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (sa.casts, sa.nodesVisited, sa.leafTests)
        dev.close()


# ------------------------------------------------------------------------------------------------------
# 4: the arithmetic options
# ------------------------------------------------------------------------------------------------------
def _grazing_scene(rng, n_tris):
    """Triangles stacked along -z with an edge the ray (0,0,0) -> (0,0,-1) passes through up to rounding (as in
    tests/test_gpu_parity.py): their binary32 edge functions are exactly zero, Mesh.cpp:38-51 decides them in binary64."""
    v = np.zeros(3 * n_tris, dtype=irl.VEC3)
    for i in range(n_tris):
        p1 = rng.uniform(0.5, 2.0, 2).astype(np.float32) * rng.choice([-1, 1], 2).astype(np.float32)
        p2 = (p1 * np.float32(-rng.uniform(0.5, 2.0))).astype(np.float32)
        p0 = rng.uniform(-3, 3, 2).astype(np.float32)
        z = np.float32(-(2.0 + i))
        for j, q in enumerate((p0, p1, p2)):
            v[3 * i + j] = (q[0], q[1], z)
    tris = np.arange(3 * n_tris, dtype=np.uint16).reshape(-1, 3)
    info = np.zeros(1, dtype=irl.MESH_INFO); info[0] = (0, 0, n_tris, 3 * n_tris)
    mats = np.zeros(1, dtype=irl.MATERIAL); mats[0]["ior"] = 1.5
    mat_ids = np.zeros(1, dtype=np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = info.ctypes.data, 1
    g.mesh_tris, g.num_tris = tris.ctypes.data, n_tris
    g.mesh_verts, g.num_verts = v.ctypes.data, len(v)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, 1
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, tris, info, mats, mat_ids]
    hs.desc.set_image(16, 8)
    return hs


def test_double_fallback_bit_exact_on_grazing_rays():
    differing = 0
    for seed in range(4):
        hs = _grazing_scene(np.random.default_rng(900 + seed), 48)
        rng = np.random.default_rng(seed)
        o = np.zeros((256, 3), np.float32)
        o[1:, :2] = (rng.normal(size=(255, 2)) * np.logspace(-7, -2, 255)[:, None]).astype(np.float32)
        d = np.tile(np.array([0, 0, -1], np.float32), (256, 1))
        rays = qb.make_rays(o, d)
        res = {}
        for df in (0, 1):
            if df:
                with ol.double_fallback():
                    want, occ, _, _ = oracle_query(hs, rays)
            else:
                want, occ, _, _ = oracle_query(hs, rays)
            for k in KERNELS:
                dev = irl.IpuScene(hs.desc).set_option("double_fallback", df).set_option("query_kernel", k)
                got = dev.intersect(rays)
                assert_bytes_equal(got, want, f"grazing rays, double_fallback {df}, query_kernel {k}, seed {seed}")
                assert np.array_equal(dev.occluded(rays), occ)
                dev.close()
            res[df] = want
        differing += int((res[0]["primID"] != res[1]["primID"]).sum())
    assert differing > 0, "the constructed rays never took the binary64 branch to a different verdict"


def test_fast_tier_names_the_same_primitives(scene_cache):
    """Option fast (the tolerance tier): camera rays of the box scene, the criterion of the render tier's test - the same
    primitive as the exact tier for every ray, t within 1e-6 relative - and the two query kernels give the same bytes."""
    hs = irl.HostScene.builtin("box")
    hs.desc.set_image(128, 128)
    rays = qb.primary_rays(hs)
    exact = irl.IpuScene(hs.desc).intersect(rays)
    got = {}
    for k in KERNELS:
        dev = irl.IpuScene(hs.desc).set_option("fast", 1).set_option("query_kernel", k)
        got[k] = dev.intersect(rays)
        occ = dev.occluded(rays)
        dev.close()
        assert np.array_equal(got[k]["primID"], exact["primID"]) and np.array_equal(got[k]["geomID"], exact["geomID"])
        h = exact["primID"] != irl.INVALID_PRIM
        assert h.mean() > 0.5
        assert np.all(np.abs(got[k]["t"][h] - exact["t"][h]) <= 1e-6 * np.abs(exact["t"][h]))
        assert np.array_equal(occ, h)
    assert_bytes_equal(got[0], got[1], "fast tier: query_kernel 0 against 1")
    with pytest.raises(irl.RaylibError, match="cannot be combined"):
        irl.IpuScene(hs.desc).set_option("fast", 1).set_option("full_stats", 1)


# ------------------------------------------------------------------------------------------------------
# 5: edges
# ------------------------------------------------------------------------------------------------------
def test_batch_sizes_and_host_batches(scene_cache):
    hs, (rays, want, occ, sc, sa) = _case(scene_cache, "box")
    for k in KERNELS:
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k)
        assert dev.intersect(rays[:0]).size == 0 and dev.occluded(rays[:0]).size == 0
        for n in (1, 63, 64, 65, 1037, 20011):
            assert_bytes_equal(dev.intersect(rays[:n]), want[:n], f"n = {n}, query_kernel {k}")
            assert np.array_equal(dev.occluded(rays[:n]), occ[:n])
        # a ragged slice at an odd (but 16-byte aligned after the copy) offset
        assert_bytes_equal(dev.intersect(rays[333:333 + 4099]), want[333:333 + 4099], f"ragged slice, query_kernel {k}")
        for batch in (4096, 1000, 7):
            dev.setRayBatch(batch)
            m = 12345 if batch != 7 else 300
            assert_bytes_equal(dev.intersect(rays[:m]), want[:m], f"host batches of {batch}, query_kernel {k}")
            assert np.array_equal(dev.occluded(rays[:m]), occ[:m])
        dev.close()


def test_torch_cast_on_a_non_default_stream(scene_cache):
    import torch
    hs, (rays, want, occ, sc, sa) = _case(scene_cache, "soup-normals")
    o = torch.from_numpy(np.stack([rays["origin"][c] for c in "xyz"], 1).copy()).cuda()
    d = torch.from_numpy(np.stack([rays["direction"][c] for c in "xyz"], 1).copy()).cuda()
    tmin = torch.from_numpy(rays["tMin"].copy()).cuda()
    tmax = torch.from_numpy(rays["tMax"].copy()).cuda()
    for k in KERNELS:
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k)
        host = dev.intersect(rays)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            r = dev.cast(o, d, tmin, tmax)
            a = dev.cast(o, d, tmin, tmax, any_hit=True)
        st.synchronize()
        assert np.array_equal(r["t"].cpu().numpy().view(np.uint32), host["t"].view(np.uint32))
        assert np.array_equal(r["prim_id"].cpu().numpy().view(np.uint32), host["primID"])
        assert np.array_equal(r["geom_id"].cpu().numpy(), host["geomID"].astype(np.int16).astype(np.int32))
        nrm = np.stack([host["normal"][c] for c in "xyz"], 1)
        assert np.array_equal(r["normal"].cpu().numpy().view(np.uint32), nrm.view(np.uint32))
        assert np.array_equal(r["bary"].cpu().numpy(), np.stack([host["b1"], host["b2"]], 1))
        assert np.array_equal(a["occluded"].cpu().numpy(), dev.occluded(rays))
        # scalar t_min / t_max
        r2 = dev.cast(o[:1000], d[:1000])
        torch.cuda.synchronize()
        plain = rays[:1000].copy(); plain["tMin"] = 0; plain["tMax"] = np.inf
        assert np.array_equal(r2["prim_id"].cpu().numpy().view(np.uint32), dev.intersect(plain)["primID"])
        dev.close()


def test_destroy_waits_for_an_enqueued_query(scene_cache):
    """A scene destroyed right after mi_query_device enqueued a large batch: destroy waits for it (the slot's lastWork event),
    and the batch's results are complete."""
    import torch
    hs = irl.HostScene.builtin("box")
    hs.desc.set_image(1024, 1024)
    ref = irl.IpuScene(hs.desc)
    prim = qb.primary_rays(hs)
    rays = qb.bounce_rays(prim, ref.intersect(prim), per_hit=4, seed=5)
    want = ref.intersect(rays)
    ref.close()
    t_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    for k in KERNELS:
        out = torch.zeros(rays.size * 32, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k)
        dev.query_device(irl.QUERY_CLOSEST, t_rays.data_ptr(), out.data_ptr(), rays.size, st.cuda_stream)
        dev.close()
        st.synchronize()
        assert_bytes_equal(out.cpu().numpy().view(irl.QUERY_HIT), want, f"destroyed behind its query, query_kernel {k}")


# ------------------------------------------------------------------------------------------------------
# 6: scale
# ------------------------------------------------------------------------------------------------------
def test_16m_diffuse_bounce_rays_both_kernels_identical():
    hs = irl.HostScene.builtin("box")
    hs.desc.set_image(1440, 1440)
    dev = irl.IpuScene(hs.desc)
    prim = qb.primary_rays(hs)
    hits = dev.intersect(prim)
    want_n = 8 * prim.size                               # 16 588 800: eight bounce rays per pixel of the frame
    per_hit = -(-want_n // int((hits["primID"] != irl.INVALID_PRIM).sum()))
    rays = qb.bounce_rays(prim, hits, per_hit=per_hit, seed=11)[:want_n]
    assert rays.size == want_n
    got = {}
    for k in KERNELS:
        dev.set_option("query_kernel", k)
        got[k] = dev.intersect(rays)
    assert got[0].tobytes() == got[1].tobytes()
    occ0 = dev.set_option("query_kernel", 0).occluded(rays)
    occ1 = dev.set_option("query_kernel", 1).occluded(rays)
    assert np.array_equal(occ0, occ1)
    dev.close()
    sample = np.random.default_rng(3).choice(rays.size, 20000, replace=False)
    want, occ, _, _ = oracle_query(hs, rays[sample])
    assert_bytes_equal(got[1][sample], want, "16.6 M bounce rays, a 20 k sample against the oracle")
    assert np.array_equal(occ1[sample], occ)
