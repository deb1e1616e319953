"""Geometry updates at their edges, on the GPU (pytest -m gpu): sequences of updates on one scene (the two compact buffers that
swap, the device copies a partial update reads, the scratch a refused update leaves behind, the host and the device entry mixed),
hand-made topologies that put the cut between refit_level_kernel and refit_top_kernel everywhere it can be
(refit_cases.retopologise; tests/test_refit_topologies.py shows each shape hitting its edge), and the values that decide a box's
bits (the extent catalogue, signed zeros, NaNs, binary32 subnormals, 65504). After EVERY update the device nodes equal the numpy
restatement and the host refit byte for byte, and closest / any hits under both query kernels equal a scene freshly created from
the cumulated arrays and those nodes, and the CPU oracle. No tolerances anywhere."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import refit_cases as rc
import test_refit_gpu as base

pytestmark = pytest.mark.gpu

FRAME = (48, 48, 8)          # every scene here is created for, and renders, this frame
N_RAYS, N_ORACLE = 20000, 2000


def _scene(desc, variants=False):
    return irl.IpuScene(base._frame(desc, *FRAME), variants=variants)


def full_check(dev, m, topology, what, variants=False, renders=None, rays=None, seed=3):
    """dev after an update against m, a Moved that holds the cumulated arrays: the nodes against numpy and against the host refit,
    the queries against a fresh scene and the oracle, and (renders: _check_renders' arguments) the frames."""
    got = dev.bvh_nodes()
    rc.assert_nodes_equal(got, rc.numpy_refit_levels(m.desc, topology), f"{what}: device nodes against numpy")
    m.set_nodes(topology).refit()
    rc.assert_nodes_equal(got, m.nodes, f"{what}: device nodes against the host refit")
    fresh = _scene(m.desc, variants)
    r = base._rays(m.nodes, N_RAYS, seed) if rays is None else rays
    base._check_queries(dev, fresh, m.desc, r, what, oracle_n=N_ORACLE)
    if renders is not None:
        base._check_renders(dev, fresh, m.desc, what, frame=FRAME, **renders)
    fresh.close()
    return got


def _as_rows(a):
    return np.ascontiguousarray(a).view(np.float32).reshape(a.size, -1).copy()


def _send(dev, how, side, **kw):
    """One update through the host entry, or through the device entry on the current stream or on `side`."""
    kw = {k: v for k, v in kw.items() if v is not None and v.size}
    if how == "host":
        dev.update_geometry(**kw)
        return
    import torch

    def put():
        dev.update_geometry_device(**{k: torch.from_numpy(_as_rows(v)).cuda() for k, v in kw.items()})
    if side is None:
        put()
    else:
        with torch.cuda.stream(side):
            put()


def _triangle_vertices(hs, mesh=0, tri=0):
    info = hs.mesh_info[mesh]
    return int(info["firstVertex"]) + hs.tris[int(info["firstIndex"]) + tri].astype(np.int64)


def _normals(hs, seed):
    n = np.random.default_rng(seed).normal(size=(hs.desc.num_normals, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = np.zeros(hs.desc.num_normals, irl.VEC3)
    out["x"], out["y"], out["z"] = n.astype(np.float32).T
    return out


# ------------------------------------------------------------------------------------------------------
# sequences
# ------------------------------------------------------------------------------------------------------
def _sequence(hs, name, dev, mode, what, variants=False):
    """One scene through: vertices, spheres, discs, normals, two refused updates, vertices again, all four, nothing, the
    original arrays. mode: "host" / "device" (every update through that entry) or "alternate" (host and device in turn, the
    device updates on a side stream, the queries of the checks on the default stream in between)."""
    side = None
    if mode != "host":
        torch = pytest.importorskip("torch")
        side = torch.cuda.Stream() if mode == "alternate" else None
    scale = 4.0 if name == "box" else 0.4
    original = {"vertices": hs.verts.copy(), "normals": hs._view(hs.desc.mesh_normals, hs.desc.num_normals, irl.VEC3).copy(),
                "spheres": hs.spheres.copy(), "discs": hs.discs.copy()}
    cur = dict(original)
    kernels = (0, 1, 2, 3) if variants else (0, 1)
    rays0 = base._rays(hs.nodes, N_RAYS, 8)
    hits0, occ0 = dev.intersect(rays0), dev.occluded(rays0)
    dev.set_option("kernel", 0)
    frame0 = base._render(dev, base._frame(hs.desc, *FRAME), irl.MODE_PATH_TRACE)
    count = [0]

    def entry():
        count[0] += 1
        if mode == "alternate":
            return ("host", None) if count[0] % 2 else ("device", side)
        return (mode, None)

    def check(label, renders=None):
        m = rc.Moved(hs, verts=cur["vertices"], normals=cur["normals"], spheres=cur["spheres"], discs=cur["discs"])
        full_check(dev, m, hs.nodes, f"{what}, step {label}", variants, renders, seed=count[0])

    def apply(label, renders=None, **kw):
        _send(dev, *entry(), **kw)
        cur.update({k: v for k, v in kw.items() if v.size})
        check(label, renders)

    def refused(label, needle, **kw):
        with pytest.raises(irl.RaylibError) as e:
            _send(dev, *entry(), **kw)
        assert "failed (1)" in str(e.value) and needle in str(e.value), str(e.value)       # MI_ERR_INVALID_ARG
        check(label)                                                                        # the cumulated arrays: unchanged

    (v1, s1, d1), (v2, s2, d2), (v3, s3, d3) = (rc.jitter(hs, seed, scale) for seed in (51, 52, 53))
    apply("1 vertices", vertices=v1)
    apply("2 spheres", spheres=s1)
    apply("3 discs", discs=d1)
    if hs.desc.num_normals:
        apply("4 normals", renders={"kernels": (0, 1), "oracle": not variants}, normals=_normals(hs, 5))
    else:
        refused("4 normals (the scene has none)", "without normals", normals=hs.verts.copy())
    t0 = _triangle_vertices(hs)
    bad = cur["vertices"].copy(); bad["x"][t0] = np.nan                        # a triangle with no finite x
    refused("5a NaN triangle", "not finite", vertices=bad, spheres=s2)
    bad = cur["vertices"].copy(); bad["x"][t0[1]] += np.float32(70000.0)       # an extent above 65504
    refused("5b extent above 65504", "65504", vertices=bad, discs=d2)
    apply("6 vertices again", vertices=v2)
    apply("7 all four", renders={"kernels": kernels, "oracle": not variants}, vertices=v3, normals=_normals(hs, 6), spheres=s3, discs=d3)
    apply("8 nothing")
    apply("9 the original arrays", renders={"kernels": kernels, "oracle": False} if variants else None, **original)
    rc.assert_nodes_equal(dev.bvh_nodes(), hs.nodes, f"{what}: back on the builder's nodes")
    base.assert_bytes_equal(dev.intersect(rays0), hits0, f"{what}: the first closest hits")
    assert np.array_equal(dev.occluded(rays0), occ0)
    dev.set_option("kernel", 0)
    base.assert_bytes_equal(base._render(dev, base._frame(hs.desc, *FRAME), irl.MODE_PATH_TRACE), frame0, f"{what}: the first frame")
    dev.close()


@pytest.mark.parametrize("mode", ["host", "device", "alternate"])
@pytest.mark.parametrize("name", ["soup-normals", "box"])
def test_sequence_of_updates(name, mode):
    hs = rc.scene(name)
    _sequence(hs, name, _scene(hs.desc), mode, f"{name} ({mode})")


@pytest.mark.parametrize("name", ["soup-normals", "box"])
def test_sequence_of_updates_on_a_blob_scene(name):
    hs = rc.scene(name)
    d = base._frame(hs.desc, *FRAME)
    _sequence(hs, name, irl.IpuScene.from_blob(irl.serialise_scene(d), d), "host", f"{name} (from_blob)")


@pytest.mark.parametrize("name", ["soup-normals", "box"])
def test_sequence_of_updates_in_the_variants_build(name):
    hs = rc.scene(name)
    _sequence(hs, name, _scene(hs.desc, variants=True), "alternate", f"{name} (variants build)", variants=True)


# ------------------------------------------------------------------------------------------------------
# topologies
# ------------------------------------------------------------------------------------------------------
SHAPES = [("caterpillar", {}), ("balanced", {}), ("level_of", {"n": 1023}), ("level_of", {"n": 1024}), ("level_of", {"n": 1025}),
          ("comb", {}), ("one", {}), ("three", {})]


@pytest.mark.parametrize("shape,kw", SHAPES, ids=lambda x: x if isinstance(x, str) else "-".join(str(v) for v in x.values()))
def test_update_of_a_hand_made_tree(shape, kw):
    hs = rc.edge_scene(shape)
    nodes, depth = rc.retopologise(hs, shape, seed=3, **kw)
    start = rc.with_topology(hs, nodes, depth)
    dev = _scene(start.desc)
    rc.assert_nodes_equal(dev.bvh_nodes(), nodes, f"{shape}: as created")
    v, s, d = rc.jitter(hs, 61, 0.75)
    _send(dev, "host", None, vertices=v, spheres=s, discs=d)
    m = rc.with_topology(hs, nodes, depth, verts=v, spheres=s, discs=d)
    got = full_check(dev, m, nodes, f"{shape} {kw}", renders={})
    assert not np.array_equal(rc.node_bytes(got), rc.node_bytes(nodes))
    # a second update, through the device entry: the other compact buffer, the same tables
    pytest.importorskip("torch")
    v, s, d = rc.jitter(hs, 62, 0.5)
    _send(dev, "device", None, vertices=v, spheres=s, discs=d)
    m = rc.with_topology(hs, nodes, depth, verts=v, spheres=s, discs=d)
    full_check(dev, m, nodes, f"{shape} {kw}, second update")
    if shape == "one":            # the root-box fields are not rewritten for a leaf root: both settings of root_start see the moved triangle
        fresh = _scene(m.desc)
        for rs in (0, 1):
            dev.set_option("root_start", rs); fresh.set_option("root_start", rs)
            base._check_renders(dev, fresh, m.desc, f"one node, root_start {rs}", frame=FRAME)
        fresh.close()
    dev.close()


# ------------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------------
def _leaf_of_triangle(nodes):
    """[triangle] -> its leaf node (one mesh)."""
    leaf = np.nonzero(nodes["geomID"] != irl.INVALID_GEOM)[0]
    out = np.zeros(leaf.size, np.int64)
    out[nodes["link"][leaf]] = leaf
    return out


def _aimed(verts, seed):
    """One ray per triangle, from a little way off towards its centroid."""
    p = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64).reshape(-1, 3, 3)
    c = p.mean(1)
    size = np.maximum((p.max(1) - p.min(1)).max(1), 1e-3)
    u = np.random.default_rng(seed).normal(size=c.shape); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + u * size[:, None] * 2
    return qb.make_rays(o.astype(np.float32), (-u).astype(np.float32))


def test_extent_catalogue_as_an_update():
    hs, verts, ext = rc.extent_catalogue()
    dev = _scene(hs.desc)
    dev.update_geometry(vertices=verts)
    m = rc.Moved(hs, verts=verts.copy())
    rays = np.concatenate([_aimed(verts, 1), base._rays(irl.refit_compact_bvh(m.desc), N_RAYS // 2, 2)])
    got = full_check(dev, m, hs.nodes, "extent catalogue", renders={}, rays=rays)
    hit = dev.intersect(rays[:ext.size])
    print(f"extent catalogue: {(hit['geomID'] != irl.INVALID_GEOM).sum()} of {ext.size} aimed rays hit")
    assert (hit["geomID"] != irl.INVALID_GEOM).sum() >= ext.size // 4
    # every probe's binary16, independently of the restatements: the smallest one that is not below the extent
    enc = got["dx"][_leaf_of_triangle(got)]
    assert (enc.view(np.float16).astype(np.float64) >= ext).all()
    below = np.where(enc > 0, enc - 1, enc).astype(np.uint16).view(np.float16).astype(np.float64)
    assert ((enc == 0) & (ext == 0) | (enc > 0) & (below < ext)).all()
    dev.close()


def test_signed_zeros_and_ignored_nans_keep_the_hosts_bits():
    K = 512
    k = np.arange(K)
    hs = rc.triangles(np.stack([(k % 32) * 3.0, (k // 32) * 3.0, np.full(K, -40.0)], 1)[:, None, :]
                      + np.array([[0, 0, 0], [1, 0, 1], [0, 1, 0]], np.float64)[None])
    p = np.zeros((K, 3, 3), np.float32)
    p[:, :, 0] = np.where((k % 2 == 0)[:, None], np.float32([0.0, -0.0, 1.0]), np.float32([-0.0, 0.0, 1.0]))   # both orders of the zeros
    p[:, :, 1] = k[:, None] + np.float32([1.0, 2.0, 5.0])
    p[k % 3 == 0, 0, 1] = np.nan                                                                               # a NaN in one vertex: ignored
    p[:, :, 2] = np.float32([-0.0, 0.0, -0.0])
    v = hs.verts.copy(); v["x"], v["y"], v["z"] = p.reshape(-1, 3).T
    dev = _scene(hs.desc)
    dev.update_geometry(vertices=v)
    got = full_check(dev, rc.Moved(hs, verts=v), hs.nodes, "signed zeros and NaNs", renders={})
    leaf = got[_leaf_of_triangle(got)]
    # the bits tests/test_refit_abi.py pins on the host: the FIRST zero seen stays, a NaN coordinate is passed over
    assert np.array_equal(leaf["min_x"].view(np.uint32), np.where(k % 2 == 0, 0x00000000, 0x80000000).astype(np.uint32))
    assert (leaf["dx"] == 0x3C00).all()
    assert np.array_equal(leaf["min_z"].view(np.uint32), np.full(K, 0x80000000, np.uint32)) and (leaf["dz"] == 0).all()
    assert np.array_equal(leaf["min_y"], np.where(k % 3 == 0, k + 2.0, k + 1.0).astype(np.float32))
    assert np.array_equal(leaf["dy"], np.where(k % 3 == 0, 0x4200, 0x4400).astype(np.uint16))                  # 3.0 / 4.0
    dev.close()


def test_binary32_subnormal_coordinates_are_not_flushed():
    K = 300
    k = np.arange(K)
    hs = rc.triangles(np.stack([(k % 20) * 3.0, (k // 20) * 3.0, np.full(K, -40.0)], 1)[:, None, :]
                      + np.array([[0, 0, 0], [1, 0, 1], [0, 1, 0]], np.float64)[None])
    rng = np.random.default_rng(9)
    bits = rng.integers(1, 1 << 23, (3 * K, 3)).astype(np.uint32) | (rng.integers(0, 2, (3 * K, 3)).astype(np.uint32) << 31)
    p = bits.view(np.float32)
    v = hs.verts.copy(); v["x"], v["y"], v["z"] = p.T
    dev = _scene(hs.desc)
    dev.update_geometry(vertices=v)
    got = full_check(dev, rc.Moved(hs, verts=v), hs.nodes, "subnormal coordinates", renders={})
    lo = np.stack([got["min_x"], got["min_y"], got["min_z"]], 1)
    assert ((lo != 0) & (np.abs(lo) < np.float32(1.1754944e-38))).all()                  # every minimum still a subnormal
    leaf = _leaf_of_triangle(got)
    assert np.array_equal(lo[leaf], p.reshape(K, 3, 3).min(1))
    assert (np.stack([got["dx"], got["dy"], got["dz"]], 1) == 1).all()                   # 0 < extent < 2^-25: up to the smallest half
    dev.close()


def test_an_extent_of_65504_is_the_last_one_accepted():
    K = 64
    k = np.arange(K)
    hs = rc.triangles(np.stack([(k % 8) * 3.0, (k // 8) * 3.0, np.full(K, -40.0)], 1)[:, None, :]
                      + np.array([[0, 0, 0], [1, 0, 1], [0, 1, 0]], np.float64)[None])
    dev = _scene(hs.desc)
    t0 = _triangle_vertices(hs)
    v = hs.verts.copy()
    v["x"][t0], v["y"][t0], v["z"][t0] = [0, 65504, 0], [0, 0, 1], [-40, -40, -41]
    dev.update_geometry(vertices=v)
    got = full_check(dev, rc.Moved(hs, verts=v), hs.nodes, "an extent of exactly 65504", renders={})
    assert int(got["dx"][0]) == 0x7BFF and int(got["dx"][_leaf_of_triangle(got)[0]]) == 0x7BFF
    above = v.copy(); above["x"][t0[1]] = np.nextafter(np.float32(65504), np.float32(np.inf))
    for how in ("host", "device"):
        if how == "device":
            pytest.importorskip("torch")
        with pytest.raises(irl.RaylibError) as e:
            _send(dev, how, None, vertices=above)
        assert "failed (1)" in str(e.value) and "65504" in str(e.value), str(e.value)
        full_check(dev, rc.Moved(hs, verts=v), hs.nodes, f"after refusing the next float ({how})")
    good = hs.verts.copy(); good["x"] += np.float32(1.5)
    dev.update_geometry(vertices=good)
    full_check(dev, rc.Moved(hs, verts=good), hs.nodes, "a good update after the refusal")
    dev.close()
