"""Scenes and moved geometry for the geometry-update tests (test_refit_abi.py and test_refit_topologies.py on the CPU,
test_refit_gpu.py and test_refit_edges_gpu.py on the GPU), and a numpy restatement of the refit: compare / select min / max,
binary32 hi - lo, binary16 rounded up - node by node (numpy_refit) and height by height (numpy_refit_levels). For the edges:
hand-made topologies over a scene's leaves (retopologise), the extent catalogue, and the closest hit over every primitive
without a BVH (brute_force_closest)."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np

import ipu_ray_lib_amd as irl

ASSETS = Path(irl.REPO_ROOT) / "assets"


def soup(seed, with_normals=False, n_tris=600, n_meshes=2, spread=10.0):
    """A random triangle soup in `n_meshes` meshes + a sphere + a disc (as tests/test_query_gpu.py builds it)."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-spread, spread, (n_tris, 3)).astype(np.float32); centers[:, 2] -= 4 * spread
    verts = (centers.repeat(3, 0) + rng.normal(scale=1.5, size=(3 * n_tris, 3))).astype(np.float32)
    cuts = np.linspace(0, n_tris, n_meshes + 1).astype(np.int64)
    tris = np.concatenate([np.arange(3 * (cuts[m + 1] - cuts[m])) for m in range(n_meshes)]).astype(np.uint16).reshape(-1, 3)
    v = np.zeros(len(verts), dtype=irl.VEC3); v["x"], v["y"], v["z"] = verts.T
    nrm = np.zeros(len(verts) if with_normals else 0, dtype=irl.VEC3)
    if with_normals:
        nn = rng.normal(size=(len(verts), 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nrm["x"], nrm["y"], nrm["z"] = nn.T
    info = np.zeros(n_meshes, dtype=irl.MESH_INFO)
    for m in range(n_meshes):
        info[m] = (cuts[m], 3 * cuts[m], cuts[m + 1] - cuts[m], 3 * (cuts[m + 1] - cuts[m]))
    sph = np.zeros(1, dtype=irl.SPHERE); sph[0] = (0, 0, -4 * spread, 3)
    dsc = np.zeros(1, dtype=irl.DISC); dsc[0] = (0, 1, 0, 3 * spread, 0, -1.2 * spread, -4 * spread)
    ng = n_meshes + 2
    mats = np.zeros(ng, dtype=irl.MATERIAL); mats["albedo"]["x"] = .5; mats["albedo"]["y"] = .6; mats["ior"] = 1.5
    mats["emission"]["x"][0] = 2.0; mats["emissive"][0] = 1
    mat_ids = np.arange(ng, dtype=np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = info.ctypes.data, n_meshes
    g.mesh_tris, g.num_tris = tris.ctypes.data, n_tris
    g.mesh_verts, g.num_verts = v.ctypes.data, len(v)
    g.mesh_normals, g.num_normals = (nrm.ctypes.data if with_normals else None), len(nrm)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, ng
    g.materials, g.num_materials = mats.ctypes.data, ng
    g.spheres, g.num_spheres = sph.ctypes.data, 1
    g.discs, g.num_discs = dsc.ctypes.data, 1
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, nrm, tris, info, sph, dsc, mats, mat_ids]
    return hs


def triangles(points):
    """A scene of the given triangles ([n, 3, 3] float32), one mesh, built by the host builder."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.zeros(len(p), dtype=irl.VEC3); v["x"], v["y"], v["z"] = p.T
    tris = np.arange(len(p), dtype=np.uint16).reshape(-1, 3)
    info = np.zeros(1, dtype=irl.MESH_INFO); info[0] = (0, 0, len(tris), len(p))
    mats = np.zeros(1, dtype=irl.MATERIAL); mat_ids = np.zeros(1, np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = info.ctypes.data, 1
    g.mesh_tris, g.num_tris = tris.ctypes.data, len(tris)
    g.mesh_verts, g.num_verts = v.ctypes.data, len(v)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, 1
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, tris, info, mats, mat_ids]
    return hs


def scene(name):
    if name == "soup":
        return soup(1234, False)
    if name == "soup-normals":
        return soup(1235, True)
    if name == "test_scene.dae":
        return irl.HostScene.import_file(ASSETS / "test_scene.dae", load_normals=True)
    if name == "monkey_bust.glb":
        return irl.HostScene.builtin("monkey", ASSETS / "monkey_bust.glb")
    return irl.HostScene.builtin(name)


class Moved:
    """hs's scene with some arrays replaced: `desc` points at the new arrays (and at `nodes`, when given)."""

    def __init__(self, hs, verts=None, normals=None, spheres=None, discs=None, nodes=None):
        self.verts = np.ascontiguousarray(verts if verts is not None else hs.verts.copy())
        self.normals = np.ascontiguousarray(normals if normals is not None else
                                            hs._view(hs.desc.mesh_normals, hs.desc.num_normals, irl.VEC3).copy())
        self.spheres = np.ascontiguousarray(spheres if spheres is not None else hs.spheres.copy())
        self.discs = np.ascontiguousarray(discs if discs is not None else hs.discs.copy())
        d = irl.SceneDesc.from_buffer_copy(hs.desc)
        if self.verts.size: d.mesh_verts = self.verts.ctypes.data
        if self.normals.size: d.mesh_normals = self.normals.ctypes.data
        if self.spheres.size: d.spheres = self.spheres.ctypes.data
        if self.discs.size: d.discs = self.discs.ctypes.data
        self.hs = hs
        self.desc = d
        self.nodes = None
        if nodes is not None:
            self.set_nodes(nodes)

    def set_nodes(self, nodes):
        self.nodes = np.ascontiguousarray(nodes)
        self.desc.bvh_nodes = self.nodes.ctypes.data
        return self

    def refit(self):
        """The host refit of these arrays, installed as the desc's nodes: the desc a fresh scene is created from."""
        return self.set_nodes(irl.refit_compact_bvh(self.desc))


# ---- moves ------------------------------------------------------------------------------------------------------
def jitter(hs, seed, scale=0.5):
    """Every vertex, sphere and disc moved by a small random displacement (radii kept)."""
    rng = np.random.default_rng(seed)
    v = hs.verts.copy()
    for c in "xyz":
        v[c] += rng.uniform(-scale, scale, v.size).astype(np.float32)
    s = hs.spheres.copy()
    for c in "xyz":
        s[c] += rng.uniform(-scale, scale, s.size).astype(np.float32)
    d = hs.discs.copy()
    for c in ("cx", "cy", "cz"):
        d[c] += rng.uniform(-scale, scale, d.size).astype(np.float32)
    return v, s, d


def rigid(hs, mesh, angle, shift):
    """Mesh `mesh` rotated about its vertices' centroid (y axis) and shifted; the other vertices kept."""
    v = hs.verts.copy()
    info = hs.mesh_info[mesh]
    a, b = int(info["firstVertex"]), int(info["firstVertex"] + info["numVertices"])
    p = np.stack([v["x"][a:b], v["y"][a:b], v["z"][a:b]], 1).astype(np.float64)
    c = p.mean(0)
    ca, sa = np.cos(angle), np.sin(angle)
    r = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    q = ((p - c) @ r.T + c + np.asarray(shift)).astype(np.float32)
    v["x"][a:b], v["y"][a:b], v["z"][a:b] = q.T
    return v


# ---- the refit restated in numpy ---------------------------------------------------------------------------------
def _grow(lo, hi, p):
    lo = np.where(p < lo, p, lo).astype(np.float32)
    hi = np.where(p > hi, p, hi).astype(np.float32)
    return lo, hi


def _half_not_smaller(e):
    h = np.float32(e).astype(np.float16)
    bits = np.array(h).view(np.uint16)
    if np.float32(h) < e:
        bits = bits + np.uint16(1)
    return int(bits)


def numpy_refit(desc, topology):
    """The nodes of `topology` (a BVH_NODE array) with every box recomputed from desc's arrays, per the rules above."""
    view = irl.HostScene._view
    geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
    info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
    tris = view(None, desc.mesh_tris, 3 * desc.num_tris, np.dtype("<u2"))
    verts = view(None, desc.mesh_verts, desc.num_verts, irl.VEC3)
    spheres = view(None, desc.spheres, desc.num_spheres, irl.SPHERE)
    discs = view(None, desc.discs, desc.num_discs, irl.DISC)
    inf = np.float32(np.inf)
    out = topology.copy()
    boxes = [None] * len(out)
    for i in range(len(out) - 1, -1, -1):
        n = out[i]
        lo, hi = np.full(3, inf, np.float32), np.full(3, -inf, np.float32)
        if n["geomID"] != irl.INVALID_GEOM:
            g = geometry[n["geomID"]]
            if g["type"] == 0:
                m = info[g["index"]]
                for k in range(3):
                    q = verts[int(m["firstVertex"]) + int(tris[3 * (int(m["firstIndex"]) + int(n["link"])) + k])]
                    lo, hi = _grow(lo, hi, np.array([q["x"], q["y"], q["z"]], np.float32))
            else:
                q = spheres[g["index"]] if g["type"] == 1 else discs[g["index"]]
                c = np.array([q["x"], q["y"], q["z"]] if g["type"] == 1 else [q["cx"], q["cy"], q["cz"]], np.float32)
                r = np.float32(q["radius"] if g["type"] == 1 else q["r"])
                lo, hi = (c - r).astype(np.float32), (c + r).astype(np.float32)
        else:
            for child in (i + 1, int(n["link"])):
                for p in boxes[child]:
                    lo, hi = _grow(lo, hi, p)
        boxes[i] = (lo, hi)
        ext = (hi - lo).astype(np.float32)
        out[i]["min_x"], out[i]["min_y"], out[i]["min_z"] = lo
        out[i]["dx"], out[i]["dy"], out[i]["dz"] = [_half_not_smaller(e) for e in ext]
    return out


def node_bytes(a):
    return a.view(np.uint8).reshape(a.size, -1)


def assert_nodes_equal(got, want, what):
    gb, wb = node_bytes(got), node_bytes(want)
    assert got.size == want.size, f"{what}: {got.size} nodes, want {want.size}"
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} nodes differ; first at {i}:\n got  {got[i]}\n want {want[i]}")


# ---- the refit restated per height (vectorised: the reference where the loop above is too slow) --------------------------------
def node_heights(topology):
    """Leaf 0, interior 1 + the higher child: the heights mi_scene_update buckets the nodes by."""
    leaf = topology["geomID"] != irl.INVALID_GEOM
    link = topology["link"].astype(np.int64)
    h = [0] * len(topology)
    for i in range(len(topology) - 1, -1, -1):
        if not leaf[i]:
            a, b = h[i + 1], h[link[i]]
            h[i] = 1 + (a if a > b else b)
    return np.array(h, np.int64)


def _grow_all(lo, hi, p):
    """Bounds::grow on [n, 3] arrays: compare / select, the held value kept on a tie or a NaN."""
    return np.where(p < lo, p, lo), np.where(p > hi, p, hi)


def half_not_smaller_bits(e):
    """[..] float32 -> the binary16 bits of round-to-nearest-even, one more where that is below e."""
    e = np.asarray(e, np.float32)
    with np.errstate(over="ignore"):
        h = e.astype(np.float16)
    bits = h.view(np.uint16).copy()
    bits[h.astype(np.float32) < e] += np.uint16(1)
    return bits


def numpy_refit_levels(desc, topology):
    """numpy_refit, one numpy step per height instead of one Python step per node (the same rules in the same order)."""
    view = irl.HostScene._view
    geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
    info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
    tris = view(None, desc.mesh_tris, 3 * desc.num_tris, np.dtype("<u2")).astype(np.int64)
    verts = view(None, desc.mesh_verts, desc.num_verts, irl.VEC3)
    spheres = view(None, desc.spheres, desc.num_spheres, irl.SPHERE)
    discs = view(None, desc.discs, desc.num_discs, irl.DISC)
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1) if verts.size else np.zeros((0, 3), np.float32)
    N = len(topology)
    out = topology.copy()
    lo = np.full((N, 3), np.inf, np.float32)
    hi = np.full((N, 3), -np.inf, np.float32)
    height = node_heights(topology)
    leaves = np.nonzero(height == 0)[0]
    leaves = leaves[topology["geomID"][leaves] != irl.INVALID_GEOM]
    g = geometry[topology["geomID"][leaves]]
    prim = topology["link"][leaves].astype(np.int64)
    tri = leaves[g["type"] == 0]
    if tri.size:
        m = info[g["index"][g["type"] == 0]]
        base = 3 * (m["firstIndex"].astype(np.int64) + prim[g["type"] == 0])
        for k in range(3):
            p = xyz[m["firstVertex"].astype(np.int64) + tris[base + k]]
            lo[tri], hi[tri] = _grow_all(lo[tri], hi[tri], p)
    for kind, recs, names in ((1, spheres, ("x", "y", "z", "radius")), (2, discs, ("cx", "cy", "cz", "r"))):
        sel = leaves[g["type"] == kind]
        if sel.size:
            q = recs[g["index"][g["type"] == kind]]
            c = np.stack([q[names[0]], q[names[1]], q[names[2]]], 1).astype(np.float32)
            r = q[names[3]].astype(np.float32)[:, None]
            lo[sel], hi[sel] = (c - r).astype(np.float32), (c + r).astype(np.float32)
    link = topology["link"].astype(np.int64)
    order = np.argsort(height, kind="stable")
    starts = np.searchsorted(height[order], np.arange(1, height.max() + 2 if N else 1))
    for k in range(len(starts) - 1):
        at = order[starts[k]:starts[k + 1]]
        a, b = at + 1, link[at]
        l, h = np.full((at.size, 3), np.inf, np.float32), np.full((at.size, 3), -np.inf, np.float32)
        for p in (lo[a], hi[a], lo[b], hi[b]):
            l, h = _grow_all(l, h, p)
        lo[at], hi[at] = l, h
    with np.errstate(invalid="ignore"):
        ext = (hi - lo).astype(np.float32)
    bits = half_not_smaller_bits(ext)
    out["min_x"], out["min_y"], out["min_z"] = lo.T
    out["dx"], out["dy"], out["dz"] = bits.T
    return out


# ---- hand-made topologies ----------------------------------------------------------------------------------------
REFIT_TOP_THREADS = 1024          # kRefitTopThreads (refit_kernels.hpp)


def top_first(heights):
    """refitTables' rule restated: the heights topFirst .. H go to the one-workgroup kernel - from the top down, every level
    of at most REFIT_TOP_THREADS nodes, never the leaves. (levels, topFirst): levels[h] = nodes of height h."""
    H = int(heights.max()) if heights.size else 0
    levels = np.bincount(heights, minlength=H + 1)
    top = H + 1
    while top > 1 and levels[top - 1] <= REFIT_TOP_THREADS:
        top -= 1
    return levels, top


class _Patch:
    def __init__(self, i):
        self.i = i


def _balanced(items):
    """items (leaf numbers or subtrees) under a tree that halves them, the larger half first."""
    items = list(items)
    while len(items) > 1:                           # pair up level by level: a perfect tree when len is a power of two
        nxt = [(items[k], items[k + 1]) for k in range(0, len(items) - 1, 2)]
        if len(items) % 2:
            nxt.append(items[-1])
        items = nxt
    return items[0]


def _caterpillar(items):
    """(leaf, (leaf, (leaf, ...))): every interior node's FIRST child is the leaf - a stack of depth two walks it."""
    t = items[-1]
    for k in range(len(items) - 2, -1, -1):
        t = (items[k], t)
    return t


def retopologise(hs, shape, n=None, spare=3, tail=300, seed=None):
    """(nodes, max_leaf_depth): leaves of hs - their (geomID, link) pairs in the builder's order, or shuffled by `seed` - hung
    into a hand-made tree, laid out depth-first with the first child adjacent; the boxes are numpy_refit_levels' of hs's arrays.
    Shapes: "caterpillar" (n leaves, default all: one node per height), "balanced" (a perfect tree over the first 2^k leaves,
    n = 2^k, default the most that fit), "level_of" (exactly n nodes of height 1: n pairs under a balanced top, `spare` leaves
    hung one by one above the root), "comb" (a perfect tree over n leaves, default 4096, whose last leaf is replaced by a
    caterpillar of `tail` leaves), "one" (a single leaf) and "three" (one pair)."""
    src = hs.nodes
    pairs = [(int(g), int(l)) for g, l in zip(src["geomID"], src["link"]) if g != irl.INVALID_GEOM]
    if seed is not None:
        pairs = [pairs[k] for k in np.random.default_rng(seed).permutation(len(pairs))]
    L = len(pairs)
    if shape == "caterpillar":
        n = L if n is None else n
        tree, used = _caterpillar(list(range(n))), n
    elif shape == "balanced":
        n = 1 << (L.bit_length() - 1) if n is None else n
        assert n & (n - 1) == 0
        tree, used = _balanced(range(n)), n
    elif shape == "level_of":
        tree = _balanced([(2 * k, 2 * k + 1) for k in range(n)])
        for k in range(spare):
            tree = (2 * n + k, tree)
        used = 2 * n + spare
    elif shape == "comb":
        n = 4096 if n is None else n
        assert n & (n - 1) == 0
        tree, used = _balanced(list(range(n - 1)) + [_caterpillar(list(range(n - 1, n - 1 + tail)))]), n - 1 + tail
    elif shape == "one":
        tree, used = 0, 1
    elif shape == "three":
        tree, used = (0, 1), 2
    else:
        raise ValueError(shape)
    assert used <= L, f"{shape}: needs {used} leaves, the scene has {L}"
    rows, depth_max = [], 0
    stack = [(tree, 1)]
    while stack:                                    # (no recursion: a caterpillar is thousands of levels deep)
        t, depth = stack.pop()
        if isinstance(t, _Patch):
            rows[t.i][1] = len(rows)                # the second child starts where the first child's subtree ended
        elif isinstance(t, tuple):
            stack.append((t[1], depth + 1)); stack.append((_Patch(len(rows)), 0)); stack.append((t[0], depth + 1))
            rows.append([irl.INVALID_GEOM, 0])
        else:
            rows.append(list(pairs[t]))
            depth_max = max(depth_max, depth)
    nodes = np.zeros(len(rows), irl.BVH_NODE)
    nodes["geomID"], nodes["link"] = [r[0] for r in rows], [r[1] for r in rows]
    return numpy_refit_levels(hs.desc, nodes), depth_max


def with_topology(hs, nodes, depth, **arrays):
    """A Moved of hs hung under `nodes` (num_nodes / max_leaf_depth set), the geometry replaced by `arrays`."""
    m = Moved(hs, **arrays)
    m.desc.num_nodes, m.desc.max_leaf_depth = len(nodes), depth
    return m.set_nodes(nodes)


def contract_walk(nodes):
    """test_host_and_abi.py::test_compact_bvh_contract's walk: preorder IS array order, every node reached once, the second child
    behind the first child's subtree. Returns (max leaf depth, leaf count)."""
    N = len(nodes)
    leaf = nodes["geomID"] != irl.INVALID_GEOM
    link = nodes["link"].astype(np.int64)
    order, depth_max = [], 0
    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        order.append(i)
        if leaf[i]:
            depth_max = max(depth_max, d)
        else:
            assert i + 1 < link[i] < N, f"node {i}: second child {link[i]}"
            stack.append((int(link[i]), d + 1)); stack.append((i + 1, d + 1))
    assert order == list(range(N)), "depth-first order is not array order"
    assert int(leaf.sum()) * 2 - 1 == N
    return depth_max, int(leaf.sum())


# ---- every primitive, no BVH --------------------------------------------------------------------------------------
def brute_force_closest(desc, rays):
    """Closest t (float32, inf = nothing) of each RAY over EVERY primitive of desc, with the oracle's own leaf tests and its
    acceptance rule (tMin < t < the best so far, from tMax), as test_oracle_pins.py::test_bvh_queries_against_brute_force."""
    import oracle_lib as ol
    o = ol.lib()
    view = irl.HostScene._view
    geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
    info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
    tris = view(None, desc.mesh_tris, 3 * desc.num_tris, np.dtype("<u2")).reshape(-1, 3)
    verts = view(None, desc.mesh_verts, desc.num_verts, irl.VEC3)
    spheres = view(None, desc.spheres, desc.num_spheres, irl.SPHERE)
    discs = view(None, desc.discs, desc.num_discs, irl.DISC)
    tri_list, others = [], []
    for ref in geometry:
        if ref["type"] == 0:
            m = info[ref["index"]]
            for p in range(int(m["numTriangles"])):
                q = [verts[int(m["firstVertex"]) + int(k)] for k in tris[int(m["firstIndex"]) + p]]
                tri_list.append([ol.Vec3(float(v["x"]), float(v["y"]), float(v["z"])) for v in q])
        elif ref["type"] == 1:
            s = spheres[ref["index"]]
            others.append((o.o_sphere_intersect, ol.Sphere(*[float(s[k]) for k in ("x", "y", "z", "radius")])))
        else:
            d = discs[ref["index"]]
            others.append((o.o_disc_intersect, ol.Disc(*[float(d[k]) for k in ("nx", "ny", "nz", "r", "cx", "cy", "cz")])))
    out = np.full(rays.size, np.inf, np.float32)
    bary = (ol.f32 * 3)()
    for i, r in enumerate(rays):
        ray = ol.Ray(ol.Vec3(*[float(r["origin"][k]) for k in "xyz"]), float(r["tMin"]),
                     ol.Vec3(*[float(r["direction"][k]) for k in "xyz"]), float(r["tMax"]))
        sh = ol.Shear(); o.o_ray_shear(C.byref(ray), C.byref(sh))
        best = float(r["tMax"])
        for p0, p1, p2 in tri_list:
            t = o.o_intersect_triangle(p0, p1, p2, C.byref(sh), float("inf"), bary)
            if t > 0.0 and t < float("inf") and t > ray.tMin and t < best:       # (leaf_intersect's test, then the walk's)
                best = t
        for fn, rec in others:
            t = fn(C.byref(rec), C.byref(ray))
            if t > ray.tMin and t < best:
                best = t
        out[i] = best if best < float(r["tMax"]) or np.isinf(best) else np.inf
    return out


# ---- scenes for the edges ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_scene(shape):
    """A scene with enough leaves for retopologise(., shape) at its default (edge-hitting) size."""
    if shape == "one":
        return triangles([[[0, 0, -5], [1, 0, -5], [0, 1, -6]]])
    if shape == "three":
        return triangles([[[0, 0, -5], [1, 0, -5], [0, 1, -6]], [[2, 0, -7], [3, 0, -7], [2, 1, -8]]])
    n_tris = {"caterpillar": 3000, "balanced": 600, "level_of": 2100, "comb": 4400}[shape]
    return soup(2000 + n_tris, False, n_tris=n_tris, n_meshes=3)


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def extent_catalogue(seed=7):
    """(hs, verts, ext): a scene of thin triangles built from a tame version of them (unit triangles on a grid), the vertex
    array that makes triangle k's x extent exactly ext[k] (x minimum -0.0 / +0.0 in turn) and its y / z extents two other
    probes above minima that make hi - lo itself round (subnormals, +-1e4, ...), and the probes: the float32 extents where
    rounding up to binary16 can go wrong. Every box stays inside [-32752, 32752] (x: [0, 65504]), so no interior extent
    passes 65504."""
    rng = np.random.default_rng(seed)
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    down = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    probes = [np.float32(0), _f32(1)]                                      # 0, the smallest binary32 subnormal
    for x in (2.0 ** -25, 2.0 ** -24, 2.0 ** -14):                         # half of, and the smallest binary16 subnormal; the smallest normal
        probes += [down(x), np.float32(x), up(x)]
    halves = list(range(1, 1024, 31)) + [1023]                             # binary16 subnormals, a coarse stride
    halves += sorted(int(b) for b in rng.integers(0x0400, 0x7BFF, 500))    # seeded normal ones (below 65504: h + 1 ulp must encode)
    for b in halves:
        h, nxt = np.array([b, b + 1], np.uint16).view(np.float16).astype(np.float32)
        mid = np.float32((np.float64(h) + np.float64(nxt)) / 2)            # exact: 12 significant bits
        probes += [h, up(h), down(mid), mid, up(mid)]
    probes.append(np.float32(65504))
    ext = np.array(probes, np.float32)
    M = ext.size
    k = np.arange(M)
    lo = np.zeros((M, 3), np.float32)
    lo[:, 0] = np.where(k % 2 == 0, np.float32(-0.0), np.float32(0.0))
    minima = np.array([1e4, -1e4, _f32(3), -_f32(0x7FFFFF), 1e-39, 3.1415927, -0.0, -7777.777, 0.1, 255.99], np.float32)
    e = np.stack([ext, ext[(k + M // 3) % M], ext[(k + 2 * (M // 3)) % M]], 1)
    for a in (1, 2):
        m = minima[(k + a) % minima.size]
        lo[:, a] = np.where(e[:, a] > 2e4, (-e[:, a] / 2).astype(np.float32), m)
    hi = (lo + e).astype(np.float32)
    assert (hi[:, 0] == ext).all() and np.abs(hi).max() <= 65504 and np.abs(lo[:, 1:]).max() <= 32752 and hi[:, 1:].max() <= 32752
    p = np.stack([lo, np.stack([hi[:, 0], lo[:, 1], hi[:, 2]], 1), np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], 1)], 1)   # [M, 3 vertices, 3]
    g = np.stack([(k % 64) * 3.0, (k // 64) * 3.0, np.full(M, -50.0)], 1)
    tame = g[:, None, :] + np.array([[0, 0, 0], [1, 0, 1], [0, 1, 0]], np.float64)[None]
    hs = triangles(tame)
    verts = hs.verts.copy()
    verts["x"], verts["y"], verts["z"] = p.reshape(-1, 3).T
    verts.setflags(write=False); ext.setflags(write=False)
    return hs, verts, ext
