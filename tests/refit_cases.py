"""Scenes and moved geometry for the geometry-update tests (test_refit_abi.py on the CPU, test_refit_gpu.py on the GPU), and a
numpy restatement of the refit: compare / select min / max, binary32 hi - lo, binary16 rounded up."""
import ctypes as C
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
