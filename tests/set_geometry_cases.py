"""Scene contents for the set-geometry tests (test_canonical_prims.py and test_set_geometry_abi.py on the CPU,
test_set_geometry_gpu.py on the GPU): `Contents` wraps the nine arrays of any desc - a named scene's or a hand-made one's - under
ONE set of render parameters (a live scene keeps the ones it was created with, so every scene compared with it is created with
the same), with the host twin's nodes, a jittered copy and the data plane as torch tensors; `hand` builds the hand-made tables:
geometries without triangles at chosen places, primitive counts round a workgroup's 256, thousands of one-sphere geometries."""
import ctypes as C

import numpy as np

import ipu_ray_lib_amd as irl
import refit_cases as rc
import rebuild_cases as bc

ARRAYS = (("geometry", "num_geometry", irl.GEOM_REF, 1), ("mesh_info", "num_meshes", irl.MESH_INFO, 1), ("mat_ids", "num_mat_ids", np.dtype("<u4"), 1),
          ("materials", "num_materials", irl.MATERIAL, 1), ("mesh_tris", "num_tris", np.dtype("<u2"), 3), ("mesh_verts", "num_verts", irl.VEC3, 1),
          ("mesh_normals", "num_normals", irl.VEC3, 1), ("spheres", "num_spheres", irl.SPHERE, 1), ("discs", "num_discs", irl.DISC, 1))


def render_params(d, size=32, spp=4):
    """The render parameters every scene of these tests is created with."""
    d.set_image(size, size)
    d.fov_radians, d.anti_alias_scale = 0.9, 0.25
    d.max_path_length, d.roulette_start_depth, d.samples_per_pixel = 10, 3, spp
    d.rng_seed, d.path_trace, d.device = 1442, 1, 0
    return d


class Contents:
    """Copies of the nine arrays `desc` points at; .desc points at the copies (no nodes)."""

    def __init__(self, desc, name="", size=32, spp=4):
        self.name = name
        self.a = {}
        d = irl.SceneDesc()
        for ptr, cnt, dtype, per in ARRAYS:
            n = int(getattr(desc, cnt))
            arr = irl.HostScene._view(None, getattr(desc, ptr), n * per, dtype).copy()
            self.a[ptr] = arr
            setattr(d, cnt, n)
            setattr(d, ptr, arr.ctypes.data if arr.size else None)
        self.desc = render_params(d, size, spp)
        self._twin = None

    def twin(self):
        """(desc under the twin's nodes, nodes, depth): what a fresh scene is created from. The oracle's stack bound is asserted."""
        if self._twin is None:
            nodes, depth = bc.twin(self.desc)
            d = irl.SceneDesc.from_buffer_copy(self.desc)
            nodes = np.ascontiguousarray(nodes)
            d.bvh_nodes, d.num_nodes, d.max_leaf_depth = (nodes.ctypes.data if nodes.size else None), len(nodes), depth
            self._twin = (d, nodes, depth)
        return self._twin

    def jittered(self, seed, scale=0.3):
        """The same contents with every vertex, sphere and disc moved a little (refit_cases.jitter on these arrays)."""
        rng = np.random.default_rng(seed)
        out = Contents(self.desc, self.name + " jittered", int(self.desc.image_width), int(self.desc.samples_per_pixel))
        for key, fields in (("mesh_verts", "xyz"), ("spheres", "xyz"), ("discs", ("cx", "cy", "cz"))):
            for c in fields:
                out.a[key][c] += rng.uniform(-scale, scale, out.a[key].size).astype(np.float32)
        return out

    def update_args(self):
        kw = {}
        for key, arg in (("mesh_verts", "vertices"), ("spheres", "spheres"), ("discs", "discs")):
            if self.a[key].size and (key != "mesh_verts" or self.desc.num_meshes):
                kw[arg] = self.a[key]
        return kw

    def tensors(self):
        """The data plane as CUDA tensors, the keywords of IpuScene.set_geometry_device."""
        import torch
        out = {}
        for key, arg, width, dt in (("mesh_tris", "tris", 3, np.int16), ("mesh_verts", "vertices", 3, np.float32), ("mesh_normals", "normals", 3, np.float32),
                                    ("spheres", "spheres", 4, np.float32), ("discs", "discs", 7, np.float32)):
            if self.a[key].size:
                out[arg] = torch.from_numpy(self.a[key].view(dt).reshape(-1, width).copy()).cuda()
        return out

    @property
    def num_prims(self):
        g, info = self.a["geometry"], self.a["mesh_info"]
        return int(sum(int(info[r["index"]]["numTriangles"]) if r["type"] == 0 else 1 for r in g))


def named(name, **kw):
    hs = rc.scene(name)
    return Contents(hs.desc, name, **kw)


def hand(spec, seed=5, **kw):
    """Hand-made contents from raw arrays. spec: a list of ("mesh", triangles) | ("sphere",) | ("disc",) in geometry order. Every
    mesh has three vertices more than its triangles use (so first_vertex differs from three times first_index, and a mesh without
    triangles still has vertices); its triangles index its own vertices in a shuffled order."""
    rng = np.random.default_rng(seed)
    geometry, info, tris, verts, spheres, discs = [], [], [], [], [], []
    for item in spec:
        if item[0] == "mesh":
            t = int(item[1])
            nv = 3 * t + 3
            assert nv <= 65535
            info.append((len(tris), len(verts), t, nv))
            geometry.append((len(info) - 1, 0, 0))
            centres = rng.uniform(-20, 20, (t + 1, 3)); centres[:, 2] -= 60
            p = centres.repeat(3, 0) + rng.normal(scale=1.0, size=(nv, 3))
            verts += p.astype(np.float32).tolist()
            tris += rng.permutation(3 * t).reshape(t, 3).tolist()
        elif item[0] == "sphere":
            geometry.append((len(spheres), 1, 0))
            c = rng.uniform(-20, 20, 3)
            spheres.append((c[0], c[1], c[2] - 60, rng.uniform(0.3, 1.5)))
        else:
            geometry.append((len(discs), 2, 0))
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            c = rng.uniform(-20, 20, 3)
            discs.append((n[0], n[1], n[2], rng.uniform(0.5, 2.0), c[0], c[1], c[2] - 60))
    G = len(geometry)
    arrays = {
        "geometry": np.array(geometry, dtype=irl.GEOM_REF) if G else np.zeros(0, irl.GEOM_REF),
        "mesh_info": np.array(info, dtype=irl.MESH_INFO) if info else np.zeros(0, irl.MESH_INFO),
        "mesh_tris": np.array(tris, dtype="<u2").reshape(-1, 3),
        "mesh_verts": np.zeros(len(verts), irl.VEC3),
        "spheres": np.array(spheres, dtype=irl.SPHERE) if spheres else np.zeros(0, irl.SPHERE),
        "discs": np.array(discs, dtype=irl.DISC) if discs else np.zeros(0, irl.DISC),
    }
    if verts:
        arrays["mesh_verts"]["x"], arrays["mesh_verts"]["y"], arrays["mesh_verts"]["z"] = np.array(verts, np.float32).T
    mats = np.zeros(3, irl.MATERIAL); mats["albedo"]["x"] = .5; mats["albedo"]["y"] = .6; mats["ior"] = 1.5
    mats["emission"]["x"][0] = 2.0; mats["emissive"][0] = 1
    mat_ids = (np.arange(G) % 3).astype(np.uint32)
    d = irl.SceneDesc()
    d.geometry, d.num_geometry = (arrays["geometry"].ctypes.data if G else None), G
    d.mesh_info, d.num_meshes = (arrays["mesh_info"].ctypes.data if info else None), len(info)
    d.mesh_tris, d.num_tris = (arrays["mesh_tris"].ctypes.data if tris else None), len(tris)
    d.mesh_verts, d.num_verts = (arrays["mesh_verts"].ctypes.data if verts else None), len(verts)
    d.spheres, d.num_spheres = (arrays["spheres"].ctypes.data if spheres else None), len(spheres)
    d.discs, d.num_discs = (arrays["discs"].ctypes.data if discs else None), len(discs)
    d.mat_ids, d.num_mat_ids = (mat_ids.ctypes.data if G else None), G
    d.materials, d.num_materials = mats.ctypes.data, 3
    return Contents(d, str(spec)[:60], **kw)


# the hand-made tables: where the search from a canonical index to its geometry can go wrong
HAND_MADE = {
    "empty mesh first": [("mesh", 0), ("mesh", 5), ("sphere",), ("mesh", 3)],
    "empty mesh last": [("mesh", 4), ("disc",), ("mesh", 2), ("mesh", 0)],
    "two empty meshes in a row": [("mesh", 3), ("mesh", 0), ("mesh", 0), ("mesh", 4), ("sphere",)],
    "empty meshes everywhere": [("mesh", 0), ("mesh", 0), ("sphere",), ("mesh", 0), ("mesh", 2), ("mesh", 0), ("mesh", 0)],
    "spheres and discs only": [("sphere",), ("disc",), ("sphere",), ("sphere",), ("disc",)],
    "one triangle": [("mesh", 1)],
    "one sphere": [("sphere",)],
    "255 primitives": [("mesh", 100), ("sphere",), ("mesh", 153), ("disc",)],
    "256 primitives": [("mesh", 100), ("sphere",), ("mesh", 154), ("disc",)],
    "257 primitives": [("mesh", 100), ("sphere",), ("mesh", 155), ("disc",)],
    "3000 single-sphere geometries": [("sphere",)] * 3000,
    "empty scene": [],
}


def canon_reference(c):
    """rebuild_cases.canonical_prims of the contents: (lo, hi, geomID, primID)."""
    return bc.canonical_prims(c.desc)


def canon_boxes(c, table):
    """(lo, hi, geomID, primID) of a CANON_PRIM table, the boxes by compare / select from the records' own indices."""
    v = c.a["mesh_verts"]
    xyz = np.stack([v["x"], v["y"], v["z"]], 1) if v.size else np.zeros((0, 3), np.float32)
    P = table.size
    lo, hi = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    tri = table["kind"] == 0
    if tri.any():
        pts = np.stack([xyz[table[k][tri]] for k in "abc"], 1)          # [T, 3 vertices, 3]
        l = np.full((pts.shape[0], 3), np.inf, np.float32); h = -l
        for k in range(3):
            l, h = np.where(pts[:, k] < l, pts[:, k], l), np.where(pts[:, k] > h, pts[:, k], h)
        lo[tri], hi[tri] = l, h
    for kind, key, names in ((1, "spheres", ("x", "y", "z", "radius")), (2, "discs", ("cx", "cy", "cz", "r"))):
        sel = table["kind"] == kind
        if sel.any():
            q = c.a[key][table["a"][sel]]
            ctr = np.stack([q[names[0]], q[names[1]], q[names[2]]], 1).astype(np.float32)
            r = q[names[3]].astype(np.float32)[:, None]
            lo[sel], hi[sel] = (ctr - r).astype(np.float32), (ctr + r).astype(np.float32)
    return lo, hi, table["geomID"].astype(np.int64), table["primID"].astype(np.int64)
