"""Rigid poses (mi_scene_set_poses*, include/mi_raylib.h): the header's text restated in numpy, one np.float32 operation per
operation (PoseChecker - it shares no code with the C++), a binary64 reference (the normalised quaternion's matrix, then s R p + t),
seeded and hand-placed poses, the 24 cube rotations, and small scenes built for the edges: vertex counts round the workgroup size,
many geometries, spheres and discs only, vertices no mesh owns. Used by test_pose_host.py, test_pose_abi.py and test_pose_gpu.py."""
import functools

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import obox_cases as oc
import point_cases as pc

F = np.float32
UNOWNED = 0xFFFF
KINDS = ("vertices", "normals", "spheres", "discs")


def arrays_of(desc):
    """desc's geometry as a dict of the four arrays (views; `vertices` as mi_scene_create keeps them: none without a mesh)."""
    view = irl.HostScene._view
    return {"vertices": view(None, desc.mesh_verts, desc.num_verts if desc.num_meshes else 0, irl.VEC3),
            "normals": view(None, desc.mesh_normals, desc.num_normals, irl.VEC3),
            "spheres": view(None, desc.spheres, desc.num_spheres, irl.SPHERE),
            "discs": view(None, desc.discs, desc.num_discs, irl.DISC)}


def xyz(a, names=("x", "y", "z")):
    return np.stack([a[n] for n in names], 1).astype(F) if a.size else np.zeros((0, 3), F)


class Refused(ValueError):
    pass


class PoseChecker:
    """The contract, from its text: owners from the geometry list, validity, identity, the frame of obox_frame, points, directions,
    spheres and discs - every operation a single binary32 one, in the order the header writes them."""

    def __init__(self, desc):
        view = irl.HostScene._view
        self.desc = desc
        self.geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
        self.info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
        self.rest = arrays_of(desc)
        self.owners = None

    def derive_owners(self):
        if self.owners is not None:
            return self.owners
        V, S, D = (self.rest[k].size for k in ("vertices", "spheres", "discs"))
        own = {"vertices": np.full(V, UNOWNED, np.int64), "spheres": np.full(S, UNOWNED, np.int64), "discs": np.full(D, UNOWNED, np.int64)}
        mesh_owner = np.full(self.info.size, UNOWNED, np.int64)
        kind = ("mesh", "sphere", "disc")
        for g, ref in enumerate(self.geometry):
            t, i = int(ref["type"]), int(ref["index"])
            table = (mesh_owner, own["spheres"], own["discs"])[t]
            if table[i] != UNOWNED:
                raise Refused(f"geometries {table[i]} and {g} both reference {kind[t]} {i}")
            table[i] = g
            if t == 0:
                a = int(self.info[i]["firstVertex"])
                b = a + int(self.info[i]["numVertices"])
                taken = own["vertices"][a:b] != UNOWNED
                if taken.any():
                    v = a + int(np.argmax(taken))
                    raise Refused(f"the vertex ranges of geometries {own['vertices'][v]} and {g} intersect (vertex {v})")
                own["vertices"][a:b] = g
        self.owners = own
        return own

    @staticmethod
    def valid(poses):
        q, t, s = poses["quat"].astype(F), poses["translation"].astype(F), poses["scale"].astype(F)
        with np.errstate(all="ignore"):
            qq = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
            inv = F(2) / qq
            return (np.isfinite(q).all(1) & np.isfinite(t).all(1) & np.isfinite(s) & (qq > 0) & np.isfinite(inv) & (s > 0))

    @staticmethod
    def identity(poses):
        q, t, s = poses["quat"], poses["translation"], poses["scale"]
        return (q[:, 0] == 0) & (q[:, 1] == 0) & (q[:, 2] == 0) & (q[:, 3] == 1) & (t == 0).all(1) & (s == 1)

    @staticmethod
    def frames(poses):
        """U, V, W [G, 3] float32: obox_frame as mi_raylib.h writes it."""
        x, y, z, w = (poses["quat"][:, k].astype(F) for k in range(4))
        with np.errstate(all="ignore"):
            qq = ((x * x + y * y) + z * z) + w * w
            s = F(2) / qq
            xs, ys, zs = x * s, y * s, z * s
            wx, wy, wz = w * xs, w * ys, w * zs
            xx, xy, xz, yy, yz, zz = x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
            one = F(1)
            U = np.stack([one - (yy + zz), xy + wz, xz - wy], 1)
            V = np.stack([xy - wz, one - (xx + zz), yz + wx], 1)
            W = np.stack([xz + wy, yz - wx, one - (xx + yy)], 1)
        assert U.dtype == F and V.dtype == F and W.dtype == F
        return U, V, W

    @staticmethod
    def _dir(U, V, W, p):
        with np.errstate(all="ignore"):
            r = (U * p[:, 0:1] + V * p[:, 1:2]) + W * p[:, 2:3]
        assert r.dtype == F
        return r

    def apply(self, poses):
        """The four posed arrays (a dict, fresh arrays), or Refused with the contract's words."""
        assert poses.dtype == irl.POSE
        if poses.size != self.geometry.size:
            raise Refused("num_geometry differs from the scene's geometry count")
        ok = self.valid(poses)
        if not ok.all():
            raise Refused(f"pose {int(np.argmin(ok))} is not valid")
        own = self.derive_owners()
        out = {k: self.rest[k].copy() for k in KINDS}
        if poses.size == 0:
            return out
        U, V, W = self.frames(poses)
        t, s = poses["translation"].astype(F), poses["scale"].astype(F)
        ident = self.identity(poses)

        def moved(owner):
            o = np.where(owner == UNOWNED, 0, owner)
            return (owner != UNOWNED) & ~ident[o], o

        with np.errstate(all="ignore"):
            m, o = moved(own["vertices"])
            if m.any():
                g = o[m]
                r = self._dir(U[g], V[g], W[g], xyz(self.rest["vertices"])[m])
                p = s[g][:, None] * r + t[g]
                assert p.dtype == F
                for k, c in enumerate("xyz"):
                    out["vertices"][c][m] = p[:, k]
                if out["normals"].size:
                    n = self._dir(U[g], V[g], W[g], xyz(self.rest["normals"])[m])
                    for k, c in enumerate("xyz"):
                        out["normals"][c][m] = n[:, k]
            m, o = moved(own["spheres"])
            if m.any():
                g = o[m]
                p = s[g][:, None] * self._dir(U[g], V[g], W[g], xyz(self.rest["spheres"])[m]) + t[g]
                for k, c in enumerate("xyz"):
                    out["spheres"][c][m] = p[:, k]
                out["spheres"]["radius"][m] = s[g] * self.rest["spheres"]["radius"][m]
            m, o = moved(own["discs"])
            if m.any():
                g = o[m]
                n = self._dir(U[g], V[g], W[g], xyz(self.rest["discs"], ("nx", "ny", "nz"))[m])
                p = s[g][:, None] * self._dir(U[g], V[g], W[g], xyz(self.rest["discs"], ("cx", "cy", "cz"))[m]) + t[g]
                for k, c in enumerate(("nx", "ny", "nz")):
                    out["discs"][c][m] = n[:, k]
                for k, c in enumerate(("cx", "cy", "cz")):
                    out["discs"][c][m] = p[:, k]
                out["discs"]["r"][m] = s[g] * self.rest["discs"]["r"][m]
        return out


# ------------------------------------------------------------------------------------------------------
# the binary64 reference and the bound
# ------------------------------------------------------------------------------------------------------
def reference_points64(checker, poses):
    """[(kind, posed coordinates float64 [n, 3], bound scale float64 [n, 3], mask of moved records)]: s R p + t with R the matrix
    of the quaternion normalised in binary64, and per coordinate scale (|x| + |y| + |z|) + |t_k| - what the bound multiplies."""
    own = checker.derive_owners()
    R = np.stack([oc.matrix64(q) for q in poses["quat"].astype(np.float64)])
    t, s = poses["translation"].astype(np.float64), poses["scale"].astype(np.float64)
    out = []
    for kind, names in (("vertices", ("x", "y", "z")), ("spheres", ("x", "y", "z")), ("discs", ("cx", "cy", "cz"))):
        rest = checker.rest[kind]
        if not rest.size:
            continue
        p = np.stack([rest[n] for n in names], 1).astype(np.float64)
        m = own[kind] != UNOWNED
        g = np.where(m, own[kind], 0)
        want = s[g][:, None] * np.einsum("nij,nj->ni", R[g], p) + t[g]
        size = s[g][:, None] * np.abs(p).sum(1)[:, None] + np.abs(t[g])
        out.append((kind, names, want, size, m))
    return out


def worst_ratio(checker, poses, got):
    """max over every moved coordinate of |got - reference| / (2^-24 (scale (|x| + |y| + |z|) + |t_k|))."""
    worst = 0.0
    for kind, names, want, size, m in reference_points64(checker, poses):
        g = np.stack([got[kind][n] for n in names], 1).astype(np.float64)
        ok = m[:, None] & (size > 0)
        if ok.any():
            worst = max(worst, float((np.abs(g - want)[ok] / (2.0 ** -24 * size[ok])).max()))
    return worst


# ------------------------------------------------------------------------------------------------------
# poses
# ------------------------------------------------------------------------------------------------------
def seeded_poses(hs, seed, n=None):
    """Uniform orientations (normalised Gaussian quaternions, rounded to binary32), translations up to the root box's size,
    scales 2^-3 .. 2^3 (log-uniform)."""
    n = hs.desc.num_geometry if n is None else n
    rng = np.random.default_rng(seed)
    lo, hi = pc.root_box(hs.nodes)
    size = float((hi - lo).max())
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-size, size, (n, 3))
    s = 2.0 ** rng.uniform(-3, 3, n)
    return qb.make_poses(n, quat=q, translation=t, scale=s)


IDENTITY = (0, 0, 0, 1, 0, 0, 0, 1)
# name -> (the eight floats, valid)
HAND = {
    "identity": (IDENTITY, True),
    "identity -0": ((-0.0, 0.0, -0.0, 1, -0.0, -0.0, 0.0, 1), True),
    "norm 1e3": ((200.0, -400.0, 400.0, 800.0, 1.0, 2.0, 3.0, 1.5), True),
    "norm 1e-18": ((2e-19, -4e-19, 4e-19, 8e-19, -1.0, 0.5, 0.25, 0.75), True),
    "norm 1e-20": ((2e-21, -4e-21, 4e-21, 8e-21, -1.0, 0.5, 0.25, 0.75), False),      # qq = 1e-40 > 0 (subnormal), 2 / qq = inf: mi_obox's rule
    "zero quaternion": ((0, 0, 0, 0, 0, 0, 0, 1), False),
    "infinite component": ((np.inf, 0, 0, 1, 0, 0, 0, 1), False),
    "infinite translation": ((0, 0, 0, 1, 0, -np.inf, 0, 1), False),
    "NaN": ((0, np.nan, 0, 1, 0, 0, 0, 1), False),
    "NaN scale": ((0, 0, 0, 1, 0, 0, 0, np.nan), False),
    "scale 0": ((0, 0, 0, 1, 0, 0, 0, 0.0), False),
    "negative scale": ((0, 0, 0, 1, 0, 0, 0, -1.0), False),
    "scale inf": ((0, 0, 0, 1, 0, 0, 0, np.inf), False),
    "norm overflows": ((3e19, 3e19, 0, 0, 0, 0, 0, 1), True),       # qq = inf, 2 / qq = 0 is finite: valid by mi_obox's rule, the frame is the unit matrix
}
TOO_FAR = (0, 0, 0, 1, 70000.0, 0, 0, 1)      # valid; on one geometry of several it pushes the root's extent past 65504


def pose_row(row):
    p = np.zeros(1, irl.POSE)
    p["quat"], p["translation"], p["scale"] = row[:4], row[4:7], row[7]
    return p


def with_pose(n, g, row):
    """n identity poses, pose g replaced by the eight floats of `row`."""
    p = qb.make_poses(n)
    p[g] = pose_row(row)[0]
    return p


def cube_poses():
    """[(quaternion with components in {0, +-1}, the rotation's integer matrix)] of the 24 cube rotations."""
    return [(q, np.rint(oc.matrix64(q)).astype(np.int64)) for q, _ in oc.cube_rotations()]


# ------------------------------------------------------------------------------------------------------
# expected scenes
# ------------------------------------------------------------------------------------------------------
class Scene:
    """A desc with what keeps its arrays alive, and its BVH nodes (a HostScene has the same two attributes). The nodes are an array
    of their own: they outlive the Scene they were taken from."""

    def __init__(self, desc, nodes, keep):
        self.desc, self.nodes, self._keep = desc, nodes, keep


def with_arrays(hs, a, topology=None):
    """hs's desc over other geometry arrays (a dict as arrays_of's), refitted on the host (irl.refit_compact_bvh): the desc a fresh
    scene is created from, and the nodes an update with those arrays must leave. topology: other nodes than hs's to refit (a
    rebuilt scene's)."""
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    keep = [hs]
    if topology is not None:
        topology = np.ascontiguousarray(topology)
        keep.append(topology)
        d.bvh_nodes, d.num_nodes = topology.ctypes.data, topology.size
    for key, ptr in (("vertices", "mesh_verts"), ("normals", "mesh_normals"), ("spheres", "spheres"), ("discs", "discs")):
        if a[key].size:
            arr = np.ascontiguousarray(a[key])
            keep.append(arr)
            setattr(d, ptr, arr.ctypes.data)
    nodes = irl.refit_compact_bvh(d)
    keep.append(nodes)
    d.bvh_nodes = nodes.ctypes.data if nodes.size else None
    return Scene(d, nodes, keep)


def posed(hs, poses, topology=None):
    """with_arrays of the twin's arrays of `poses`: the scene mi_scene_set_poses must leave."""
    return with_arrays(hs, irl.pose_geometry_host(hs.desc, poses), topology)


def update_args(a):
    """The keywords of IpuScene.update_geometry for a dict of arrays (only the kinds the scene has)."""
    return {k: v for k, v in a.items() if v.size}


def assert_arrays_equal(got, want, what):
    for k in KINDS:
        assert got[k].dtype == want[k].dtype and got[k].size == want[k].size, f"{what}: {k} {got[k].size} records, want {want[k].size}"
        if got[k].tobytes() != want[k].tobytes():
            gb, wb = got[k].view(np.uint8).reshape(got[k].size, -1), want[k].view(np.uint8).reshape(want[k].size, -1)
            i = int(np.nonzero((gb != wb).any(1))[0][0])
            raise AssertionError(f"{what}: {k} differ, first at {i}:\n got  {got[k][i]}\n want {want[k][i]}")


# ------------------------------------------------------------------------------------------------------
# scenes for the edges
# ------------------------------------------------------------------------------------------------------
def edge_scene(mesh_verts=(), n_spheres=0, n_discs=0, gaps=None, spare_spheres=0, normals=False, seed=3):
    """Meshes of the given vertex counts (triangles over random vertex triples of their own mesh, at least one each), n_spheres
    spheres and n_discs discs, one geometry each, in that order. gaps[i] = vertices no mesh owns in front of mesh i (gaps[len] =
    behind the last); spare_spheres = spheres at the end of the array that no geometry references."""
    rng = np.random.default_rng(seed)
    M = len(mesh_verts)
    gaps = list(gaps) if gaps is not None else [0] * (M + 1)
    V = sum(mesh_verts) + sum(gaps)
    p = rng.uniform(-20, 20, (V, 3)).astype(F); p[:, 2] -= 60
    v = np.zeros(V, irl.VEC3); v["x"], v["y"], v["z"] = p.T
    nrm = np.zeros(V if normals else 0, irl.VEC3)
    if normals:
        nn = rng.normal(size=(V, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nrm["x"], nrm["y"], nrm["z"] = nn.T
    info = np.zeros(M, irl.MESH_INFO)
    tris, at, first_tri = [], 0, 0
    for i, nv in enumerate(mesh_verts):
        at += gaps[i]
        nt = max(1, nv // 3)
        idx = rng.integers(0, nv, (nt, 3)) if nv < 3 else np.stack([rng.permutation(nv)[:3] for _ in range(nt)])
        tris.append(idx.astype(np.uint16))
        info[i] = (first_tri, at, nt, nv)
        first_tri += nt
        at += nv
    tri = np.concatenate(tris) if tris else np.zeros((0, 3), np.uint16)
    S = n_spheres + spare_spheres
    sph = np.zeros(S, irl.SPHERE)
    c = rng.uniform(-20, 20, (S, 3)).astype(F)
    sph["x"], sph["y"], sph["z"], sph["radius"] = c[:, 0], c[:, 1], c[:, 2] - 60, rng.uniform(0.5, 3, S).astype(F)
    dsc = np.zeros(n_discs, irl.DISC)
    c = rng.uniform(-20, 20, (n_discs, 3)).astype(F)
    nn = rng.normal(size=(n_discs, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    dsc["nx"], dsc["ny"], dsc["nz"], dsc["r"] = nn[:, 0], nn[:, 1], nn[:, 2], rng.uniform(0.5, 3, n_discs).astype(F)
    dsc["cx"], dsc["cy"], dsc["cz"] = c[:, 0], c[:, 1], c[:, 2] - 60
    G = M + n_spheres + n_discs
    geom = np.zeros(G, irl.GEOM_REF)
    geom["index"] = np.concatenate([np.arange(M), np.arange(n_spheres), np.arange(n_discs)])
    geom["type"] = np.concatenate([np.zeros(M), np.ones(n_spheres), np.full(n_discs, 2)])
    mats = np.zeros(1, irl.MATERIAL); mats["albedo"]["x"] = .5; mats["ior"] = 1.5
    mat_ids = np.zeros(max(G, 1), np.uint32)
    g = irl.SceneDesc()
    g.geometry, g.num_geometry = geom.ctypes.data, G
    g.mesh_info, g.num_meshes = (info.ctypes.data if M else None), M
    g.mesh_tris, g.num_tris = (tri.ctypes.data if M else None), len(tri)
    g.mesh_verts, g.num_verts = (v.ctypes.data if V else None), V
    g.mesh_normals, g.num_normals = (nrm.ctypes.data if nrm.size else None), nrm.size
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, G
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.spheres, g.num_spheres = (sph.ctypes.data if S else None), S
    g.discs, g.num_discs = (dsc.ctypes.data if n_discs else None), n_discs
    g.fov_radians, g.anti_alias_scale = 0.9, 0.25
    g.max_path_length, g.roulette_start_depth, g.samples_per_pixel = 10, 3, 4
    g.rng_seed, g.path_trace, g.device = 1442, 1, 0
    g.set_image(16, 16)
    nodes, depth = irl.build_lbvh(g)      # (the host builder repacks the arrays: gaps and spare spheres need a desc made by hand)
    g.bvh_nodes, g.num_nodes, g.max_leaf_depth = (nodes.ctypes.data if nodes.size else None), nodes.size, depth
    return Scene(g, nodes, [geom, info, tri, v, nrm, sph, dsc, mats, mat_ids])


EDGES = {
    "1 vertex": dict(mesh_verts=(1,), n_spheres=1),
    "255 vertices": dict(mesh_verts=(255,)),
    "256 vertices": dict(mesh_verts=(256,)),
    "257 vertices": dict(mesh_verts=(257,), normals=True),
    "2049 vertices": dict(mesh_verts=(2049,)),
    "2 geometries": dict(mesh_verts=(130, 127)),
    "300 geometries": dict(mesh_verts=(3,) * 290, n_spheres=6, n_discs=4, normals=True),
    "spheres and discs": dict(n_spheres=3, n_discs=2),
    "unowned": dict(mesh_verts=(100, 157), gaps=(1, 2, 1), n_spheres=1, spare_spheres=2),
}


@functools.lru_cache(maxsize=None)
def edge(name):
    return edge_scene(**EDGES[name])
