"""Shared by the crossing-count tests (test_count_abi.py, test_count_checker.py, test_count_gpu.py): scenes, ray and point sets,
analytic inside answers, and THE CHECKER - a Python walk of a scene's compact nodes built only from what tests/oracle_lib.py
exports: the oracle's box test over the fixed interval, its shear and triangle test, its disc test, and sphere_crossings restated in
numpy binary32 from the contract's text (include/mi_raylib.h), one np.float32 operation per operation. It is slow per ray, which is
why every batch checked with it is a few thousand rays at most."""
import ctypes as C

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
from refit_cases import soup      # the 600-triangle soup of tests/test_query_gpu.py: two meshes + a sphere + a disc

F = np.float32
INF = F(np.inf)
DEFAULT_DIR = np.array(irl.DEFAULT_INSIDE_DIR, F)


# ------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------
def mesh_scene(verts, tris, spheres=(), discs=()):
    """A scene of one mesh (verts [V, 3], tris [T, 3]; none when T == 0) + spheres [(x, y, z, r)] + discs [(nx, ny, nz, r, cx, cy,
    cz)]. Geometry order: the mesh, spheres, discs. The BVH is the host builder's."""
    verts = np.asarray(verts, F).reshape(-1, 3)
    tris = np.ascontiguousarray(np.asarray(tris, np.uint16).reshape(-1, 3))
    nm = 1 if len(tris) else 0
    v = np.zeros(len(verts), dtype=irl.VEC3); v["x"], v["y"], v["z"] = verts.T
    info = np.zeros(nm, dtype=irl.MESH_INFO)
    if nm:
        info[0] = (0, 0, len(tris), len(verts))
    sph = np.zeros(len(spheres), dtype=irl.SPHERE)
    for i, s in enumerate(spheres):
        sph[i] = tuple(F(x) for x in s)
    dsc = np.zeros(len(discs), dtype=irl.DISC)
    for i, d in enumerate(discs):
        dsc[i] = tuple(F(x) for x in d)
    G = nm + len(sph) + len(dsc)
    mats = np.zeros(1, dtype=irl.MATERIAL); mats["ior"] = 1.5
    mat_ids = np.zeros(max(G, 1), dtype=np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = (info.ctypes.data if nm else None), nm
    g.mesh_tris, g.num_tris = (tris.ctypes.data if nm else None), len(tris)
    g.mesh_verts, g.num_verts = (v.ctypes.data if nm else None), (len(v) if nm else 0)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, G
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.spheres, g.num_spheres = (sph.ctypes.data if len(sph) else None), len(sph)
    g.discs, g.num_discs = (dsc.ctypes.data if len(dsc) else None), len(dsc)
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, tris, info, sph, dsc, mats, mat_ids]
    hs.desc.set_image(8, 8)
    return hs


def cube_mesh(shift=(0.0, 0.0, 0.0)):
    """The closed cube [-1, 1]^3 (moved by `shift`): 8 vertices, 12 triangles, outward winding."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F) + np.asarray(shift, F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [(a, b, c) for a, b, c, d in quads] + [(a, c, d) for a, b, c, d in quads]
    return v.astype(F), np.array(t, np.uint16)


def icosphere_mesh(subdivisions=2):
    """The unit icosphere: an icosahedron subdivided `subdivisions` times, every vertex pushed onto the unit sphere (2: 162
    vertices, 320 triangles). Its facets lie inside the sphere: the midpoint of an edge of length e is at sqrt(1 - e^2 / 4)."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid = {}

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[k] = len(v) - 1
            return mid[k]
        t2 = []
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            t2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = t2
    return np.array(v, np.float64).astype(F), np.array(t, np.uint16)


THREE_SPHERES = ((4.0, 0.0, 0.0, 1.0), (0.0, 4.0, 0.5, 1.5), (-4.0, -1.0, 0.0, 0.75))      # disjoint, and clear of the cube
ONE_DISC = ((0.0, 1.0, 0.0, 2.0, 0.0, -3.0, 0.0),)


def scene(name):
    """box, box-simple, spheres (builtins) | soup (600 triangles + a sphere + a disc) | soup-tris (600 triangles, nothing else) |
    cube | icosphere | mixed (3 disjoint spheres + 1 disc + the cube) | three-spheres"""
    if name == "soup":
        hs = soup(1234, False)
    elif name == "soup-tris":
        src = soup(1234, False)
        verts = np.stack([src.verts[c] for c in "xyz"], 1)
        hs = mesh_scene(verts, np.arange(len(verts), dtype=np.uint16).reshape(-1, 3))
    elif name == "cube":
        hs = mesh_scene(*cube_mesh())
    elif name == "icosphere":
        hs = mesh_scene(*icosphere_mesh(2))
    elif name == "mixed":
        hs = mesh_scene(*cube_mesh(), spheres=THREE_SPHERES, discs=ONE_DISC)
    elif name == "three-spheres":
        hs = mesh_scene(np.zeros((0, 3), F), np.zeros((0, 3), np.uint16), spheres=THREE_SPHERES)
    else:
        hs = irl.HostScene.builtin(name)
    hs.desc.set_image(64, 64)
    return hs


def grazing_scene(rng, n_tris):
    """Triangles stacked along -z with an edge the ray (0,0,0) -> (0,0,-1) passes through up to rounding (as tests/test_query_gpu.py
    builds it): their binary32 edge functions are exactly zero, Mesh.cpp:38-51 decides them in binary64."""
    v = np.zeros((3 * n_tris, 3), F)
    for i in range(n_tris):
        p1 = rng.uniform(0.5, 2.0, 2).astype(F) * rng.choice([-1, 1], 2).astype(F)
        p2 = (p1 * F(-rng.uniform(0.5, 2.0))).astype(F)
        p0 = rng.uniform(-3, 3, 2).astype(F)
        z = F(-(2.0 + i))
        for j, q in enumerate((p0, p1, p2)):
            v[3 * i + j] = (q[0], q[1], z)
    return mesh_scene(v, np.arange(3 * n_tris, dtype=np.uint16).reshape(-1, 3))


def grazing_rays(seed, n=256):
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), F)
    o[1:, :2] = (rng.normal(size=(n - 1, 2)) * np.logspace(-7, -2, n - 1)[:, None]).astype(F)
    return qb.make_rays(o, np.tile(np.array([0, 0, -1], F), (n, 1)))


def root_box(hs):
    n = hs.nodes[0]
    lo = np.array([n["min_x"], n["min_y"], n["min_z"]], F)
    ext = np.array([n["dx"], n["dy"], n["dz"]], np.uint16).view(np.float16).astype(F)
    return lo, (lo + ext).astype(F)


# ------------------------------------------------------------------------------------------------------
# rays and points
# ------------------------------------------------------------------------------------------------------
def mixed_rays(hs, n, seed):
    """n RAY records: origins inside the root box (65 %) and around it, random unit directions, a finite t_max on a tenth, a
    positive t_min on a tenth, and a few rays with one or two zero direction components and with t_min > t_max."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(hs)
    size = (hi - lo).astype(F)
    o = rng.uniform(lo, hi, (n, 3)).astype(F)
    out = rng.random(n) < 0.35
    o[out] = rng.uniform(lo - size, hi + size, (int(out.sum()), 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    k = max(n // 100, 1)
    for a in range(3):
        d[a * k:(a + 1) * k, a] = 0.0                      # one zero component
    d[3 * k:3 * k + 4] = [0, 0, -1]                         # two zero components
    d[3 * k + 4:3 * k + 8] = [1, 0, 0]
    rays = qb.make_rays(o, d)
    diag = float(np.linalg.norm(size))
    sel = rng.random(n) < 0.1
    rays["tMax"][sel] = rng.uniform(0, diag, int(sel.sum()))
    sel = rng.random(n) < 0.1
    rays["tMin"][sel] = rng.uniform(0, diag / 4, int(sel.sum()))
    rays["tMin"][4 * k:4 * k + 4] = F(0.75 * diag); rays["tMax"][4 * k:4 * k + 4] = F(0.25 * diag)      # t_min > t_max
    return rays


def points_of(pos, radius=np.inf):
    return qb.make_points(np.asarray(pos, F).reshape(-1, 3), np.broadcast_to(F(radius), (len(pos),)).astype(F))


def sign_rays(points, direction=None):
    """The rays an inside test walks: origin = the point, the direction, t_min = 0, t_max = +inf."""
    d = DEFAULT_DIR if direction is None else np.asarray(direction, F)
    pos = np.stack([points[c] for c in "xyz"], 1)
    return qb.make_rays(pos, np.tile(d, (len(pos), 1)))


def cube_points():
    """The cube inputs: 4 096 random points of [-1.5, 1.5]^3 and every point of the 0.25-spaced grid on it whose coordinates all
    differ from +-1 (a point ON a face has no inside). Returns (positions [N, 3] float32, inside [N] bool): the analytic answer."""
    rnd = np.random.default_rng(7).uniform(-1.5, 1.5, (4096, 3)).astype(F)
    g = np.arange(-1.5, 1.5 + 1e-9, 0.25)
    grid = np.array([[x, y, z] for x in g for y in g for z in g], F)
    grid = grid[(np.abs(grid) != 1.0).all(1)]
    pos = np.concatenate([rnd, grid])
    return pos, (np.abs(pos) < 1.0).all(1)


def icosphere_points():
    """The icosphere inputs: 2 000 random points of [-1.2, 1.2]^3 without those whose norm lies in (0.93, 1.0) - between the
    facets and the sphere, where the mesh's inside is not the sphere's. Returns (positions, inside)."""
    pos = np.random.default_rng(5).uniform(-1.2, 1.2, (2000, 3)).astype(F)
    r = np.linalg.norm(pos.astype(np.float64), axis=1)
    keep = ~((r > 0.93) & (r < 1.0))
    return pos[keep], (r < 1.0)[keep]


def sphere_points(spheres, n, seed, margin=1e-3):
    """Points around the given spheres, none within `margin` of a shell; for each sphere some whose ray along the default
    direction leaves the sphere with the centre BEHIND the origin (the case the reference's sphere test gives up on). Returns
    (positions, inside)."""
    rng = np.random.default_rng(seed)
    c = np.array([s[:3] for s in spheres], np.float64); r = np.array([s[3] for s in spheres], np.float64)
    lo, hi = (c - r[:, None]).min(0) - 1.0, (c + r[:, None]).max(0) + 1.0
    pos = [rng.uniform(lo, hi, (n // 2, 3))]
    for ci, ri in zip(c, r):
        u = rng.normal(size=(n // (2 * len(c)), 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        pos.append(ci + u * rng.uniform(0, 1.3 * ri, (len(u), 1)))
        ahead = DEFAULT_DIR.astype(np.float64) / np.linalg.norm(DEFAULT_DIR)
        pos.append(ci + ahead * rng.uniform(0.05, 0.95, (16, 1)) * ri)               # inside, the centre behind the ray
    pos = np.concatenate(pos).astype(F)
    dist = np.linalg.norm(pos.astype(np.float64)[:, None, :] - c[None], axis=2) - r[None]
    keep = (np.abs(dist) > margin).all(1)
    return pos[keep], (dist < 0).any(1)[keep]


# ------------------------------------------------------------------------------------------------------
# sphere_crossings in numpy binary32, from the contract's text
# ------------------------------------------------------------------------------------------------------
def dot32(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def sphere_crossings32(c, radius2, o, d, t_min, t_max):
    c, o, d = np.asarray(c, F), np.asarray(o, F), np.asarray(d, F)
    radius2, t_min, t_max = F(radius2), F(t_min), F(t_max)
    with np.errstate(all="ignore"):
        f = (c - o).astype(F)
        dd = dot32(d, d)
        tca = F(dot32(f, d) / dd)
        l = (f - (d * tca).astype(F)).astype(F)
        l2 = dot32(l, l)
        if not (l2 <= radius2):
            return 0
        td = F(np.sqrt(F(F(radius2 - l2) / dd)))
        t0, t1 = F(tca - td), F(tca + td)
        return int(t0 > t_min and t0 < t_max) + int(t1 > t_min and t1 < t_max)


def sphere_crossings64(c, radius, o, d, t_min, t_max):
    """(count, roots) in binary64 with the true radius; roots is None when the line misses the sphere."""
    c, o, d = (np.asarray(x, np.float64) for x in (c, o, d))
    f = c - o
    dd = d @ d
    tca = (f @ d) / dd
    l2 = (f - d * tca) @ (f - d * tca)
    if l2 > radius * radius:
        return 0, None
    td = np.sqrt((radius * radius - l2) / dd)
    roots = (tca - td, tca + td)
    return sum(1 for t in roots if t_min < t < t_max), roots


# ------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------
class _Prims(dict):
    """Checker's leaf primitives by node index, an entry made when it is first read."""

    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, i):
        self[i] = self.make(i)
        return self[i]


class Checker:
    """The crossing count of a ray on a host scene's compact nodes: the reference's walk (a stack, first child first) with the
    oracle's box test over the FIXED interval [t_min, t_max] and, at every leaf whose box is hit, the oracle's primitive test."""

    def __init__(self, hs, lazy=False):
        """lazy: a leaf's primitive is resolved when a walk first reaches it (a tree of hundreds of thousands of nodes)."""
        self.desc = hs.desc
        nodes = np.ascontiguousarray(hs.nodes)
        self.n = nodes.size
        self.nodes = (ol.Node * max(self.n, 1)).from_buffer_copy(nodes.tobytes() if self.n else bytes(C.sizeof(ol.Node)))
        self.link = nodes["link"].tolist()
        self.geom = nodes["geomID"].tolist()
        self.prims = _Prims(lambda i: self._prim_of(hs, i))
        if not lazy:
            for i in range(self.n):
                if self.geom[i] != irl.INVALID_GEOM:
                    self.prims[i]

    @classmethod
    def lazy(cls, hs):
        return cls(hs, lazy=True)

    def _prim_of(self, hs, i):
        ref = hs.geometry[self.geom[i]]
        if ref["type"] == 0:
            info = hs.mesh_info[ref["index"]]
            tri = hs.tris.reshape(-1, 3)[int(info["firstIndex"]) + self.link[i]]
            v = hs.verts[int(info["firstVertex"]) + tri.astype(np.int64)]
            return (0, [ol.Vec3(float(p["x"]), float(p["y"]), float(p["z"])) for p in v])
        if ref["type"] == 1:
            s = hs.spheres[ref["index"]]
            return (1, (np.array([s["x"], s["y"], s["z"]], F), F(F(s["radius"]) * F(s["radius"]))))
        return (2, ol.Disc.from_buffer_copy(hs.discs[ref["index"]].tobytes()))

    def count(self, ray):
        """(crossings, box tests, primitive tests) of one RAY record."""
        o = ol.lib()
        if self.n == 0:
            return 0, 0, 0
        r = ol.Ray.from_buffer_copy(np.asarray(ray).tobytes())
        t_min, t_max = F(r.tMin), F(r.tMax)
        with np.errstate(all="ignore"):
            inv = [float(F(1) / F(x)) for x in (r.direction.x, r.direction.y, r.direction.z)]
        inv = ol.Vec3(*inv)
        sh = None
        bary = (C.c_float * 3)()
        t0, t1 = C.c_float(), C.c_float()
        crossings = boxes = tests = 0
        stack = [0]
        while stack:
            cur = stack.pop()
            boxes += 1
            t0.value, t1.value = r.tMin, r.tMax
            if not o.o_node_intersect(C.byref(self.nodes[cur]), r.origin, inv, C.byref(t0), C.byref(t1)):
                continue
            if self.geom[cur] == irl.INVALID_GEOM:
                stack.append(self.link[cur])      # the second child
                stack.append(cur + 1)             # the first child is visited first
                continue
            tests += 1
            kind, prim = self.prims[cur]
            if kind == 0:
                if sh is None:
                    sh = ol.Shear()
                    o.o_ray_shear(C.byref(r), C.byref(sh))
                t = F(o.o_intersect_triangle(prim[0], prim[1], prim[2], C.byref(sh), INF, bary))
                crossings += int(t > 0 and t < INF and t > t_min and t < t_max)
            elif kind == 1:
                crossings += sphere_crossings32(prim[0], prim[1], (r.origin.x, r.origin.y, r.origin.z),
                                                (r.direction.x, r.direction.y, r.direction.z), t_min, t_max)
            else:
                t = F(o.o_disc_intersect(C.byref(prim), C.byref(r)))
                crossings += int(t > t_min and t < t_max)
        return crossings, boxes, tests

    def counts(self, rays):
        """(uint32 counts, total box tests, total primitive tests) of a RAY array."""
        out = np.zeros(rays.size, np.uint32)
        boxes = tests = 0
        for i in range(rays.size):
            out[i], b, t = self.count(rays[i])
            boxes += b; tests += t
        return out, boxes, tests

    def inside(self, pos, direction=None):
        """Parity of the count of the rays sign_rays gives for positions [N, 3]: a bool array."""
        return (self.counts(sign_rays(points_of(pos), direction))[0] & 1).astype(bool)


def brute_force_parity(hs, pos, direction=None):
    """Parity of the crossings of every triangle of a mesh-only scene, no BVH: the oracle's triangle test on all of them."""
    o = ol.lib()
    tris = hs.tris.reshape(-1, 3).astype(np.int64)
    vv = [ol.Vec3(float(p["x"]), float(p["y"]), float(p["z"])) for p in hs.verts]
    rays = sign_rays(points_of(pos), direction)
    out = np.zeros(len(pos), bool)
    bary = (C.c_float * 3)()
    for i in range(rays.size):
        r = ol.Ray.from_buffer_copy(rays[i].tobytes())
        sh = ol.Shear()
        o.o_ray_shear(C.byref(r), C.byref(sh))
        k = 0
        for a, b, c in tris:
            t = F(o.o_intersect_triangle(vv[a], vv[b], vv[c], C.byref(sh), INF, bary))
            k += int(t > 0 and t < INF)
        out[i] = bool(k & 1)
    return out


def centre_behind_inside_sphere(hs, rays):
    """Rays that start strictly inside one of the scene's spheres with its centre behind them ((c - o).d < 0), in binary64: the
    one place where a crossing count and the reference's any-hit answer differ by design (its sphere test gives up there)."""
    if not hs.spheres.size:
        return np.zeros(rays.size, bool)
    o = np.stack([rays["origin"][c] for c in "xyz"], 1).astype(np.float64)
    d = np.stack([rays["direction"][c] for c in "xyz"], 1).astype(np.float64)
    out = np.zeros(rays.size, bool)
    for s in hs.spheres:
        f = np.array([s["x"], s["y"], s["z"]], np.float64) - o
        out |= ((f * f).sum(1) < float(s["radius"]) ** 2) & ((f * d).sum(1) < 0)
    return out
