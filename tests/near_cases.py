"""Shared by the neighbour-list tests (test_near_host.py, test_near_abi.py, test_near_gpu.py): the checker - a Python walk of the
compact nodes written from the contract's text (include/mi_raylib.h, the neighbour-list block) with the binary32 restatements of
tests/point_cases.py, one np.float32 operation per operation -, the scenes and point sets, a float64 brute force over every
primitive with the points it leaves a margin for, and the packing of lists into NEIGHBOUR records."""
import numpy as np

import ipu_ray_lib_amd as irl
import point_cases as pc

F = np.float32
INF = F(np.inf)
REL = 1e-5                 # the margin: relative distance of a primitive from the radius, and of the K-th from the (K + 1)-th
KS = (1, 4, 16)
SENTINEL = (F(-7.5), 0xABCD1234, 0x5A5A, 0xA5A5, 0xDEADBEEF)


# ------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------
def key(rec):
    """The order of a list: dist2 as a float, then geomID, then primID. rec = (d2, geomID, primID)."""
    return (float(rec[0]), int(rec[1]), int(rec[2]))


class _LazyLeaves:
    """NearChecker.lazy's `leaf`: a sequence whose entries are made when they are first read."""

    def __init__(self, hs, nodes, verts, leaf_of):
        self.hs, self.nodes, self.verts, self.leaf_of, self.made = hs, nodes, verts, leaf_of, {}

    def __getitem__(self, i):
        if i not in self.made:
            self.made[i] = self.leaf_of(self.hs, self.verts, self.nodes[i])
        return self.made[i]


class NearChecker:
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives)."""

    def __init__(self, hs, nodes=None):
        nodes = hs.nodes if nodes is None else np.asarray(nodes, irl.BVH_NODE)
        self.n = len(nodes)
        self.lo, self.hi, self.skip, self.leaf = [], [], [0] * self.n, []
        verts = self._verts(hs)
        for i in range(self.n):
            nd = nodes[i]
            lo = np.array([nd["min_x"], nd["min_y"], nd["min_z"]], F)
            ext = np.array([nd["dx"], nd["dy"], nd["dz"]], np.uint16).view(np.float16).astype(F)
            self.lo.append(tuple(lo)); self.hi.append(tuple((lo + ext).astype(F)))       # max = min + (float)extent: one rounded add
            self.leaf.append(self._leaf_of(hs, verts, nd))
        for i in range(self.n - 1, -1, -1):              # the node behind a node's subtree
            self.skip[i] = i + 1 if self.leaf[i] is not None else self.skip[int(nodes[i]["link"])]

    @staticmethod
    def _verts(hs):
        return np.stack([hs.verts[c] for c in "xyz"], 1).astype(F) if hs.verts.size else np.zeros((0, 3), F)

    @staticmethod
    def _leaf_of(hs, verts, nd):
        """A node's entry of `leaf`: None for an interior node, else (kind, the primitive's data, geomID, primID)."""
        g = int(nd["geomID"])
        if g == irl.INVALID_GEOM:
            return None
        ref = hs.geometry[g]
        if ref["type"] == 0:
            m = hs.mesh_info[ref["index"]]
            prim = int(nd["link"])
            t = hs.tris[int(m["firstIndex"]) + prim].astype(np.int64) + int(m["firstVertex"])
            return (0, (verts[t[0]], verts[t[1]], verts[t[2]]), g, prim)
        if ref["type"] == 1:
            s = hs.spheres[ref["index"]]
            return (1, ((s["x"], s["y"], s["z"]), s["radius"]), g, 0)
        d = hs.discs[ref["index"]]
        return (2, ((d["nx"], d["ny"], d["nz"]), (d["cx"], d["cy"], d["cz"]), d["r"]), g, 0)

    @classmethod
    def lazy(cls, hs, nodes=None):
        """The same checker for a tree of hundreds of thousands of nodes, made in milliseconds: boxes and skip links by numpy, a
        leaf's entry (_leaf_of, as above) when a walk first reads it."""
        nodes = np.ascontiguousarray(hs.nodes if nodes is None else nodes, irl.BVH_NODE)
        ck = cls.__new__(cls)
        ck.n = len(nodes)
        lo = np.stack([nodes["min_x"], nodes["min_y"], nodes["min_z"]], 1).astype(F)
        ext = np.stack([nodes["dx"], nodes["dy"], nodes["dz"]], 1).astype(np.uint16).view(np.float16).astype(F)
        ck.lo, ck.hi = lo, (lo + ext).astype(F)              # max = min + (float)extent: one rounded add
        link, interior = nodes["link"].tolist(), (nodes["geomID"] == irl.INVALID_GEOM).tolist()
        ck.skip = [0] * ck.n
        for i in range(ck.n - 1, -1, -1):
            ck.skip[i] = ck.skip[link[i]] if interior[i] else i + 1
        ck.leaf = _LazyLeaves(hs, nodes, cls._verts(hs), cls._leaf_of)
        return ck

    def _d2(self, i, p):
        kind, data, _, _ = self.leaf[i]
        if kind == 0:
            q = pc.tri_closest32(*data, p)[0]
        elif kind == 1:
            q = pc.sphere_closest32(data[0], data[1], p)
        else:
            q = pc.disc_closest32(data[0], data[1], data[2], p)
        with np.errstate(all="ignore"):
            return pc.dist2_32(p, q)

    def _walk(self, pt, length):
        """The fill's walk for a segment of `length` records (None: the count walk, nothing kept, the fixed bound alone):
        (the records kept or every neighbour in visit order, box tests, primitive evaluations)."""
        p = (F(pt["x"]), F(pt["y"]), F(pt["z"]))
        radius = F(pt["radius"])
        boxes = prims = 0
        seg = []
        if not (all(np.isfinite(x) for x in p) and radius >= 0):          # a NaN radius fails the compare
            return seg, 0, 0
        with np.errstate(all="ignore"):
            r2 = F(radius * radius)
        i = 0
        while i < self.n:
            boxes += 1
            with np.errstate(all="ignore"):
                db = pc.box_dist2_32(self.lo[i], self.hi[i], p)
            enter = db < r2
            if enter and length is not None and len(seg) == length:
                enter = db <= seg[-1][0]
            if not enter:
                i = self.skip[i]
                continue
            if self.leaf[i] is None:
                i += 1
                continue
            prims += 1
            d2 = self._d2(i, p)
            if d2 < r2:                                                     # strictly; a NaN never
                rec = (d2, self.leaf[i][2], self.leaf[i][3])
                if length is None or len(seg) < length:
                    seg.append(rec)
                elif key(rec) < key(seg[-1]):
                    seg[-1] = rec
                if length is not None:
                    seg.sort(key=key)
            i = self.skip[i]
        return seg, boxes, prims

    def neighbours(self, pt):
        """(every neighbour of the point sorted by the key, box tests, primitive evaluations) of the count walk."""
        found, boxes, prims = self._walk(pt, None)
        return sorted(found, key=key), boxes, prims

    def fill(self, pt, length):
        """(the records the fill keeps in a segment of `length`, box tests, primitive evaluations); nothing is walked for 0."""
        if length == 0:
            return [], 0, 0
        return self._walk(pt, length)


def records(found, point, length=None):
    """`found` [(d2, geomID, primID)] as NEIGHBOUR records of point `point`, cut or padded to `length`."""
    length = len(found) if length is None else length
    out = np.zeros(length, irl.NEIGHBOUR)
    out["dist2"], out["primID"], out["geomID"], out["flags"], out["point"] = INF, irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, point
    for j, (d2, g, q) in enumerate(found[:length]):
        out[j] = (d2, q, g, 0, point)
    return out


def packed(lists):
    """(offsets, recs) of per-point lists."""
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    recs = np.concatenate([records(x, i) for i, x in enumerate(lists)]) if lists else np.zeros(0, irl.NEIGHBOUR)
    return offsets, recs.astype(irl.NEIGHBOUR)


def split(offsets, recs):
    """Per-point [(d2, geomID, primID)] lists of an (offsets, recs) pair."""
    return [[(r["dist2"], int(r["geomID"]), int(r["primID"])) for r in recs[int(offsets[i]):int(offsets[i + 1])]]
            for i in range(len(offsets) - 1)]


def sentinel_buffer(n_records):
    """A 16-byte aligned NEIGHBOUR array of `n_records` + 64 records, every one the sentinel."""
    buf = irl.aligned_bytes((n_records + 64) * irl.NEIGHBOUR.itemsize).view(irl.NEIGHBOUR)
    buf[:] = SENTINEL
    return buf


def k_offsets(n, k):
    return (np.arange(n + 1, dtype=np.uint64) * np.uint64(k)).astype(np.uint64)


def assert_same(got, want, what):
    """(offsets, recs) pairs, exactly."""
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at points {np.nonzero(np.asarray(got[0][1:]) != np.asarray(want[0][1:]))[0][:4]}"
    pc.assert_bytes_equal(np.ascontiguousarray(got[1]).reshape(-1), np.ascontiguousarray(want[1]).reshape(-1), what)


# ------------------------------------------------------------------------------------------------------
# scenes and point sets
# ------------------------------------------------------------------------------------------------------
TRI = ((1.0, 1.0, 0.0), (5.0, 1.5, 0.25), (2.0, 4.0, -0.5))
DOT = (2.0, -1.0, 0.5)
TIES_QUERY = (0.0, 0.0, 10.0)


def ties_scene():
    """Geometries 0, 1: two coincident triangles; 2: a triangle collapsed to a point; 3, 4: two unit spheres whose shells lie exactly
    3 away from TIES_QUERY (centres 4 away along -x and +x: every step of the sphere formula is exact, dist2 = 9 for both)."""
    return pc.hand_scene(tris=[TRI, TRI, (DOT, DOT, DOT)], spheres=[(-4.0, 0.0, 10.0, 1.0), (4.0, 0.0, 10.0, 1.0)])


def empty_desc():
    return irl.SceneDesc()


_scenes, _cases, _twins, _margins = {}, {}, {}, {}


def scene(name):
    if name not in _scenes:
        if name == "ties":
            _scenes[name] = ties_scene()
        elif name == "one":
            _scenes[name] = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 1.0)])
        else:
            _scenes[name] = pc.scene(name)
    return _scenes[name]


def points_of(name):
    """The POINT array of a case. soup: 400 mixed points - inside the root box, far outside, exactly on vertices and centres - with
    radii from none to dozens of neighbours (the soup's triangles are about 3 across, 600 of them in a cube of 20); a few queries
    that are not walked."""
    hs = scene(name)
    if name == "soup":
        pts = pc.mixed_points(hs, 400, seed=41)
        rng = np.random.default_rng(42)
        pts["radius"] = rng.choice(np.array([0.0, 1.0, 2.5, 5.0], F), pts.size, p=[0.05, 0.25, 0.35, 0.35])
        pts["x"][7] = np.nan; pts["z"][8] = np.inf; pts["radius"][9] = np.nan; pts["radius"][10] = -1.0
        return pts
    if name == "box":
        pts = pc.mixed_points(hs, 300, seed=43)
        lo, hi = pc.root_box(hs.nodes)
        diag = F(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(44)
        pts["radius"] = (rng.choice(np.array([0.0, 0.005, 0.015, 0.03], F), pts.size) * diag).astype(F)
        return pts
    if name == "ties":
        return pc.points([TIES_QUERY + (np.inf,), TIES_QUERY + (3.0,), TIES_QUERY + (np.nextafter(F(3), F(4)),), DOT + (np.inf,)])
    if name == "one":
        return pc.points([(0.0, 5.0, 0.0, np.inf), (0.0, 5.0, 0.0, 4.0), (0.0, 5.0, 0.0, 4.5), (0.25, 0.0, 0.0, 1.0), (np.nan, 0.0, 0.0, 1.0)])
    raise KeyError(name)


CASES = ("soup", "box", "ties", "one")


def case(name):
    """(scene, points, the checker's sorted lists, its box tests and primitive evaluations of the count walk per point), computed
    once."""
    if name not in _cases:
        hs, pts = scene(name), points_of(name)
        ck = NearChecker(hs)
        res = [ck.neighbours(pt) for pt in pts]
        _cases[name] = (hs, pts, [r[0] for r in res], np.array([r[1] for r in res], np.int64), np.array([r[2] for r in res], np.int64))
    return _cases[name]


def twin(name):
    """(scene, points, the twin's offsets, its records, the visits of its two steps), computed once: what the device must equal."""
    if name not in _twins:
        hs, pts = scene(name), points_of(name)
        offsets, vo = irl.near_offsets_host(hs.desc, pts)
        recs, vf = irl.near_fill_host(hs.desc, pts, offsets)
        _twins[name] = (hs, pts, offsets, recs, vo, vf)
    return _twins[name]


def twin_k(name, k, radius=None):
    """(the twin's [n, k] K-nearest records, its visits) of a case's points (radius: overrides the points' own), computed once."""
    tag = (name, k, radius)
    if tag not in _twins:
        hs, pts = scene(name), points_of(name).copy()
        if radius is not None:
            pts["radius"] = radius
        recs, v = irl.near_fill_host(hs.desc, pts, k_offsets(pts.size, k), capacity=pts.size * k)
        _twins[tag] = (recs.reshape(pts.size, k), v)
    return _twins[tag]


# ------------------------------------------------------------------------------------------------------
# float64 brute force and the points with margin
# ------------------------------------------------------------------------------------------------------
def all_dist64(hs, pos):
    """(D [N, P], geom [P], prim [P]): the distance in binary64 of every point from EVERY primitive of the scene."""
    pr = pc.primitives(hs)
    P = np.asarray(pos, np.float64)
    cols, geom, prim = [], [], []
    A, B, Cc, tg, tp = pr["tri"]
    if len(A):
        cols.append(pc.tri_dist64(P[:, None, :], A[None], B[None], Cc[None])); geom.append(tg); prim.append(tp)
    c, r, g = pr["sphere"]
    if len(c):
        cols.append(np.abs(np.sqrt(((P[:, None, :] - c[None]) ** 2).sum(-1)) - r[None])); geom.append(g); prim.append(np.zeros(len(g), np.int64))
    n, c, r, g = pr["disc"]
    if len(c):
        nh = n / np.linalg.norm(n, axis=1, keepdims=True)
        v = P[:, None, :] - c[None]
        h = (v * nh[None]).sum(-1)
        u = np.sqrt(np.maximum(((v - nh[None] * h[..., None]) ** 2).sum(-1), 0.0))
        cols.append(np.where(u <= r[None], np.abs(h), np.sqrt(h * h + (u - r[None]) ** 2))); geom.append(g); prim.append(np.zeros(len(g), np.int64))
    return np.concatenate(cols, 1), np.concatenate(geom), np.concatenate(prim)


def soup_margin():
    """(D, geom, prim, margin [N] bool) for the soup's points: margin marks the valid queries for which no primitive's distance lies
    within REL relative of the radius and, for each K of KS, the K-th and (K + 1)-th nearest distances differ by more than REL
    relative. The soup shares no edges, so near-ties are accidents there: at least 95 % of the points have margin."""
    if "soup" not in _margins:
        hs, pts = scene("soup"), points_of("soup")
        pos = np.stack([pts[c] for c in "xyz"], 1).astype(np.float64)
        valid = np.isfinite(pos).all(1) & (pts["radius"] >= 0)
        D, geom, prim = all_dist64(hs, np.where(valid[:, None], pos, 0.0))
        r = pts["radius"].astype(np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            ok = valid & ~(np.abs(D - r) <= REL * r).any(1)
        S = np.sort(D, 1)
        for k in KS:
            ok &= (S[:, k] - S[:, k - 1]) > REL * S[:, k]
        assert ok.mean() >= 0.95, f"only {ok.mean():.3f} of the soup's points have margin: change the seed"
        _margins["soup"] = (D, geom, prim, ok)
    return _margins["soup"]
