"""Shared by the triangle-query tests (test_tri_host.py, test_tri_abi.py, test_tri_gpu.py): the checker - a Python walk of the
compact nodes written from the contract's text (include/mi_raylib.h, the triangle-query block), one np.float32 operation per
operation -, the scenes and query sets, the float64 references (segment against triangle, the 17-axis signed separation, the
sphere's distance bounds, an exact disc test) and the packing of lists into CONTACT records."""
import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import near_cases as nc
import point_cases as pc

F = np.float32
SENTINEL = (0xABCD1234, 0x5A5A, 0xA5A5, 0xDEADBEEF, 0x0BADF00D)
ANY, COUNT = irl.TRI_ANY, irl.TRI_COUNT
AXES = ["nQ", "nT"] + [f"e{i} x f{j}" for i in range(3) for j in range(3)] + [f"nT x e{i}" for i in range(3)] + [f"nQ x f{j}" for j in range(3)]


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32
# ------------------------------------------------------------------------------------------------------
def cross32(a, v):
    return np.array([F(F(a[1] * v[2]) - F(a[2] * v[1])), F(F(a[2] * v[0]) - F(a[0] * v[2])), F(F(a[0] * v[1]) - F(a[1] * v[0]))], F)


def _meet(mn, mx, qmn, qmx):
    return bool((mn <= qmx).all() and (mx >= qmn).all())


def query_bounds(q):
    q = np.asarray(q, F)
    return q.min(0), q.max(0)


def sat_axes32(a, b, c, q):
    """(the 17 axes in the contract's order, the moved vertices u [3, 3], the query's v [3, 3]), binary32."""
    q0, q1, q2 = (pc._v(x) for x in q)
    u = [pc._v(a) - q0, pc._v(b) - q0, pc._v(c) - q0]
    v = [np.zeros(3, F), q1 - q0, q2 - q0]
    e = [u[1] - u[0], u[2] - u[1], u[0] - u[2]]
    f = [v[1], v[2] - v[1], -v[2]]
    nT, nQ = cross32(e[0], e[1]), cross32(f[0], f[1])
    axes = [nQ, nT] + [cross32(e[i], f[j]) for i in range(3) for j in range(3)] + [cross32(nT, e[i]) for i in range(3)] + [cross32(nQ, f[j]) for j in range(3)]
    return axes, u, v


def separators32(a, b, c, q):
    """The indices of the axes that separate, in binary32 as the contract evaluates them (every axis: no early exit)."""
    with np.errstate(all="ignore"):
        axes, u, v = sat_axes32(a, b, c, q)
        out = []
        for k, x in enumerate(axes):
            pT = [pc.dot32(x, w) for w in u]
            pQ = [F(0), pc.dot32(x, v[1]), pc.dot32(x, v[2])]
            if all(t > s for t in pT for s in pQ) or all(t < s for t in pT for s in pQ):
                out.append(k)
        return out


def tri_touch32(a, b, c, q):
    V = np.array([a, b, c], F)
    qmn, qmx = query_bounds(q)
    if not _meet(V.min(0), V.max(0), qmn, qmx):
        return False
    return not separators32(a, b, c, q)


def tri_dist2_32(q, p):
    with np.errstate(all="ignore"):
        return pc.dist2_32(p, pc.tri_closest32(q[0], q[1], q[2], p)[0])


def sphere_touch32(c, radius, q):
    c, radius = pc._v(c), F(radius)
    qmn, qmx = query_bounds(q)
    with np.errstate(all="ignore"):
        r2 = F(radius * radius)
        if not _meet(c - radius, c + radius, qmn, qmx):
            return False
        dmin2 = tri_dist2_32(q, c)
        d = [pc.dist2_32(pc._v(x), c) for x in q]
        m = d[0] if d[0] > d[1] else d[1]
        dmax2 = m if m > d[2] else d[2]
        return bool((not dmin2 > r2) and (not dmax2 < r2))


def disc_touch32(n, c, r, q):
    n, c = pc._v(n), pc._v(c)
    qmn, qmx = query_bounds(q)
    with np.errstate(all="ignore"):
        r2 = F(F(r) * F(r))
        rr = np.sqrt(r2)
        nn = pc.dot32(n, n)
        t = F(1) - n * n / nn
        t = np.where(t > 0, t, F(0)).astype(F)
        ext = rr * np.sqrt(t)
        if not _meet(c - ext, c + ext, qmn, qmx):
            return False
        s = [pc.dot32(n, pc._v(x) - c) for x in q]
        if all(x > 0 for x in s) or all(x < 0 for x in s):
            return False
        return bool(not tri_dist2_32(q, c) > r2)


def corners(tri):
    """The three corners of one TRI record as a [3, 3] binary32 array."""
    return np.array([tri["a"], tri["b"], tri["c"]], F)


class TriChecker(nc.NearChecker):
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives): NearChecker's table
    of boxes, skip links and leaf primitives, walked with a triangle."""

    def _touch(self, i, q):
        kind, data, _, _ = self.leaf[i]
        if kind == 0:
            return tri_touch32(*data, q)
        if kind == 1:
            return sphere_touch32(data[0], data[1], q)
        return disc_touch32(data[0], data[1], data[2], q)

    def walk(self, tri, first_only=False):
        """(the touching primitives [(geomID, primID)] in visit order, box tests, primitive tests)."""
        q = corners(tri)
        found, boxes, prims = [], 0, 0
        if not np.isfinite(q).all():
            return found, 0, 0
        qmn, qmx = query_bounds(q)
        i = 0
        while i < self.n:
            boxes += 1
            if not _meet(np.array(self.lo[i], F), np.array(self.hi[i], F), qmn, qmx):
                i = self.skip[i]
                continue
            if self.leaf[i] is None:
                i += 1
                continue
            prims += 1
            if self._touch(i, q):
                found.append((self.leaf[i][2], self.leaf[i][3]))
                if first_only:
                    break
            i = self.skip[i]
        return found, boxes, prims

    def contacts(self, tri):
        """(every touching primitive sorted by (geomID, primID), box tests, primitive tests)."""
        found, boxes, prims = self.walk(tri)
        return sorted(found), boxes, prims


# ------------------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------------------
def tris(rows):
    """A TRI array from rows (q0, q1, q2)."""
    return qb.make_tris(*(np.array([r[k] for r in rows], F).reshape(-1, 3) for k in range(3)))


def records(found, tri, length=None):
    """`found` [(geomID, primID)] as CONTACT records of query `tri`, cut or padded to `length`."""
    length = len(found) if length is None else length
    out = np.zeros(length, irl.CONTACT)
    out["primID"], out["geomID"], out["flags"], out["tri"] = irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, tri
    for j, (g, p) in enumerate(found[:length]):
        out[j] = (p, g, 0, tri, 0)
    return out


def packed(lists):
    """(offsets, recs) of per-query sorted lists."""
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    recs = np.concatenate([records(x, i) for i, x in enumerate(lists)]) if lists else np.zeros(0, irl.CONTACT)
    return offsets, recs.astype(irl.CONTACT)


def ids(recs):
    """The (geomID, primID) pairs of records, as a set."""
    return {(int(r["geomID"]), int(r["primID"])) for r in recs}


def sentinel_buffer(n_records):
    """A 16-byte aligned CONTACT array of `n_records` + 64 records, every one the sentinel."""
    buf = irl.aligned_bytes((n_records + 64) * irl.CONTACT.itemsize).view(irl.CONTACT)
    buf[:] = SENTINEL
    return buf


def is_sentinel(recs):
    want = np.zeros((), irl.CONTACT)
    want[()] = SENTINEL
    return (np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1) == want.reshape(1).view(np.uint8)).all(1)


k_offsets = nc.k_offsets


def assert_same(got, want, what):
    """(offsets, recs) pairs, exactly."""
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at triangles {np.nonzero(np.asarray(got[0][1:]) != np.asarray(want[0][1:]))[0][:4]}"
    pc.assert_bytes_equal(np.ascontiguousarray(got[1]).reshape(-1), np.ascontiguousarray(want[1]).reshape(-1), what)


# ------------------------------------------------------------------------------------------------------
# scenes and query sets
# ------------------------------------------------------------------------------------------------------
_scenes, _twins = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = pc.scene(name)
    return _scenes[name]


def scene_tris32(hs):
    """The scene's own triangles as a [T, 3, 3] binary32 array, geometry by geometry."""
    A, B, Cc, _, _ = pc.primitives(hs)["tri"]
    return np.stack([A, B, Cc], 1).astype(F)


def tris_of(name, n=None):
    """The TRI array of a case: 150 queries (or n) - centred inside the root box, far outside, exactly on vertices and centres -
    whose edges run from a twentieth of the scene to most of it, so that they touch none, a few and dozens of primitives. From
    index 7 on: a NaN, an infinity, a segment, a point, a query whose products overflow, one spanning the scene, then eight of the
    scene's own triangles (exact contact with themselves and their neighbours), one of them in another vertex order."""
    hs = scene(name)
    seed = {"soup": 61, "box": 63, "spheres": 65}[name]
    count = 150 if n is None else n
    pts = pc.mixed_points(hs, count, seed=seed)
    centre = np.stack([pts[c] for c in "xyz"], 1).astype(F)
    lo, hi = pc.root_box(hs.nodes)
    size = float((hi - lo).max())
    rng = np.random.default_rng(seed + 1)
    steps = np.array([0.05, 0.15, 0.4, 0.8], F)
    scale = (rng.choice(steps, (count, 1, 1), p=[0.25, 0.35, 0.25, 0.15]) * F(size)).astype(F)
    q = (centre[:, None, :] + scale * rng.uniform(-0.5, 0.5, (count, 3, 3)).astype(F)).astype(F)
    if count > 24:
        q[7, 1, 0] = np.nan
        q[8, 2, 2] = np.inf
        q[9, 2] = q[9, 1]                                            # a segment
        q[10, 1] = q[10, 2] = q[10, 0]                              # a point
        q[11] = np.array([[-1e30, -1e30, -1e30], [1e30, 1e30, -1e30], [0, 1e30, 1e30]], F)      # products overflow: errs towards listing
        q[12] = np.array([lo, [hi[0], lo[1], hi[2]], hi], F)         # spans the scene
        own = scene_tris32(hs)
        if len(own):                                                 # (the spheres scene has no triangle)
            q[13:21] = own[rng.integers(0, len(own), 8)]
            q[20] = q[20][[2, 0, 1]]
    return qb.make_tris(q[:, 0], q[:, 1], q[:, 2])


def twin(name, n=None):
    """(scene, queries, the twin's offsets, its records, its counts, its any bytes, the visits of the four), computed once: what the
    device must equal."""
    tag = (name, n)
    if tag not in _twins:
        hs, tq = scene(name), tris_of(name, n)
        offsets, vo = irl.tri_offsets_host(hs.desc, tq)
        recs, vf = irl.tri_fill_host(hs.desc, tq, offsets)
        counts, vc = irl.tri_query_host(hs.desc, COUNT, tq)
        anys, va = irl.tri_query_host(hs.desc, ANY, tq)
        _twins[tag] = (hs, tq, offsets, recs, counts, anys, {"offsets": vo, "fill": vf, "count": vc, "any": va})
    return _twins[tag]


def listed(offsets, recs, n_queries):
    """{(query, geomID, primID)} of a packed list."""
    which = np.repeat(np.arange(n_queries), np.diff(offsets).astype(np.int64))
    return {(int(i), int(r["geomID"]), int(r["primID"])) for i, r in zip(which, recs)}


# ------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------
def _cross64(a, b):
    return np.cross(a, b)


def _segment_hits_triangle64(p, q, a, b, c):
    """[...] bool: the closed segment p q crosses the closed triangle a b c (all [..., 3], binary64). A segment parallel to the
    triangle's plane - in it or beside it - crosses nothing here: such pairs are decided by the other triangle's edges or are not
    clear."""
    n = _cross64(b - a, c - a)
    dp, dq = ((p - a) * n).sum(-1), ((q - a) * n).sum(-1)
    cuts = (dp * dq <= 0) & (dp != dq)
    t = np.where(cuts, dp / np.where(cuts, dp - dq, 1.0), 0.0)
    x = p + (q - p) * t[..., None]
    inside = ((_cross64(b - a, x - a) * n).sum(-1) >= 0) & ((_cross64(c - b, x - b) * n).sum(-1) >= 0) & ((_cross64(a - c, x - c) * n).sum(-1) >= 0)
    return cuts & inside


def tri_touch64(Q, T):
    """[N, M] bool: query triangles Q [N, 3, 3] against scene triangles T [M, 3, 3] in binary64, by the six segment-triangle tests:
    an edge of one crosses the other's closed triangle."""
    Q = np.asarray(Q, np.float64)[:, None]
    T = np.asarray(T, np.float64)[None]
    hit = np.zeros((Q.shape[0], T.shape[1]), bool)
    for k in range(3):
        hit |= _segment_hits_triangle64(Q[:, :, k], Q[:, :, (k + 1) % 3], T[:, :, 0], T[:, :, 1], T[:, :, 2])
        hit |= _segment_hits_triangle64(T[:, :, k], T[:, :, (k + 1) % 3], Q[:, :, 0], Q[:, :, 1], Q[:, :, 2])
    return hit


def tri_gap64(Q, T):
    """[N, M]: the signed separation s of every pair in binary64 - the maximum over the 17 normalised axes of the gap between the
    two triangles' projections (> 0 apart by at least that much, < 0 overlapping on every axis by that much); axes shorter than
    1e-12 are skipped."""
    Q = np.asarray(Q, np.float64)[:, None]
    T = np.asarray(T, np.float64)[None]
    q0 = Q[:, :, 0]
    u = [T[:, :, k] - q0 for k in range(3)]
    v = [Q[:, :, k] - q0 for k in range(3)]
    e = [u[1] - u[0], u[2] - u[1], u[0] - u[2]]
    f = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    shape = np.broadcast_shapes(u[0].shape, v[1].shape)
    e = [np.broadcast_to(x, shape) for x in e]
    f = [np.broadcast_to(x, shape) for x in f]
    nT, nQ = np.cross(e[0], e[1]), np.cross(f[0], f[1])
    axes = [nQ, nT] + [np.cross(e[i], f[j]) for i in range(3) for j in range(3)] + [np.cross(nT, e[i]) for i in range(3)] + [np.cross(nQ, f[j]) for j in range(3)]
    gap = np.full(shape[:2], -np.inf)
    for x in axes:
        ln = np.linalg.norm(x, axis=-1)
        ok = ln > 1e-12
        x = x / np.where(ok, ln, 1.0)[..., None]
        pT = np.stack([(x * w).sum(-1) for w in u], 0)
        pQ = np.stack([(x * w).sum(-1) for w in v], 0)
        g = np.maximum(pT.min(0) - pQ.max(0), pQ.min(0) - pT.max(0))
        gap = np.maximum(gap, np.where(ok, g, -np.inf))
    return gap


def pair_scale(Q, T):
    """[N, M]: L, the largest coordinate magnitude in each pair."""
    return np.maximum(np.abs(np.asarray(Q, np.float64)).max((1, 2))[:, None], np.abs(np.asarray(T, np.float64)).max((1, 2))[None])


def bounds_meet64(Q, T):
    Q, T = np.asarray(Q, np.float64), np.asarray(T, np.float64)
    return ((T.min(1)[None] <= Q.max(1)[:, None]) & (T.max(1)[None] >= Q.min(1)[:, None])).all(-1)


def tri_point_dist64(q, p):
    """The distance of p from the triangle q [3, 3], binary64."""
    return float(pc.tri_dist64(np.asarray(p, np.float64), *(np.asarray(x, np.float64) for x in q)))


def sphere_gap64(q, c, r):
    """max(dmin - r, r - dmax) of one query triangle and one sphere: > 0 the triangle misses the shell by that much (outside or
    inside), < 0 it crosses it."""
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    dmax = float(np.linalg.norm(q - c, axis=1).max())
    return max(tri_point_dist64(q, c) - r, r - dmax)


def disc_gap64(q, n, c, r):
    """One query triangle against one disc, exactly: the triangle clipped with the disc's plane is a segment (or a point, or - for a
    triangle in the plane - the triangle); the disc touches when that comes within r of the centre. Returns the distance of the
    clip from c minus r; +inf when the plane misses the triangle."""
    q, n, c = (np.asarray(x, np.float64) for x in (q, n, c))
    n = n / np.linalg.norm(n)
    d = (q - c) @ n
    if d.min() > 0 or d.max() < 0:
        return np.inf
    if (d == 0).all():
        return tri_point_dist64(q, c) - r
    pts = [q[k] for k in range(3) if d[k] == 0]
    for k in range(3):
        a, b = k, (k + 1) % 3
        if d[a] * d[b] < 0:
            pts.append(q[a] + (q[b] - q[a]) * (d[a] / (d[a] - d[b])))
    best = min(float(np.linalg.norm(x - c)) for x in pts)
    for i in range(len(pts)):
        for j in range(i + 1, len(pts)):
            best = min(best, pc._seg_dist(c, pts[i], pts[j]))
    return best - r
