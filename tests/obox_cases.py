"""Shared by the oriented-box-query tests (test_obox_host.py, test_obox_gpu.py): the checker - a Python walk of the compact nodes
written from the contract's text (include/mi_raylib.h, the oriented-box block), one np.float32 operation per operation, with the
box family's primitive tests of box_cases.py for the step in the box's frame -, the scenes and query sets, the 24 exact rotations,
and a float64 reference that shares no code with the library: its own rotation matrix, the triangle clipped against the box's six
planes, the sphere from the closest and the farthest point of the box."""
import itertools

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import near_cases as nc
import point_cases as pc
import box_cases as bc

F = np.float32
ANY, COUNT = irl.OBOX_ANY, irl.OBOX_COUNT
records, packed, ids, sentinel_buffer, is_sentinel, k_offsets, assert_same = (bc.records, bc.packed, bc.ids, bc.sentinel_buffer,
                                                                                bc.is_sentinel, bc.k_offsets, bc.assert_same)


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32
# ------------------------------------------------------------------------------------------------------
class Query32:
    """One query as the contract derives it: valid, centre c, half h, the frame U, V, W and the world bounds qmn, qmx."""

    def __init__(self, obox):
        with np.errstate(all="ignore"):
            c, h, q = np.asarray(obox["centre"], F), np.asarray(obox["half"], F), np.asarray(obox["quat"], F)
            x, y, z, w = q
            qq = F(F(F(F(x * x) + F(y * y)) + F(z * z)) + F(w * w))
            s = F(F(2) / qq)
            self.valid = bool(np.isfinite(c).all() and np.isfinite(h).all() and np.isfinite(q).all() and (h >= 0).all() and qq > 0 and np.isfinite(s))
            xs, ys, zs = F(x * s), F(y * s), F(z * s)
            wx, wy, wz = F(w * xs), F(w * ys), F(w * zs)
            xx, xy, xz, yy, yz, zz = F(x * xs), F(x * ys), F(x * zs), F(y * ys), F(y * zs), F(z * zs)
            one = F(1)
            self.c, self.h = c, h
            self.U = np.array([F(one - F(yy + zz)), F(xy + wz), F(xz - wy)], F)
            self.V = np.array([F(xy - wz), F(one - F(xx + zz)), F(yz + wx)], F)
            self.W = np.array([F(xz + wy), F(yz - wx), F(one - F(xx + yy))], F)
            aU, aV, aW = np.abs(self.U), np.abs(self.V), np.abs(self.W)
            ext = np.array([F(F(F(aU[k] * h[0]) + F(aV[k] * h[1])) + F(aW[k] * h[2])) for k in range(3)], F)
            self.qmn, self.qmx = (c - ext).astype(F), (c + ext).astype(F)

    def meets(self, mn, mx):
        """obox_meets_bounds."""
        mn, mx = np.asarray(mn, F), np.asarray(mx, F)
        with np.errstate(all="ignore"):
            if not ((mn <= self.qmx).all() and (mx >= self.qmn).all()):
                return False
            dl, dh = (mn - self.c).astype(F), (mx - self.c).astype(F)
            for A, hA in ((self.U, self.h[0]), (self.V, self.h[1]), (self.W, self.h[2])):
                t = [F(A[k] * dh[k]) if A[k] > 0 else F(A[k] * dl[k]) for k in range(3)]
                u = [F(A[k] * dl[k]) if A[k] > 0 else F(A[k] * dh[k]) for k in range(3)]
                up, dn = F(F(t[0] + t[1]) + t[2]), F(F(u[0] + u[1]) + u[2])
                if dn > hA or up < -hA:
                    return False
            return True

    def local_dir(self, d):
        d = np.asarray(d, F)
        with np.errstate(all="ignore"):
            return np.array([pc.dot32(self.U, d), pc.dot32(self.V, d), pc.dot32(self.W, d)], F)

    def local_point(self, p):
        with np.errstate(all="ignore"):
            return self.local_dir((np.asarray(p, F) - self.c).astype(F))

    def touches(self, kind, data):
        """(touching, contained) of a leaf's primitive (NearChecker's leaf entry): the bounds, then box_cases' tests in the frame."""
        lo, hi = (-self.h).astype(F), self.h
        with np.errstate(all="ignore"):
            if kind == 0:
                V = np.array(data, F)
                if not self.meets(V.min(0), V.max(0)):
                    return False, False
                return bc.tri_touch32(*(self.local_point(v) for v in V), lo, hi)
            if kind == 1:
                c, radius = pc._v(data[0]), F(data[1])
                if not self.meets(c - radius, c + radius):
                    return False, False
                return bc.sphere_touch32(self.local_point(c), radius, lo, hi)
            n, c, r = pc._v(data[0]), pc._v(data[1]), F(data[2])
            r2 = F(r * r)
            t = F(1) - n * n / pc.dot32(n, n)
            ext = np.sqrt(r2) * np.sqrt(np.where(t > 0, t, F(0)).astype(F))
            if not self.meets(c - ext, c + ext):
                return False, False
            return bc.disc_touch32(self.local_dir(n), self.local_point(c), r, lo, hi)


class OBoxChecker(nc.NearChecker):
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives)."""

    def walk(self, obox, first_only=False):
        """(the touching primitives [(geomID, primID, contained)] in visit order, box tests, primitive tests)."""
        q = Query32(obox)
        found, boxes, prims = [], 0, 0
        if not q.valid:
            return found, 0, 0
        i = 0
        while i < self.n:
            boxes += 1
            if not q.meets(self.lo[i], self.hi[i]):
                i = self.skip[i]
                continue
            if self.leaf[i] is None:
                i += 1
                continue
            prims += 1
            kind, data, g, p = self.leaf[i]
            touch, contained = q.touches(kind, data)
            if touch:
                found.append((g, p, contained))
                if first_only:
                    break
            i = self.skip[i]
        return found, boxes, prims

    def overlaps(self, obox):
        found, boxes, prims = self.walk(obox)
        return sorted(found), boxes, prims


# ------------------------------------------------------------------------------------------------------
# records and query sets
# ------------------------------------------------------------------------------------------------------
def oboxes(rows):
    """An OBOX array from rows (centre, half, quat)."""
    rows = list(rows)
    return qb.make_oboxes(np.array([r[0] for r in rows], F).reshape(-1, 3), np.array([r[1] for r in rows], F).reshape(-1, 3),
                          quat=np.array([r[2] for r in rows], F).reshape(-1, 4))


def random_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


SPECIAL = 14      # the number of hand-placed queries at the end of a set


def oboxes_of(name, n=150):
    """The OBOX array of a case: uniform orientations, centres in the root box, the longest half extent from a thousandth of the
    root box to the whole of it, aspects 1:1:1 to 1:1:16 with the long axis anywhere; from index n - SPECIAL on: a NaN, an infinity,
    a negative half extent, a zero quaternion, a quaternion of norm 1e-20 (s overflows), one of norm 1e3, a flat box, a segment, a
    point, a box spanning the scene, a -0 half extent, an infinite quaternion component, and two long thin diagonals."""
    hs = bc.scene(name)
    seed = {"soup": 61, "box": 63, "spheres": 65}[name]
    rng = np.random.default_rng(seed)
    lo, hi = pc.root_box(hs.nodes)
    size = float((hi - lo).max())
    centre = rng.uniform(lo, hi, (n, 3)).astype(F)
    longest = (0.5 * size * 10.0 ** (-3.0 * rng.uniform(0.0, 1.0, n) ** 3)).astype(F)      # (most of them large enough to list something)
    aspect = rng.choice(np.array([1, 2, 4, 16], F), n)
    half = np.repeat((longest / aspect)[:, None], 3, 1).astype(F)
    half[np.arange(n), rng.integers(0, 3, n)] = longest
    half = (half * rng.uniform(0.7, 1.0, (n, 3))).astype(F)
    b = qb.make_oboxes(centre, half, quat=random_quats(rng, n))
    k = n - SPECIAL
    mid = ((lo + hi) * F(0.5)).astype(F)
    if k >= 0:
        b["half"][k:] = F(0.2 * size) * np.array([1.0, 0.5, 0.25], F)
        b["centre"][k:] = mid + rng.uniform(-0.2 * size, 0.2 * size, (SPECIAL, 3)).astype(F)
        b["centre"][k, 1] = np.nan
        b["half"][k + 1, 2] = np.inf
        b["half"][k + 2, 0] = -1e-3
        b["quat"][k + 3] = 0
        b["quat"][k + 4] = b["quat"][k + 4] * F(1e-20)
        b["quat"][k + 5] = b["quat"][k + 5] * F(1e3)
        b["half"][k + 6, 2] = 0                                 # flat
        b["half"][k + 7, 1:] = 0                                # a segment
        b["half"][k + 8] = 0                                    # a point
        b["centre"][k + 9], b["half"][k + 9] = mid, F(2 * size)      # spans the scene
        b["half"][k + 10, 1] = -0.0
        b["quat"][k + 11, 3] = np.inf
        b["half"][k + 12] = F(size) * np.array([0.6, 0.01, 0.01], F)
        b["half"][k + 13] = F(size) * np.array([0.02, 0.7, 0.02], F)
    return b


_twins = {}


def twin(name, n=150):
    """(scene, oboxes, the twin's offsets, its records, its counts, its any bytes, the visits of the four), computed once: what the
    device must equal."""
    tag = (name, n)
    if tag not in _twins:
        hs, bx = bc.scene(name), oboxes_of(name, n)
        offsets, vo = irl.obox_offsets_host(hs.desc, bx)
        recs, vf = irl.obox_fill_host(hs.desc, bx, offsets)
        counts, vc = irl.obox_query_host(hs.desc, COUNT, bx)
        anys, va = irl.obox_query_host(hs.desc, ANY, bx)
        _twins[tag] = (hs, bx, offsets, recs, counts, anys, {"offsets": vo, "fill": vf, "count": vc, "any": va})
    return _twins[tag]


def full(desc, bx):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.obox_offsets_host(desc, bx)
    recs, _ = irl.obox_fill_host(desc, bx, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


# ------------------------------------------------------------------------------------------------------
# the 24 rotations of the cube: quaternions with components in {0, +-1}
# ------------------------------------------------------------------------------------------------------
def matrix64(q):
    """The rotation matrix of a quaternion (x, y, z, w) in binary64, columns = the box's axes: the textbook formula on the
    normalised quaternion (not the contract's)."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def cube_rotations():
    """[(quaternion, |R| as an integer matrix)] of the 24 rotations: one, two or four components +-1, q and -q counted once."""
    out, seen = [], set()
    for q in itertools.product((0, 1, -1), repeat=4):
        if sum(abs(v) for v in q) not in (1, 2, 4):
            continue
        R = np.rint(matrix64(q)).astype(np.int64)
        key = R.tobytes()
        if key in seen:
            continue
        seen.add(key)
        assert np.array_equal(R @ R.T, np.eye(3, dtype=np.int64)) and round(np.linalg.det(R)) == 1
        out.append((q, np.abs(R)))
    assert len(out) == 24
    return out


def dyadic_scene():
    """A hand scene on small numbers whose every product in the tests is exact: 40 triangles with integer vertices in [-8, 8], two
    spheres and two discs with integer centres, radii and normals."""
    rng = np.random.default_rng(71)
    base = rng.integers(-7, 6, (40, 1, 3))
    tris = [tuple(tuple(float(v) for v in p) for p in t) for t in (base + rng.integers(-1, 3, (40, 3, 3)))]
    spheres = [(2.0, -3.0, 1.0, 2.0), (-4.0, 4.0, -2.0, 1.0)]
    discs = [(0.0, 0.0, 1.0, 2.0, 3.0, 3.0, -1.0), (1.0, 0.0, 0.0, 1.0, -2.0, -5.0, 2.0)]
    return pc.hand_scene(tris=tris, spheres=spheres, discs=discs)


# ------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------
def clip_nonempty64(P, h):
    """Whether the polygon P [k, 3] (local coordinates, binary64) clipped against the six planes |x_a| <= h_a keeps a point:
    Sutherland-Hodgman, closed. A point counts as inside a plane within 1e-10 of the pair's size - binary64's own rounding of the
    cut points, which a box of zero thickness would otherwise lose; the bound the twin is held to is ten thousand times that."""
    pts = [np.asarray(p, np.float64) for p in P]
    tol = 1e-10 * (float(np.abs(h).max()) + max(float(np.abs(p).max()) for p in pts))
    for a in range(3):
        for sgn in (1.0, -1.0):
            if not pts:
                return False
            d = [h[a] - sgn * p[a] for p in pts]                      # >= 0 inside
            nxt = []
            for i in range(len(pts)):
                j = (i + 1) % len(pts)
                if d[i] >= -tol:
                    nxt.append(pts[i])
                if (d[i] >= -tol) != (d[j] >= -tol):
                    nxt.append(pts[i] + (pts[j] - pts[i]) * (d[i] / (d[i] - d[j])))
            pts = nxt
    return bool(pts)


def local64(obox):
    """(R^T as rows = the box's axes, centre, half) of one query in binary64."""
    return matrix64(obox["quat"].astype(np.float64)).T, obox["centre"].astype(np.float64), obox["half"].astype(np.float64)


def corners64(obox):
    Rt, c, h = local64(obox)
    return np.array([c + Rt.T @ (np.array(s) * h) for s in itertools.product((-1.0, 1.0), repeat=3)])
