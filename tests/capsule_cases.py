"""Shared by the capsule-query tests (test_capsule_host.py, test_capsule_abi.py, test_capsule_gpu.py): the checker - a Python walk
of the compact nodes written from the contract's text (include/mi_raylib.h, the capsule block), one np.float32 operation per
operation, sharing no code with csrc/capsule_math.hpp -, the scenes and query sets, and a float64 reference with code of its own:
the segment-to-triangle distance as the minimum over the features (ends against the triangle, the segment against the edges, each
edge pair from its end points and the lines' critical point) with a segment-plane crossing test, the sphere from the nearest and
the farthest point of the segment."""
import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import near_cases as nc
import point_cases as pc
import box_cases as bc

F = np.float32
ANY, COUNT = irl.CAPSULE_ANY, irl.CAPSULE_COUNT
records, packed, ids, sentinel_buffer, is_sentinel, k_offsets, assert_same = (bc.records, bc.packed, bc.ids, bc.sentinel_buffer,
                                                                                bc.is_sentinel, bc.k_offsets, bc.assert_same)
ZERO, ONE = F(0), F(1)


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32: every helper is one rounded operation per operation of the text
# ------------------------------------------------------------------------------------------------------
def v3(x):
    return (F(x[0]), F(x[1]), F(x[2]))


def sub(a, b):
    return (F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2]))


def add(a, b):
    return (F(a[0] + b[0]), F(a[1] + b[1]), F(a[2] + b[2]))


def scale(a, s):
    return (F(a[0] * s), F(a[1] * s), F(a[2] * s))


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross(a, v):
    return (F(F(a[1] * v[2]) - F(a[2] * v[1])), F(F(a[2] * v[0]) - F(a[0] * v[2])), F(F(a[0] * v[1]) - F(a[1] * v[0])))


def dist2(p, q):
    d = sub(p, q)
    return dot(d, d)


def sel_min(x, y):
    return x if x < y else y


def sel_max(x, y):
    return x if x > y else y


def clamp(x):
    return ZERO if x < 0 else (ONE if x > 1 else x)


class Query32:
    """One query as the contract derives it: valid, a, b, d, radius, r2, dd, the world bounds and the four widths."""

    def __init__(self, cap):
        with np.errstate(all="ignore"):
            a, b, radius = v3(cap["a"]), v3(cap["b"]), F(cap["radius"])
            self.valid = bool(np.isfinite(np.array(a + b + (radius,))).all() and radius >= 0)
            self.a, self.b, self.radius = a, b, radius
            d = self.d = sub(b, a)
            self.r2 = F(radius * radius)
            self.dd = dot(d, d)
            self.qmn = tuple(F(sel_min(a[k], b[k]) - radius) for k in range(3))
            self.qmx = tuple(F(sel_max(a[k], b[k]) + radius) for k in range(3))
            # X0 = (0, d.z, -d.y), X1 = (-d.z, 0, d.x), X2 = (d.y, -d.x, 0): (the two world axes, the two components)
            self.lateral = (((1, 2), (d[2], -d[1])), ((0, 2), (-d[2], d[0])), ((0, 1), (d[1], -d[0])))
            xx, yy, zz = F(d[0] * d[0]), F(d[1] * d[1]), F(d[2] * d[2])
            self.R = (self.width(F(zz + yy)), self.width(F(zz + xx)), self.width(F(yy + xx)))
            self.Rd = self.width(self.dd)

    def width(self, ll):
        """radius sqrtf(ll), or +inf for a squared length below the smallest normal binary32 (2^-126): that axis separates nothing."""
        return F(self.radius * np.sqrt(ll)) if ll >= F(2.0 ** -126) else F(np.inf)

    def meets(self, mn, mx):
        """capsule_meets_bounds."""
        mn, mx = v3(mn), v3(mx)
        with np.errstate(all="ignore"):
            for k in range(3):
                if not (mn[k] <= self.qmx[k] and mx[k] >= self.qmn[k]):
                    return False
            dl, dh = sub(mn, self.a), sub(mx, self.a)
            for (axes, comps), R in zip(self.lateral, self.R):
                t = [F(x * dh[k]) if x > 0 else F(x * dl[k]) for k, x in zip(axes, comps)]
                u = [F(x * dl[k]) if x > 0 else F(x * dh[k]) for k, x in zip(axes, comps)]
                up, dn = F(t[0] + t[1]), F(u[0] + u[1])
                if dn > R or up < -R:
                    return False
            d = self.d
            t = [F(d[k] * dh[k]) if d[k] > 0 else F(d[k] * dl[k]) for k in range(3)]
            u = [F(d[k] * dl[k]) if d[k] > 0 else F(d[k] * dh[k]) for k in range(3)]
            up, dn = F(F(t[0] + t[1]) + t[2]), F(F(u[0] + u[1]) + u[2])
            if dn > F(self.dd + self.Rd) or up < -self.Rd:
                return False
            return True

    def point_seg_dist2(self, p):
        t = dot(sub(p, self.a), self.d)
        if t <= 0:
            return dist2(p, self.a)
        if t >= self.dd:
            return dist2(p, self.b)
        return dist2(p, add(self.a, scale(self.d, F(t / self.dd))))

    def seg_seg_dist2(self, P, Q):
        """Ericson 5.1.9 as the header states it."""
        a, d, dd = self.a, self.d, self.dd
        d2, r = sub(Q, P), sub(a, P)
        e, f = dot(d2, d2), dot(d2, r)
        if dd <= 0 and e <= 0:
            return dot(r, r)
        if dd <= 0:
            s, t = ZERO, clamp(F(f / e))
        else:
            c = dot(d, r)
            if e <= 0:
                t, s = ZERO, clamp(F(-c / dd))
            else:
                bb = dot(d, d2)
                denom = F(F(dd * e) - F(bb * bb))
                s = clamp(F(F(F(bb * f) - F(c * e)) / denom)) if denom != 0 else ZERO
                t = F(F(F(bb * s) + f) / e)
                if t < 0:
                    t, s = ZERO, clamp(F(-c / dd))
                elif t > 1:
                    t, s = ONE, clamp(F(F(bb - c) / dd))
        c1, c2 = add(a, scale(d, s)), add(P, scale(d2, t))
        v = sub(c1, c2)
        return dot(v, v)

    def tri(self, A, B, C):
        """(touching, contained) of a triangle whose bounds are met."""
        r2 = self.r2
        touch = False
        for p in (self.a, self.b):
            if not touch and not (pc.dist2_32(p, pc.tri_closest32(A, B, C, p)[0]) > r2):
                touch = True
        for P, Q in ((A, B), (B, C), (C, A)):
            if not touch and not (self.seg_seg_dist2(P, Q) > r2):
                touch = True
        if not touch:
            n = cross(sub(B, A), sub(C, A))
            sa, sb = dot(n, sub(self.a, A)), dot(n, sub(self.b, A))
            if not (sa > 0 and sb > 0) and not (sa < 0 and sb < 0) and not (sa == 0 and sb == 0):
                u0, u1, u2 = sub(A, self.a), sub(B, self.a), sub(C, self.a)
                w = (dot(self.d, cross(u0, u1)), dot(self.d, cross(u1, u2)), dot(self.d, cross(u2, u0)))
                touch = all(x >= 0 for x in w) or all(x <= 0 for x in w)
        if not touch:
            return False, False
        return True, all(self.point_seg_dist2(V) <= r2 for V in (A, B, C))

    def sphere(self, c, R):
        dmin2 = self.point_seg_dist2(c)
        dmax2 = sel_max(dist2(self.a, c), dist2(self.b, c))
        s, m = F(R + self.radius), F(R - self.radius)
        if dmin2 > F(s * s) or (m > 0 and dmax2 < F(m * m)):
            return False, False
        return True, bool(F(np.sqrt(dmin2) + R) <= self.radius)

    def disc(self, n, c, rp):
        sa, sb = dot(n, sub(self.a, c)), dot(n, sub(self.b, c))
        rn = F(self.radius * np.sqrt(dot(n, n)))
        if (sa > rn and sb > rn) or (sa < -rn and sb < -rn):
            return False, False
        s = F(rp + self.radius)
        dmin2 = self.point_seg_dist2(c)
        if dmin2 > F(s * s):
            return False, False
        return True, bool(F(np.sqrt(dmin2) + rp) <= self.radius)

    def touches(self, kind, data):
        """(touching, contained) of a leaf's primitive (NearChecker's leaf entry): its own bounds, then the test of its kind."""
        with np.errstate(all="ignore"):
            if kind == 0:
                V = np.array(data, F)
                if not self.meets(V.min(0), V.max(0)):
                    return False, False
                return self.tri(v3(V[0]), v3(V[1]), v3(V[2]))
            if kind == 1:
                c, R = pc._v(data[0]), F(data[1])
                if not self.meets(c - R, c + R):
                    return False, False
                return self.sphere(v3(c), R)
            n, c, r = pc._v(data[0]), pc._v(data[1]), F(data[2])
            r2 = F(r * r)
            t = F(1) - n * n / pc.dot32(n, n)
            ext = np.sqrt(r2) * np.sqrt(np.where(t > 0, t, F(0)).astype(F))
            if not self.meets(c - ext, c + ext):
                return False, False
            return self.disc(v3(n), v3(c), F(np.sqrt(r2)))


class CapsuleChecker(nc.NearChecker):
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives)."""

    def walk(self, cap, first_only=False):
        """(the touching primitives [(geomID, primID, contained)] in visit order, box tests, primitive tests)."""
        q = Query32(cap)
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

    def overlaps(self, cap):
        found, boxes, prims = self.walk(cap)
        return sorted(found), boxes, prims


# ------------------------------------------------------------------------------------------------------
# records and query sets
# ------------------------------------------------------------------------------------------------------
def capsules(rows):
    """A CAPSULE array from rows (a, b, radius)."""
    rows = list(rows)
    return qb.make_capsules(np.array([r[0] for r in rows], F).reshape(-1, 3), np.array([r[1] for r in rows], F).reshape(-1, 3),
                            np.array([r[2] for r in rows], F))


SPECIAL = 12      # the number of hand-placed queries at the end of a set
NOT_WALKED, WALKED = (0, 1, 2), (3, 4, 5, 6, 7, 8, 9, 10, 11)


def capsules_of(name, n=150):
    """The CAPSULE array of a case: uniform directions, centres in the root box, lengths from zero to the root box's diagonal, radii
    from a thousandth of the root box to a quarter of it; from index n - SPECIAL on: a NaN, an infinity, a negative radius, a -0
    radius, a == b, radius == 0 on a diagonal and on an axis, a capsule spanning the scene, a length of 1e-30 (dd underflows),
    coordinates of 1e19 (products overflow: it errs towards listing), and two thin diagonals."""
    hs = bc.scene(name)
    seed = {"soup": 91, "box": 93, "spheres": 95}[name]
    rng = np.random.default_rng(seed)
    lo, hi = pc.root_box(hs.nodes)
    size = float((hi - lo).max())
    diag = float(np.linalg.norm((hi - lo).astype(np.float64)))
    centre = rng.uniform(lo, hi, (n, 3))
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    length = diag * rng.uniform(0.0, 1.0, n)
    length[::17] = 0.0
    radius = 0.25 * size * 10.0 ** (np.log10(0.004) * rng.uniform(0.0, 1.0, n) ** 3)      # (most of them large enough to list something)
    c = qb.make_capsules((centre - dirs * length[:, None] * 0.5).astype(F), (centre + dirs * length[:, None] * 0.5).astype(F), radius.astype(F))
    k = n - SPECIAL
    mid = ((lo + hi) * F(0.5)).astype(F)
    if k >= 0:
        c["a"][k:] = mid + rng.uniform(-0.2 * size, 0.2 * size, (SPECIAL, 3)).astype(F)
        c["b"][k:] = mid + rng.uniform(-0.2 * size, 0.2 * size, (SPECIAL, 3)).astype(F)
        c["radius"][k:] = F(0.05 * size)
        c["a"][k, 1] = np.nan
        c["b"][k + 1, 2] = np.inf
        c["radius"][k + 2] = -1e-3
        c["radius"][k + 3] = -0.0
        c["b"][k + 4] = c["a"][k + 4]                                      # a ball
        c["a"][k + 5], c["b"][k + 5], c["radius"][k + 5] = lo, hi, 0.0     # a bare segment on the root box's diagonal
        c["a"][k + 6], c["b"][k + 6], c["radius"][k + 6] = (lo[0], mid[1], mid[2]), (hi[0], mid[1], mid[2]), 0.0      # and along x
        c["a"][k + 7], c["b"][k + 7], c["radius"][k + 7] = lo, hi, F(2 * size)      # spans the scene
        c["a"][k + 8, 0] = 0.0                                             # (from x = 0, where 1e-30 is not rounded away)
        c["b"][k + 8] = c["a"][k + 8]
        c["b"][k + 8, 0] = 1e-30
        c["a"][k + 9], c["b"][k + 9] = mid - F(1e19), mid + F(1e19)
        c["a"][k + 10], c["b"][k + 10], c["radius"][k + 10] = lo, hi, F(0.01 * size)
        c["a"][k + 11], c["b"][k + 11], c["radius"][k + 11] = (lo[0], hi[1], lo[2]), (hi[0], lo[1], hi[2]), F(0.02 * size)
    return c


_twins = {}


def twin(name, n=150):
    """(scene, capsules, the twin's offsets, its records, its counts, its any bytes, the visits of the four), computed once: what
    the device must equal."""
    tag = (name, n)
    if tag not in _twins:
        hs, cp = bc.scene(name), capsules_of(name, n)
        offsets, vo = irl.capsule_offsets_host(hs.desc, cp)
        recs, vf = irl.capsule_fill_host(hs.desc, cp, offsets)
        counts, vc = irl.capsule_query_host(hs.desc, COUNT, cp)
        anys, va = irl.capsule_query_host(hs.desc, ANY, cp)
        _twins[tag] = (hs, cp, offsets, recs, counts, anys, {"offsets": vo, "fill": vf, "count": vc, "any": va})
    return _twins[tag]


def full(desc, cp):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.capsule_offsets_host(desc, cp)
    recs, _ = irl.capsule_fill_host(desc, cp, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


# ------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------
def _point_seg64(p, a, b):
    """Distances of points p [..., 3] from segments a, b [..., 3] (broadcast)."""
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0)
    q = a + ab * np.clip(t, 0.0, 1.0)[..., None]
    return np.sqrt(((p - q) ** 2).sum(-1))


def seg_seg_dist64(a, b, P, Q):
    """Distances of the segment [a, b] (3,) from the segments [P, Q] [T, 3]: the minimum is taken at an end of one of the two, or
    where both lines' critical point lies inside both - four point-segment distances and, for lines that are not parallel, the
    lines' distance when its feet lie inside."""
    d = np.minimum(np.minimum(_point_seg64(a[None], P, Q), _point_seg64(b[None], P, Q)),
                   np.minimum(_point_seg64(P, a[None], b[None]), _point_seg64(Q, a[None], b[None])))
    u, v, w = (b - a)[None], Q - P, a[None] - P
    n = np.cross(u, v)
    nn = (n * n).sum(-1)
    ok = nn > 1e-24 * (u * u).sum(-1) * (v * v).sum(-1)
    nn1 = np.where(ok, nn, 1.0)
    s = -(np.cross(v, n) * w).sum(-1) / nn1         # a + u s and P + v t are the feet of the common perpendicular: (w + u s - v t) is
    t = -(np.cross(u, n) * w).sum(-1) / nn1         # parallel to n; dotted with v x n and u x n, with u.(v x n) = |n|^2 = -v.(u x n)
    inside = ok & (s > 0) & (s < 1) & (t > 0) & (t < 1)
    line = np.abs((w * n).sum(-1)) / np.sqrt(nn1)
    return np.where(inside, np.minimum(d, line), d)


def seg_tri_dist64(a, b, A, B, C):
    """Distances of the segment [a, b] (3,) from the triangles A, B, C [T, 3] in binary64: zero where the segment crosses the
    triangle (the plane's crossing point lies inside it), else the least of the two ends' distances and the three edges'."""
    d = np.minimum(pc.tri_dist64(a[None, None], A[None], B[None], C[None])[0], pc.tri_dist64(b[None, None], A[None], B[None], C[None])[0])
    for P, Q in ((A, B), (B, C), (C, A)):
        d = np.minimum(d, seg_seg_dist64(a, b, P, Q))
    n = np.cross(B - A, C - A)
    sa, sb = ((a[None] - A) * n).sum(-1), ((b[None] - A) * n).sum(-1)
    cut = (sa * sb <= 0) & (sa != sb)
    t = sa / np.where(cut, sa - sb, 1.0)
    x = a[None] + (b - a)[None] * t[:, None]
    inside = cut
    for u, v in ((A, B), (B, C), (C, A)):
        inside = inside & ((np.cross(v - u, x - u) * n).sum(-1) >= 0)
    return np.where(inside, 0.0, d)


def sphere_gap64(a, b, radius, c, R):
    """max(distance of the segment from the centre - R - radius, R - radius - the farthest end's distance): <= 0 when the capsule
    reaches the shell from outside and from inside."""
    dmin = float(_point_seg64(c, a, b))
    dmax = max(float(np.linalg.norm(a - c)), float(np.linalg.norm(b - c)))
    return max(dmin - R - radius, R - radius - dmax)


def disc_dist64(a, b, n, c, r, steps=2048):
    """The distance of the segment [a, b] from the disc (unit normal made here), by dense sampling of the segment against the exact
    point-disc distance, refined around the best sample: good to far below the band the tests leave out."""
    n = n / np.linalg.norm(n)

    def point_disc(p):
        v = p - c
        h = v @ n
        u = v - np.outer(h, n)
        ul = np.linalg.norm(u, axis=1)
        return np.sqrt(h * h + np.maximum(ul - r, 0.0) ** 2)

    lo_t, hi_t = 0.0, 1.0
    best = np.inf
    for _ in range(4):
        ts = np.linspace(lo_t, hi_t, steps)
        dd = point_disc(a[None] + (b - a)[None] * ts[:, None])
        j = int(np.argmin(dd))
        best = min(best, float(dd[j]))
        step = (hi_t - lo_t) / (steps - 1)
        lo_t, hi_t = max(0.0, ts[j] - step), min(1.0, ts[j] + step)
    return best
