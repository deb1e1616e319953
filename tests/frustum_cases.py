"""Shared by the frustum-query tests (test_frustum_host.py, test_frustum_abi.py, test_frustum_gpu.py): the checker - a Python walk
of the compact nodes written from the contract's text (include/mi_raylib.h, the frustum block), one np.float32 operation per
operation, sharing no code with csrc/frustum_math.hpp -, the scenes and query sets, and a float64 reference with code of its own:
a Sutherland-Hodgman clip of the triangle (or of a polygon inscribed in or circumscribed about a disc) against the six planes, and
for a sphere the distance of its centre from the region as the least over the feasible projections onto the affine hulls of all
subsets of at most three planes."""
import itertools

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import near_cases as nc
import point_cases as pc
import box_cases as bc

F = np.float32
ANY, COUNT = irl.FRUSTUM_ANY, irl.FRUSTUM_COUNT
records, packed, ids, sentinel_buffer, is_sentinel, k_offsets, assert_same = (bc.records, bc.packed, bc.ids, bc.sentinel_buffer,
                                                                                bc.is_sentinel, bc.k_offsets, bc.assert_same)
ZERO, ONE = F(0), F(1)
PAIRS = tuple(itertools.combinations(range(6), 2))      # the 15 pairs i < j, in the contract's order


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32: every helper is one rounded operation per operation of the text
# ------------------------------------------------------------------------------------------------------
def v3(x):
    return (F(x[0]), F(x[1]), F(x[2]))


def sub(a, b):
    return (F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2]))


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross(a, v):
    return (F(F(a[1] * v[2]) - F(a[2] * v[1])), F(F(a[2] * v[0]) - F(a[0] * v[2])), F(F(a[0] * v[1]) - F(a[1] * v[0])))


def sel_min(x, y):
    return x if x < y else y


def sel_max(x, y):
    return x if x > y else y


class Query32:
    """One query as the contract reads it: valid, the six normals n[k] and offsets d[k]."""

    def __init__(self, fr):
        P = np.asarray(fr["planes"], F).reshape(6, 4)
        self.valid = bool(np.isfinite(P).all())
        self.n = [v3(P[k, :3]) for k in range(6)]
        self.d = [F(P[k, 3]) for k in range(6)]

    def at(self, k, p):
        return F(dot(self.n[k], p) + self.d[k])

    def meets(self, mn, mx):
        """frustum_meets_bounds."""
        mn, mx = v3(mn), v3(mx)
        with np.errstate(all="ignore"):
            for k in range(6):
                n = self.n[k]
                t = [F(n[a] * mx[a]) if n[a] > 0 else F(n[a] * mn[a]) for a in range(3)]
                up = F(F(F(t[0] + t[1]) + t[2]) + self.d[k])
                if up < 0:
                    return False
            return True

    def tri(self, A, B, C):
        """(touching, contained, the stage that decided: 1, 2, 3 or 0) of a triangle whose bounds are met."""
        V = (A, B, C)
        s = [[self.at(k, p) for k in range(6)] for p in V]
        ins = [all(x >= 0 for x in row) for row in s]
        if any(ins):
            return True, all(ins), 1
        for a, b in ((0, 1), (1, 2), (2, 0)):
            t0, t1, miss = ZERO, ONE, False
            for k in range(6):
                sa, sb = s[a][k], s[b][k]
                if sa < 0 and sb < 0:
                    miss = True
                elif sa < 0:
                    t0 = sel_max(t0, F(sa / F(sa - sb)))
                elif sb < 0:
                    t1 = sel_min(t1, F(sa / F(sa - sb)))
            if not miss and t0 <= t1:
                return True, False, 2
        m = cross(sub(B, A), sub(C, A))
        mA = dot(m, A)
        for i, j in PAIRS:
            ni, nj = self.n[i], self.n[j]
            c = cross(ni, nj)
            det = dot(c, m)
            if not (det != 0):
                continue
            u, w = cross(nj, m), cross(m, ni)
            ndi, dj = F(-self.d[i]), self.d[j]
            x = tuple(F(F(F(F(ndi * u[a]) - F(dj * w[a])) + F(mA * c[a])) / det) for a in range(3))
            if not all(self.at(k, x) >= 0 for k in range(6) if k != i and k != j):
                continue
            if (dot(m, cross(sub(B, A), sub(x, A))) >= 0 and dot(m, cross(sub(C, B), sub(x, B))) >= 0 and
                    dot(m, cross(sub(A, C), sub(x, C))) >= 0):
                return True, False, 3
        return False, False, 0

    def ball(self, c, R2):
        rejects, holds = False, True
        for k in range(6):
            s, nn = self.at(k, c), dot(self.n[k], self.n[k])
            ss, rn = F(s * s), F(R2 * nn)
            if s < 0 and ss > rn:
                rejects = True
            if not (s >= 0 and ss >= rn):
                holds = False
        return (not rejects), (holds and not rejects)

    def touches(self, kind, data):
        """(touching, contained) of a leaf's primitive (NearChecker's leaf entry): its own bounds, then the test of its kind."""
        with np.errstate(all="ignore"):
            if kind == 0:
                V = np.array(data, F)
                if not self.meets(V.min(0), V.max(0)):
                    return False, False
                return self.tri(v3(V[0]), v3(V[1]), v3(V[2]))[:2]
            if kind == 1:
                c, R = pc._v(data[0]), F(data[1])
                if not self.meets(c - R, c + R):
                    return False, False
                return self.ball(v3(c), F(R * R))
            n, c, r = pc._v(data[0]), pc._v(data[1]), F(data[2])
            r2 = F(r * r)
            t = F(1) - n * n / pc.dot32(n, n)
            ext = np.sqrt(r2) * np.sqrt(np.where(t > 0, t, F(0)).astype(F))
            if not self.meets(c - ext, c + ext):
                return False, False
            return self.ball(v3(c), r2)


class FrustumChecker(nc.NearChecker):
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives)."""

    def walk(self, fr, first_only=False):
        """(the touching primitives [(geomID, primID, contained)] in visit order, box tests, primitive tests)."""
        q = Query32(fr)
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

    def overlaps(self, fr):
        found, boxes, prims = self.walk(fr)
        return sorted(found), boxes, prims


# ------------------------------------------------------------------------------------------------------
# records and query sets
# ------------------------------------------------------------------------------------------------------
def frusta(rows):
    """A FRUSTUM array from rows of up to six planes (nx, ny, nz, d); missing planes are absent."""
    rows = list(rows)
    pl = np.zeros((len(rows), 6, 4), F)
    for i, r in enumerate(rows):
        r = np.asarray(r, F).reshape(-1, 4)
        pl[i, :len(r)] = r
    return qb.make_frusta(planes=pl)


def cube(lo, hi):
    """The six planes of the closed box [lo, hi]."""
    return [(1, 0, 0, -lo[0]), (-1, 0, 0, hi[0]), (0, 1, 0, -lo[1]), (0, -1, 0, hi[1]), (0, 0, 1, -lo[2]), (0, 0, -1, hi[2])]


SPECIAL = 13      # the number of hand-placed queries at the end of a set
NOT_WALKED, WALKED = (0, 1), (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
S_NAN, S_INF, S_ALL, S_HALF, S_SLAB, S_CONTRA, S_ZERO_NEG, S_ZERO_MINUS0, S_TINY, S_HUGE, S_HOLDS, S_NEEDLE, S_FAR = range(13)


def frusta_of(name, n=150):
    """The FRUSTUM array of a case: seeded cameras inside and outside the root box looking at points in it, fields of view from 1 to
    150 degrees, the far plane from a thousandth of the root box's diagonal to beyond it, a quarter of them with one to three planes
    absent; from index n - SPECIAL on: a NaN, an infinity, six absent planes, one half-space, a slab of no thickness, contradictory
    planes, a zero normal with d < 0, a zero normal with d = -0, normals scaled by 1e-20 and by 1e15, a frustum that contains the
    scene, a needle (0.01 degrees) along the scene's diagonal, and a camera 1e19 away."""
    hs = bc.scene(name)
    seed = {"soup": 191, "box": 193, "spheres": 195}[name]
    rng = np.random.default_rng(seed)
    lo, hi = pc.root_box(hs.nodes)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    size = float((hi64 - lo64).max())
    diag = float(np.linalg.norm(hi64 - lo64))
    mid = 0.5 * (lo64 + hi64)
    out = np.zeros(n, irl.FRUSTUM)
    for i in range(n):
        spread = 0.5 if i % 2 == 0 else 2.0                                   # inside the root box, or around it
        eye = mid + rng.uniform(-spread, spread, 3) * (hi64 - lo64)
        target = rng.uniform(lo64, hi64)
        fwd = target - eye
        up = rng.normal(size=3)
        fovy = np.radians(10.0 ** rng.uniform(0.0, np.log10(150.0)))
        far = diag * 10.0 ** rng.uniform(-3.0, 0.5)
        near = far * 10.0 ** rng.uniform(-3.0, -0.5)
        out[i] = qb.make_frusta(eye=eye, forward=fwd, up=up, fovy=fovy, aspect=rng.uniform(0.5, 2.0), near=near, far=far,
                                depth="zo" if i % 3 else "no")[0]
        if i % 4 == 0:
            out["planes"][i, rng.choice(6, 1 + i // 4 % 3, replace=False)] = 0.0
    k = n - SPECIAL
    if k >= 0:
        inner = frusta([cube(mid - 0.2 * size, mid + 0.2 * size)])[0]
        for j in range(SPECIAL):
            out[k + j] = inner
        P = out["planes"]
        P[k + S_NAN, 2, 1] = np.nan
        P[k + S_INF, 4, 3] = np.inf
        P[k + S_ALL] = 0.0
        P[k + S_HALF] = 0.0
        P[k + S_HALF, 3] = (0.3, -0.5, 0.8, -(0.3 * mid[0] - 0.5 * mid[1] + 0.8 * mid[2]))
        P[k + S_SLAB] = 0.0
        P[k + S_SLAB, 0], P[k + S_SLAB, 1] = (1, 0, 0, -F(mid[0])), (-1, 0, 0, F(mid[0]))      # x == mid.x: thinner than any ulp
        P[k + S_CONTRA, 0], P[k + S_CONTRA, 1] = (1, 0, 0, -(mid[0] + 1.0)), (-1, 0, 0, mid[0] - 1.0)
        P[k + S_ZERO_NEG, 5] = (0, 0, 0, -1e-30)
        P[k + S_ZERO_MINUS0, 5] = (0, 0, 0, -0.0)
        P[k + S_TINY] = (inner["planes"].astype(np.float64) * 1e-20).astype(F)
        P[k + S_HUGE] = (inner["planes"].astype(np.float64) * 1e15).astype(F)
        P[k + S_HOLDS] = frusta([cube(lo64 - 2 * size, hi64 + 2 * size)])["planes"][0]
        P[k + S_NEEDLE] = qb.make_frusta(eye=lo64 - 0.01 * (hi64 - lo64), forward=hi64 - lo64, up=(0.1, 1.0, 0.2), fovy=np.radians(0.01),
                                         aspect=1.0, near=1e-3 * diag, far=2 * diag)["planes"][0]
        P[k + S_FAR] = qb.make_frusta(eye=mid + np.array([1e19, 0, 0]), forward=(-1, 0, 0), up=(0, 1, 0), fovy=np.radians(60.0), aspect=1.0,
                                      near=1.0, far=np.inf)["planes"][0]
    return out


_twins = {}


def twin(name, n=150):
    """(scene, frusta, the twin's offsets, its records, its counts, its any bytes, the visits of the four), computed once: what
    the device must equal."""
    tag = (name, n)
    if tag not in _twins:
        hs, fr = bc.scene(name), frusta_of(name, n)
        offsets, vo = irl.frustum_offsets_host(hs.desc, fr)
        recs, vf = irl.frustum_fill_host(hs.desc, fr, offsets)
        counts, vc = irl.frustum_query_host(hs.desc, COUNT, fr)
        anys, va = irl.frustum_query_host(hs.desc, ANY, fr)
        _twins[tag] = (hs, fr, offsets, recs, counts, anys, {"offsets": vo, "fill": vf, "count": vc, "any": va})
    return _twins[tag]


def full(desc, fr):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.frustum_offsets_host(desc, fr)
    recs, _ = irl.frustum_fill_host(desc, fr, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


# ------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------
def planes64(fr):
    """(N [P, 3], d [P], M, empty) of a query in binary64: its present planes - an absent plane and a zero normal with d >= 0 hold
    everywhere and are dropped -, M the largest |d| / |n| among them, empty = a zero normal with d < 0 (the region is empty)."""
    P = np.asarray(fr["planes"], np.float64).reshape(6, 4)
    ln = np.linalg.norm(P[:, :3], axis=1)
    empty = bool(((ln == 0) & (P[:, 3] < 0)).any())
    P, ln = P[ln > 0], ln[ln > 0]
    M = float((np.abs(P[:, 3]) / ln).max()) if len(P) else 0.0
    return P[:, :3] / ln[:, None], P[:, 3] / ln, M, empty      # unit normals: moving a plane by eps is d -+ eps


def clip64(poly, N, d):
    """Sutherland-Hodgman: the polygon poly [V, 3] clipped against the half-spaces N.p + d >= 0, closed; [] when nothing is left."""
    for n, dk in zip(N, d):
        if len(poly) == 0:
            break
        s = poly @ n + dk
        out = []
        for a in range(len(poly)):
            b = (a + 1) % len(poly)
            if s[a] >= 0:
                out.append(poly[a])
                if s[b] < 0:
                    out.append(poly[a] + (poly[b] - poly[a]) * (s[a] / (s[a] - s[b])))
            elif s[b] >= 0:
                out.append(poly[a] + (poly[b] - poly[a]) * (s[a] / (s[a] - s[b])))
        poly = np.array(out).reshape(-1, 3)
    return poly


def verdict64(poly_in, poly_out, N, d, eps):
    """+1: poly_in still touches with every plane moved inward by eps; -1: poly_out still misses with every plane moved outward by
    eps; 0: unclear."""
    if len(clip64(poly_in, N, d - eps)):
        return 1
    if len(clip64(poly_out, N, d + eps)) == 0:
        return -1
    return 0


def region_distance64(c, N, d):
    """The distance of the point c from the region N.p + d >= 0 (unit normals): 0 inside, else the least |x - c| over the feasible
    projections x of c onto the affine hulls of all subsets of at most three planes. inf for an empty region."""
    s = N @ c + d
    if (s >= 0).all():
        return 0.0
    scale = max(1.0, float(np.abs(c).max()), float(np.abs(d).max()))
    best = np.inf
    for m in (1, 2, 3):
        for S in itertools.combinations(range(len(N)), m):
            A, b = N[list(S)], s[list(S)]
            G = A @ A.T
            if abs(np.linalg.det(G)) < 1e-12:
                continue
            x = c - A.T @ np.linalg.solve(G, b)
            if (N @ x + d >= -1e-9 * scale).all():
                best = min(best, float(np.linalg.norm(x - c)))
    return best


def region_farthest64(c, N, d, reach):
    """The largest distance of a point of the region from c, the region cut by a cube of half side `reach` about c so that it is
    bounded: the farthest of its corners (three planes meeting, feasible). -inf for an empty region."""
    cubeN = np.concatenate([np.eye(3), -np.eye(3)])
    cubed = np.concatenate([reach - c, reach + c])
    N, d = np.concatenate([N, cubeN]), np.concatenate([d, cubed])
    best = -np.inf
    for S in itertools.combinations(range(len(N)), 3):
        A = N[list(S)]
        if abs(np.linalg.det(A)) < 1e-12:
            continue
        x = np.linalg.solve(A, -d[list(S)])
        if (N @ x + d >= -1e-9 * reach).all():
            best = max(best, float(np.linalg.norm(x - c)))
    return best


def disc_polygons64(n, c, r, sides=256):
    """(inscribed, circumscribed) regular polygons of the disc, [sides, 3] each."""
    n = n / np.linalg.norm(n)
    a = np.cross(n, (1.0, 0.0, 0.0) if abs(n[0]) < 0.9 else (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    ang = np.linspace(0.0, 2 * np.pi, sides, endpoint=False)
    ring = np.cos(ang)[:, None] * a[None] + np.sin(ang)[:, None] * b[None]
    return c + r * ring, c + r / np.cos(np.pi / sides) * ring
