"""Shared by the box-query tests (test_box_host.py, test_box_abi.py, test_box_gpu.py): the checker - a Python walk of the compact
nodes written from the contract's text (include/mi_raylib.h, the box-query block), one np.float32 operation per operation -, the
scenes and box sets, a float64 brute force over every primitive with the boxes it leaves a margin for, and the packing of lists
into OVERLAP records."""
import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import near_cases as nc
import point_cases as pc

F = np.float32
HALF = F(0.5)
SENTINEL = (0xABCD1234, 0x5A5A, 0xA5A5, 0xDEADBEEF, 0x0BADF00D)
ANY, COUNT = irl.BOX_ANY, irl.BOX_COUNT


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32
# ------------------------------------------------------------------------------------------------------
def _bounds(mn, mx, lo, hi):
    """(the bounds meet the box, the box holds the bounds): closed compares."""
    return bool((mn <= hi).all() and (mx >= lo).all()), bool((mn >= lo).all() and (mx <= hi).all())


def _sum3(a, b, c):
    return F(F(a + b) + c)


def tri_touch32(a, b, c, lo, hi):
    V = np.array([a, b, c], F)
    lo, hi = pc._v(lo), pc._v(hi)
    meets, contained = _bounds(V.min(0), V.max(0), lo, hi)
    if not meets:
        return False, contained
    if any(bool(((v >= lo) & (v <= hi)).all()) for v in V):
        return True, contained
    with np.errstate(all="ignore"):
        cb = HALF * lo + HALF * hi
        h = HALF * hi - HALF * lo
        W = V - cb
        e0, e1, e2 = W[1] - W[0], W[2] - W[1], W[0] - W[2]

        def separates(p, r):
            return bool((p > r).all() or (p < -r).all())

        for e in (e0, e1, e2):
            ae = np.abs(e)
            if separates(e[1] * W[:, 2] - e[2] * W[:, 1], F(h[1] * ae[2] + h[2] * ae[1])):
                return False, contained
            if separates(e[2] * W[:, 0] - e[0] * W[:, 2], F(h[0] * ae[2] + h[2] * ae[0])):
                return False, contained
            if separates(e[0] * W[:, 1] - e[1] * W[:, 0], F(h[0] * ae[1] + h[1] * ae[0])):
                return False, contained
        n = np.array([e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]], F)
        an = np.abs(n)
        s = pc.dot32(n, W[0])
        r = _sum3(h[0] * an[0], h[1] * an[1], h[2] * an[2])
        return (not (s > r or s < -r)), contained


def sphere_touch32(c, radius, lo, hi):
    c, lo, hi, radius = pc._v(c), pc._v(lo), pc._v(hi), F(radius)
    with np.errstate(all="ignore"):
        r2 = F(radius * radius)
        meets, contained = _bounds(c - radius, c + radius, lo, hi)
        if not meets:
            return False, contained
        dmin2 = pc.box_dist2_32(lo, hi, c)
        f = np.maximum(np.abs(c - lo), np.abs(hi - c))
        dmax2 = _sum3(f[0] * f[0], f[1] * f[1], f[2] * f[2])
        return (not dmin2 > r2) and (not dmax2 < r2), contained


def disc_touch32(n, c, r, lo, hi):
    n, c, lo, hi = pc._v(n), pc._v(c), pc._v(lo), pc._v(hi)
    with np.errstate(all="ignore"):
        r2 = F(F(r) * F(r))
        rr = np.sqrt(r2)
        nn = pc.dot32(n, n)
        t = F(1) - n * n / nn
        t = np.where(t > 0, t, F(0)).astype(F)
        ext = rr * np.sqrt(t)
        meets, contained = _bounds(c - ext, c + ext, lo, hi)
        if not meets:
            return False, contained
        cb = HALF * lo + HALF * hi
        h = HALF * hi - HALF * lo
        an = np.abs(n)
        s = pc.dot32(n, cb - c)
        rad = _sum3(h[0] * an[0], h[1] * an[1], h[2] * an[2])
        if np.abs(s) > rad:
            return False, contained
        return (not pc.box_dist2_32(lo, hi, c) > r2), contained


def box_valid(lo, hi):
    return bool(np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all())


class BoxChecker(nc.NearChecker):
    """The contract over a host scene's compact nodes (or `nodes`, a BVH_NODE array over the same primitives): NearChecker's table
    of boxes, skip links and leaf primitives, walked with a box."""

    def _touch(self, i, lo, hi):
        kind, data, _, _ = self.leaf[i]
        if kind == 0:
            return tri_touch32(*data, lo, hi)
        if kind == 1:
            return sphere_touch32(data[0], data[1], lo, hi)
        return disc_touch32(data[0], data[1], data[2], lo, hi)

    def walk(self, box, first_only=False):
        """(the touching primitives [(geomID, primID, contained)] in visit order, box tests, primitive tests)."""
        lo, hi = np.asarray(box["lo"], F), np.asarray(box["hi"], F)
        found, boxes, prims = [], 0, 0
        if not box_valid(lo, hi):
            return found, 0, 0
        i = 0
        while i < self.n:
            boxes += 1
            nlo, nhi = np.array(self.lo[i], F), np.array(self.hi[i], F)
            if not ((nlo <= hi).all() and (nhi >= lo).all()):
                i = self.skip[i]
                continue
            if self.leaf[i] is None:
                i += 1
                continue
            prims += 1
            touch, contained = self._touch(i, lo, hi)
            if touch:
                found.append((self.leaf[i][2], self.leaf[i][3], contained))
                if first_only:
                    break
            i = self.skip[i]
        return found, boxes, prims

    def overlaps(self, box):
        """(every touching primitive sorted by (geomID, primID), box tests, primitive tests)."""
        found, boxes, prims = self.walk(box)
        return sorted(found), boxes, prims


# ------------------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------------------
def boxes(rows):
    """A BOX array from rows ((lox, loy, loz), (hix, hiy, hiz))."""
    rows = list(rows)
    return qb.make_boxes(np.array([r[0] for r in rows], F).reshape(-1, 3), np.array([r[1] for r in rows], F).reshape(-1, 3))


def records(found, box, length=None):
    """`found` [(geomID, primID, contained)] as OVERLAP records of box `box`, cut or padded to `length`."""
    length = len(found) if length is None else length
    out = np.zeros(length, irl.OVERLAP)
    out["primID"], out["geomID"], out["flags"], out["box"] = irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, box
    for j, (g, q, contained) in enumerate(found[:length]):
        out[j] = (q, g, irl.OVERLAP_CONTAINED if contained else 0, box, 0)
    return out


def packed(lists):
    """(offsets, recs) of per-box sorted lists."""
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    recs = np.concatenate([records(x, i) for i, x in enumerate(lists)]) if lists else np.zeros(0, irl.OVERLAP)
    return offsets, recs.astype(irl.OVERLAP)


def ids(recs):
    """The (geomID, primID) pairs of records, as a set."""
    return {(int(r["geomID"]), int(r["primID"])) for r in recs}


def sentinel_buffer(n_records):
    """A 16-byte aligned OVERLAP array of `n_records` + 64 records, every one the sentinel."""
    buf = irl.aligned_bytes((n_records + 64) * irl.OVERLAP.itemsize).view(irl.OVERLAP)
    buf[:] = SENTINEL
    return buf


def is_sentinel(recs):
    want = np.zeros((), irl.OVERLAP)
    want[()] = SENTINEL
    return (np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1) == want.reshape(1).view(np.uint8)).all(1)


k_offsets = nc.k_offsets


def assert_same(got, want, what):
    """(offsets, recs) pairs, exactly."""
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at boxes {np.nonzero(np.asarray(got[0][1:]) != np.asarray(want[0][1:]))[0][:4]}"
    pc.assert_bytes_equal(np.ascontiguousarray(got[1]).reshape(-1), np.ascontiguousarray(want[1]).reshape(-1), what)


# ------------------------------------------------------------------------------------------------------
# scenes and box sets
# ------------------------------------------------------------------------------------------------------
_scenes, _twins, _checked = {}, {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = pc.scene(name)
    return _scenes[name]


def boxes_of(name, n=None):
    """The BOX array of a case. soup: 400 boxes - centred inside the root box, far outside, exactly on vertices and centres - with
    half sizes from a point to a tenth of the scene (the soup's triangles are about 3 across, 600 of them in a cube of 20), so that
    they hold none, a few and dozens of primitives; a few queries that are not walked. box / spheres: 300 boxes sized to the scene."""
    hs = scene(name)
    seed = {"soup": 51, "box": 53, "spheres": 55}[name]
    count = {"soup": 400, "box": 300, "spheres": 300}[name] if n is None else n
    pts = pc.mixed_points(hs, count, seed=seed)
    centre = np.stack([pts[c] for c in "xyz"], 1).astype(F)
    lo, hi = pc.root_box(hs.nodes)
    size = float((hi - lo).max())
    rng = np.random.default_rng(seed + 1)
    steps = [0.0, 0.02, 0.05, 0.1, 0.25] if name == "soup" else [0.0, 0.01, 0.03, 0.08, 0.2]
    half = (rng.choice(np.array(steps, F), (count, 1), p=[0.05, 0.25, 0.3, 0.25, 0.15]) * F(size)
            * rng.uniform(0.5, 1.0, (count, 3)).astype(F)).astype(F)
    b = qb.make_boxes((centre - half).astype(F), (centre + half).astype(F))
    if count > 12:
        b["lo"][7, 0] = np.nan; b["hi"][8, 2] = np.inf; b["lo"][9, 1] = -np.inf
        b["lo"][10] = b["hi"][10] + F(1)                       # lo > hi
    return b


def twin(name, n=None):
    """(scene, boxes, the twin's offsets, its records, its counts, its any bytes, the visits of the four), computed once: what the
    device must equal."""
    tag = (name, n)
    if tag not in _twins:
        hs, bx = scene(name), boxes_of(name, n)
        offsets, vo = irl.box_offsets_host(hs.desc, bx)
        recs, vf = irl.box_fill_host(hs.desc, bx, offsets)
        counts, vc = irl.box_query_host(hs.desc, COUNT, bx)
        anys, va = irl.box_query_host(hs.desc, ANY, bx)
        _twins[tag] = (hs, bx, offsets, recs, counts, anys, {"offsets": vo, "fill": vf, "count": vc, "any": va})
    return _twins[tag]


# ------------------------------------------------------------------------------------------------------
# float64 brute force: the signed gap of every primitive from every box
# ------------------------------------------------------------------------------------------------------
def tri_gap64(lo, hi, A, B, Cc):
    """[N, T]: the largest signed gap over the 13 normalised axes of boxes lo, hi [N, 3] and triangles A, B, Cc [T, 3] in binary64:
    > 0 separated by at least that much, < 0 overlapping on every axis by at least that much. An edge x axis product shorter than
    1e-9 of the edge is skipped."""
    lo, hi = np.asarray(lo, np.float64)[:, None, :], np.asarray(hi, np.float64)[:, None, :]
    cb, h = (lo + hi) / 2, (hi - lo) / 2
    V = np.stack([A, B, Cc], 0)[:, None, :, :] - cb[None]           # [3, N, T, 3]
    gap = np.full(V.shape[1:3], -np.inf)

    def axis(ax, ok=None):                                         # ax [1 or N, T, 3], unit length
        nonlocal gap
        p = (V * ax[None]).sum(-1)
        r = (h * np.abs(ax)).sum(-1)
        g = np.maximum(p.min(0) - r, -r - p.max(0))
        gap = np.maximum(gap, g if ok is None else np.where(ok, g, -np.inf))

    eye = np.eye(3)
    for k in range(3):
        axis(np.broadcast_to(eye[k], (1, A.shape[0], 3)))
    E = [B - A, Cc - B, A - Cc]
    n = np.cross(E[0], E[1])
    ln = np.linalg.norm(n, axis=1)
    axis((n / np.where(ln > 0, ln, 1.0)[:, None])[None], (ln > 0)[None])
    for e in E:
        le = np.linalg.norm(e, axis=1)
        for k in range(3):
            x = np.cross(eye[k][None], e)
            lx = np.linalg.norm(x, axis=1)
            ok = lx > 1e-9 * le
            axis((x / np.where(ok, lx, 1.0)[:, None])[None], ok[None])
    return gap


def sphere_gap64(lo, hi, c, r):
    """[N, S]: max(dmin - r, r - dmax): > 0 the box misses the shell by that much (outside or inside), < 0 it crosses it."""
    lo, hi = np.asarray(lo, np.float64)[:, None, :], np.asarray(hi, np.float64)[:, None, :]
    dmin = np.sqrt((np.maximum(np.maximum(lo - c[None], c[None] - hi), 0.0) ** 2).sum(-1))
    dmax = np.sqrt((np.maximum(np.abs(c[None] - lo), np.abs(hi - c[None])) ** 2).sum(-1))
    return np.maximum(dmin - r[None], r[None] - dmax)


def _seg_dist(p, a, b):
    ab = b - a
    den = ab @ ab
    t = np.clip(((p - a) @ ab) / den, 0.0, 1.0) if den > 0 else 0.0
    return float(np.linalg.norm(p - (a + ab * t)))


_EDGES = [(a, a | (1 << k)) for a in range(8) for k in range(3) if not a & (1 << k)]       # corner numbers: bit k = the hi side of axis k


def disc_gap64(lo, hi, n, c, r):
    """One box against one disc, exactly: the box clipped with the disc's plane is a convex polygon (its corners: where the box's
    edges cross the plane, its sides: the polygon's cut through each face); the disc touches the box when that polygon comes
    within r of the centre. Returns (gap, plane_gap): gap = the polygon's distance from c minus r (+inf when the plane misses the
    box), plane_gap = how far the plane misses the box (<= 0: it does not)."""
    lo, hi, n, c = (np.asarray(x, np.float64) for x in (lo, hi, n, c))
    n = n / np.linalg.norm(n)
    corners = np.array([[hi[k] if a & (1 << k) else lo[k] for k in range(3)] for a in range(8)])
    d = (corners - c) @ n
    plane_gap = max(d.min(), -d.max())
    if plane_gap > 0:
        return np.inf, plane_gap
    if ((c >= lo) & (c <= hi)).all():
        return -r, plane_gap
    faces = {}                                                    # (axis, side) -> the polygon's points on that face
    for a, b in _EDGES:
        if d[a] * d[b] > 0:
            continue
        ends = [corners[a]] if d[a] == 0 else []
        if d[b] == 0:
            ends.append(corners[b])
        if not ends:
            ends = [corners[a] + (corners[b] - corners[a]) * (d[a] / (d[a] - d[b]))]
        for k in range(3):
            if (a >> k) & 1 == (b >> k) & 1:                       # the edge lies in this face of axis k
                faces.setdefault((k, (a >> k) & 1), []).extend(ends)
    best = np.inf
    for pts in faces.values():
        for i in range(len(pts)):
            best = min(best, float(np.linalg.norm(pts[i] - c)))
            for j in range(i + 1, len(pts)):
                best = min(best, _seg_dist(c, pts[i], pts[j]))
    return best - r, plane_gap


def disc_reach64(lo, hi, n, c, r):
    """An upper bound of the disc's distance from the box: y = the box's point nearest c; its projection y' into the plane is no
    farther from c than y is, so when y lies within r of c, y' is a point of the disc, |n.(y - c)| away from y. Where y' lies
    outside the rim, what it lies outside by is added."""
    lo, hi, n, c = (np.asarray(x, np.float64) for x in (lo, hi, n, c))
    n = n / np.linalg.norm(n)
    y = np.clip(c, lo, hi)
    h = (y - c) @ n
    return abs(h) + max(0.0, float(np.linalg.norm(y - n * h - c)) - r)
