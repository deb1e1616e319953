"""Shared by the point-query tests (test_point_query_host.py, test_point_query_abi.py, test_point_query_gpu.py): scenes, point
sets, a float64 brute-force reference and numpy binary32 restatements of the contract's formulas (include/mi_raylib.h, the
point-query block), written from the contract's text - an if-chain over the regions, one np.float32 operation per operation -
and not from csrc/point_math.hpp's select form."""
import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
from refit_cases import soup      # the 600-triangle soup of tests/test_query_gpu.py: two meshes + a sphere + a disc

F = np.float32
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------
def scene(name):
    if name == "soup":
        hs = soup(1234, False)
    elif name == "soup-normals":
        hs = soup(1235, True)
    else:
        hs = irl.HostScene.builtin(name)
    hs.desc.set_image(64, 64)
    return hs


def hand_scene(tris=(), spheres=(), discs=()):
    """A scene of the given primitives, one geometry each: tris = [(a, b, c)] (a mesh of one triangle each), spheres =
    [(x, y, z, r)], discs = [(nx, ny, nz, r, cx, cy, cz)]. Geometry order: triangles, spheres, discs. The BVH is the host builder's."""
    nt, ns, nd = len(tris), len(spheres), len(discs)
    v = np.zeros(3 * nt, dtype=irl.VEC3)
    for i, t in enumerate(tris):
        for k in range(3):
            v[3 * i + k] = tuple(F(x) for x in t[k])
    idx = np.tile(np.arange(3, dtype=np.uint16), (max(nt, 1), 1))[:nt]
    info = np.zeros(nt, dtype=irl.MESH_INFO)
    for i in range(nt):
        info[i] = (i, 3 * i, 1, 3)
    sph = np.zeros(ns, dtype=irl.SPHERE)
    for i, s in enumerate(spheres):
        sph[i] = tuple(F(x) for x in s)
    dsc = np.zeros(nd, dtype=irl.DISC)
    for i, d in enumerate(discs):
        dsc[i] = tuple(F(x) for x in d)
    G = nt + ns + nd
    mats = np.zeros(1, dtype=irl.MATERIAL); mats["ior"] = 1.5
    mat_ids = np.zeros(max(G, 1), dtype=np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = (info.ctypes.data if nt else None), nt
    g.mesh_tris, g.num_tris = (idx.ctypes.data if nt else None), nt
    g.mesh_verts, g.num_verts = (v.ctypes.data if nt else None), len(v)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, G
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.spheres, g.num_spheres = (sph.ctypes.data if ns else None), ns
    g.discs, g.num_discs = (dsc.ctypes.data if nd else None), nd
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, idx, info, sph, dsc, mats, mat_ids]
    hs.desc.set_image(8, 8)
    return hs


def with_nodes(desc, nodes, **arrays):
    """A copy of desc with other BVH nodes (a BVH_NODE array) and, optionally, other arrays (field name = numpy array)."""
    d = irl.SceneDesc.from_buffer_copy(desc)
    nodes = np.ascontiguousarray(nodes, dtype=irl.BVH_NODE)
    d.bvh_nodes, d.num_nodes = (nodes.ctypes.data if nodes.size else None), nodes.size
    d._keep = [nodes]
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        setattr(d, name, a.ctypes.data)
        d._keep.append(a)
    return d


def compact_node(lo, hi, link, geom=irl.INVALID_GEOM):
    """A compact node by hand: min as binary32, the extents rounded UP to binary16; link = second child (interior) or primID."""
    n = np.zeros((), irl.BVH_NODE)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    ext = (hi - lo).astype(F)
    h = ext.astype(np.float16)
    h = np.where(h.astype(F) < ext, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)
    n["min_x"], n["min_y"], n["min_z"] = lo
    n["dx"], n["dy"], n["dz"] = h.view(np.uint16)
    n["link"], n["geomID"] = link, geom
    return n


def root_box(nodes):
    n = nodes[0]
    lo = np.array([n["min_x"], n["min_y"], n["min_z"]], F)
    ext = np.array([n["dx"], n["dy"], n["dz"]], np.uint16).view(np.float16).astype(F)
    return lo, (lo + ext).astype(F)


# ------------------------------------------------------------------------------------------------------
# a scene's primitives, in binary64, and the brute-force reference
# ------------------------------------------------------------------------------------------------------
def primitives(hs):
    """{"tri": (A, B, C [T, 3] float64, geom [T], prim [T]), "sphere": (c [S, 3], r [S], geom [S]), "disc": (n [D, 3], c [D, 3],
    r [D], geom [D])} of a host scene."""
    verts = np.stack([hs.verts[c] for c in "xyz"], 1).astype(np.float64)
    tris = hs.tris.astype(np.int64)
    A, B, Cc, tg, tp, sc, sr, sg, dn, dc, dr, dg = ([] for _ in range(12))
    for g, ref in enumerate(hs.geometry):
        if ref["type"] == 0:
            m = hs.mesh_info[ref["index"]]
            t = tris[m["firstIndex"]:m["firstIndex"] + m["numTriangles"]] + int(m["firstVertex"])
            A.append(verts[t[:, 0]]); B.append(verts[t[:, 1]]); Cc.append(verts[t[:, 2]])
            tg.append(np.full(len(t), g)); tp.append(np.arange(len(t)))
        elif ref["type"] == 1:
            s = hs.spheres[ref["index"]]
            sc.append([s["x"], s["y"], s["z"]]); sr.append(s["radius"]); sg.append(g)
        else:
            d = hs.discs[ref["index"]]
            dn.append([d["nx"], d["ny"], d["nz"]]); dc.append([d["cx"], d["cy"], d["cz"]]); dr.append(d["r"]); dg.append(g)
    cat = lambda x, w: np.concatenate(x) if x else np.zeros((0,) + w)
    return {"tri": (cat(A, (3,)), cat(B, (3,)), cat(Cc, (3,)), cat(tg, ()).astype(np.int64), cat(tp, ()).astype(np.int64)),
            "sphere": (np.array(sc, np.float64).reshape(-1, 3), np.array(sr, np.float64), np.array(sg, np.int64)),
            "disc": (np.array(dn, np.float64).reshape(-1, 3), np.array(dc, np.float64).reshape(-1, 3), np.array(dr, np.float64),
                     np.array(dg, np.int64))}


def scene_max_abs(hs):
    """The largest absolute coordinate of the scene: vertices, and sphere / disc centres plus radius."""
    pr = primitives(hs)
    m = 0.0
    for a in pr["tri"][:3]:
        if a.size:
            m = max(m, float(np.abs(a).max()))
    for c, r in ((pr["sphere"][0], pr["sphere"][1]), (pr["disc"][1], pr["disc"][2])):
        if c.size:
            m = max(m, float((np.abs(c) + r[:, None]).max()))
    return m


def _seg_dist(p, a, b):
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0)
    q = a + ab * np.clip(t, 0.0, 1.0)[..., None]
    return np.sqrt(((p - q) ** 2).sum(-1))


def tri_dist64(p, a, b, c):
    """True distance of points p [N, 1, 3] from triangles a, b, c [1, T, 3] in binary64: the nearest of the three edges and, where
    the point projects inside the triangle, the plane. Not the contract's region logic - an independent statement."""
    d = np.minimum(np.minimum(_seg_dist(p, a, b), _seg_dist(p, b, c)), _seg_dist(p, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    h = ((p - a) * n).sum(-1) / nn1                       # (signed plane distance / |n|)
    proj = p - n * h[..., None]
    inside = ok
    for u, v in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(v - u, proj - u) * n).sum(-1) >= 0)
    return np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn1)), d)


def brute_force(hs, pts, margin):
    """Per point (pts [N, 3]): (distance to the nearest primitive, its geomID, its primID, distance to the second nearest) in
    binary64 over every primitive of the scene. Triangles whose bounding sphere lies farther than the nearest centroid + margin
    cannot be nearest, nor within `margin` of the nearest, and are skipped: the second distance is exact where it is below
    nearest + margin and +inf or larger than that otherwise."""
    pr = primitives(hs)
    P = np.asarray(pts, np.float64)
    N = len(P)
    best = np.full(N, np.inf); second = np.full(N, np.inf)
    bg = np.full(N, -1, np.int64); bp = np.full(N, -1, np.int64)

    def merge(d, geom, prim):            # d [N, K], K small
        nonlocal best, second, bg, bp
        for k in range(d.shape[1]):
            d1 = d[:, k]
            better = d1 < best
            second = np.where(better, best, np.minimum(second, d1))
            bg = np.where(better, geom[k], bg); bp = np.where(better, prim[k], bp)
            best = np.where(better, d1, best)

    A, B, Cc, tg, tp = pr["tri"]
    if len(A):
        cen = (A + B + Cc) / 3.0
        R = np.sqrt(np.maximum(np.maximum(((A - cen) ** 2).sum(1), ((B - cen) ** 2).sum(1)), ((Cc - cen) ** 2).sum(1)))
        step = max(1, 1_000_000 // len(A))
        for i in range(0, N, step):
            Q = P[i:i + step]
            dc = np.sqrt(((Q[:, None, :] - cen[None]) ** 2).sum(-1))             # a triangle is never farther than its centroid
            pi, ti = np.nonzero(dc - R[None] <= (dc.min(1) + margin)[:, None])
            d = tri_dist64(Q[pi][:, None, :], A[ti][:, None, :], B[ti][:, None, :], Cc[ti][:, None, :])[:, 0]
            order = np.lexsort((d, pi))
            pi, ti, d = pi[order], ti[order], d[order]
            first = np.nonzero(np.r_[True, pi[1:] != pi[:-1]])[0]                # (every point has at least one candidate)
            nxt = first + 1
            has2 = (nxt < len(pi)) & (pi[np.minimum(nxt, len(pi) - 1)] == pi[first])
            sl = slice(i, i + len(Q))
            best[sl] = d[first]; bg[sl] = tg[ti[first]]; bp[sl] = tp[ti[first]]
            second[sl] = np.where(has2, d[np.minimum(nxt, len(pi) - 1)], np.inf)
    c, r, g = pr["sphere"]
    if len(c):
        merge(np.abs(np.sqrt(((P[:, None, :] - c[None]) ** 2).sum(-1)) - r[None]), g, np.zeros(len(g), np.int64))
    n, c, r, g = pr["disc"]
    if len(c):
        nh = n / np.linalg.norm(n, axis=1, keepdims=True)
        v = P[:, None, :] - c[None]
        h = (v * nh[None]).sum(-1)
        u = np.sqrt(np.maximum(((v - nh[None] * h[..., None]) ** 2).sum(-1), 0.0))
        merge(np.where(u <= r[None], np.abs(h), np.sqrt(h * h + (u - r[None]) ** 2)), g, np.zeros(len(g), np.int64))
    return best, bg, bp, second


def prim_dist64(hs, pts, geom, prim):
    """Distance in binary64 of each point from the primitive named (geom, prim) for it."""
    pr = primitives(hs)
    P = np.asarray(pts, np.float64)
    out = np.full(len(P), np.nan)
    A, B, Cc, tg, tp = pr["tri"]
    key = {(int(g), int(q)): i for i, (g, q) in enumerate(zip(tg, tp))}
    sk = {int(g): i for i, g in enumerate(pr["sphere"][2])}
    dk = {int(g): i for i, g in enumerate(pr["disc"][3])}
    ti = np.array([key.get((int(g), int(q)), -1) for g, q in zip(geom, prim)])
    m = ti >= 0
    if m.any():
        out[m] = tri_dist64(P[m][:, None, :], A[ti[m]][:, None, :], B[ti[m]][:, None, :], Cc[ti[m]][:, None, :])[:, 0]
    for i in np.nonzero(~m)[0]:
        g = int(geom[i])
        if g in sk:
            c, r = pr["sphere"][0][sk[g]], pr["sphere"][1][sk[g]]
            out[i] = abs(np.linalg.norm(P[i] - c) - r)
        elif g in dk:
            n, c, r = pr["disc"][0][dk[g]], pr["disc"][1][dk[g]], pr["disc"][2][dk[g]]
            n = n / np.linalg.norm(n)
            v = P[i] - c; h = v @ n; u = np.linalg.norm(v - n * h)
            out[i] = abs(h) if u <= r else np.hypot(h, u - r)
    return out


# ------------------------------------------------------------------------------------------------------
# the contract in numpy binary32: one np.float32 operation per operation of the text
# ------------------------------------------------------------------------------------------------------
def _v(x):
    return np.asarray(x, F)


def dot32(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def box_dist2_32(lo, hi, p):
    e = [max(max(F(lo[k] - p[k]), F(p[k] - hi[k])), F(0)) for k in range(3)]
    return F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))


def tri_closest32(a, b, c, p):
    """(q, v, w, region) of the contract's triangle formulas."""
    a, b, c, p = _v(a), _v(b), _v(c), _v(p)
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot32(ab, ap), dot32(ac, ap), dot32(ab, bp), dot32(ac, bp), dot32(ab, cp), dot32(ac, cp)
        vc = F(F(d1 * d4) - F(d3 * d2)); vb = F(F(d5 * d2) - F(d1 * d6)); va = F(F(d3 * d6) - F(d5 * d4))
        if d1 <= 0 and d2 <= 0:
            v, w, reg = F(0), F(0), "A"
        elif d3 >= 0 and d4 <= d3:
            v, w, reg = F(1), F(0), "B"
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            v, w, reg = F(d1 / F(d1 - d3)), F(0), "AB"
        elif d6 >= 0 and d5 <= d6:
            v, w, reg = F(0), F(1), "C"
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            v, w, reg = F(0), F(d2 / F(d2 - d6)), "AC"
        elif va <= 0 and F(d4 - d3) >= 0 and F(d5 - d6) >= 0:
            w = F(F(d4 - d3) / F(F(d4 - d3) + F(d5 - d6)))
            v, reg = F(F(1) - w), "BC"
        else:
            den = F(F(1) / F(F(va + vb) + vc))
            v, w, reg = F(vb * den), F(vc * den), "face"
        q = ((a + ab * v).astype(F) + (ac * w).astype(F)).astype(F)
    return q, v, w, reg


def sphere_closest32(c, radius, p):
    c, p, radius = _v(c), _v(p), F(radius)
    with np.errstate(all="ignore"):
        v = p - c
        ln = np.sqrt(dot32(v, v))
        if ln > 0:
            return (c + (v * F(radius / ln)).astype(F)).astype(F)
        return _v([F(c[0] + radius), c[1], c[2]])


def disc_closest32(n, c, r, p):
    n, c, p = _v(n), _v(c), _v(p)
    r2 = F(F(r) * F(r))
    with np.errstate(all="ignore"):
        v = p - c
        h = dot32(v, n)
        q0 = (p - (n * h).astype(F)).astype(F)
        u = q0 - c
        uu = dot32(u, u)
        if uu <= r2:
            return q0
        return (c + (u * F(np.sqrt(r2) / np.sqrt(uu))).astype(F)).astype(F)


def dist2_32(p, q):
    d = _v(p) - _v(q)
    return dot32(d, d)


def found_record(p, q, geom, prim, v=0.0, w=0.0):
    h = np.zeros((), irl.POINT_HIT)
    with np.errstate(all="ignore"):
        h["dist"] = np.sqrt(dist2_32(p, q))
    h["primID"], h["geomID"], h["flags"] = prim, geom, 0
    h["point"] = tuple(q)
    h["b1"], h["b2"] = v, w
    return h


def nothing_record(radius):
    h = np.zeros((), irl.POINT_HIT)
    h["dist"] = radius
    h["primID"], h["geomID"], h["flags"] = irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED
    return h


def points(rows):
    """A POINT array from rows (x, y, z, radius)."""
    a = np.zeros(len(rows), irl.POINT)
    for i, r in enumerate(rows):
        a[i] = tuple(F(x) for x in r)
    return a


def assert_bytes_equal(got, want, what):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gb, wb = got.view(np.uint8).reshape(got.size, -1), want.view(np.uint8).reshape(want.size, -1)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} records differ; first at {i}:\n got  {got[i]}\n want {want[i]}")


# ------------------------------------------------------------------------------------------------------
# point sets
# ------------------------------------------------------------------------------------------------------
def mixed_points(hs, n, seed, surface=None):
    """n POINT records: inside the root box, far outside it, exactly on vertices (and sphere / disc centres), on surfaces
    (`surface`: [K, 3] positions, e.g. the hit points of a cast; fewer when None), radii mixed among +inf, 1 % of the root box's
    diagonal and 0."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(hs.nodes)
    size = (hi - lo).astype(F)
    diag = F(np.linalg.norm(size))
    pos = rng.uniform(lo, hi, (n, 3)).astype(F)
    k = n // 5
    pos[:k] = rng.uniform(lo - 3 * size, hi + 3 * size, (k, 3)).astype(F)                       # far outside (mostly)
    verts = np.stack([hs.verts[c] for c in "xyz"], 1).astype(F)
    anchors = [verts] if len(verts) else []
    if hs.spheres.size:
        anchors.append(np.stack([hs.spheres[c] for c in "xyz"], 1).astype(F))
    if hs.discs.size:
        anchors.append(np.stack([hs.discs[c] for c in ("cx", "cy", "cz")], 1).astype(F))
    anchors = np.concatenate(anchors)
    pos[k:2 * k] = anchors[rng.integers(0, len(anchors), k)]                                    # exactly on vertices / centres
    if surface is not None and len(surface):
        s = np.asarray(surface, F)
        pos[2 * k:3 * k] = s[rng.integers(0, len(s), k)]
    radius = rng.choice(np.array([np.inf, 0.01 * diag, 0.0], F), n, p=[0.5, 0.4, 0.1]).astype(F)
    rng.shuffle(pos, axis=0)
    return qb.make_points(pos, radius)
