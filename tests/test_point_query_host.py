"""Point queries on the host (no GPU): mi_point_query_host, the twin the device results are compared with byte for byte
(tests/test_point_query_gpu.py), against a float64 brute force over every primitive, against the contract's formulas restated in
numpy binary32 (exact expected bytes), and at the edges of radius, coordinates and scene."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import point_cases as pc

F = np.float32
CLOSEST, WITHIN = irl.POINT_CLOSEST, irl.POINT_WITHIN


def _closest(desc, pts):
    """The twin's CLOSEST result, with WITHIN == `found` checked for every case that goes through here."""
    out, _ = irl.point_query_host(desc, CLOSEST, pts)
    inside, _ = irl.point_query_host(desc, WITHIN, pts)
    found = out["primID"] != irl.INVALID_PRIM
    assert np.array_equal(inside, found), "WITHIN differs from CLOSEST found"
    assert np.all(out["flags"][found] == 0) and np.all(out["geomID"][~found] == irl.INVALID_GEOM)
    assert np.all(out["flags"][~found] == irl.FLAG_ESCAPED)
    return out


# ------------------------------------------------------------------------------------------------------
# the twin against a float64 brute force
# ------------------------------------------------------------------------------------------------------
def _surface_offset_points(hs, n, rng):
    """Points a short way off the interior of random triangles, along the face normal: barycentric weights at least 0.15 each (away
    from the edges neighbours share) and a height of 5 % of the triangle's shortest edge, so the nearest primitive is unique but
    for the rare point that another surface is as near to."""
    pr = pc.primitives(hs)
    A, B, Cc = pr["tri"][:3]
    t = rng.integers(0, len(A), n)
    w = 0.15 + 0.55 * rng.dirichlet(np.ones(3), n)
    a, b, c = A[t], B[t], Cc[t]
    nrm = np.cross(b - a, c - a)
    ln = np.linalg.norm(nrm, axis=1)
    ok = ln > 0
    edge = np.minimum(np.minimum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1)), np.linalg.norm(a - c, axis=1))
    pos = a * w[:, :1] + b * w[:, 1:2] + c * w[:, 2:] + nrm / np.where(ok, ln, 1.0)[:, None] * (0.05 * edge * rng.choice([-1.0, 1.0], n))[:, None]
    return pos[ok].astype(F)


def _brute_case(name):
    hs = pc.scene(name)
    rng = np.random.default_rng(5)
    lo, hi = pc.root_box(hs.nodes)
    size = hi - lo
    if name == "box":
        # 4032 triangles in closed meshes: a uniform point is as near to two triangles that share an edge as often as not, so the
        # points of this case lie off the triangles' interiors
        pos = _surface_offset_points(hs, 3000, rng)
    else:
        pos = rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (20000, 3)).astype(F)
    return hs, pos


@pytest.mark.parametrize("name", ["soup", "box", "spheres"])
def test_twin_against_float64_brute_force(name):
    hs, pos = _brute_case(name)
    out = _closest(hs.desc, qb.make_points(pos, np.inf))
    assert np.all(out["primID"] != irl.INVALID_PRIM)
    M = np.maximum(np.abs(pos.astype(np.float64)).max(1), pc.scene_max_abs(hs))
    bound = 32 * pc.EPS * M
    true, geom, prim, second = pc.brute_force(hs, pos, margin=4 * float(bound.max()))
    err = np.abs(out["dist"].astype(np.float64) - true)
    print(f"{name}: worst |dist - true| = {(err / (pc.EPS * M)).max():.2f} * 2^-24 * M")
    assert np.all(err <= bound)
    # the returned point: on the named primitive, and dist away from p
    q = np.stack([out["point"][c] for c in "xyz"], 1).astype(np.float64)
    on = pc.prim_dist64(hs, q, out["geomID"], out["primID"])
    away = np.abs(np.linalg.norm(pos.astype(np.float64) - q, axis=1) - out["dist"])
    print(f"{name}: point off its primitive by at most {(on / (pc.EPS * M)).max():.2f}, |p - point| off dist by at most {(away / (pc.EPS * M)).max():.2f} (* 2^-24 * M)")
    assert np.all(on <= bound) and np.all(away <= bound)
    # the named primitive is the brute force's, except where two true distances are nearer than the bound (at most 1 % of the points)
    tie = (second - true) < bound
    print(f"{name}: {tie.sum()} of {len(pos)} points excused as ties")
    assert tie.mean() <= 0.01
    same = (out["geomID"] == geom) & (out["primID"] == prim)
    assert np.all(same | tie), f"{(~same & ~tie).sum()} points name another primitive than the brute force"
    # barycentrics reproduce the point of a triangle
    tri = hs.geometry["type"][out["geomID"]] == 0
    assert np.all(out["b1"][~tri] == 0) and np.all(out["b2"][~tri] == 0)
    assert np.all(out["b1"][tri] >= 0) and np.all(out["b2"][tri] >= 0) and np.all(out["b1"][tri] + out["b2"][tri] <= 1 + 4 * pc.EPS)


# ------------------------------------------------------------------------------------------------------
# hand-made cases with exact expected bytes
# ------------------------------------------------------------------------------------------------------
TRI = ((1.0, 1.0, 0.0), (5.0, 1.5, 0.25), (2.0, 4.0, -0.5))       # a, b, c


def _tri_point(v, w, off=0.0):
    """a + ab v + ac w, moved `off` along the face normal (float64, then rounded: just a position)."""
    a, b, c = (np.array(x, np.float64) for x in TRI)
    n = np.cross(b - a, c - a); n /= np.linalg.norm(n)
    return tuple((a + (b - a) * v + (c - a) * w + n * off).astype(F))


# region -> a point in it: outside barycentrics for the vertex and edge regions, with a height above the plane
REGION_POINTS = {
    "A": _tri_point(-0.5, -0.5, 0.7), "B": _tri_point(1.6, -0.3, -0.4), "C": _tri_point(-0.3, 1.7, 0.2),
    "AB": _tri_point(0.4, -0.6, 0.5), "AC": _tri_point(-0.6, 0.45, -0.3), "BC": _tri_point(0.8, 0.8, 0.9),
    "face": _tri_point(0.3, 0.25, 1.3),
}
ON_POINTS = {"vertex": TRI[1], "edge": tuple((np.array(TRI[0], F) + np.array(TRI[2], F)) * F(0.5)), "on the face": _tri_point(0.25, 0.5, 0.0)}


def test_triangle_regions_exact_bytes():
    hs = pc.hand_scene(tris=[TRI])
    assert hs.desc.num_nodes == 1
    rows, want = [], []
    for name, p in {**REGION_POINTS, **ON_POINTS}.items():
        q, v, w, reg = pc.tri_closest32(*TRI, p)
        if name in REGION_POINTS:
            assert reg == name, f"the point made for region {name} lies in {reg}"
        rows.append(p + (np.inf,))
        want.append(pc.found_record(p, q, 0, 0, v, w))
    got = _closest(hs.desc, pc.points(rows))
    pc.assert_bytes_equal(got, np.array(want), "one triangle, a point per Voronoi region and on a vertex, an edge, the face")
    assert got["dist"][list(ON_POINTS).index("vertex") + len(REGION_POINTS)] == 0


def test_sphere_and_disc_exact_bytes():
    sph = (1.0, -2.0, 3.0, 1.5)
    hs = pc.hand_scene(spheres=[sph])
    ps = [(4.0, 0.5, 3.25), (1.25, -2.5, 3.5), (1.0, -2.0, 3.0)]                    # outside, inside, at the centre
    want = [pc.found_record(p, pc.sphere_closest32(sph[:3], sph[3], p), 0, 0) for p in ps]
    got = _closest(hs.desc, pc.points([p + (np.inf,) for p in ps]))
    pc.assert_bytes_equal(got, np.array(want), "a sphere: outside, inside, at the centre")
    assert tuple(got["point"][2]) == (F(2.5), F(-2.0), F(3.0)) and got["dist"][2] == F(1.5)
    assert got["dist"][1] < F(1.5)                                                  # inside: the distance to the shell

    nrm = np.array([1.0, 2.0, -2.0], F) / F(3.0)
    disc = (nrm[0], nrm[1], nrm[2], 2.0, 0.5, 0.25, -1.0)                            # n, r, c
    hs = pc.hand_scene(discs=[disc])
    c = np.array(disc[4:], np.float64)
    n64 = nrm.astype(np.float64)
    t = np.cross(n64, [0.0, 0.0, 1.0]); t /= np.linalg.norm(t)
    ps = [tuple((c + t * 0.7 + n64 * 1.1).astype(F)),          # above the interior
          tuple((c + t * 3.5 - n64 * 0.6).astype(F)),          # beyond the rim
          tuple((c + n64 * 2.0).astype(F)),                    # on the axis
          tuple((c + t * 5.0).astype(F))]                      # in the plane, outside
    want = [pc.found_record(p, pc.disc_closest32(disc[:3], disc[4:], disc[3], p), 0, 0) for p in ps]
    got = _closest(hs.desc, pc.points([p + (np.inf,) for p in ps]))
    pc.assert_bytes_equal(got, np.array(want), "a disc: above the interior, beyond the rim, on the axis, in the plane")
    assert abs(float(got["dist"][1]) - np.hypot(0.6, 1.5)) < 1e-5 and abs(float(got["dist"][3]) - 3.0) < 1e-5


def test_coincident_triangles_first_leaf_in_preorder_wins():
    hs = pc.hand_scene(tris=[TRI, TRI])
    lo = np.min(np.array(TRI, F), 0); hi = np.max(np.array(TRI, F), 0)
    p = REGION_POINTS["face"]
    q, v, w, _ = pc.tri_closest32(*TRI, p)
    for first in (0, 1):
        nodes = np.array([pc.compact_node(lo, hi, 2), pc.compact_node(lo, hi, 0, first), pc.compact_node(lo, hi, 0, 1 - first)])
        got = _closest(pc.with_nodes(hs.desc, nodes), pc.points([p + (np.inf,)]))
        pc.assert_bytes_equal(got, np.array([pc.found_record(p, q, first, 0, v, w)]), f"coincident triangles, geometry {first} first")


def test_triangle_collapsed_to_a_point():
    z = (2.0, -1.0, 0.5)
    hs = pc.hand_scene(tris=[(z, z, z)])
    p = (3.0, 1.0, 2.5)
    q, v, w, reg = pc.tri_closest32(z, z, z, p)
    assert reg == "A" and tuple(q) == tuple(F(x) for x in z)
    got = _closest(hs.desc, pc.points([p + (np.inf,), z + (np.inf,)]))
    pc.assert_bytes_equal(got, np.array([pc.found_record(p, q, 0, 0, v, w), pc.found_record(z, q, 0, 0, 0, 0)]), "a triangle collapsed to a point")
    assert got["dist"][0] == F(3.0) and got["dist"][1] == 0


# ------------------------------------------------------------------------------------------------------
# radius, coordinate and scene edges
# ------------------------------------------------------------------------------------------------------
def test_radius_and_coordinate_edges():
    hs = pc.hand_scene(tris=[TRI])
    p = REGION_POINTS["face"]
    q, v, w, _ = pc.tri_closest32(*TRI, p)
    found = pc.found_record(p, q, 0, 0, v, w)
    d2 = pc.dist2_32(p, q)
    # a radius whose square is exactly d2: a unit sphere from 3 away, d2 = 4
    sph = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 1.0)])
    on_axis = (3.0, 0.0, 0.0)                         # closest point (1, 0, 0), d2 = 4 exactly
    assert pc.dist2_32(on_axis, pc.sphere_closest32((0, 0, 0), 1.0, on_axis)) == F(4)
    got = _closest(sph.desc, pc.points([on_axis + (2.0,), on_axis + (np.nextafter(F(2), F(3)),), on_axis + (np.nextafter(F(2), F(1)),)]))
    want = np.array([pc.nothing_record(F(2)), pc.found_record(on_axis, (1.0, 0.0, 0.0), 0, 0), pc.nothing_record(np.nextafter(F(2), F(1)))])
    pc.assert_bytes_equal(got, want, "radius^2 == d2 is not found (strict); one ulp more is")
    nan, inf = F("nan"), F("inf")
    rows = [p + (0.0,), p + (-0.0,), p + (-1.0,), p + (-inf,), p + (nan,), p + (inf,), p + (np.sqrt(d2) * F(1.01),),
            (nan,) + p[1:] + (inf,), p[:1] + (inf,) + p[2:] + (inf,), p[:2] + (-inf, inf), (nan, nan, nan, nan)]
    want = [pc.nothing_record(r[3]) for r in rows]
    want[5] = found; want[6] = found
    got = _closest(hs.desc, pc.points(rows))
    pc.assert_bytes_equal(got, np.array(want), "radius 0, -0, negative, -inf, NaN, +inf, just enough; NaN and inf coordinates")
    assert np.signbit(got["dist"][1]) and np.isnan(got["dist"][4]) and got["dist"][3] == -inf
    # a point ON the primitive with radius 0: d2 = 0 is not below 0
    got = _closest(hs.desc, pc.points([TRI[0] + (0.0,), TRI[0] + (1e-10,)]))      # (1e-10 squared is still a binary32 number above 0)
    assert got["primID"][0] == irl.INVALID_PRIM and got["primID"][1] == 0 and got["dist"][1] == 0


def test_scene_edges():
    # an empty scene
    empty = irl.SceneDesc()
    pts = pc.points([(0.0, 0.0, 0.0, np.inf), (1.0, 2.0, 3.0, 5.0)])
    got = _closest(empty, pts)
    pc.assert_bytes_equal(got, np.array([pc.nothing_record(np.inf), pc.nothing_record(5.0)]), "empty scene")
    out, visits = irl.point_query_host(empty, CLOSEST, pts)
    assert visits == {"box_tests": 0, "prim_evals": 0}
    # no points
    out, visits = irl.point_query_host(empty, CLOSEST, pts[:0])
    assert out.size == 0 and visits == {"box_tests": 0, "prim_evals": 0}
    # one primitive: a single leaf root
    hs = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 1.0)])
    assert hs.desc.num_nodes == 1
    out, visits = irl.point_query_host(hs.desc, CLOSEST, pc.points([(0.0, 5.0, 0.0, np.inf), (0.0, 5.0, 0.0, 1.0)]))
    assert visits == {"box_tests": 2, "prim_evals": 1}
    pc.assert_bytes_equal(out, np.array([pc.found_record((0, 5, 0), (0, 1, 0), 0, 0), pc.nothing_record(1.0)]), "a single leaf root")


def test_visits_of_a_three_leaf_tree_counted_by_hand():
    """Three unit triangles in the plane z = 0 at x = 0, 10, 20; nodes 0 = root (second child 2), 1 = leaf A, 2 = interior (second
    child 4), 3 = leaf B, 4 = leaf C. Every point lies at z = 1 above a triangle's interior."""
    def tri(x):
        return ((x, 0.0, 0.0), (x + 1.0, 0.0, 0.0), (x, 1.0, 0.0))
    hs = pc.hand_scene(tris=[tri(0.0), tri(10.0), tri(20.0)])
    box = lambda x0, x1: ((x0, 0.0, 0.0), (x1, 1.0, 0.0))
    nodes = np.array([pc.compact_node(*box(0, 21), 2), pc.compact_node(*box(0, 1), 0, 0), pc.compact_node(*box(10, 21), 4),
                      pc.compact_node(*box(10, 11), 0, 1), pc.compact_node(*box(20, 21), 0, 2)])
    desc = pc.with_nodes(hs.desc, nodes)
    cases = [
        # above B, radius inf: root in (0 < inf); A evaluated, best = 9.25^2 + .. ; node 2 in (1 < best); B evaluated, best = 1;
        # C's box is 9.25^2 + 1 away: passed.                                                  5 box tests, 2 evaluations
        ((10.25, 0.25, 1.0, np.inf), (5, 2), 1),
        # the same point, radius 0.5: the root's box is 1 away, 1 < 0.25 fails.                1 box test, 0 evaluations
        ((10.25, 0.25, 1.0, 0.5), (1, 0), None),
        # above C, radius inf: root in; A evaluated (best about 411); node 2 in; B's box 9.25^2 + 1 away: in, B evaluated
        # (best about 86.6); C's box 1 away: in, C evaluated.                                  5 box tests, 3 evaluations
        ((20.25, 0.25, 1.0, np.inf), (5, 3), 2),
        # above A, radius 2: root in (1 < 4); A evaluated, best = 1; node 2's box 8.75^2 + 1 away: passed (its subtree with it).
        #                                                                                      3 box tests, 1 evaluation
        ((0.25, 0.25, 1.0, 2.0), (3, 1), 0),
    ]
    total = [0, 0]
    for row, (boxes, prims), winner in cases:
        out, visits = irl.point_query_host(desc, CLOSEST, pc.points([row]))
        assert (visits["box_tests"], visits["prim_evals"]) == (boxes, prims), row
        assert (None if out["primID"][0] == irl.INVALID_PRIM else int(out["geomID"][0])) == winner
        if winner is not None:
            assert out["dist"][0] == 1 and tuple(out["point"][0]) == (F(row[0]), F(row[1]), F(0))
        total[0] += boxes; total[1] += prims
    out, visits = irl.point_query_host(desc, CLOSEST, pc.points([c[0] for c in cases]))
    assert (visits["box_tests"], visits["prim_evals"]) == tuple(total) == (14, 6)
    # WITHIN stops at the first accept: above C with radius inf, A is accepted at once.        2 box tests, 1 evaluation
    inside, visits = irl.point_query_host(desc, WITHIN, pc.points([cases[2][0]]))
    assert inside[0] and (visits["box_tests"], visits["prim_evals"]) == (2, 1)


def test_refusals():
    hs = pc.hand_scene(tris=[TRI])
    lib = irl.host_lib()
    pts = pc.points([(0.0, 0.0, 0.0, 1.0)])
    out = np.zeros(1, irl.POINT_HIT)
    import ctypes as C
    bad = {"null desc": (None, 0, pts.ctypes.data, out.ctypes.data, 1), "unknown kind": (C.byref(hs.desc), 2, pts.ctypes.data, out.ctypes.data, 1),
           "null points": (C.byref(hs.desc), 0, None, out.ctypes.data, 1), "null out": (C.byref(hs.desc), 1, pts.ctypes.data, None, 1)}
    for what, args in bad.items():
        assert lib.mi_point_query_host(*args, None) == 1, what
        assert b"mi_point_query_host" in lib.mi_host_last_error(), what
    # nodes that are not a depth-first BVH2
    lo, hi = (0, 0, 0), (1, 1, 1)
    broken = np.array([pc.compact_node(lo, hi, 5), pc.compact_node(lo, hi, 0, 0), pc.compact_node(lo, hi, 0, 0)])
    with pytest.raises(irl.RaylibError, match="depth-first"):
        irl.point_query_host(pc.with_nodes(hs.desc, broken), CLOSEST, pts)
    with pytest.raises(irl.RaylibError, match="geomID out of range"):
        irl.point_query_host(pc.with_nodes(hs.desc, np.array([pc.compact_node(lo, hi, 0, 7)])), CLOSEST, pts)
