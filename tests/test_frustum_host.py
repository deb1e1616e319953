"""Frustum queries on the host (no GPU): mi_frustum_query_host / mi_frustum_offsets_host / mi_frustum_fill_host, the twins the
device results are compared with byte for byte (tests/test_frustum_gpu.py), against the checker of tests/frustum_cases.py - the
contract's text in numpy binary32 -, against a float64 reference that shares no code, and at the edges of contact, containment,
validity, monotonicity, order and caller-supplied offsets."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import box_cases as bc
import frustum_cases as fc

F = np.float32
CONTAINED = irl.OVERLAP_CONTAINED
UNIT = fc.cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def above(x):
    return float(np.nextafter(F(x), F(np.inf)))


def _listed(hs, planes, nodes=None):
    """The (geomID, primID, flags) the twin lists for one frustum, its any / count answers checked against the list, and the
    checker asked to confirm every one of them before it is asserted."""
    fr = fc.frusta([planes])
    desc = hs.desc if nodes is None else pc.with_nodes(hs.desc, nodes)
    offsets, recs = fc.full(desc, fr)
    assert irl.frustum_query_host(desc, fc.COUNT, fr)[0][0] == recs.size and bool(irl.frustum_query_host(desc, fc.ANY, fr)[0][0]) == (recs.size > 0)
    assert np.all(recs["box"] == 0) and np.all(recs["reserved"] == 0)
    got = [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in recs]
    want = [(g, p, CONTAINED if c else 0) for g, p, c in fc.FrustumChecker(hs, nodes).overlaps(fr[0])[0]]
    assert got == want, "the twin and the checker"
    return got


def _stage(planes, tri):
    """The stage of the triangle test that decides (1, 2, 3; 0 = none touches), from the checker."""
    with np.errstate(all="ignore"):
        return fc.Query32(fc.frusta([planes])[0]).tri(*(fc.v3(p) for p in tri))[2]


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "spheres", "box"])
def test_twin_equals_the_checker(name):
    hs, fr, offsets, recs, counts, anys, v = fc.twin(name)
    ck = fc.FrustumChecker(hs)
    res = [ck.overlaps(f) for f in fr]
    lists = [r[0] for r in res]
    want_counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_counts), "offsets are the running total of the counts"
    fc.assert_same((offsets, recs), fc.packed(lists), f"{name}: the full lists")
    assert np.array_equal(counts, want_counts.astype(np.uint32)) and np.array_equal(anys, want_counts > 0)
    walk = (sum(r[1] for r in res), sum(r[2] for r in res))
    assert (v["offsets"]["box_tests"], v["offsets"]["prim_evals"]) == walk, "the count walk's visits"
    assert (v["count"]["box_tests"], v["count"]["prim_evals"]) == walk
    kept = [r for r in res if r[0]]
    assert (v["fill"]["box_tests"], v["fill"]["prim_evals"]) == (sum(r[1] for r in kept), sum(r[2] for r in kept)), "the fill's visits"
    first = [ck.walk(f, first_only=True) for f in fr]
    assert (v["any"]["box_tests"], v["any"]["prim_evals"]) == (sum(r[1] for r in first), sum(r[2] for r in first)), "ANY stops at the first accept"
    assert np.array_equal(recs["box"], np.repeat(np.arange(fr.size, dtype=np.uint32), want_counts.astype(np.int64)))
    assert np.all((recs["flags"] == 0) | (recs["flags"] == CONTAINED)) and np.all(recs["reserved"] == 0)
    # the hand-placed queries: the two that are not valid find nothing and are not walked; the others are
    k = fr.size - fc.SPECIAL
    for j in fc.NOT_WALKED:
        assert res[k + j] == ([], 0, 0) and counts[k + j] == 0, f"special {j} is not valid"
    for j in fc.WALKED:
        assert res[k + j][1] > 0, f"special {j} is walked"
    leaves = [lf for lf in ck.leaf if lf is not None]
    everything = sorted((lf[2], lf[3]) for lf in leaves)
    for j in (fc.S_ALL, fc.S_HOLDS, fc.S_FAR):
        assert [(g, p) for g, p, _ in lists[k + j]] == everything, f"special {j} lists every primitive"
    assert all(c for _, _, c in lists[k + fc.S_ALL]) and all(c for _, _, c in lists[k + fc.S_HOLDS]), "and holds every one of them"
    assert res[k + fc.S_ZERO_NEG] == ([], 1, 0), "a zero normal with d < 0: valid, empty by the arithmetic - the root box is separated"
    # contradictory planes (x >= mid + 1, x <= mid - 1): no triangle is listed; a sphere or a disc wider than the gap, which no
    # single plane has behind it, is - the documented conservatism
    assert all(int(hs.geometry[g]["type"]) != 0 for g, _, _ in lists[k + fc.S_CONTRA]) and res[k + fc.S_CONTRA][1] > 1
    base = fc.frusta([fc.cube(*_inner(hs))[:5]])[0]
    assert lists[k + fc.S_ZERO_MINUS0] == ck.overlaps(base)[0], "a zero normal with d = -0 is an absent plane"
    assert 0 < counts[k + fc.S_HALF] <= len(leaves) and (name == "spheres" or counts[k + fc.S_HALF] < len(leaves)), "the half-space through the middle lists a part of the scene"
    if name == "soup":
        assert len(leaves) == 602
        kinds = {int(hs.geometry[g]["type"]) for g in np.unique(recs["geomID"])}
        assert kinds == {0, 1, 2}, "triangles, the sphere and the disc are all listed somewhere"
        assert (recs["flags"] == CONTAINED).sum() > 20 and (recs["flags"] == 0).sum() > 20
        hist = np.bincount(np.minimum(want_counts, 24).astype(np.int64), minlength=25)
        print(f"{name}: frusta with 0 / 1-9 / 10-23 / 24+ primitives: {hist[0]} / {hist[1:10].sum()} / {hist[10:24].sum()} / {hist[24]}")
        assert hist[0] > 10 and hist[1:24].sum() > 10 and hist[24] > 10, "the frusta span none, a few and dozens of primitives"
    if name in ("soup", "box"):
        # the stages of the triangle test all decide somewhere: the soup's small triangles by a vertex or an edge, the box scene's
        # walls and floor - far larger than a tile of a view - by the region through the face
        stages = np.zeros(4, np.int64)
        with np.errstate(all="ignore"):
            for f in fr[::3]:
                q = fc.Query32(f)
                if q.valid:
                    for lf in leaves:
                        if lf[0] == 0:
                            V = np.array(lf[1], F)
                            if q.meets(V.min(0), V.max(0)):
                                stages[q.tri(fc.v3(V[0]), fc.v3(V[1]), fc.v3(V[2]))[2]] += 1
        print(f"{name}: triangles past their bounds decided by no stage / 1 / 2 / 3: {stages.tolist()}")
        assert (stages[:3] > 0).all() if name == "soup" else stages[3] > 0


def _inner(hs):
    lo, hi = pc.root_box(hs.nodes)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    size, mid = float((hi64 - lo64).max()), 0.5 * (lo64 + hi64)
    return mid - 0.2 * size, mid + 0.2 * size


# ------------------------------------------------------------------------------------------------------
# a catalogue by hand, on small integers and halves: every product below is exact
# ------------------------------------------------------------------------------------------------------
def test_the_unit_cube_as_six_planes_lists_what_the_box_query_lists():
    """Triangles on small integers around the cube [0, 2]^3: the six planes x >= 0, x <= 2, ... are the box's faces, the triangle test
    is exact on both sides and CONTAINED means the same - all three vertices in the closed cube."""
    tris = [((0, 0, 0), (1, 0, 0), (0, 1, 1)),          # inside, vertices on faces: contained
            ((1, 1, 1), (3, 1, 1), (1, 3, 1)),          # a vertex inside
            ((3, -1, 1), (-1, 3, 1), (3, 3, 1)),        # no vertex inside, the edge x + y = 2 crosses the cube
            ((3, 0, 1), (0, 3, 1), (3, 3, 1)),          # the edge x + y = 3 crosses the cube's corner region
            ((3, 2, 1), (2, 3, 1), (3, 3, 1)),          # the edge x + y = 5 misses; the vertex bounds touch the corner (2, 2)
            ((-4, -4, 1), (8, -4, 1), (-4, 8, 1)),      # the cube's cross-section lies inside the face
            ((2, 0, 0), (4, 0, 0), (4, 2, 2)),          # touches the face x = 2 at a vertex
            ((5, 5, 5), (6, 5, 5), (5, 6, 5)),          # far away
            ((-1, -1, -1), (-1, -1, 3), (3, 3, 1))]     # pierces the cube obliquely
    hs = pc.hand_scene(tris=tris)
    planes = fc.cube((0.0, 0.0, 0.0), (2.0, 2.0, 2.0))
    got = _listed(hs, planes)
    box = bc.boxes([((0.0, 0.0, 0.0), (2.0, 2.0, 2.0))])
    boffsets, _ = irl.box_offsets_host(hs.desc, box)
    brecs, _ = irl.box_fill_host(hs.desc, box, boffsets)
    assert got == [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in brecs]
    assert got == [(0, 0, CONTAINED), (1, 0, 0), (2, 0, 0), (3, 0, 0), (5, 0, 0), (6, 0, 0), (8, 0, 0)]


def test_a_vertex_on_a_plane_and_one_ulp_outside_it():
    """A = (1, 0.5, 0.5) lies on the face x = 1 of the unit cube: s = -1 + 1 = 0 >= 0, stage 1. An ulp beyond, the triangle's own
    bounds are behind that plane: up = -1.0000001 + 1 < 0."""
    t = ((1.0, 0.5, 0.5), (3.0, 0.5, 0.5), (3.0, 1.5, 0.5))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == [(0, 0, 0)] and _stage(UNIT, t) == 1
    t = ((above(1.0), 0.5, 0.5), (3.0, 0.5, 0.5), (3.0, 1.5, 0.5))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == []


def test_an_edge_across_a_corner_of_the_region():
    """In the plane z = 0.5 the edge from (1.5, 0.5) to (0.5, 1.5) passes through (1, 1), the cube's edge: against x <= 1 the ends
    have s = -0.5 and 0.5, t0 = 0.5; against y <= 1 they have 0.5 and -0.5, t1 = 0.5; t0 <= t1 and contact counts. No vertex is inside.
    With B an ulp higher the second cut is 0.5 / 1.0000001 < 0.5 and the edge misses; the other edges and the face miss too."""
    t = ((1.5, 0.5, 0.5), (0.5, 1.5, 0.5), (2.0, 2.0, 0.5))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == [(0, 0, 0)] and _stage(UNIT, t) == 2
    t = ((1.5, 0.5, 0.5), (0.5, above(1.5), 0.5), (2.0, 2.0, 0.5))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == [] and _stage(UNIT, t) == 0


COLUMN = fc.cube((-0.25, -0.25, -1.0), (0.25, 0.25, 1.0))


def test_a_thin_frustum_through_the_middle_of_a_large_triangle():
    """The column |x|, |y| <= 0.25 passes through the face of a triangle 20 across: no vertex in it, no edge near it; the planes
    x >= -0.25 and y >= -0.25 meet the triangle's plane at (-0.25, -0.25, 0), inside the other four planes and inside the triangle:
    stage 3. CONTAINED is not set."""
    t = ((-10.0, -10.0, 0.0), (10.0, -10.0, 0.0), (0.0, 10.0, 0.0))
    assert _listed(pc.hand_scene(tris=[t]), COLUMN) == [(0, 0, 0)] and _stage(COLUMN, t) == 3
    # the same with the far and near planes absent (an unbounded column), and with the triangle's winding reversed
    assert _listed(pc.hand_scene(tris=[t]), COLUMN[:4]) == [(0, 0, 0)]
    assert _listed(pc.hand_scene(tris=[(t[0], t[2], t[1])]), COLUMN) == [(0, 0, 0)]


def test_the_same_frustum_beside_the_triangle():
    """The right triangle with the hypotenuse x + y = 0 and the column about (5, 5): inside the triangle's bounds [-10, 10]^2, beyond
    the hypotenuse. Every corner of the cross-section fails the edge's triple product."""
    t = ((-10.0, -10.0, 0.0), (10.0, -10.0, 0.0), (-10.0, 10.0, 0.0))
    col = fc.cube((4.75, 4.75, -1.0), (5.25, 5.25, 1.0))
    q = fc.Query32(fc.frusta([col])[0])
    assert q.meets((-10, -10, 0), (10, 10, 0))
    assert _listed(pc.hand_scene(tris=[t]), col) == [] and _stage(col, t) == 0
    # moved under the face it is stage 3 again
    col = fc.cube((-5.25, -5.25, -1.0), (-4.75, -4.75, 1.0))
    assert _listed(pc.hand_scene(tris=[t]), col) == [(0, 0, 0)] and _stage(col, t) == 3
    # and a column that stops short of the triangle's plane touches nothing
    assert _listed(pc.hand_scene(tris=[t]), fc.cube((-5.25, -5.25, 0.5), (-4.75, -4.75, 1.0))) == []


def test_degenerate_triangles():
    seg = ((-1.0, 0.5, 0.5), (2.0, 0.5, 0.5), (2.0, 0.5, 0.5))
    assert _listed(pc.hand_scene(tris=[seg]), UNIT) == [(0, 0, 0)] and _stage(UNIT, seg) == 2, "a segment through the cube"
    seg = ((-1.0, 1.0, 0.5), (2.0, 1.0, 0.5), (-1.0, 1.0, 0.5))
    assert _listed(pc.hand_scene(tris=[seg]), UNIT) == [(0, 0, 0)], "a segment in the face y = 1"
    seg = ((-1.0, 0.5, 1.5), (2.0, 0.5, 1.5), (2.0, 0.5, 1.5))
    assert _listed(pc.hand_scene(tris=[seg]), UNIT) == [], "a segment above the cube"
    # a segment whose bounds pass - it runs beside the column diagonally - and that no stage accepts: m = 0 skips every pair
    seg = ((1.0, -0.5, 0.0), (-0.5, 1.0, 0.0), (1.0, -0.5, 0.0))
    assert fc.Query32(fc.frusta([COLUMN])[0]).meets((-0.5, -0.5, 0), (1, 1, 0))
    assert _listed(pc.hand_scene(tris=[seg]), COLUMN) == [(0, 0, 0)], "x + y = 0.5 crosses the column's corner (0.25, 0.25)"
    seg = ((1.5, -0.5, 0.0), (-0.5, 1.5, 0.0), (1.5, -0.5, 0.0))
    assert _listed(pc.hand_scene(tris=[seg]), COLUMN) == [] and _stage(COLUMN, seg) == 0, "x + y = 1 passes it"
    pt = ((0.5, 0.5, 0.5),) * 3
    assert _listed(pc.hand_scene(tris=[pt]), UNIT) == [(0, 0, CONTAINED)], "a point inside"
    pt = ((1.0, 1.0, 1.0),) * 3
    assert _listed(pc.hand_scene(tris=[pt]), UNIT) == [(0, 0, CONTAINED)], "a point on the corner"
    pt = ((1.0, 1.0, above(1.0)),) * 3
    assert _listed(pc.hand_scene(tris=[pt]), UNIT) == []


def test_contained_on_and_an_ulp_off():
    t = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 1.0))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == [(0, 0, CONTAINED)]
    t = ((0.0, 0.0, 0.0), (above(1.0), 0.0, 0.0), (0.0, 1.0, 1.0))
    assert _listed(pc.hand_scene(tris=[t]), UNIT) == [(0, 0, 0)]
    # a half-space holds whatever lies on its side; the plane itself belongs to it
    half = [(0.0, 0.0, -2.0, 2.0)]                                        # z <= 1, the normal not unit
    assert _listed(pc.hand_scene(tris=[t]), half) == [(0, 0, CONTAINED)]
    t = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, above(1.0)))
    assert _listed(pc.hand_scene(tris=[t]), half) == [(0, 0, 0)]


def test_a_sphere_outside_near_an_edge_is_listed_conservatively():
    """Centre (1.5, 1.5, 0.5), radius 0.625: the nearest point of the unit cube is its edge at (1, 1, 0.5), sqrt(0.5) = 0.707 away - the
    sphere does not touch. But no single plane has the whole ball behind it: against x <= 1 and y <= 1, s = -0.5 and s s = 0.25 is
    not above R R = 0.390625. Listed, the documented conservatism. With radius 0.5 the plane x <= 1 has it (s s = 0.25 > 0.25 fails:
    contact still lists; below 0.5 it rejects)."""
    hs = pc.hand_scene(spheres=[(1.5, 1.5, 0.5, 0.625)])
    assert _listed(hs, UNIT) == [(0, 0, 0)]
    N, d, _, _ = fc.planes64(fc.frusta([UNIT])[0])
    assert fc.region_distance64(np.array([1.5, 1.5, 0.5]), N, d) > 0.7
    assert _listed(pc.hand_scene(spheres=[(1.5, 1.5, 0.5, 0.5)]), UNIT) == [(0, 0, 0)]
    assert _listed(pc.hand_scene(spheres=[(1.5, 1.5, 0.5, below(0.5))]), UNIT) == []
    # a ball in front of a face touches exactly: centre (1.5, 0.5, 0.5), radius 0.5 reaches x = 1
    assert _listed(pc.hand_scene(spheres=[(1.5, 0.5, 0.5, 0.5)]), UNIT) == [(0, 0, 0)]
    # the whole ball in the region: CONTAINED on (s = 0.25 on every side, s s = R R) and an ulp off
    assert _listed(pc.hand_scene(spheres=[(0.5, 0.5, 0.5, 0.5)]), UNIT) == [(0, 0, CONTAINED)]
    assert _listed(pc.hand_scene(spheres=[(0.5, 0.5, 0.5, above(0.5))]), UNIT) == [(0, 0, 0)]


def test_a_region_strictly_inside_a_sphere_is_listed_conservatively():
    """The unit cube inside a sphere of radius 8 about its centre: its farthest corner is 0.866 from the centre, far from the shell,
    and queries see surfaces - nothing is touched. No plane rejects (s = 0.5 >= 0 on all six): listed, flags 0."""
    hs = pc.hand_scene(spheres=[(0.5, 0.5, 0.5, 8.0)])
    assert _listed(hs, UNIT) == [(0, 0, 0)]
    N, d, _, _ = fc.planes64(fc.frusta([UNIT])[0])
    assert fc.region_farthest64(np.array([0.5, 0.5, 0.5]), N, d, 1e6) < 0.87
    # a disc goes by its tight bounds and the ball of its radius: the unit disc in z = 0.5 about (1.5, 1.5) beside the cube's edge
    hs = pc.hand_scene(discs=[(0.0, 0.0, 1.0, 0.625, 1.5, 1.5, 0.5)])
    assert _listed(hs, UNIT) == [(0, 0, 0)]
    hs = pc.hand_scene(discs=[(0.0, 0.0, 1.0, 0.25, 0.5, 0.5, 0.5)])
    assert _listed(hs, UNIT) == [(0, 0, CONTAINED)]


def test_one_plane_prunes_the_second_subtree():
    """Root -> (leaf t0, interior -> (leaf t1, leaf t2)) and the half-space x <= 1: the root's box and t0's pass, the interior node's
    box (x from 2.3) lies behind the plane - up = -2.3 + 1 < 0 - and is passed with its two leaves: 3 box tests, 1 primitive test."""
    t0 = ((-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0))
    t1 = ((2.3, -2.5, 0.0), (2.5, -2.5, 0.0), (2.3, -2.3, 0.0))
    t2 = ((2.6, -2.8, 0.0), (2.8, -2.8, 0.0), (2.6, -2.6, 0.0))
    hs = pc.hand_scene(tris=[t0, t1, t2])
    bb = [(np.array(t, F).min(0), np.array(t, F).max(0)) for t in (t0, t1, t2)]
    inner = (np.minimum(bb[1][0], bb[2][0]), np.maximum(bb[1][1], bb[2][1]))
    root = (np.minimum(bb[0][0], inner[0]), np.maximum(bb[0][1], inner[1]))
    nodes = np.array([pc.compact_node(*root, 2), pc.compact_node(*bb[0], 0, 0), pc.compact_node(*inner, 4), pc.compact_node(*bb[1], 0, 1),
                      pc.compact_node(*bb[2], 0, 2)])
    desc = pc.with_nodes(hs.desc, nodes)
    fr = fc.frusta([[(-1.0, 0.0, 0.0, 1.0)]])
    q = fc.Query32(fr[0])
    assert q.valid and q.meets(*root) and not q.meets(*inner)
    offsets, vo = irl.frustum_offsets_host(desc, fr)
    recs, vf = irl.frustum_fill_host(desc, fr, offsets)
    fc.assert_same((offsets, recs), fc.packed([[(0, 0, True)]]), "the one triangle on the near side, held")
    assert (vo["box_tests"], vo["prim_evals"]) == (3, 1) and (vf["box_tests"], vf["prim_evals"]) == (3, 1)
    assert fc.FrustumChecker(hs, nodes).overlaps(fr[0]) == ([(0, 0, True)], 3, 1)
    # all six planes absent: every node, every leaf
    everything = fc.frusta([[]])
    assert irl.frustum_offsets_host(desc, everything)[1] == {"box_tests": 5, "prim_evals": 3}


def test_scaled_normals_list_the_same_bytes():
    """Every plane times 1024: every s, every product of the edge cuts' quotient and every numerator and det of a corner scale by a
    power of two, exactly. The queries whose planes are scaled by 1e-20 and 1e15 already are left as they are: their products
    underflow and overflow."""
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    scaled = fr.copy()
    k = fr.size - fc.SPECIAL
    keep = np.ones(fr.size, bool)
    keep[[k + fc.S_TINY, k + fc.S_HUGE]] = False
    scaled["planes"][keep] = fr["planes"][keep] * F(1024.0)
    fc.assert_same(fc.full(hs.desc, scaled), (offsets, recs), "normals scaled by 1024")


# ------------------------------------------------------------------------------------------------------
# monotonicity, pinned directly
# ------------------------------------------------------------------------------------------------------
def test_bounds_that_contain_other_bounds_pass_whenever_those_do():
    """10^5 seeded pairs of nested bounds A >= B against random valid queries, magnitudes from 1e-3 to 1e6, through the function the
    kernels and the twins run: frustum_meets_bounds(B) implies frustum_meets_bounds(A). This is what makes a list the same bytes
    whatever tree is walked."""
    n = 100_000
    rng = np.random.default_rng(201)
    scale = (10.0 ** rng.uniform(-3.0, 6.0, (n, 1)))
    centre = rng.uniform(-1, 1, (n, 3)) * scale
    normals = rng.normal(size=(n, 6, 3)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, 6, 1))
    normals[rng.uniform(size=(n, 6, 3)) < 0.1] = 0.0                                    # axis-parallel and zero normals among them
    through = centre[:, None, :] + rng.normal(size=(n, 6, 3)) * scale[:, None, :] * 0.5      # a point of each plane, near the centre
    d = -(normals * through).sum(-1)
    d[(normals == 0).all(-1)] = 0.0
    planes = np.concatenate([normals, d[:, :, None]], axis=2).astype(F)
    planes[rng.uniform(size=(n, 6)) < 0.4] = 0.0                                        # absent planes: about half of the inner bounds pass
    fr = fc.qb.make_frusta(planes=planes)
    bh = (rng.uniform(0, 1, (n, 3)) * scale * 0.3).astype(F)
    bc_ = (centre + rng.normal(size=(n, 3)) * scale * 0.3).astype(F)
    b_mn, b_mx = (bc_ - bh).astype(F), (bc_ + bh).astype(F)
    grow = rng.choice(3, (2, n, 3))
    lots = (rng.uniform(0, 1, (2, n, 3)) * scale).astype(F)
    a_mn = np.where(grow[0] == 0, b_mn, np.where(grow[0] == 1, np.nextafter(b_mn, F(-np.inf)), b_mn - lots[0])).astype(F)
    a_mx = np.where(grow[1] == 0, b_mx, np.where(grow[1] == 1, np.nextafter(b_mx, F(np.inf)), b_mx + lots[1])).astype(F)
    assert (a_mn <= b_mn).all() and (a_mx >= b_mx).all()
    fn = irl.host_lib().mi_frustum_meets_bounds_host
    arrays = [np.ascontiguousarray(x) for x in (fr, b_mn, b_mx, a_mn, a_mx)]
    po, pbn, pbx, pan, pax = (x.ctypes.data for x in arrays)
    passed = 0
    for i in range(n):
        if fn(po + 96 * i, pbn + 12 * i, pbx + 12 * i):
            passed += 1
            assert fn(po + 96 * i, pan + 12 * i, pax + 12 * i), f"pair {i}: the inner bounds pass and the outer ones do not"
    print(f"monotonicity: {passed} of {n} inner bounds pass")
    assert n // 10 < passed < n - n // 10
    # the exported helper is the checker's test
    for i in range(0, 2000):
        assert bool(fn(po + 96 * i, pbn + 12 * i, pbx + 12 * i)) == fc.Query32(fr[i]).meets(b_mn[i], b_mx[i]), i
    assert fn(None, pbn, pbx) == 0
    bad = fr[:1].copy()
    bad["planes"][0, 3, 2] = np.nan
    assert fn(bad.ctypes.data, pbn, pbx) == 0 and not irl.frustum_meets_bounds_host(bad[0], b_mn[0], b_mx[0])


def test_order_does_not_depend_on_the_tree():
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    lbvh = irl.build_lbvh(hs.desc)[0]
    refit = irl.refit_compact_bvh(hs.desc)
    assert not np.array_equal(np.asarray(lbvh).view(np.uint8), np.asarray(hs.nodes).view(np.uint8)), "the LBVH is another tree"
    for what, nodes in (("the LBVH", lbvh), ("a refit of unchanged geometry", refit)):
        fc.assert_same(fc.full(pc.with_nodes(hs.desc, nodes), fr), (offsets, recs), what)
    assert np.all(np.diff(recs["geomID"].astype(np.int64) * (1 << 32) + recs["primID"])[np.diff(recs["box"].astype(np.int64)) == 0] > 0), "keys ascend strictly within a frustum"


# ------------------------------------------------------------------------------------------------------
# against float64
# ------------------------------------------------------------------------------------------------------
K_BOUND = 32


def _pow2_at_least(x):
    k = 32
    while k < x:
        k *= 2
    return k


def _reference_pairs(hs, fr, far_own_scene=False):
    """Every (query, triangle) pair of a scene against the binary64 clip, banded by eps = k 2^-24 M, M the largest magnitude among
    the triangle's coordinates and the |d| / |n| of the present planes. Returns (held, worst): held = (query, key, listed by the
    checker, verdict at k: a function of k) rows, worst = the largest band a disagreeing pair needs, in units of 2^-24 M."""
    pr = pc.primitives(hs)
    A, B, Cc, tg, tp = pr["tri"]
    leaf = {(lf[2], lf[3]): lf for lf in fc.FrustumChecker(hs).leaf if lf is not None}
    tri_m = np.maximum(np.maximum(np.abs(A), np.abs(B)), np.abs(Cc)).max(1)
    rows = []
    for i, f in enumerate(fr):
        q = fc.Query32(f)
        if not q.valid:
            continue
        N, d, qm, empty = fc.planes64(f)
        for j in range(len(tg)):
            key = (int(tg[j]), int(tp[j]))
            M = max(qm, float(tri_m[j]))
            with np.errstate(all="ignore"):
                mine = q.touches(*leaf[key][:2])[0]
            rows.append((i, key, mine, N, d, empty, np.stack([A[j], B[j], Cc[j]]), M))
    return rows


def _verdict(row, k):
    i, key, mine, N, d, empty, poly, M = row
    if empty:
        return -1
    return fc.verdict64(poly, poly, N, d, k * pc.EPS * M)


def test_id_sets_equal_a_float64_reference_that_shares_no_code():
    """Every (query, primitive) pair of the soup against binary64: the triangle clipped against the six planes (Sutherland-Hodgman).
    A pair counts as touching when something is left with every plane moved inward by eps, as apart when nothing is left with every
    plane moved outward by eps, eps = k 2^-24 M, M the largest magnitude among the triangle's coordinates and the |d| / |n| of the
    present planes; every other pair is unclear and skipped.
    k is set by the CHECKER, as for the rigid poses: the smallest power of two, never below 32, at which no pair outside the band
    has the checker and the reference disagree. Measured on this seeded set (88 800 pairs): no pair outside the band disagrees at 32, so
    k stays the box family's 32; 79 pairs (0.09 %) are unclear (at most 5 % may be, which is asserted). The camera 1e19 away does
    not fill the band as the capsules' query did: its planes are that far from the scene and still hold all of it when moved by the
    band's width. Spheres and discs: every pair the reference calls touching is listed; the pairs
    listed although the reference calls them apart - the documented conservatism - are counted and printed (31 of 296)."""
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    rows = _reference_pairs(hs, fr)
    pairs = len(rows)
    k_bound = 32
    while True:
        bad = [r for r in rows if (v := _verdict(r, k_bound)) != 0 and r[2] != (v > 0)]
        if not bad or k_bound >= 1 << 20:
            break
        k_bound *= 2
    unclear = checked = 0
    for r in rows:
        i, key = r[0], r[1]
        v = _verdict(r, k_bound)
        if v == 0:
            unclear += 1
            continue
        listed = key in fc.ids(recs[int(offsets[i]):int(offsets[i + 1])])
        assert listed == (v > 0), f"query {i}, primitive {key}: the twin lists {listed}, the reference says {v}"
        checked += 1
    share = unclear / pairs
    # spheres and discs: never missed; over-listing counted
    pr = pc.primitives(hs)
    sc, sr, sg = pr["sphere"]
    dn, dc, dr, dg = pr["disc"]
    lo, hi = pc.root_box(hs.nodes)
    reach = 1e3 * float(np.abs(np.concatenate([lo, hi])).max())
    round_pairs = extra = 0
    for i, f in enumerate(fr):
        if not fc.Query32(f).valid:
            continue
        N, d, qm, empty = fc.planes64(f)
        mine = fc.ids(recs[int(offsets[i]):int(offsets[i + 1])])
        for j in range(len(sg)):
            key, c, R = (int(sg[j]), 0), sc[j], float(sr[j])
            eps = K_BOUND * pc.EPS * max(qm, float(np.abs(c).max()) + R)
            round_pairs += 1
            if empty:
                assert key not in mine
                continue
            dist, farthest = fc.region_distance64(c, N, d), fc.region_farthest64(c, N, d, reach)
            if dist <= R - eps and farthest >= R + eps:             # the region reaches the shell, from outside or from inside
                assert key in mine, f"query {i}: a touching sphere is missed"
            elif key in mine and (dist > R + eps or farthest < R - eps):
                extra += 1
        for j in range(len(dg)):
            key = (int(dg[j]), 0)
            eps = K_BOUND * pc.EPS * max(qm, float(np.abs(dc[j]).max()) + float(dr[j]))
            round_pairs += 1
            if empty:
                assert key not in mine
                continue
            inner, outer = fc.disc_polygons64(dn[j], dc[j], float(dr[j]))
            v = fc.verdict64(inner, outer, N, d, eps)
            if v > 0:
                assert key in mine, f"query {i}: a touching disc is missed"
            elif v < 0 and key in mine:
                extra += 1
    print(f"soup: {pairs} triangle pairs, {checked} checked, {unclear} unclear ({100 * share:.2f} %), k = {k_bound}; "
          f"{round_pairs} sphere and disc pairs, {extra} listed that are not touched")
    assert k_bound == K_BOUND, "the bound the checker needs is still the recorded one"
    assert checked > 3000 and share <= 0.05


# ------------------------------------------------------------------------------------------------------
# the usual list rules
# ------------------------------------------------------------------------------------------------------
def test_invalid_queries_and_empty_scene():
    hs = bc.scene("soup")
    rows = []
    for bad, (p, c) in zip((np.nan, np.inf, -np.inf, np.nan), ((0, 0), (1, 3), (5, 2), (3, 3))):
        pl = np.array(UNIT, F)
        pl[p, c] = bad
        rows.append(pl)
    fr = fc.frusta(rows)
    offsets, vo = irl.frustum_offsets_host(hs.desc, fr)
    assert not offsets.any() and (vo["box_tests"], vo["prim_evals"]) == (0, 0)
    for kind in (fc.ANY, fc.COUNT):
        out, v = irl.frustum_query_host(hs.desc, kind, fr)
        assert not out.any() and (v["box_tests"], v["prim_evals"]) == (0, 0)
    recs, vf = irl.frustum_fill_host(hs.desc, fr, fc.k_offsets(fr.size, 2))
    pc.assert_bytes_equal(recs, np.concatenate([fc.records([], i, 2) for i in range(fr.size)]), "padded segments of queries that are not walked")
    assert (vf["box_tests"], vf["prim_evals"]) == (0, 0)
    # the edges that ARE valid: no plane at all, a half-space that holds the scene, huge finite offsets, and the empty regions
    ok = fc.frusta([[], [(0, 0, 1, 1e30)], [(1, 0, 0, 3e38), (-1, 0, 0, 3e38)], [(0, 0, 0, 1.0)]])
    assert irl.frustum_query_host(hs.desc, fc.COUNT, ok)[0].tolist() == [602, 602, 602, 602]
    none = fc.frusta([[(0, 0, 0, -1.0)], [(0, 0, 1, -1e30)], [(1, 0, 0, -1e4), (-1, 0, 0, -1e4)]])
    counts, v = irl.frustum_query_host(hs.desc, fc.COUNT, none)
    assert counts.tolist() == [0, 0, 0] and (v["box_tests"], v["prim_evals"]) == (3, 0), "valid, walked, parted from the root box"
    # an empty scene
    empty = irl.SceneDesc()
    one = fc.frusta([UNIT])
    assert not irl.frustum_offsets_host(empty, one)[0].any() and not irl.frustum_query_host(empty, fc.ANY, one)[0].any()
    recs, v = irl.frustum_fill_host(empty, one, np.array([0, 3], np.uint64))
    pc.assert_bytes_equal(recs, fc.records([], 0, 3), "an empty scene pads")
    assert irl.frustum_offsets_host(hs.desc, fr[:0])[0].tolist() == [0]


def test_caller_supplied_offsets_are_honoured():
    hs, fr, offsets, recs, _, _, _ = fc.twin("soup")
    n = fr.size
    counts = np.diff(offsets).astype(np.int64)
    for k in (1, 4):
        got, v = irl.frustum_fill_host(hs.desc, fr, fc.k_offsets(n, k))
        want = np.concatenate([np.concatenate([recs[int(offsets[i]):int(offsets[i]) + min(k, int(counts[i]))], fc.records([], i, max(k - int(counts[i]), 0))]) for i in range(n)])
        pc.assert_bytes_equal(got, want, f"K = {k}: the head of the full list, padded")
    # decreasing pairs, a start at or past capacity, capacity cutting a segment in the middle; canaries everywhere else
    sub = np.nonzero(counts >= 6)[0][:6]
    assert sub.size == 6
    c6 = fr[sub]
    offs = np.array([0, 5, 3, 9, 30, 24, 12], np.uint64)      # segments [0, 5) [5, 3) - [3, 9) [9, 30) cut at 12 [30, 24) - [24, 12) -
    capacity = 12
    buf = fc.sentinel_buffer(40)
    got, v = irl.frustum_fill_host(hs.desc, c6, offs, capacity=capacity, hits=buf)
    full = [recs[int(offsets[i]):int(offsets[i + 1])].copy() for i in sub]
    for j, f in enumerate(full):
        f["box"] = j
    pc.assert_bytes_equal(got[9:12], full[3][:3], "capacity cuts frustum 3's segment in the middle: the 3 smallest keys")
    pc.assert_bytes_equal(got[3:9], full[2][:6], "frustum 2")
    pc.assert_bytes_equal(got[0:3], full[0][:3], "frustum 0's head (frustum 2's segment overlaps its tail)")
    assert fc.is_sentinel(got[12:]).all(), "nothing at or past capacity"
    walked = irl.frustum_offsets_host(hs.desc, c6[[0, 2, 3]])[1]
    assert (v["box_tests"], v["prim_evals"]) == (walked["box_tests"], walked["prim_evals"])
    offs = np.array([2, 4, 4, 4, 4, 4, 4], np.uint64)
    buf = fc.sentinel_buffer(8)
    got, _ = irl.frustum_fill_host(hs.desc, c6, offs, hits=buf)
    assert fc.is_sentinel(got[:2]).all() and fc.is_sentinel(got[4:]).all()
    pc.assert_bytes_equal(got[2:4], full[0][:2], "a segment between canaries")
    # unaligned buffers are read and written as they lie
    raw = np.zeros(fr.nbytes + 1, np.uint8)
    raw[1:] = fr.view(np.uint8)
    off_raw = np.zeros(offsets.nbytes + 3, np.uint8)
    host = irl.host_lib()
    assert host.mi_frustum_offsets_host(C.byref(hs.desc), raw.ctypes.data + 1, off_raw.ctypes.data + 3, n, None) == 0
    assert off_raw[3:].tobytes() == offsets.tobytes()
    hit_raw = np.full(recs.nbytes + 5, 0xEE, np.uint8)
    assert host.mi_frustum_fill_host(C.byref(hs.desc), raw.ctypes.data + 1, off_raw.ctypes.data + 3, hit_raw.ctypes.data + 5, recs.size, n, None) == 0
    assert hit_raw[5:].tobytes() == recs.tobytes() and (hit_raw[:5] == 0xEE).all()
    cnt_raw = np.zeros(4 * n + 1, np.uint8)
    assert host.mi_frustum_query_host(C.byref(hs.desc), fc.COUNT, raw.ctypes.data + 1, cnt_raw.ctypes.data + 1, n, None) == 0
    assert cnt_raw[1:].tobytes() == counts.astype(np.uint32).tobytes()
