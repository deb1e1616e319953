"""Oriented-box queries on the host (no GPU): mi_obox_query_host / mi_obox_offsets_host / mi_obox_fill_host, the twins the device
results are compared with byte for byte (tests/test_obox_gpu.py), against the checker of tests/obox_cases.py - the contract's text
in numpy binary32 -, against mi_box_*_host under the 24 exact rotations, against a float64 reference that shares no code, and at
the edges of contact, containment, validity, monotonicity, order and caller-supplied offsets."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import box_cases as bc
import obox_cases as oc

F = np.float32
CONTAINED = irl.OVERLAP_CONTAINED
IDENT = (0.0, 0.0, 0.0, 1.0)
Z90 = (0.0, 0.0, 1.0, 1.0)                                        # a quarter turn about z: not unit, qq = 2, s = 1, all exact
Z45 = (0.0, 0.0, float(np.sin(np.pi / 8)), float(np.cos(np.pi / 8)))


def _listed(desc, centre, half, quat):
    """The (geomID, primID, flags) the twin lists for one oriented box, and its any / count answers checked against the list."""
    bx = oc.oboxes([(centre, half, quat)])
    offsets, recs = oc.full(desc, bx)
    assert irl.obox_query_host(desc, oc.COUNT, bx)[0][0] == recs.size and bool(irl.obox_query_host(desc, oc.ANY, bx)[0][0]) == (recs.size > 0)
    assert np.all(recs["box"] == 0) and np.all(recs["reserved"] == 0)
    return [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in recs]


def _box_listed(desc, lo, hi):
    bx = bc.boxes([(lo, hi)])
    offsets, _ = irl.box_offsets_host(desc, bx)
    recs, _ = irl.box_fill_host(desc, bx, offsets)
    return [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in recs]


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "spheres", "box"])
def test_twin_equals_the_checker(name):
    hs, bx, offsets, recs, counts, anys, v = oc.twin(name)
    ck = oc.OBoxChecker(hs)
    res = [ck.overlaps(b) for b in bx]
    lists = [r[0] for r in res]
    want_counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_counts), "offsets are the running total of the counts"
    oc.assert_same((offsets, recs), oc.packed(lists), f"{name}: the full lists")
    assert np.array_equal(counts, want_counts.astype(np.uint32)) and np.array_equal(anys, want_counts > 0)
    walk = (sum(r[1] for r in res), sum(r[2] for r in res))
    assert (v["offsets"]["box_tests"], v["offsets"]["prim_evals"]) == walk, "the count walk's visits"
    assert (v["count"]["box_tests"], v["count"]["prim_evals"]) == walk
    kept = [r for r in res if r[0]]
    assert (v["fill"]["box_tests"], v["fill"]["prim_evals"]) == (sum(r[1] for r in kept), sum(r[2] for r in kept)), "the fill's visits"
    first = [ck.walk(b, first_only=True) for b in bx]
    assert (v["any"]["box_tests"], v["any"]["prim_evals"]) == (sum(r[1] for r in first), sum(r[2] for r in first)), "ANY stops at the first accept"
    assert np.array_equal(recs["box"], np.repeat(np.arange(bx.size, dtype=np.uint32), want_counts.astype(np.int64)))
    assert np.all((recs["flags"] == 0) | (recs["flags"] == CONTAINED)) and np.all(recs["reserved"] == 0)
    # the hand-placed queries: the six that are not valid find nothing and are not walked; the others are
    k = bx.size - oc.SPECIAL
    for j in (0, 1, 2, 3, 4, 11):
        assert res[k + j] == ([], 0, 0) and counts[k + j] == 0, f"special {j} is not valid"
    for j in (5, 6, 7, 8, 9, 10, 12, 13):
        assert res[k + j][1] > 0, f"special {j} is walked"
    total = sum(1 for lf in ck.leaf if lf is not None)
    assert counts[k + 9] == total, "the box spanning the scene lists every primitive"
    if name == "soup":
        assert total == 602
        kinds = {int(hs.geometry[g]["type"]) for g in np.unique(recs["geomID"])}
        assert kinds == {0, 1, 2}, "triangles, the sphere and the disc are all listed somewhere"
        assert (recs["flags"] == CONTAINED).sum() > 20 and (recs["flags"] == 0).sum() > 20
        hist = np.bincount(np.minimum(want_counts, 24).astype(np.int64), minlength=25)
        print(f"{name}: oriented boxes with 0 / 1-9 / 10-23 / 24+ primitives: {hist[0]} / {hist[1:10].sum()} / {hist[10:24].sum()} / {hist[24]}")
        assert hist[0] > 10 and hist[1:24].sum() > 10 and hist[24] > 10, "the boxes span none, a few and dozens of primitives"


def test_a_scaled_quaternion_is_the_same_rotation():
    """On dyadic inputs a quaternion scaled by 1024 (a norm of about 1e3) lists the bytes of the unscaled one: s is exact in both."""
    hs = oc.dyadic_scene()
    rows, scaled = [], []
    for q, _ in oc.cube_rotations():
        rows.append(((0.5, -1.0, 0.5), (3.0, 1.5, 5.0), q))
        scaled.append(((0.5, -1.0, 0.5), (3.0, 1.5, 5.0), tuple(1024.0 * v for v in q)))
    a, b = oc.full(hs.desc, oc.oboxes(rows)), oc.full(hs.desc, oc.oboxes(scaled))
    assert a[0][-1] > 100
    oc.assert_same(b, a, "quaternions scaled by 1024")
    # the identity scaled by 1000: every off-diagonal term is an exact zero whatever s rounds to
    a = oc.full(hs.desc, oc.oboxes([((0.5, -1.0, 0.5), (3.0, 1.5, 5.0), IDENT)]))
    b = oc.full(hs.desc, oc.oboxes([((0.5, -1.0, 0.5), (3.0, 1.5, 5.0), (0.0, 0.0, 0.0, 1000.0))]))
    oc.assert_same(b, a, "the identity scaled by 1000")


# ------------------------------------------------------------------------------------------------------
# exact rotations: mi_box_*_host's bytes
# ------------------------------------------------------------------------------------------------------
def test_the_24_cube_rotations_return_the_box_familys_bytes():
    hs = oc.dyadic_scene()
    d = hs.desc
    rng = np.random.default_rng(72)
    listed = contained = 0
    for q, absR in oc.cube_rotations():
        centre = (rng.integers(-12, 13, (12, 3)) * 0.5).astype(F)
        half = (rng.integers(0, 13, (12, 3)) * 0.5).astype(F)
        world = (half.astype(np.float64) @ absR.T).astype(F)           # the half extents permuted: |R| half
        ob = oc.oboxes(zip(centre, half, [q] * 12))
        ab = bc.boxes(zip(centre - world, centre + world))
        for what, got, want in (("offsets", irl.obox_offsets_host(d, ob), irl.box_offsets_host(d, ab)),
                                ("count", irl.obox_query_host(d, oc.COUNT, ob), irl.box_query_host(d, bc.COUNT, ab)),
                                ("any", irl.obox_query_host(d, oc.ANY, ob), irl.box_query_host(d, bc.ANY, ab))):
            assert np.array_equal(got[0], want[0]), f"{q}: {what}"
            assert got[1] == want[1], f"{q}: the visits of {what}: the slabs pass exactly what the six compares pass"
        offsets = irl.obox_offsets_host(d, ob)[0]
        got, vg = irl.obox_fill_host(d, ob, offsets)
        want, vw = irl.box_fill_host(d, ab, offsets)
        pc.assert_bytes_equal(got, want, f"{q}: the lists, flags included")
        assert vg == vw
        listed += got.size
        contained += int((got["flags"] == CONTAINED).sum())
    assert listed > 1000 and contained > 100 and contained < listed


# ------------------------------------------------------------------------------------------------------
# a hand-made catalogue
# ------------------------------------------------------------------------------------------------------
def test_a_turned_box_drops_the_corners_of_its_bounds():
    """A box of half extents (2, 2, 1) turned 45 degrees about z: its world bounds reach 2.83 on x and y, and what lies in their
    corners - a triangle, a sphere, a disc - is listed by mi_box_* on the bounds and not by this family."""
    w = 2.0 * np.sqrt(2.0)
    tri = ((2.3, 2.3, 0.0), (2.7, 2.4, 0.0), (2.4, 2.7, 0.5))
    for kw in ({"tris": [tri]}, {"spheres": [(2.5, 2.5, 0.0, 0.25)]}, {"discs": [(0.0, 0.0, 1.0, 0.25, 2.5, -2.5, 0.0)]}):
        hs = pc.hand_scene(**kw)
        assert _box_listed(hs.desc, (-w, -w, -1.0), (w, w, 1.0)) == [(0, 0, CONTAINED)], kw
        assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), Z45) == [], kw
        assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), IDENT) == [], kw          # (nor by the box before it is turned)
        assert _listed(hs.desc, (0.0, 0.0, 0.0), (4.0, 4.0, 1.0), Z45) == [(0, 0, CONTAINED)], kw
    # along the diagonal the turned box reaches 2 (1.41, 1.41), the unturned one does not
    hs = pc.hand_scene(tris=[((1.3, 1.3, 0.0), (1.4, 1.3, 0.0), (1.3, 1.4, 0.0))])
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 0.1, 1.0), Z45) == [(0, 0, CONTAINED)]
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 0.1, 1.0), IDENT) == []
    # a margin either side of the 45-degree face x + y = 2 sqrt 2 (the rotation itself is rounded: no exact contact to ask for)
    for off, want in ((-1e-4, [(0, 0, 0)]), (1e-4, [])):
        p = np.sqrt(2.0) + off
        hs = pc.hand_scene(tris=[((p, p, 0.0), (p + 1.0, p + 0.5, 0.0), (p + 0.5, p + 1.0, 0.0))])
        assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), Z45) == want, off


def test_contact_counts_on_a_turned_box():
    """A quarter turn about z is exact: the box of half extents (2, 1, 1) about (1, 1, 0) covers [0, 2] x [-1, 3] x [-1, 1]."""
    c, h = (1.0, 1.0, 0.0), (2.0, 1.0, 1.0)
    up = float(np.nextafter(F(2), F(3)))
    # a face: the triangle lies in the plane x = 2
    hs = pc.hand_scene(tris=[((2.0, 0.0, -0.5), (2.0, 1.0, -0.5), (2.0, 0.0, 0.5))])
    assert _listed(hs.desc, c, h, Z90) == [(0, 0, CONTAINED)]
    assert _listed(hs.desc, c, h, IDENT) == [(0, 0, CONTAINED)]                  # (unturned it covers [-1, 3] x [0, 2])
    hs = pc.hand_scene(tris=[((up, 0.0, -0.5), (up, 1.0, -0.5), (up, 0.0, 0.5))])
    assert _listed(hs.desc, c, h, Z90) == [] and _listed(hs.desc, c, h, IDENT) == [(0, 0, CONTAINED)]
    # an edge: the triangle's edge on the box's edge x = 2, z = 1
    hs = pc.hand_scene(tris=[((2.0, 0.0, 1.0), (2.0, 2.0, 1.0), (3.0, 1.0, 2.0))])
    assert _listed(hs.desc, c, h, Z90) == [(0, 0, 0)]
    # a vertex: the triangle's vertex on the box's corner (2, 3, 1)
    hs = pc.hand_scene(tris=[((2.0, 3.0, 1.0), (3.0, 4.0, 1.0), (3.0, 3.0, 2.0))])
    assert _listed(hs.desc, c, h, Z90) == [(0, 0, 0)]
    hs = pc.hand_scene(tris=[((up, 3.0, 1.0), (3.0, 4.0, 1.0), (3.0, 3.0, 2.0))])
    assert _listed(hs.desc, c, h, Z90) == []
    # the hypotenuse passes the corner (2, 3) of the turned box outside: only an edge axis in the box's frame tells
    hs = pc.hand_scene(tris=[((1.5, 4.0, 0.0), (3.5, 2.0, 0.0), (3.5, 4.0, 0.0))])
    assert _listed(hs.desc, c, h, Z90) == []
    hs = pc.hand_scene(tris=[((1.0, 4.0, 0.0), (3.0, 2.0, 0.0), (3.5, 4.0, 0.0))])
    assert _listed(hs.desc, c, h, Z90) == [(0, 0, 0)]                             # (through the corner)


def test_sphere_shell_and_contained():
    hs = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 5.0)])
    d = hs.desc
    # a flat box of half extents (2, 1.5, 0) about (1.5, 2, 0), a quarter turn: [0, 3] x [0, 4]. Its farthest corner lies on the shell:
    # reached from inside only
    assert _listed(d, (1.5, 2.0, 0.0), (2.0, 1.5, 0.0), Z90) == [(0, 0, 0)]
    assert _listed(d, (1.5, 2.0, 0.0), (2.0 - 2.0 ** -21, 1.5, 0.0), Z90) == []      # (fy = 2 + half.x must round below 4: four ulps of 2)
    assert _listed(d, (1.5, 2.0, 0.0), (2.0, 1.5, 0.0), IDENT) == []                # unturned: [-0.5, 3.5] x [0.5, 3.5], wholly inside
    assert _listed(d, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), Z45) == []                  # wholly inside, away from the shell
    assert _listed(d, (0.0, 0.0, 0.0), (5.0, 5.0, 5.0), Z90) == [(0, 0, CONTAINED)]  # closed
    assert _listed(d, (0.0, 0.0, 0.0), (8.0, 8.0, 8.0), Z45) == [(0, 0, CONTAINED)]
    assert _listed(d, (7.0, 0.0, 0.0), (1.0, 3.0, 1.0), Z90) == [(0, 0, 0)]          # half (1, 3, 1) turned covers x in [4, 10]: it crosses the shell
    assert _listed(d, (7.0, 0.0, 0.0), (1.0, 3.0, 1.0), IDENT) == []                 # unturned x in [6, 8]: outside
    # CONTAINED of a triangle is exact: on the faces of the turned box, and one ulp off
    tri = ((2.0, -1.0, -1.0), (2.0, 3.0, 1.0), (0.0, 3.0, -1.0))
    hs = pc.hand_scene(tris=[tri])
    assert _listed(hs.desc, (1.0, 1.0, 0.0), (2.0, 1.0, 1.0), Z90) == [(0, 0, CONTAINED)]
    assert _listed(hs.desc, (1.0, 1.0, 0.0), (float(np.nextafter(F(2), F(1))), 1.0, 1.0), Z90) == [(0, 0, 0)]
    # a triangle whose WORLD bounds stick out of the turned box's world bounds nowhere, but whose vertex lies outside the box: not CONTAINED
    # (the turned square cuts the diagonal at 2: (1.6, 1.6) lies 2.26 out)
    hs = pc.hand_scene(tris=[((0.0, 0.0, 0.0), (1.6, 1.6, 0.0), (0.0, 1.0, 0.0))])
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), Z45) == [(0, 0, 0)]
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), (0.0, 0.0, 0.0, 2.0)) == [(0, 0, CONTAINED)]      # (unturned it holds the vertex)
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (3.0, 3.0, 1.0), Z45) == [(0, 0, CONTAINED)]


def test_a_slab_prunes_a_subtree_the_bounds_meet():
    """Root -> (leaf t0, interior -> (leaf t1, leaf t2)): t1 and t2 lie in a corner of the turned box's world bounds. The six compares
    meet the interior node's box, the slab along (1, 1, 0) separates it: 3 box tests and 1 primitive test, where mi_box_* on the
    bounds makes 5 and 3."""
    t0 = ((-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0))
    t1 = ((2.3, 2.3, 0.0), (2.5, 2.3, 0.0), (2.3, 2.5, 0.0))
    t2 = ((2.6, 2.6, 0.0), (2.8, 2.6, 0.0), (2.6, 2.8, 0.0))
    hs = pc.hand_scene(tris=[t0, t1, t2])
    bb = [(np.array(t, F).min(0), np.array(t, F).max(0)) for t in (t0, t1, t2)]
    inner = (np.minimum(bb[1][0], bb[2][0]), np.maximum(bb[1][1], bb[2][1]))
    root = (np.minimum(bb[0][0], inner[0]), np.maximum(bb[0][1], inner[1]))
    nodes = np.array([pc.compact_node(*root, 2), pc.compact_node(*bb[0], 0, 0), pc.compact_node(*inner, 4), pc.compact_node(*bb[1], 0, 1),
                      pc.compact_node(*bb[2], 0, 2)])
    desc = pc.with_nodes(hs.desc, nodes)
    ob = oc.oboxes([((0.0, 0.0, 0.0), (2.0, 2.0, 1.0), Z45)])
    q = oc.Query32(ob[0])
    assert q.valid and (inner[0] <= q.qmx).all() and (inner[1] >= q.qmn).all(), "the world bounds meet the second subtree"
    offsets, vo = irl.obox_offsets_host(desc, ob)
    recs, vf = irl.obox_fill_host(desc, ob, offsets)
    oc.assert_same((offsets, recs), oc.packed([[(0, 0, True)]]), "the one triangle inside")
    assert (vo["box_tests"], vo["prim_evals"]) == (3, 1) and (vf["box_tests"], vf["prim_evals"]) == (3, 1)
    ck = oc.OBoxChecker(hs, nodes)
    assert ck.overlaps(ob[0]) == ([(0, 0, True)], 3, 1)
    ab = bc.boxes([(q.qmn, q.qmx)])
    boffsets, vb = irl.box_offsets_host(desc, ab)
    assert boffsets[-1] == 3 and (vb["box_tests"], vb["prim_evals"]) == (5, 3)


# ------------------------------------------------------------------------------------------------------
# monotonicity, pinned directly
# ------------------------------------------------------------------------------------------------------
def test_a_box_that_contains_another_passes_whenever_that_one_does():
    """10^5 seeded pairs of nested bounds A >= B against random valid queries, magnitudes from 1e-3 to 1e6, through the function the
    kernels and the twins run: obox_meets_bounds(B) implies obox_meets_bounds(A). This is what makes a list the same bytes
    whatever tree is walked."""
    n = 100_000
    rng = np.random.default_rng(81)
    scale = (10.0 ** rng.uniform(-3.0, 6.0, (n, 1)))
    centre = (rng.uniform(-1, 1, (n, 3)) * scale).astype(F)
    half = (rng.uniform(0, 1, (n, 3)) * scale * 10.0 ** rng.uniform(-2.0, 0.0, (n, 1))).astype(F)
    quat = oc.random_quats(rng, n) * (10.0 ** rng.uniform(-3.0, 3.0, (n, 1))).astype(F)
    ob = oc.qb.make_oboxes(centre, half, quat=quat)
    # B: bounds near the query, so that it passes about half of the time; A: B grown by nothing, an ulp or a lot, side by side
    reach = half.max(1, keepdims=True).astype(np.float64)
    bc_ = centre + (rng.normal(size=(n, 3)) * reach * 0.8).astype(F)
    bh = (rng.uniform(0, 1, (n, 3)) * reach * 0.5).astype(F)
    b_mn, b_mx = (bc_ - bh).astype(F), (bc_ + bh).astype(F)
    grow = rng.choice(3, (2, n, 3))
    lots = (rng.uniform(0, 1, (2, n, 3)) * scale).astype(F)
    a_mn = np.where(grow[0] == 0, b_mn, np.where(grow[0] == 1, np.nextafter(b_mn, F(-np.inf)), b_mn - lots[0])).astype(F)
    a_mx = np.where(grow[1] == 0, b_mx, np.where(grow[1] == 1, np.nextafter(b_mx, F(np.inf)), b_mx + lots[1])).astype(F)
    assert (a_mn <= b_mn).all() and (a_mx >= b_mx).all()
    fn = irl.host_lib().mi_obox_meets_bounds_host
    arrays = [np.ascontiguousarray(x) for x in (ob, b_mn, b_mx, a_mn, a_mx)]
    po, pbn, pbx, pan, pax = (x.ctypes.data for x in arrays)
    passed = 0
    for i in range(n):
        if fn(po + 48 * i, pbn + 12 * i, pbx + 12 * i):
            passed += 1
            assert fn(po + 48 * i, pan + 12 * i, pax + 12 * i), f"pair {i}: the inner bounds pass and the outer ones do not"
    print(f"monotonicity: {passed} of {n} inner bounds pass")
    assert n // 10 < passed < n - n // 10
    # the exported helper is the checker's test
    for i in range(0, 2000):
        assert bool(fn(po + 48 * i, pbn + 12 * i, pbx + 12 * i)) == oc.Query32(ob[i]).meets(b_mn[i], b_mx[i]), i
    assert fn(None, pbn, pbx) == 0
    bad = ob[:1].copy()
    bad["quat"] = 0
    assert fn(bad.ctypes.data, pbn, pbx) == 0 and not irl.obox_meets_bounds_host(bad[0], b_mn[0], b_mx[0])


def test_order_does_not_depend_on_the_tree():
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    lbvh = irl.build_lbvh(hs.desc)[0]
    refit = irl.refit_compact_bvh(hs.desc)
    assert not np.array_equal(np.asarray(lbvh).view(np.uint8), np.asarray(hs.nodes).view(np.uint8)), "the LBVH is another tree"
    for what, nodes in (("the LBVH", lbvh), ("a refit of unchanged geometry", refit)):
        oc.assert_same(oc.full(pc.with_nodes(hs.desc, nodes), bx), (offsets, recs), what)
    assert np.all(np.diff(recs["geomID"].astype(np.int64) * (1 << 32) + recs["primID"])[np.diff(recs["box"].astype(np.int64)) == 0] > 0), "keys ascend strictly within a box"


# ------------------------------------------------------------------------------------------------------
# against float64
# ------------------------------------------------------------------------------------------------------
K_BOUND = 32


def test_id_sets_equal_a_float64_reference_that_shares_no_code():
    """Every (query, primitive) pair of the soup whose world bounds meet, against binary64: the triangle moved into the box's frame
    by a rotation matrix of its own and clipped against the six planes (the remainder is non-empty); the sphere from the box's
    closest and farthest points; the disc never missed, its over-listing counted. The twin must agree on every pair whose gap - the
    separation or the penetration depth over the 13 axes of the pair - exceeds K_BOUND x 2^-24 x M, M the largest coordinate
    magnitude of the pair, the box's corners included.
    Measured on this seeded set (12 826 pairs): the twin and the reference disagree on no pair at all, so the largest |gap| /
    (2^-24 M) among disagreeing pairs is 0 and K_BOUND stays the box family's 32; no pair is left out as unclear (0.00 %; at most
    5 % may be, which is asserted). Both figures are printed."""
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    pr = pc.primitives(hs)
    A, B, Cc, tg, tp = pr["tri"]
    sc, sr, sg = pr["sphere"]
    dn, dc, dr, dg = pr["disc"]
    scene_m = pc.scene_max_abs(hs)
    tri_mn, tri_mx = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    pairs = unclear = checked = disc_extra = 0
    worst = 0.0
    for i, ob in enumerate(bx):
        if not oc.Query32(ob).valid:
            assert offsets[i + 1] == offsets[i]
            continue
        Rt, c, h = oc.local64(ob)
        corners = oc.corners64(ob)
        wmn, wmx = corners.min(0), corners.max(0)
        mine = oc.ids(recs[int(offsets[i]):int(offsets[i + 1])])
        # triangles whose bounds meet the query's world bounds
        cand = np.nonzero((tri_mn <= wmx).all(1) & (tri_mx >= wmn).all(1))[0]
        if cand.size:
            la, lb, lc = (A[cand] - c) @ Rt.T, (B[cand] - c) @ Rt.T, (Cc[cand] - c) @ Rt.T
            gap = bc.tri_gap64(-h[None], h[None], la, lb, lc)[0]
            M = np.maximum(np.abs(corners).max(), np.maximum(np.abs(tri_mn[cand]), np.abs(tri_mx[cand])).max(1))
            bound = K_BOUND * pc.EPS * M
            for k, j in enumerate(cand):
                pairs += 1
                key = (int(tg[j]), int(tp[j]))
                touching = oc.clip_nonempty64([la[k], lb[k], lc[k]], h)
                if (key in mine) != touching:
                    worst = max(worst, abs(gap[k]) / (pc.EPS * M[k]))
                if abs(gap[k]) <= bound[k]:
                    unclear += 1
                    continue
                assert touching == (gap[k] <= 0), f"query {i}, triangle {key}: the clip and the axes disagree at gap {gap[k]}"
                assert (key in mine) == touching, f"query {i}, triangle {key}: gap {gap[k]}, bound {bound[k]}"
                checked += 1
        outside = {(int(tg[j]), int(tp[j])) for j in np.setdiff1d(np.arange(len(tg)), cand)}
        assert not (mine & outside), f"query {i}: a triangle outside the world bounds is listed"
        for j in range(len(sg)):
            if not ((sc[j] - sr[j] <= wmx).all() and (sc[j] + sr[j] >= wmn).all()):
                assert (int(sg[j]), 0) not in mine
                continue
            pairs += 1
            p = Rt @ (sc[j] - c)
            dmin = np.linalg.norm(p - np.clip(p, -h, h))
            dmax = np.linalg.norm(np.abs(p) + h)
            gap = max(dmin - sr[j], sr[j] - dmax)
            M = max(np.abs(corners).max(), (np.abs(sc[j]) + sr[j]).max())
            if (((int(sg[j]), 0) in mine) != (gap <= 0)):
                worst = max(worst, abs(gap) / (pc.EPS * M))
            if abs(gap) <= K_BOUND * pc.EPS * M:
                unclear += 1
                continue
            assert ((int(sg[j]), 0) in mine) == (gap <= 0), f"query {i}, sphere {j}: gap {gap}"
            checked += 1
        for j in range(len(dg)):
            ln, lc_ = Rt @ dn[j], Rt @ (dc[j] - c)
            gap, plane_gap = bc.disc_gap64(-h, h, ln, lc_, dr[j])
            M = max(np.abs(corners).max(), (np.abs(dc[j]) + dr[j]).max())
            if min(abs(gap), abs(plane_gap)) <= K_BOUND * pc.EPS * M:
                continue
            if gap <= 0:
                assert (int(dg[j]), 0) in mine, f"query {i}: a touching disc is missed"
            elif (int(dg[j]), 0) in mine:
                assert bc.disc_reach64(-h, h, ln, lc_, dr[j]) <= 2 * np.linalg.norm(h) * (1 + 1e-6) + K_BOUND * pc.EPS * M, f"query {i}: a listed disc is farther than the box's diagonal"
                disc_extra += 1
    share = unclear / pairs
    print(f"soup: {pairs} pairs whose world bounds meet, {checked} checked, {unclear} unclear ({100 * share:.2f} %), {disc_extra} discs listed within a "
          f"diagonal of the rim; the largest |gap| / (2^-24 M) among disagreeing pairs: {worst:.2f}")
    assert checked > 3000 and share <= 0.05
    assert worst <= K_BOUND / 2, "K_BOUND is at least twice the largest disagreement"


# ------------------------------------------------------------------------------------------------------
# the usual list rules
# ------------------------------------------------------------------------------------------------------
def test_invalid_queries_and_empty_scene():
    hs = bc.scene("soup")
    nan, inf = np.nan, np.inf
    h, q = (1.0, 1.0, 1.0), IDENT
    bx = oc.oboxes([((nan, 0, 0), h, q), ((0, inf, 0), h, q), ((0, 0, 0), (1, nan, 1), q), ((0, 0, 0), (1, 1, inf), q), ((0, 0, 0), (-1, 1, 1), q),
                    ((0, 0, 0), h, (0, 0, 0, 0)), ((0, 0, 0), h, (0, nan, 0, 1)), ((0, 0, 0), h, (inf, 0, 0, 1)), ((0, 0, 0), h, (1e-20, 0, 0, 1e-20)),
                    ((0, 0, 0), h, (0, 0, -0.0, 0.0)), ((0, 0, 0), h, (1e-30, 0, 0, 0))])
    offsets, vo = irl.obox_offsets_host(hs.desc, bx)
    assert not offsets.any() and (vo["box_tests"], vo["prim_evals"]) == (0, 0)
    for kind in (oc.ANY, oc.COUNT):
        out, v = irl.obox_query_host(hs.desc, kind, bx)
        assert not out.any() and (v["box_tests"], v["prim_evals"]) == (0, 0)
    recs, vf = irl.obox_fill_host(hs.desc, bx, oc.k_offsets(bx.size, 2))
    pc.assert_bytes_equal(recs, np.concatenate([oc.records([], i, 2) for i in range(bx.size)]), "padded segments of queries that are not walked")
    assert (vf["box_tests"], vf["prim_evals"]) == (0, 0)
    # the edges that ARE valid: a tiny and a huge quaternion whose s is finite, zero half extents, a huge finite box
    lo, hi = pc.root_box(hs.nodes)
    mid = tuple(((lo + hi) * F(0.5)).tolist())
    ok = oc.oboxes([(mid, (100.0, 100.0, 100.0), (1e-18, 0, 0, 0)), (mid, (100.0, 100.0, 100.0), (0, 1e18, 0, 0)), (mid, (1e30, 1e30, 1e30), (1, 2, 3, 4)),
                    (mid, (100.0, 100.0, 100.0), (3e38, 0, 0, 0))])
    assert irl.obox_query_host(hs.desc, oc.COUNT, ok)[0].tolist() == [602, 602, 602, 602]          # (qq = inf gives s = 0: the identity)
    flat = oc.oboxes([(mid, (100.0, 100.0, 0.0), Z45), (mid, (100.0, 0.0, 0.0), Z45), (mid, (0.0, 0.0, 0.0), Z45)])
    counts = irl.obox_query_host(hs.desc, oc.COUNT, flat)[0]
    assert counts[0] > counts[1] >= counts[2], "a rectangle, a segment, a point"
    # an empty scene
    empty = irl.SceneDesc()
    one = oc.oboxes([((0, 0, 0), h, q)])
    assert not irl.obox_offsets_host(empty, one)[0].any() and not irl.obox_query_host(empty, oc.ANY, one)[0].any()
    recs, v = irl.obox_fill_host(empty, one, np.array([0, 3], np.uint64))
    pc.assert_bytes_equal(recs, oc.records([], 0, 3), "an empty scene pads")
    assert irl.obox_offsets_host(hs.desc, bx[:0])[0].tolist() == [0]


def test_caller_supplied_offsets_are_honoured():
    hs, bx, offsets, recs, _, _, _ = oc.twin("soup")
    n = bx.size
    counts = np.diff(offsets).astype(np.int64)
    for k in (1, 4):
        got, v = irl.obox_fill_host(hs.desc, bx, oc.k_offsets(n, k))
        want = np.concatenate([np.concatenate([recs[int(offsets[i]):int(offsets[i]) + min(k, int(counts[i]))], oc.records([], i, max(k - int(counts[i]), 0))]) for i in range(n)])
        pc.assert_bytes_equal(got, want, f"K = {k}: the head of the full list, padded")
    # decreasing pairs, a start at or past capacity, capacity cutting a segment in the middle; canaries everywhere else
    sub = np.nonzero(counts >= 6)[0][:6]
    assert sub.size == 6
    b6 = bx[sub]
    offs = np.array([0, 5, 3, 9, 30, 24, 12], np.uint64)      # segments [0, 5) [5, 3) - [3, 9) [9, 30) cut at 12 [30, 24) - [24, 12) -
    capacity = 12
    buf = oc.sentinel_buffer(40)
    got, v = irl.obox_fill_host(hs.desc, b6, offs, capacity=capacity, hits=buf)
    full = [recs[int(offsets[i]):int(offsets[i + 1])].copy() for i in sub]
    for j, f in enumerate(full):
        f["box"] = j
    pc.assert_bytes_equal(got[9:12], full[3][:3], "capacity cuts box 3's segment in the middle: the 3 smallest keys")
    pc.assert_bytes_equal(got[3:9], full[2][:6], "box 2")
    pc.assert_bytes_equal(got[0:3], full[0][:3], "box 0's head (box 2's segment overlaps its tail)")
    assert oc.is_sentinel(got[12:]).all(), "nothing at or past capacity"
    walked = irl.obox_offsets_host(hs.desc, b6[[0, 2, 3]])[1]
    assert (v["box_tests"], v["prim_evals"]) == (walked["box_tests"], walked["prim_evals"])
    offs = np.array([2, 4, 4, 4, 4, 4, 4], np.uint64)
    buf = oc.sentinel_buffer(8)
    got, _ = irl.obox_fill_host(hs.desc, b6, offs, hits=buf)
    assert oc.is_sentinel(got[:2]).all() and oc.is_sentinel(got[4:]).all()
    pc.assert_bytes_equal(got[2:4], full[0][:2], "a segment between canaries")
    # unaligned buffers are read and written as they lie
    raw = np.zeros(bx.nbytes + 1, np.uint8)
    raw[1:] = bx.view(np.uint8)
    off_raw = np.zeros(offsets.nbytes + 3, np.uint8)
    host = irl.host_lib()
    assert host.mi_obox_offsets_host(C.byref(hs.desc), raw.ctypes.data + 1, off_raw.ctypes.data + 3, n, None) == 0
    assert off_raw[3:].tobytes() == offsets.tobytes()
