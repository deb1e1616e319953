"""Capsule queries on the host (no GPU): mi_capsule_query_host / mi_capsule_offsets_host / mi_capsule_fill_host, the twins the
device results are compared with byte for byte (tests/test_capsule_gpu.py), against the checker of tests/capsule_cases.py - the
contract's text in numpy binary32 -, against a float64 reference that shares no code, and at the edges of contact, containment,
validity, monotonicity, order and caller-supplied offsets."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import box_cases as bc
import capsule_cases as cc

F = np.float32
CONTAINED = irl.OVERLAP_CONTAINED
TRI = ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))


def below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def above(x):
    return float(np.nextafter(F(x), F(np.inf)))


def _listed(hs, a, b, radius, nodes=None):
    """The (geomID, primID, flags) the twin lists for one capsule, its any / count answers checked against the list, and the
    checker asked to confirm every one of them before it is asserted."""
    cp = cc.capsules([(a, b, radius)])
    desc = hs.desc if nodes is None else pc.with_nodes(hs.desc, nodes)
    offsets, recs = cc.full(desc, cp)
    assert irl.capsule_query_host(desc, cc.COUNT, cp)[0][0] == recs.size and bool(irl.capsule_query_host(desc, cc.ANY, cp)[0][0]) == (recs.size > 0)
    assert np.all(recs["box"] == 0) and np.all(recs["reserved"] == 0)
    got = [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in recs]
    want = [(g, p, CONTAINED if c else 0) for g, p, c in cc.CapsuleChecker(hs, nodes).overlaps(cp[0])[0]]
    assert got == want, "the twin and the checker"
    return got


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "spheres", "box"])
def test_twin_equals_the_checker(name):
    hs, cp, offsets, recs, counts, anys, v = cc.twin(name)
    ck = cc.CapsuleChecker(hs)
    res = [ck.overlaps(c) for c in cp]
    lists = [r[0] for r in res]
    want_counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_counts), "offsets are the running total of the counts"
    cc.assert_same((offsets, recs), cc.packed(lists), f"{name}: the full lists")
    assert np.array_equal(counts, want_counts.astype(np.uint32)) and np.array_equal(anys, want_counts > 0)
    walk = (sum(r[1] for r in res), sum(r[2] for r in res))
    assert (v["offsets"]["box_tests"], v["offsets"]["prim_evals"]) == walk, "the count walk's visits"
    assert (v["count"]["box_tests"], v["count"]["prim_evals"]) == walk
    kept = [r for r in res if r[0]]
    assert (v["fill"]["box_tests"], v["fill"]["prim_evals"]) == (sum(r[1] for r in kept), sum(r[2] for r in kept)), "the fill's visits"
    first = [ck.walk(c, first_only=True) for c in cp]
    assert (v["any"]["box_tests"], v["any"]["prim_evals"]) == (sum(r[1] for r in first), sum(r[2] for r in first)), "ANY stops at the first accept"
    assert np.array_equal(recs["box"], np.repeat(np.arange(cp.size, dtype=np.uint32), want_counts.astype(np.int64)))
    assert np.all((recs["flags"] == 0) | (recs["flags"] == CONTAINED)) and np.all(recs["reserved"] == 0)
    # the hand-placed queries: the three that are not valid find nothing and are not walked; the others are
    k = cp.size - cc.SPECIAL
    for j in cc.NOT_WALKED:
        assert res[k + j] == ([], 0, 0) and counts[k + j] == 0, f"special {j} is not valid"
    for j in cc.WALKED:
        assert res[k + j][1] > 0, f"special {j} is walked"
    leaves = [lf for lf in ck.leaf if lf is not None]
    assert counts[k + 7] == len(leaves), "the capsule spanning the scene lists every primitive"
    assert counts[k + 9] >= sum(1 for lf in leaves if lf[0] == 0), "coordinates of 1e19: the segment tests turn NaN and every triangle is listed"
    if name == "soup":
        assert len(leaves) == 602
        kinds = {int(hs.geometry[g]["type"]) for g in np.unique(recs["geomID"])}
        assert kinds == {0, 1, 2}, "triangles, the sphere and the disc are all listed somewhere"
        assert (recs["flags"] == CONTAINED).sum() > 20 and (recs["flags"] == 0).sum() > 20
        hist = np.bincount(np.minimum(want_counts, 24).astype(np.int64), minlength=25)
        print(f"{name}: capsules with 0 / 1-9 / 10-23 / 24+ primitives: {hist[0]} / {hist[1:10].sum()} / {hist[10:24].sum()} / {hist[24]}")
        assert hist[0] > 10 and hist[1:24].sum() > 10 and hist[24] > 10, "the capsules span none, a few and dozens of primitives"


# ------------------------------------------------------------------------------------------------------
# a catalogue by hand, on small integers: every product below is exact
# ------------------------------------------------------------------------------------------------------
def test_a_triangle_at_the_radius_of_an_end():
    """(1, 1, 2)-(1, 1, 5) stands over the triangle's face: the end a is nearest, its foot is (1, 1, 0) - the face region,
    va = 128, vb = vc = 64, 1 / 256, v = w = 1 / 4 - at distance 2: dist2 = 4 = r2, and contact counts. An ulp less and r2 < 4; the edges
    lie at dist2 5, 6 and 5, and both ends lie on one side of the plane (sa = 32, sb = 80)."""
    hs = pc.hand_scene(tris=[TRI])
    assert _listed(hs, (1, 1, 2), (1, 1, 5), 2.0) == [(0, 0, 0)]
    assert _listed(hs, (1, 1, 2), (1, 1, 5), below(2.0)) == []


def test_a_bare_segment_pierces_touches_and_crosses():
    hs = pc.hand_scene(tris=[TRI])
    # through the face at (1, 1, 0): no end and no edge is at distance 0 (1, 1 and 1), sa = -16, sb = 16, w = (8, 16, 8)
    assert _listed(hs, (1, 1, -1), (1, 1, 1), 0.0) == [(0, 0, 0)]
    # the same line stopped short of the plane: sa, sb < 0
    assert _listed(hs, (1, 1, -2), (1, 1, -1), 0.0) == []
    # the line passes the triangle outside the hypotenuse, through (3, 3, 0): w = (24, -32, 24), signs differ
    assert _listed(hs, (3, 3, -1), (3, 3, 1), 0.0) == []
    # one end in the plane, inside the face: its distance is 0
    assert _listed(hs, (1, 1, 0), (1, 1, 3), 0.0) == [(0, 0, 0)]
    # coplanar, crossing the edge CA at (0, 1, 0): the end (1, 1, 0) lies in the face
    assert _listed(hs, (-1, 1, 0), (1, 1, 0), 0.0) == [(0, 0, 0)]
    # coplanar, both ends outside, crossing CA at (0, 2, 0) and BC at (2, 2, 0): against CA, s = 1 / 4 and t = 1 / 2 are exact
    assert _listed(hs, (-1, 2, 0), (3, 2, 0), 0.0) == [(0, 0, 0)]
    # coplanar and far: sa = sb = 0 and w = (0, 0, 0). This one is outside the triangle's bounds already ...
    assert _listed(hs, (10, 10, 0), (12, 10, 0), 0.0) == []
    # ... and this one is inside them, beyond the hypotenuse (x + y = 6 and 8): its bounds pass - the axis (1, -1, 0) does not part it
    # from the bounds' corner (4, 4) -, no end and no edge is at distance 0, and only the both-in-plane exclusion keeps the three zero
    # w from listing it
    q = cc.Query32(cc.capsules([((3, 3, 0), (4, 4, 0), 0.0)])[0])
    assert q.meets((0, 0, 0), (4, 4, 0))
    assert _listed(hs, (3, 3, 0), (4, 4, 0), 0.0) == []
    # lifted off the plane by an end it is still not listed (one side), pushed through it is not either (w's signs differ)
    assert _listed(hs, (3, 3, 1), (4, 4, 1), 0.0) == [] and _listed(hs, (3, 3, -1), (4, 4, 1), 0.0) == []


def test_a_segment_parallel_to_an_edge_at_three_four_five():
    """(1, -3, 4)-(3, -3, 4) runs along the edge AB (y = z = 0) at distance sqrt(9 + 16) = 5: the ends' feet are (1, 0, 0) and
    (3, 0, 0), dist2 = 25; against AB denom = 4 x 16 - 8 x 8 = 0, s = 0, t = 4 / 16, dist2 = 25."""
    hs = pc.hand_scene(tris=[TRI])
    assert _listed(hs, (1, -3, 4), (3, -3, 4), 5.0) == [(0, 0, 0)]
    assert _listed(hs, (1, -3, 4), (3, -3, 4), below(5.0)) == []
    # longer than the edge on both sides: the ends' feet are the vertices at dist2 26, the parallel branch finds 25
    assert _listed(hs, (-1, -3, 4), (5, -3, 4), 5.0) == [(0, 0, 0)]
    assert _listed(hs, (-1, -3, 4), (5, -3, 4), below(5.0)) == []


def test_sphere_shell_from_inside_and_outside():
    hs = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 8.0)])
    # a short capsule at the centre: m = 7 > 0 and dmax2 = 1 < 49 - wholly inside the ball, away from the shell
    assert _listed(hs, (0, 0, 0), (1, 0, 0), 1.0) == []
    # its far end reaches the shell from inside: dmax2 = 49 = m m
    assert _listed(hs, (0, 0, 0), (7, 0, 0), 1.0) == [(0, 0, 0)]
    assert _listed(hs, (0, 0, 0), (below(7.0), 0, 0), 1.0) == []
    # from outside at exactly R + radius: (6, 6, 3) is at distance 9, t = -81 <= 0, dmin2 = 81 = s s
    assert _listed(hs, (6, 6, 3), (12, 12, 6), 1.0) == [(0, 0, 0)]
    # an ulp farther: 36.000004 + 36 + 9 rounds above 81 (the bounds still meet: 5.0000005 <= 8)
    assert _listed(hs, (above(6.0), 6, 3), (12, 12, 6), 1.0) == []
    # the whole sphere inside the capsule: sqrtf(0) + 8 <= 8
    assert _listed(hs, (0, 0, 0), (1, 0, 0), 8.0) == [(0, 0, CONTAINED)]
    assert _listed(hs, (0, 0, 0), (1, 0, 0), below(8.0)) == [(0, 0, 0)]
    assert _listed(hs, (-3, 0, 0), (3, 0, 0), 8.0) == [(0, 0, CONTAINED)]


def test_contained_is_exact_for_a_triangle():
    """The capsule along AB with radius 4: A and B lie on the segment, C = (0, 4, 0) has t = 0 and dist2 = 16 = r2."""
    hs = pc.hand_scene(tris=[TRI])
    assert _listed(hs, (0, 0, 0), (4, 0, 0), 4.0) == [(0, 0, CONTAINED)]
    assert _listed(hs, (0, 0, 0), (4, 0, 0), below(4.0)) == [(0, 0, 0)]
    # one vertex an ulp outside
    hs = pc.hand_scene(tris=[((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, above(4.0), 0.0))])
    assert _listed(hs, (0, 0, 0), (4, 0, 0), 4.0) == [(0, 0, 0)]


def test_disc_is_conservative_and_the_slab_rejects():
    # the unit disc in the plane z = 0; a ball of radius 1 about (1.5, 0, 0.875) is sqrt(0.25 + 0.765625) = 1.0078 from the rim - it does
    # not touch - but its bounds meet, it stands in the plane's slab (0.875 <= 1) and it reaches the ball (3.015625 <= 4): listed, the
    # documented conservatism
    hs = pc.hand_scene(discs=[(0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0)])
    assert _listed(hs, (1.5, 0, 0.875), (1.5, 0, 0.875), 1.0) == [(0, 0, 0)]
    assert cc.disc_dist64(np.array([1.5, 0, 0.875]), np.array([1.5, 0, 0.875]), np.array([0.0, 0, 1]), np.zeros(3), 1.0) > 1.0
    # a capsule that holds the whole disc
    assert _listed(hs, (0, 0, 0), (0, 0, 1), 1.0) == [(0, 0, CONTAINED)]
    # a disc tilted to the normal (1, 0, 1), not unit: the capsule's bounds meet the disc's, it reaches the ball (0.5 <= 1.5625), but
    # both ends clear the slab: sa = sb = 1 > rn = 0.25 sqrtf(2)
    hs = pc.hand_scene(discs=[(1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0)])
    q = cc.Query32(cc.capsules([((0.5, 0, 0.5), (0.5, 0.5, 0.5), 0.25)])[0])
    h = float(np.sqrt(0.5))
    assert q.meets((-h, -1, -h), (h, 1, h)) and q.point_seg_dist2(cc.v3((0, 0, 0))) <= F(1.25 * 1.25)
    assert _listed(hs, (0.5, 0, 0.5), (0.5, 0.5, 0.5), 0.25) == []
    # with one end below the slab's top it is listed
    assert _listed(hs, (0.5, 0, 0.5), (0.0, 0.5, 0.25), 0.25) == [(0, 0, 0)]


def test_a_lateral_axis_prunes_a_subtree_the_world_bounds_meet():
    """Root -> (leaf t0, interior -> (leaf t1, leaf t2)): the capsule runs along the diagonal y = x, t1 and t2 lie in the other
    corner of its world bounds. The six compares meet the interior node's box, the lateral axis X2 = (6, -6, 0) separates it
    (dn = 27.6 > R2 = 4.24): 3 box tests and 1 primitive test, where mi_box_* on the world bounds makes 5 and 3."""
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
    cp = cc.capsules([((-3, -3, 0), (3, 3, 0), 0.5)])
    q = cc.Query32(cp[0])
    assert q.valid and (inner[0] <= np.array(q.qmx)).all() and (inner[1] >= np.array(q.qmn)).all(), "the world bounds meet the second subtree"
    assert not q.meets(*inner)
    offsets, vo = irl.capsule_offsets_host(desc, cp)
    recs, vf = irl.capsule_fill_host(desc, cp, offsets)
    cc.assert_same((offsets, recs), cc.packed([[(0, 0, False)]]), "the one triangle on the diagonal")
    assert (vo["box_tests"], vo["prim_evals"]) == (3, 1) and (vf["box_tests"], vf["prim_evals"]) == (3, 1)
    ck = cc.CapsuleChecker(hs, nodes)
    assert ck.overlaps(cp[0]) == ([(0, 0, False)], 3, 1)
    ab = bc.boxes([(q.qmn, q.qmx)])
    boffsets, vb = irl.box_offsets_host(desc, ab)
    assert boffsets[-1] == 3 and (vb["box_tests"], vb["prim_evals"]) == (5, 3)
    assert vo["box_tests"] < vb["box_tests"] and vo["prim_evals"] < vb["prim_evals"]


# ------------------------------------------------------------------------------------------------------
# monotonicity, pinned directly
# ------------------------------------------------------------------------------------------------------
def test_bounds_that_contain_other_bounds_pass_whenever_those_do():
    """10^5 seeded pairs of nested bounds A >= B against random valid queries, magnitudes from 1e-3 to 1e6, through the function the
    kernels and the twins run: capsule_meets_bounds(B) implies capsule_meets_bounds(A). This is what makes a list the same bytes
    whatever tree is walked."""
    n = 100_000
    rng = np.random.default_rng(101)
    scale = (10.0 ** rng.uniform(-3.0, 6.0, (n, 1)))
    centre = (rng.uniform(-1, 1, (n, 3)) * scale).astype(F)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    length = rng.uniform(0, 1, (n, 1)) * scale * 10.0 ** rng.uniform(-2.0, 0.0, (n, 1))
    length[::13] = 0.0
    radius = (rng.uniform(0, 1, n) * scale[:, 0] * 10.0 ** rng.uniform(-3.0, 0.0, n)).astype(F)
    radius[::11] = 0.0
    cp = cc.qb.make_capsules((centre - dirs * length * 0.5).astype(F), (centre + dirs * length * 0.5).astype(F), radius)
    # B: bounds near the query, so that it passes about half of the time; A: B grown by nothing, an ulp or a lot, side by side
    reach = np.maximum(length, radius[:, None].astype(np.float64))
    bc_ = centre + (rng.normal(size=(n, 3)) * reach * 0.6).astype(F)
    bh = (rng.uniform(0, 1, (n, 3)) * reach * 0.3).astype(F)
    b_mn, b_mx = (bc_ - bh).astype(F), (bc_ + bh).astype(F)
    grow = rng.choice(3, (2, n, 3))
    lots = (rng.uniform(0, 1, (2, n, 3)) * scale).astype(F)
    a_mn = np.where(grow[0] == 0, b_mn, np.where(grow[0] == 1, np.nextafter(b_mn, F(-np.inf)), b_mn - lots[0])).astype(F)
    a_mx = np.where(grow[1] == 0, b_mx, np.where(grow[1] == 1, np.nextafter(b_mx, F(np.inf)), b_mx + lots[1])).astype(F)
    assert (a_mn <= b_mn).all() and (a_mx >= b_mx).all()
    fn = irl.host_lib().mi_capsule_meets_bounds_host
    arrays = [np.ascontiguousarray(x) for x in (cp, b_mn, b_mx, a_mn, a_mx)]
    po, pbn, pbx, pan, pax = (x.ctypes.data for x in arrays)
    passed = 0
    for i in range(n):
        if fn(po + 32 * i, pbn + 12 * i, pbx + 12 * i):
            passed += 1
            assert fn(po + 32 * i, pan + 12 * i, pax + 12 * i), f"pair {i}: the inner bounds pass and the outer ones do not"
    print(f"monotonicity: {passed} of {n} inner bounds pass")
    assert n // 10 < passed < n - n // 10
    # the exported helper is the checker's test
    for i in range(0, 2000):
        assert bool(fn(po + 32 * i, pbn + 12 * i, pbx + 12 * i)) == cc.Query32(cp[i]).meets(b_mn[i], b_mx[i]), i
    assert fn(None, pbn, pbx) == 0
    bad = cp[:1].copy()
    bad["radius"] = -1.0
    assert fn(bad.ctypes.data, pbn, pbx) == 0 and not irl.capsule_meets_bounds_host(bad[0], b_mn[0], b_mx[0])


def test_order_does_not_depend_on_the_tree():
    hs, cp, offsets, recs, _, _, _ = cc.twin("soup")
    lbvh = irl.build_lbvh(hs.desc)[0]
    refit = irl.refit_compact_bvh(hs.desc)
    assert not np.array_equal(np.asarray(lbvh).view(np.uint8), np.asarray(hs.nodes).view(np.uint8)), "the LBVH is another tree"
    for what, nodes in (("the LBVH", lbvh), ("a refit of unchanged geometry", refit)):
        cc.assert_same(cc.full(pc.with_nodes(hs.desc, nodes), cp), (offsets, recs), what)
    assert np.all(np.diff(recs["geomID"].astype(np.int64) * (1 << 32) + recs["primID"])[np.diff(recs["box"].astype(np.int64)) == 0] > 0), "keys ascend strictly within a capsule"


# ------------------------------------------------------------------------------------------------------
# against float64
# ------------------------------------------------------------------------------------------------------
K_BOUND = 32


def _pow2_at_least(x):
    k = 32
    while k < x:
        k *= 2
    return k


def test_id_sets_equal_a_float64_reference_that_shares_no_code():
    """Every (query, primitive) pair of the soup whose bounds meet the capsule's world bounds, against binary64: the distance of the
    segment from the triangle as the least over its features, zero where the segment crosses the face; the sphere from the nearest
    and the farthest point of the segment; the disc never missed, its over-listing counted. gap = distance - radius (the inner
    shell: R - radius - dmax). The twin must agree on every pair with |gap| > K_BOUND x 2^-24 x M, M the largest coordinate magnitude
    of the pair, a, b and radius included.
    K_BOUND is set by the CHECKER, as for the rigid poses: the largest |gap| / (2^-24 M) among the pairs on which the checker and
    the reference disagree, doubled, rounded up to a power of two, never below 32. Measured on this seeded set (29 181 pairs): the checker and
    the reference disagree on no pair at all, so the ratio is 0 and K_BOUND stays the box family's 32 - the nearly parallel segment
    pairs, where 5.1.9 is weakest, do not push it up here; 602 pairs (2.06 %) are left out as unclear, all of them the query of
    coordinates 1e19, whose M makes the band wider than the scene (at most 5 % may be, which is asserted). The test recomputes the
    ratio, asserts that it still gives K_BOUND, prints both figures, and holds the twin to it."""
    hs, cp, offsets, recs, _, _, _ = cc.twin("soup")
    pr = pc.primitives(hs)
    A, B, Cc, tg, tp = pr["tri"]
    sc, sr, sg = pr["sphere"]
    dn, dc, dr, dg = pr["disc"]
    leaf = {(lf[2], lf[3]): lf for lf in cc.CapsuleChecker(hs).leaf if lf is not None}
    tri_mn, tri_mx = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    tri_m = np.maximum(np.abs(tri_mn), np.abs(tri_mx)).max(1)
    pairs = checked = disc_extra = 0
    worst = 0.0
    held = []                                      # (query, key, listed by the twin, gap, M): judged once the bound is known
    for i, c in enumerate(cp):
        q = cc.Query32(c)
        if not q.valid:
            assert offsets[i + 1] == offsets[i]
            continue
        a, b, radius = c["a"].astype(np.float64), c["b"].astype(np.float64), float(c["radius"])
        wmn, wmx = np.minimum(a, b) - radius, np.maximum(a, b) + radius
        qm = max(float(np.abs(a).max()), float(np.abs(b).max()), radius)
        mine = cc.ids(recs[int(offsets[i]):int(offsets[i + 1])])
        cand = np.nonzero((tri_mn <= wmx).all(1) & (tri_mx >= wmn).all(1))[0]
        if cand.size:
            gap = cc.seg_tri_dist64(a, b, A[cand], B[cand], Cc[cand]) - radius
            for k, j in enumerate(cand):
                pairs += 1
                key = (int(tg[j]), int(tp[j]))
                M = max(qm, float(tri_m[j]))
                if q.touches(*leaf[key][:2])[0] != (gap[k] <= 0):
                    worst = max(worst, abs(gap[k]) / (pc.EPS * M))
                held.append((i, key, key in mine, float(gap[k]), M))
        outside = {(int(tg[j]), int(tp[j])) for j in np.setdiff1d(np.arange(len(tg)), cand)}
        assert not (mine & outside), f"query {i}: a triangle outside the world bounds is listed"
        for j in range(len(sg)):
            key = (int(sg[j]), 0)
            if not ((sc[j] - sr[j] <= wmx).all() and (sc[j] + sr[j] >= wmn).all()):
                assert key not in mine
                continue
            pairs += 1
            gap = cc.sphere_gap64(a, b, radius, sc[j], sr[j])
            M = max(qm, float((np.abs(sc[j]) + sr[j]).max()))
            if q.touches(*leaf[key][:2])[0] != (gap <= 0):
                worst = max(worst, abs(gap) / (pc.EPS * M))
            held.append((i, key, key in mine, gap, M))
        for j in range(len(dg)):
            key = (int(dg[j]), 0)
            gap = cc.disc_dist64(a, b, dn[j], dc[j], dr[j]) - radius
            M = max(qm, float((np.abs(dc[j]) + dr[j]).max()))
            if gap < -1e-4 * M:                      # (the sampled distance is good to far less)
                assert key in mine, f"query {i}: a touching disc is missed"
            elif key in mine and gap > 1e-4 * M:
                assert gap <= dr[j] * (1 + 1e-6), f"query {i}: a listed disc is farther than its own radius from the capsule"
                disc_extra += 1
    k_bound = _pow2_at_least(2 * worst)
    unclear = 0
    for i, key, listed, gap, M in held:
        if abs(gap) <= k_bound * pc.EPS * M:
            unclear += 1
            continue
        assert listed == (gap <= 0), f"query {i}, primitive {key}: gap {gap}, bound {k_bound * pc.EPS * M}"
        checked += 1
    share = unclear / pairs
    print(f"soup: {pairs} pairs whose bounds meet, {checked} checked, {unclear} unclear ({100 * share:.2f} %), {disc_extra} discs listed that are "
          f"not touched; the largest |gap| / (2^-24 M) among the pairs the checker decides otherwise: {worst:.2f}, which gives k = {k_bound}")
    assert k_bound == K_BOUND, "the measured ratio still gives the recorded bound"
    assert checked > 3000 and share <= 0.05


# ------------------------------------------------------------------------------------------------------
# the usual list rules
# ------------------------------------------------------------------------------------------------------
def test_invalid_queries_and_empty_scene():
    hs = bc.scene("soup")
    nan, inf = np.nan, np.inf
    z = (0.0, 0.0, 0.0)
    cp = cc.capsules([((nan, 0, 0), z, 1.0), (z, (0, inf, 0), 1.0), ((0, 0, -inf), z, 1.0), (z, (1, 1, 1), nan), (z, (1, 1, 1), inf), (z, (1, 1, 1), -1e-30),
                      (z, (1, 1, 1), -inf)])
    offsets, vo = irl.capsule_offsets_host(hs.desc, cp)
    assert not offsets.any() and (vo["box_tests"], vo["prim_evals"]) == (0, 0)
    for kind in (cc.ANY, cc.COUNT):
        out, v = irl.capsule_query_host(hs.desc, kind, cp)
        assert not out.any() and (v["box_tests"], v["prim_evals"]) == (0, 0)
    recs, vf = irl.capsule_fill_host(hs.desc, cp, cc.k_offsets(cp.size, 2))
    pc.assert_bytes_equal(recs, np.concatenate([cc.records([], i, 2) for i in range(cp.size)]), "padded segments of queries that are not walked")
    assert (vf["box_tests"], vf["prim_evals"]) == (0, 0)
    # the edges that ARE valid: -0, a ball, a bare segment, a huge finite radius, a length whose square underflows
    lo, hi = pc.root_box(hs.nodes)
    mid = tuple(((lo + hi) * F(0.5)).tolist())
    ok = cc.capsules([(mid, mid, 1e30), (lo, hi, 1e30), (mid, mid, 3e38), (lo, hi, 100.0)])
    assert irl.capsule_query_host(hs.desc, cc.COUNT, ok)[0].tolist() == [602, 602, 602, 602]
    thin = cc.capsules([(lo, hi, 1.0), (lo, hi, 0.0), (lo, hi, -0.0), (mid, mid, 1.0), (mid, mid, 0.0)])
    counts = irl.capsule_query_host(hs.desc, cc.COUNT, thin)[0]
    assert counts[0] > counts[1] == counts[2] and counts[3] >= counts[4], "a capsule, its bare segment (0 and -0), a ball, a point"
    reach = float((hi - lo).max())                                       # (from x = 0, where 1e-30 is not rounded away)
    tiny = cc.capsules([((0, mid[1], mid[2]), (1e-30, mid[1], mid[2]), reach), ((0, mid[1], mid[2]), (0, mid[1], mid[2]), reach)])
    assert cc.Query32(tiny[0]).dd == 0 and cc.Query32(tiny[0]).d[0] > 0
    a, b = cc.full(hs.desc, tiny[:1]), cc.full(hs.desc, tiny[1:])
    assert a[1].size > 0 and cc.ids(a[1]) == cc.ids(b[1]), "a length of 1e-30 lists what the ball lists"
    # an empty scene
    empty = irl.SceneDesc()
    one = cc.capsules([(z, (1, 1, 1), 1.0)])
    assert not irl.capsule_offsets_host(empty, one)[0].any() and not irl.capsule_query_host(empty, cc.ANY, one)[0].any()
    recs, v = irl.capsule_fill_host(empty, one, np.array([0, 3], np.uint64))
    pc.assert_bytes_equal(recs, cc.records([], 0, 3), "an empty scene pads")
    assert irl.capsule_offsets_host(hs.desc, cp[:0])[0].tolist() == [0]


def test_caller_supplied_offsets_are_honoured():
    hs, cp, offsets, recs, _, _, _ = cc.twin("soup")
    n = cp.size
    counts = np.diff(offsets).astype(np.int64)
    for k in (1, 4):
        got, v = irl.capsule_fill_host(hs.desc, cp, cc.k_offsets(n, k))
        want = np.concatenate([np.concatenate([recs[int(offsets[i]):int(offsets[i]) + min(k, int(counts[i]))], cc.records([], i, max(k - int(counts[i]), 0))]) for i in range(n)])
        pc.assert_bytes_equal(got, want, f"K = {k}: the head of the full list, padded")
    # decreasing pairs, a start at or past capacity, capacity cutting a segment in the middle; canaries everywhere else
    sub = np.nonzero(counts >= 6)[0][:6]
    assert sub.size == 6
    c6 = cp[sub]
    offs = np.array([0, 5, 3, 9, 30, 24, 12], np.uint64)      # segments [0, 5) [5, 3) - [3, 9) [9, 30) cut at 12 [30, 24) - [24, 12) -
    capacity = 12
    buf = cc.sentinel_buffer(40)
    got, v = irl.capsule_fill_host(hs.desc, c6, offs, capacity=capacity, hits=buf)
    full = [recs[int(offsets[i]):int(offsets[i + 1])].copy() for i in sub]
    for j, f in enumerate(full):
        f["box"] = j
    pc.assert_bytes_equal(got[9:12], full[3][:3], "capacity cuts capsule 3's segment in the middle: the 3 smallest keys")
    pc.assert_bytes_equal(got[3:9], full[2][:6], "capsule 2")
    pc.assert_bytes_equal(got[0:3], full[0][:3], "capsule 0's head (capsule 2's segment overlaps its tail)")
    assert cc.is_sentinel(got[12:]).all(), "nothing at or past capacity"
    walked = irl.capsule_offsets_host(hs.desc, c6[[0, 2, 3]])[1]
    assert (v["box_tests"], v["prim_evals"]) == (walked["box_tests"], walked["prim_evals"])
    offs = np.array([2, 4, 4, 4, 4, 4, 4], np.uint64)
    buf = cc.sentinel_buffer(8)
    got, _ = irl.capsule_fill_host(hs.desc, c6, offs, hits=buf)
    assert cc.is_sentinel(got[:2]).all() and cc.is_sentinel(got[4:]).all()
    pc.assert_bytes_equal(got[2:4], full[0][:2], "a segment between canaries")
    # unaligned buffers are read and written as they lie
    raw = np.zeros(cp.nbytes + 1, np.uint8)
    raw[1:] = cp.view(np.uint8)
    off_raw = np.zeros(offsets.nbytes + 3, np.uint8)
    host = irl.host_lib()
    assert host.mi_capsule_offsets_host(C.byref(hs.desc), raw.ctypes.data + 1, off_raw.ctypes.data + 3, n, None) == 0
    assert off_raw[3:].tobytes() == offsets.tobytes()
    hit_raw = np.full(recs.nbytes + 5, 0xEE, np.uint8)
    assert host.mi_capsule_fill_host(C.byref(hs.desc), raw.ctypes.data + 1, off_raw.ctypes.data + 3, hit_raw.ctypes.data + 5, recs.size, n, None) == 0
    assert hit_raw[5:].tobytes() == recs.tobytes() and (hit_raw[:5] == 0xEE).all()
    cnt_raw = np.zeros(4 * n + 1, np.uint8)
    assert host.mi_capsule_query_host(C.byref(hs.desc), cc.COUNT, raw.ctypes.data + 1, cnt_raw.ctypes.data + 1, n, None) == 0
    assert cnt_raw[1:].tobytes() == counts.astype(np.uint32).tobytes()
