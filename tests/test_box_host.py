"""Box queries on the host (no GPU): mi_box_query_host / mi_box_offsets_host / mi_box_fill_host, the twins the device results are
compared with byte for byte (tests/test_box_gpu.py), against the checker of tests/box_cases.py - the contract's text in numpy
binary32 -, against a float64 brute force over every primitive on the boxes it leaves a margin for, and at the edges of contact,
containment, validity, order and caller-supplied offsets."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import box_cases as bc

F = np.float32
CONTAINED = irl.OVERLAP_CONTAINED


def _full(desc, bx):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.box_offsets_host(desc, bx)
    recs, _ = irl.box_fill_host(desc, bx, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


def _listed(desc, lo, hi):
    """The (geomID, primID, flags) the twin lists for one box, and its any / count answers checked against the list."""
    bx = bc.boxes([(lo, hi)])
    offsets, recs = _full(desc, bx)
    assert irl.box_query_host(desc, bc.COUNT, bx)[0][0] == recs.size and bool(irl.box_query_host(desc, bc.ANY, bx)[0][0]) == (recs.size > 0)
    assert np.all(recs["box"] == 0) and np.all(recs["reserved"] == 0)
    return [(int(r["geomID"]), int(r["primID"]), int(r["flags"])) for r in recs]


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "spheres"])
def test_twin_equals_the_checker(name):
    hs, bx, offsets, recs, counts, anys, v = bc.twin(name)
    ck = bc.BoxChecker(hs)
    res = [ck.overlaps(b) for b in bx]
    lists = [r[0] for r in res]
    want_counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_counts), "offsets are the running total of the counts"
    bc.assert_same((offsets, recs), bc.packed(lists), f"{name}: the full lists")
    assert np.array_equal(counts, want_counts.astype(np.uint32)) and np.array_equal(anys, want_counts > 0)
    walk = (sum(r[1] for r in res), sum(r[2] for r in res))
    assert (v["offsets"]["box_tests"], v["offsets"]["prim_evals"]) == walk, "the count walk's visits"
    assert (v["count"]["box_tests"], v["count"]["prim_evals"]) == walk
    # the fill cannot prune: it walks what the count walk walks, over the boxes whose segment is not empty
    kept = [r for r in res if r[0]]
    assert (v["fill"]["box_tests"], v["fill"]["prim_evals"]) == (sum(r[1] for r in kept), sum(r[2] for r in kept)), "the fill's visits"
    first = [ck.walk(b, first_only=True) for b in bx]
    assert (v["any"]["box_tests"], v["any"]["prim_evals"]) == (sum(r[1] for r in first), sum(r[2] for r in first)), "ANY stops at the first accept"
    assert np.array_equal(recs["box"], np.repeat(np.arange(bx.size, dtype=np.uint32), want_counts.astype(np.int64)))
    assert np.all((recs["flags"] == 0) | (recs["flags"] == CONTAINED)) and np.all(recs["reserved"] == 0)
    if name == "soup":
        kinds = {int(hs.geometry[g]["type"]) for g in np.unique(recs["geomID"])}
        assert kinds == {0, 1, 2}, "triangles, the sphere and the disc are all listed somewhere"
        assert (recs["flags"] == CONTAINED).sum() > 20 and (recs["flags"] == 0).sum() > 20
        hist = np.bincount(np.minimum(want_counts, 24).astype(np.int64), minlength=25)
        print(f"{name}: boxes with 0 / 1-9 / 10-23 / 24+ primitives: {hist[0]} / {hist[1:10].sum()} / {hist[10:24].sum()} / {hist[24]}")
        assert hist[0] > 20 and hist[1:10].sum() > 20 and hist[24] > 20, "the boxes span none, a few and dozens of primitives"


def test_hand_made_trees():
    """Two triangles under one root, in either leaf order, and a tree whose leaf box misses a box that the root's meets: the lists
    do not depend on the order, the visits are counted by hand."""
    t0 = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    t1 = ((4.0, 0.0, 0.0), (5.0, 0.0, 0.0), (4.0, 1.0, 0.0))
    hs = pc.hand_scene(tris=[t0, t1])
    b0, b1 = (np.array(t0, F).min(0), np.array(t0, F).max(0)), (np.array(t1, F).min(0), np.array(t1, F).max(0))
    root = (np.minimum(b0[0], b1[0]), np.maximum(b0[1], b1[1]))
    bx = bc.boxes([((-1, -1, -1), (6, 2, 1)), ((3.5, -1, -1), (6, 2, 1)), ((2, -1, -1), (3, 2, 1)), ((7, 0, 0), (8, 1, 1))])
    want = [[(0, 0, True), (1, 0, True)], [(1, 0, True)], [], []]
    for first in (0, 1):
        leaves = [pc.compact_node(*b0, 0, 0), pc.compact_node(*b1, 0, 1)]
        nodes = np.array([pc.compact_node(*root, 2), leaves[first], leaves[1 - first]])
        desc = pc.with_nodes(hs.desc, nodes)
        ck = bc.BoxChecker(hs, nodes)
        offsets, vo = irl.box_offsets_host(desc, bx)
        recs, vf = irl.box_fill_host(desc, bx, offsets)
        bc.assert_same((offsets, recs), bc.packed(want), f"leaf order {first}")
        assert [ck.overlaps(b)[0] for b in bx] == want
        # box 0: 3 boxes, 2 primitives; box 1: 3 boxes, 1 primitive; box 2: 3 boxes (the root's is met), none; box 3: the root alone
        assert (vo["box_tests"], vo["prim_evals"]) == (10, 3) and (vf["box_tests"], vf["prim_evals"]) == (6, 3)
        _, va = irl.box_query_host(desc, bc.ANY, bx)
        assert (va["box_tests"], va["prim_evals"]) == (2 + (3 if first == 0 else 2) + 3 + 1, 2)


# ------------------------------------------------------------------------------------------------------
# against float64, on the boxes with margin
# ------------------------------------------------------------------------------------------------------
def test_id_sets_equal_the_float64_brute_force():
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    lo, hi = bx["lo"].astype(np.float64), bx["hi"].astype(np.float64)
    valid = np.array([bc.box_valid(b["lo"], b["hi"]) for b in bx])
    lo_v, hi_v = np.where(valid[:, None], lo, 0.0), np.where(valid[:, None], hi, 0.0)
    pr = pc.primitives(hs)
    A, B, Cc, tg, tp = pr["tri"]
    sc, sr, sg = pr["sphere"]
    dn, dc, dr, dg = pr["disc"]
    gt = bc.tri_gap64(lo_v, hi_v, A, B, Cc)
    gs = bc.sphere_gap64(lo_v, hi_v, sc, sr)
    M = np.maximum(np.maximum(np.abs(lo_v), np.abs(hi_v)).max(1), pc.scene_max_abs(hs))
    bound = 32 * pc.EPS * M                               # the bound and the M of tests/test_point_query_host.py
    margin = valid & ~(np.abs(gt) <= bound[:, None]).any(1) & ~(np.abs(gs) <= bound[:, None]).any(1)
    disc = {}
    for i in np.nonzero(valid)[0]:
        for j in range(len(dg)):
            gap, plane_gap = bc.disc_gap64(lo[i], hi[i], dn[j], dc[j], dr[j])
            disc[(i, j)] = gap
            if abs(gap) <= bound[i] or abs(plane_gap) <= bound[i]:
                margin[i] = False
    left_out = int(valid.sum() - margin.sum())
    print(f"soup: {margin.sum()} of {bx.size} boxes have margin ({left_out} valid ones left out, {int((~valid).sum())} not walked)")
    assert left_out <= bx.size // 4
    checked = 0
    for i in np.nonzero(margin)[0]:
        mine = bc.ids(recs[int(offsets[i]):int(offsets[i + 1])])
        exact = {(int(tg[j]), int(tp[j])) for j in np.nonzero(gt[i] <= 0)[0]} | {(int(sg[j]), 0) for j in np.nonzero(gs[i] <= 0)[0]}
        discs = {(int(dg[j]), 0) for j in range(len(dg))}
        assert mine - discs == exact, f"box {i}: triangles and spheres"
        touching = {(int(dg[j]), 0) for j in range(len(dg)) if disc[(i, j)] <= 0}
        assert touching <= mine, f"box {i}: a touching disc is missed"
        diag = float(np.linalg.norm(hi[i] - lo[i]))
        for j in range(len(dg)):
            if (int(dg[j]), 0) in mine:
                assert bc.disc_reach64(lo[i], hi[i], dn[j], dc[j], dr[j]) <= diag * (1 + 1e-6) + bound[i], f"box {i}: a listed disc is farther than the box's diagonal"
        checked += len(mine)
    assert checked > 1000
    assert all(len(bc.ids(recs[int(offsets[i]):int(offsets[i + 1])])) == 0 for i in np.nonzero(~valid)[0])


def test_disc_is_conservative_and_never_missed():
    """One tilted disc, boxes sampled around it: every box the exact test says touches is listed, every listed one lies within its
    own diagonal of the disc, and both kinds occur."""
    disc = (1.0, 2.0, -0.5, 3.0, 0.5, -1.0, 2.0)          # normal (not unit), radius, centre
    hs = pc.hand_scene(discs=[disc])
    n, r, c = np.array(disc[:3]), disc[3], np.array(disc[4:])
    rng = np.random.default_rng(77)
    centre = (c + rng.uniform(-3.0, 3.0, (300, 3))).astype(F)
    half = rng.uniform(0.05, 0.8, (300, 3)).astype(F)
    bx = bc.boxes(zip(centre - half, centre + half))
    got, _ = irl.box_query_host(hs.desc, bc.ANY, bx)
    exact = extra = 0
    for i, b in enumerate(bx):
        lo, hi = b["lo"].astype(np.float64), b["hi"].astype(np.float64)
        gap, plane_gap = bc.disc_gap64(lo, hi, n, c, r)
        if min(abs(gap), abs(plane_gap)) <= 1e-5:
            continue
        if gap <= 0:
            assert got[i], f"box {i} touches the disc and is not listed"
            exact += 1
        elif got[i]:
            assert bc.disc_reach64(lo, hi, n, c, r) <= np.linalg.norm(hi - lo) * (1 + 1e-6)
            extra += 1
    print(f"disc: {exact} touching boxes listed, {extra} listed within their diagonal of the rim")
    assert exact > 20 and got.sum() < bx.size


# ------------------------------------------------------------------------------------------------------
# edges
# ------------------------------------------------------------------------------------------------------
TRI = ((1.0, 1.0, 0.0), (5.0, 1.0, 0.0), (1.0, 4.0, 0.0))


def test_contact_counts():
    hs = pc.hand_scene(tris=[TRI])
    d = hs.desc
    # sharing a face: the triangle lies in the plane z = 0, the box's top face
    assert _listed(d, (2.0, 1.5, -1.0), (2.5, 2.0, 0.0)) == [(0, 0, 0)]
    # sharing an edge: the box's face x = 1 ... y = 1 edge against the triangle's edge y = 1
    assert _listed(d, (2.0, 0.0, -1.0), (3.0, 1.0, 1.0)) == [(0, 0, 0)]
    assert _listed(d, (2.0, 0.0, -1.0), (3.0, 1.0, 0.0)) == [(0, 0, 0)]       # (a box edge on a triangle edge)
    # sharing a vertex: the box's corner on the triangle's vertex
    assert _listed(d, (5.0, 1.0, 0.0), (6.0, 2.0, 1.0)) == [(0, 0, 0)]
    assert _listed(d, (0.0, 0.0, -1.0), (1.0, 1.0, 0.0)) == [(0, 0, 0)]
    # one ulp apart: nothing
    up = np.nextafter(F(5), F(6))
    assert _listed(d, (up, 1.0, 0.0), (6.0, 2.0, 1.0)) == []
    assert _listed(d, (2.0, 1.5, -1.0), (2.5, 2.0, np.nextafter(F(0), F(-1)))) == []
    # a point box on a vertex, in the interior, and off the plane
    assert _listed(d, TRI[1], TRI[1]) == [(0, 0, 0)]
    assert _listed(d, (2.0, 2.0, 0.0), (2.0, 2.0, 0.0)) == [(0, 0, 0)]
    assert _listed(d, (2.0, 2.0, 0.5), (2.0, 2.0, 0.5)) == []


def test_triangle_axes():
    # the plane through the box, all three vertices outside: listed
    big = ((-10.0, -10.0, 0.25), (30.0, -10.0, 0.25), (-10.0, 30.0, 0.25))
    hs = pc.hand_scene(tris=[big])
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) == [(0, 0, 0)]          # wholly containing the cross-section: not CONTAINED
    assert _listed(hs.desc, (0.0, 0.0, 0.5), (1.0, 1.0, 1.0)) == []                    # the plane misses the box (the bounds' z)
    # a slanted plane whose bounds meet the box and which passes the box's corner: the plane axis alone separates
    slant = ((4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, 0.0, 4.0))
    hs = pc.hand_scene(tris=[slant])
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) == []
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (1.5, 1.5, 1.5)) == [(0, 0, 0)]
    assert _listed(hs.desc, (1.0, 1.0, 1.0), (1.5, 1.5, 1.5)) == [(0, 0, 0)]
    assert _listed(hs.desc, (0.0, 0.0, 0.0), (4.0 / 3.0, 4.0 / 3.0, 1.25)) == []
    # a cross-product axis alone separates: the bounds overlap, the plane z = 0 passes through the box, the hypotenuse x + y = 4
    # passes the box's corner (3, 3) outside - only e x Z tells
    flat = ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    hs = pc.hand_scene(tris=[flat])
    assert _listed(hs.desc, (2.5, 2.5, -1.0), (3.5, 3.5, 1.0)) == []
    assert _listed(hs.desc, (2.0, 2.0, -1.0), (3.5, 3.5, 1.0)) == [(0, 0, 0)]          # the corner (2, 2) lies on the hypotenuse
    assert _listed(hs.desc, (1.5, 1.5, -1.0), (3.5, 3.5, 1.0)) == [(0, 0, 0)]


def test_contained_is_closed():
    hs = pc.hand_scene(tris=[TRI])
    assert _listed(hs.desc, (1.0, 1.0, 0.0), (5.0, 4.0, 0.0)) == [(0, 0, CONTAINED)]   # every vertex on a face of a flat box
    assert _listed(hs.desc, (0.0, 0.0, -1.0), (5.0, 4.0, 1.0)) == [(0, 0, CONTAINED)]  # two vertices on faces
    assert _listed(hs.desc, (0.0, 0.0, -1.0), (np.nextafter(F(5), F(4)), 4.0, 1.0)) == [(0, 0, 0)]
    # a collapsed triangle: a point
    z = (2.0, -1.0, 0.5)
    hs = pc.hand_scene(tris=[(z, z, z)])
    assert _listed(hs.desc, (1.0, -2.0, 0.0), (3.0, 0.0, 1.0)) == [(0, 0, CONTAINED)]
    assert _listed(hs.desc, z, z) == [(0, 0, CONTAINED)]
    assert _listed(hs.desc, (2.5, -2.0, 0.0), (3.0, 0.0, 1.0)) == []
    # collapsed to a segment that crosses the box without a vertex in it
    a, b = (0.0, 0.0, 0.0), (4.0, 4.0, 0.0)
    hs = pc.hand_scene(tris=[(a, b, b)])
    assert _listed(hs.desc, (1.0, 1.5, -1.0), (3.0, 2.5, 1.0)) == [(0, 0, 0)]
    assert _listed(hs.desc, (3.0, 0.0, -1.0), (4.0, 1.0, 1.0)) == []


def test_sphere_shell():
    hs = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 5.0)])
    d = hs.desc
    assert _listed(d, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)) == []                       # wholly inside, away from the shell
    assert _listed(d, (-6.0, -6.0, -6.0), (6.0, 6.0, 6.0)) == [(0, 0, CONTAINED)]      # containing the sphere
    assert _listed(d, (-5.0, -5.0, -5.0), (5.0, 5.0, 5.0)) == [(0, 0, CONTAINED)]      # (closed)
    assert _listed(d, (4.0, -1.0, -1.0), (6.0, 1.0, 1.0)) == [(0, 0, 0)]               # crossing the shell
    assert _listed(d, (0.0, 0.0, 0.0), (3.0, 4.0, 0.0)) == [(0, 0, 0)]                 # the farthest corner exactly on the shell: dmax2 = 25
    assert _listed(d, (0.0, 0.0, 0.0), (3.0, np.nextafter(F(4), F(3)), 0.0)) == []
    assert _listed(d, (5.0, -1.0, -1.0), (6.0, 1.0, 1.0)) == [(0, 0, 0)]               # touching from outside: dmin2 = 25
    assert _listed(d, (np.nextafter(F(5), F(6)), -1.0, -1.0), (6.0, 1.0, 1.0)) == []
    assert _listed(d, (4.0, 4.0, 4.0), (6.0, 6.0, 6.0)) == []                          # the bounds meet, the corner region does not: dmin2 = 48


def test_invalid_boxes_and_empty_scene():
    hs = bc.scene("soup")
    nan, inf = np.nan, np.inf
    bx = bc.boxes([((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1)), ((-inf, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, inf)),
                   ((2, 0, 0), (1, 1, 1)), ((0, 0, 3), (1, 1, 1)), ((-inf, -inf, -inf), (inf, inf, inf))])
    offsets, vo = irl.box_offsets_host(hs.desc, bx)
    assert not offsets.any() and (vo["box_tests"], vo["prim_evals"]) == (0, 0)
    for kind in (bc.ANY, bc.COUNT):
        out, v = irl.box_query_host(hs.desc, kind, bx)
        assert not out.any() and (v["box_tests"], v["prim_evals"]) == (0, 0)
    # with caller offsets the segments are padded, still without a walk
    recs, vf = irl.box_fill_host(hs.desc, bx, bc.k_offsets(bx.size, 2))
    pc.assert_bytes_equal(recs, np.concatenate([bc.records([], i, 2) for i in range(bx.size)]), "padded segments of boxes that are not walked")
    assert (vf["box_tests"], vf["prim_evals"]) == (0, 0)
    # a huge finite box is walked and lists everything
    big = bc.boxes([((-3e38, -3e38, -3e38), (3e38, 3e38, 3e38))])
    assert irl.box_query_host(hs.desc, bc.COUNT, big)[0][0] == 602
    # an empty scene
    empty = irl.SceneDesc()
    ok = bc.boxes([((0, 0, 0), (1, 1, 1))])
    assert not irl.box_offsets_host(empty, ok)[0].any() and not irl.box_query_host(empty, bc.ANY, ok)[0].any()
    recs, v = irl.box_fill_host(empty, ok, np.array([0, 3], np.uint64))
    pc.assert_bytes_equal(recs, bc.records([], 0, 3), "an empty scene pads")
    assert irl.box_offsets_host(hs.desc, bx[:0])[0].tolist() == [0]


def test_order_does_not_depend_on_the_tree():
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    lbvh = irl.build_lbvh(hs.desc)[0]
    refit = irl.refit_compact_bvh(hs.desc)
    assert not np.array_equal(np.asarray(lbvh).view(np.uint8), np.asarray(hs.nodes).view(np.uint8)), "the LBVH is another tree"
    for what, nodes in (("the LBVH", lbvh), ("a refit of unchanged geometry", refit)):
        bc.assert_same(_full(pc.with_nodes(hs.desc, nodes), bx), (offsets, recs), what)
    assert np.all(np.diff(recs["geomID"].astype(np.int64) * (1 << 32) + recs["primID"])[np.diff(recs["box"].astype(np.int64)) == 0] > 0), "keys ascend strictly within a box"


def test_caller_supplied_offsets_are_honoured():
    hs, bx, offsets, recs, _, _, _ = bc.twin("soup")
    n = bx.size
    counts = np.diff(offsets).astype(np.int64)
    for k in (1, 4):
        got, v = irl.box_fill_host(hs.desc, bx, bc.k_offsets(n, k))
        want = np.concatenate([np.concatenate([recs[int(offsets[i]):int(offsets[i]) + min(k, int(counts[i]))], bc.records([], i, max(k - int(counts[i]), 0))]) for i in range(n)])
        pc.assert_bytes_equal(got, want, f"K = {k}: the head of the full list, padded")
    # decreasing pairs, a start at or past capacity, capacity cutting a segment in the middle; canaries everywhere else
    sub = np.nonzero(counts >= 6)[0][:6]
    assert sub.size == 6
    b6 = bx[sub]
    offs = np.array([0, 5, 3, 9, 30, 24, 12], np.uint64)      # segments [0, 5) [5, 3) - [3, 9) [9, 30) cut at 12 [30, 24) - [24, 12) -
    capacity = 12
    buf = bc.sentinel_buffer(40)
    got, v = irl.box_fill_host(hs.desc, b6, offs, capacity=capacity, hits=buf)
    full = [recs[int(offsets[i]):int(offsets[i + 1])].copy() for i in sub]
    for j, f in enumerate(full):
        f["box"] = j
    pc.assert_bytes_equal(got[9:12], full[3][:3], "capacity cuts box 3's segment in the middle: the 3 smallest keys")
    pc.assert_bytes_equal(got[3:9], full[2][:6], "box 2")
    pc.assert_bytes_equal(got[0:3], full[0][:3], "box 0's head (box 2's segment overlaps its tail)")
    assert bc.is_sentinel(got[12:]).all(), "nothing at or past capacity"
    # boxes 0, 2 and 3 alone are walked
    walked = irl.box_offsets_host(hs.desc, b6[[0, 2, 3]])[1]
    assert (v["box_tests"], v["prim_evals"]) == (walked["box_tests"], walked["prim_evals"])
    # disjoint segments with gaps between them stay clean
    offs = np.array([2, 4, 4, 4, 4, 4, 4], np.uint64)
    buf = bc.sentinel_buffer(8)
    got, _ = irl.box_fill_host(hs.desc, b6, offs, hits=buf)
    assert bc.is_sentinel(got[:2]).all() and bc.is_sentinel(got[4:]).all()
    pc.assert_bytes_equal(got[2:4], full[0][:2], "a segment between canaries")
