"""Neighbour lists on the host (no GPU): mi_near_offsets_host / mi_near_fill_host, the twins the device results are compared with
byte for byte (tests/test_near_gpu.py), against the checker of tests/near_cases.py - the contract's text in numpy binary32 -,
against a float64 brute force over every primitive on the points it leaves a margin for, against mi_point_query_host, and at the
edges of ties, radius, scene, visits and caller-supplied offsets."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import near_cases as nc

F = np.float32


def _full(desc, pts):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.near_offsets_host(desc, pts)
    recs, _ = irl.near_fill_host(desc, pts, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.CASES)
def test_twin_equals_the_checker_on_both_steps(name):
    hs, pts, lists, boxes, prims = nc.case(name)
    _, _, offsets, recs, vo, vf = nc.twin(name)
    counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), counts), "offsets are the running total of the counts"
    nc.assert_same((offsets, recs), nc.packed(lists), f"{name}: the full lists")
    assert (vo["box_tests"], vo["prim_evals"]) == (boxes.sum(), prims.sum()), "the count walk's visits"
    # with the offsets of the count walk a segment is full only once the point's last neighbour is placed: the same records, and
    # no more visits than the count walk (an empty segment is not walked, a full one passes the boxes beyond its last record)
    assert vf["box_tests"] <= vo["box_tests"] and vf["prim_evals"] <= vo["prim_evals"]
    ck = nc.NearChecker(hs)
    sub = slice(0, 100)                                  # (the checker walks in Python)
    res = [ck.fill(pt, len(found)) for pt, found in zip(pts[sub], lists[sub])]
    sub_off, sub_recs = nc.packed(lists[sub])
    got, v = irl.near_fill_host(hs.desc, pts[sub], sub_off)
    pc.assert_bytes_equal(got, sub_recs, f"{name}: the fill of the first points alone")
    assert (v["box_tests"], v["prim_evals"]) == (sum(r[1] for r in res), sum(r[2] for r in res)), "the fill's visits"
    assert np.all(recs["flags"] == 0) and np.array_equal(recs["point"], np.repeat(np.arange(pts.size, dtype=np.uint32), counts.astype(np.int64)))
    if name in ("soup", "box"):
        hist = np.bincount(np.minimum(counts, 24).astype(np.int64), minlength=25)
        print(f"{name}: points with 0 / 1-9 / 10-23 / 24+ neighbours: {hist[0]} / {hist[1:10].sum()} / {hist[10:24].sum()} / {hist[24]}")
        assert hist[0] > 20 and hist[1:10].sum() > 20 and (name == "box" or hist[24] > 20), "the radii span no, few and dozens of neighbours"


@pytest.mark.parametrize("name", nc.CASES)
@pytest.mark.parametrize("k", [1, 4])
def test_pruned_fill_equals_the_checker(name, k):
    hs, pts, lists, _, _ = nc.case(name)
    ck = nc.NearChecker(hs)
    sub = slice(0, 120)                                  # (the checker walks in Python)
    res = [ck.fill(pt, k) for pt in pts[sub]]
    want = np.concatenate([nc.records(r[0], i, k) for i, r in enumerate(res)])
    n = len(res)
    got, v = irl.near_fill_host(hs.desc, pts[sub], nc.k_offsets(n, k))
    pc.assert_bytes_equal(got, want, f"{name}: the {k} nearest within the radius")
    assert (v["box_tests"], v["prim_evals"]) == (sum(r[1] for r in res), sum(r[2] for r in res)), "the pruned walk's visits"
    # the property: the len smallest of the unpruned list (these fixed cases have no rounding accident)
    pc.assert_bytes_equal(got, np.concatenate([nc.records(lists[i], i, k) for i in range(n)]), f"{name}: the first {k} of the full list")


# ------------------------------------------------------------------------------------------------------
# against float64, on the points with margin
# ------------------------------------------------------------------------------------------------------
def test_id_sets_equal_the_float64_brute_force():
    hs, pts, offsets, recs, _, _ = nc.twin("soup")
    D, geom, prim, margin = nc.soup_margin()
    print(f"soup: {margin.sum()} of {pts.size} points have margin")
    checked = 0
    for i in np.nonzero(margin)[0]:
        mine = {(int(r["geomID"]), int(r["primID"])) for r in recs[int(offsets[i]):int(offsets[i + 1])]}
        inside = np.nonzero(D[i] < float(pts["radius"][i]))[0]
        assert mine == {(int(geom[j]), int(prim[j])) for j in inside}, f"point {i}"
        checked += len(mine)
    assert checked > 1000
    # and the distances: sqrt(dist2) against the float64 distance of the named primitive
    M = max(float(np.abs(np.stack([pts[c] for c in "xyz"], 1)[margin]).max()), pc.scene_max_abs(hs))
    index = {(int(g), int(q)): j for j, (g, q) in enumerate(zip(geom, prim))}
    owner = recs["point"].astype(np.int64)
    keep = margin[owner]
    cols = np.array([index[(int(g), int(q))] for g, q in zip(recs["geomID"][keep], recs["primID"][keep])])
    err = np.abs(np.sqrt(recs["dist2"][keep].astype(np.float64)) - D[owner[keep], cols])
    print(f"soup: worst |sqrt(dist2) - true| = {(err / (pc.EPS * M)).max():.2f} * 2^-24 * M")
    assert np.all(err <= 32 * pc.EPS * M)                  # the bound of tests/test_point_query_host.py


@pytest.mark.parametrize("k", nc.KS)
def test_k_nearest_is_the_head_of_the_full_list(k):
    hs, pts = nc.scene("soup"), nc.points_of("soup").copy()
    pts["radius"] = np.inf
    if "full-inf" not in nc._twins:
        nc._twins["full-inf"] = _full(hs.desc, pts)
    offsets, recs = nc._twins["full-inf"]
    _, _, _, margin = nc.soup_margin()
    valid = np.diff(offsets) > 0
    assert np.all(np.diff(offsets)[valid] == 602) and np.array_equal(valid, np.isfinite(np.stack([pts[c] for c in "xyz"], 1)).all(1))
    near, _ = nc.twin_k("soup", k, np.inf)
    for i in np.nonzero(margin)[0]:
        pc.assert_bytes_equal(near[i], recs[int(offsets[i]):int(offsets[i]) + k], f"point {i}, k = {k}")
    assert np.all(near[~valid]["primID"] == irl.INVALID_PRIM) and np.all(np.isposinf(near[~valid]["dist2"]))


def test_first_record_is_the_closest_point_query():
    hs, pts = nc.scene("soup"), nc.points_of("soup").copy()
    pts["radius"] = np.inf
    near, _ = nc.twin_k("soup", 2, np.inf)
    hit, _ = irl.point_query_host(hs.desc, irl.POINT_CLOSEST, pts)
    found = hit["primID"] != irl.INVALID_PRIM
    assert np.array_equal(found, near[:, 0]["primID"] != irl.INVALID_PRIM) and found.sum() > 390
    tie = near[:, 0]["dist2"] == near[:, 1]["dist2"]      # exact ties: the list breaks them by ids, CLOSEST by preorder
    use = found & ~tie
    assert use.sum() > 380
    first = near[use, 0]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.sqrt(first["dist2"]).view(np.uint32), hit["dist"][use].view(np.uint32))
    assert np.array_equal(first["primID"], hit["primID"][use]) and np.array_equal(first["geomID"], hit["geomID"][use])
    # and where they tie, the distance is CLOSEST's all the same
    assert np.array_equal(np.sqrt(near[found, 0]["dist2"]).view(np.uint32), hit["dist"][found].view(np.uint32))


# ------------------------------------------------------------------------------------------------------
# ties, radius and scene edges
# ------------------------------------------------------------------------------------------------------
def test_ties_scene_exact_order():
    hs, pts = nc.scene("ties"), nc.points_of("ties")
    offsets, recs = _full(hs.desc, pts)
    lists = nc.split(offsets, recs)
    p = nc.TIES_QUERY
    d_tri = pc.dist2_32(p, pc.tri_closest32(*nc.TRI, p)[0])
    d_dot = pc.dist2_32(p, nc.DOT)
    assert d_dot == F(95.25) and d_tri > d_dot
    # radius inf: the two spheres at 9 by geomID, the collapsed triangle, the coincident triangles by geomID
    assert lists[0] == [(F(9), 3, 0), (F(9), 4, 0), (d_dot, 2, 0), (d_tri, 0, 0), (d_tri, 1, 0)]
    # radius 3: the spheres lie exactly AT the radius (9 < 9 fails) and are not listed; one ulp more lists both
    assert lists[1] == [] and lists[2] == [(F(9), 3, 0), (F(9), 4, 0)]
    # on the collapsed triangle: distance 0 first
    assert lists[3][0] == (F(0), 2, 0) and len(lists[3]) == 5
    # K = 1 and K = 4 cut the same order, whatever the tree: the first of a tie has the smaller geomID
    for k in (1, 4):
        got, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(pts.size, k))
        pc.assert_bytes_equal(got, np.concatenate([nc.records(x, i, k) for i, x in enumerate(lists)]), f"ties, k = {k}")


def test_tie_order_is_the_key_not_the_visit_order():
    """Two coincident triangles under hand-made nodes, either one first in preorder: MI_POINT_CLOSEST names the first leaf visited,
    the list orders by geomID both times - the two differ on an exact tie, as the contract says."""
    hs = pc.hand_scene(tris=[nc.TRI, nc.TRI])
    lo = np.min(np.array(nc.TRI, F), 0); hi = np.max(np.array(nc.TRI, F), 0)
    pts = pc.points([(2.5, 2.0, 1.5, np.inf)])
    for first in (0, 1):
        nodes = np.array([pc.compact_node(lo, hi, 2), pc.compact_node(lo, hi, 0, first), pc.compact_node(lo, hi, 0, 1 - first)])
        desc = pc.with_nodes(hs.desc, nodes)
        offsets, recs = _full(desc, pts)
        assert recs["geomID"].tolist() == [0, 1] and recs["dist2"][0] == recs["dist2"][1]
        hit, _ = irl.point_query_host(desc, irl.POINT_CLOSEST, pts)
        assert hit["geomID"][0] == first
        one, _ = irl.near_fill_host(desc, pts, nc.k_offsets(1, 1))
        assert one["geomID"][0] == 0, "an equal-distance primitive with a smaller id displaces the last record (<= in the bound)"
        ck = nc.NearChecker(hs, nodes)
        assert [x[1] for x in ck.fill(pts[0], 1)[0]] == [0]


def test_invalid_queries_and_infinite_radius():
    hs = nc.scene("ties")
    p = nc.TIES_QUERY
    nan, inf = F("nan"), F("inf")
    rows = [(nan,) + p[1:] + (inf,), p[:1] + (inf,) + p[2:] + (inf,), p[:2] + (-inf, inf), p + (nan,), p + (-1.0,), p + (-inf,), p + (0.0,),
            p + (inf,)]
    pts = pc.points(rows)
    offsets, vo = irl.near_offsets_host(hs.desc, pts)
    assert offsets.tolist() == [0] * 8 + [5], "only radius = +inf finds anything here"
    assert vo["box_tests"] == 1 + hs.desc.num_nodes, "invalid queries are not walked; radius 0 fails at the root"
    got, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(8, 2))
    want = np.concatenate([nc.records([], i, 2) for i in range(7)] + [nc.records([(F(9), 3, 0), (F(9), 4, 0)], 7, 2)])
    pc.assert_bytes_equal(got, want, "invalid queries give padded segments")
    assert np.all(np.isposinf(got["dist2"][:14])) and np.all(got["flags"][:14] == irl.FLAG_ESCAPED) and np.all(got["geomID"][:14] == irl.INVALID_GEOM)


def test_scene_edges():
    pts = pc.points([(0.0, 0.0, 0.0, np.inf), (1.0, 2.0, 3.0, 5.0)])
    offsets, v = irl.near_offsets_host(nc.empty_desc(), pts)
    assert offsets.tolist() == [0, 0, 0] and v == {"box_tests": 0, "prim_evals": 0}
    got, v = irl.near_fill_host(nc.empty_desc(), pts, nc.k_offsets(2, 3))
    pc.assert_bytes_equal(got, np.concatenate([nc.records([], 0, 3), nc.records([], 1, 3)]), "an empty scene pads")
    assert v == {"box_tests": 0, "prim_evals": 0}
    offsets, v = irl.near_offsets_host(nc.empty_desc(), pts[:0])
    assert offsets.tolist() == [0]
    # one primitive: a single leaf root. From (0, 5, 0) the unit sphere's shell is 4 away: radius 4 does not list it
    hs, one = nc.scene("one"), nc.points_of("one")
    assert hs.desc.num_nodes == 1
    offsets, recs = _full(hs.desc, one)
    assert offsets.tolist() == [0, 1, 1, 2, 3, 3] and recs["dist2"].tolist() == [16.0, 16.0, 0.5625] and recs["point"].tolist() == [0, 2, 3]


# ------------------------------------------------------------------------------------------------------
# visits
# ------------------------------------------------------------------------------------------------------
def test_an_infinite_radius_walks_every_node_and_the_pruned_fill_does_not():
    hs, pts = nc.scene("soup"), nc.points_of("soup").copy()
    pts["radius"] = np.inf
    valid = int(np.isfinite(np.stack([pts[c] for c in "xyz"], 1)).all(1).sum())
    n_nodes = hs.desc.num_nodes
    _, v = irl.near_offsets_host(hs.desc, pts)
    assert (v["box_tests"], v["prim_evals"]) == (valid * n_nodes, valid * (n_nodes + 1) // 2)
    _, vk = nc.twin_k("soup", 4, np.inf)
    print(f"soup, radius inf: {v['box_tests'] / valid:.0f} box tests per point unpruned, {vk['box_tests'] / valid:.0f} for the 4 nearest")
    assert vk["box_tests"] < v["box_tests"] and vk["prim_evals"] < v["prim_evals"]
    assert vk["box_tests"] < v["box_tests"] // 2, "the bound shrinks to the 4th distance: far less than the whole tree"


def test_visits_of_a_three_leaf_tree_counted_by_hand():
    """The tree of tests/test_point_query_host.py: three unit triangles in the plane z = 0 at x = 0, 10, 20; nodes 0 = root (second
    child 2), 1 = leaf A, 2 = interior (second child 4), 3 = leaf B, 4 = leaf C. Every point lies at z = 1 above a triangle."""
    def tri(x):
        return ((x, 0.0, 0.0), (x + 1.0, 0.0, 0.0), (x, 1.0, 0.0))
    hs = pc.hand_scene(tris=[tri(0.0), tri(10.0), tri(20.0)])
    box = lambda x0, x1: ((x0, 0.0, 0.0), (x1, 1.0, 0.0))
    nodes = np.array([pc.compact_node(*box(0, 21), 2), pc.compact_node(*box(0, 1), 0, 0), pc.compact_node(*box(10, 21), 4),
                      pc.compact_node(*box(10, 11), 0, 1), pc.compact_node(*box(20, 21), 0, 2)])
    desc = pc.with_nodes(hs.desc, nodes)
    above_b, above_a = (10.25, 0.25, 1.0), (0.25, 0.25, 1.0)
    cases = [
        # the count walk, radius inf: every box is nearer than inf, every primitive evaluated.        5 box tests, 3 evaluations
        (above_b + (np.inf,), None, (5, 3), [1, 0, 2]),
        # the count walk, radius 0.5: the root's box is 1 away, 1 < 0.25 fails.                        1 box test
        (above_b + (0.5,), None, (1, 0), []),
        # len 1, radius inf: root in; A evaluated (d2 = 9.25^2 + .25^2 + 1 = 86.625), held = len, bound = 86.625; node 2 in
        # (1 <= bound); B's box in, B evaluated: 1 displaces A, bound = 1; C's box is 9.75^2 + 1 away: passed.      5 and 2
        (above_b + (np.inf,), 1, (5, 2), [1]),
        # len 2: A, then B (held = len, kept B, A; bound = 86.625); C's box 96.0625 away: passed.                    5 and 2
        (above_b + (np.inf,), 2, (5, 2), [1, 0]),
        # len 3: never full before the walk ends: every box, every primitive.                                        5 and 3
        (above_b + (np.inf,), 3, (5, 3), [1, 0, 2]),
        # len 1 above A: root in; A evaluated, bound = 1; node 2's box 9.75^2 + 1 away: passed with its subtree.     3 and 1
        (above_a + (np.inf,), 1, (3, 1), [0]),
        # len 1, radius 0.5: the root fails; the segment is padded.                                                  1 and 0
        (above_b + (0.5,), 1, (1, 0), []),
        # len 0: not walked.                                                                                          0 and 0
        (above_b + (np.inf,), 0, (0, 0), []),
    ]
    ck = nc.NearChecker(hs, nodes)
    for row, length, visits, geoms in cases:
        pts = pc.points([row])
        if length is None:
            offsets, v = irl.near_offsets_host(desc, pts)
            recs, _ = irl.near_fill_host(desc, pts, offsets)
            mine = ck.neighbours(pts[0])
        else:
            recs, v = irl.near_fill_host(desc, pts, nc.k_offsets(1, length))
            mine = ck.fill(pts[0], length)
        assert (v["box_tests"], v["prim_evals"]) == visits == mine[1:], (row, length)
        found = recs[recs["primID"] != irl.INVALID_PRIM]
        assert found["geomID"].tolist() == geoms == [x[1] for x in mine[0]], (row, length)
        assert recs.size == (len(geoms) if length is None else length)


# ------------------------------------------------------------------------------------------------------
# caller-supplied offsets
# ------------------------------------------------------------------------------------------------------
def _fill_by_hand(lists, offsets, capacity, total):
    """What a fill must leave in a sentinel buffer of `total` records: every point's own segment, cut at capacity, nothing else."""
    want = nc.sentinel_buffer(total)
    for i, found in enumerate(lists):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if hi > lo and lo < capacity:
            hi = min(hi, capacity)
            want[lo:hi] = nc.records(found, i, hi - lo)
    return want


def test_caller_supplied_offsets_are_honoured():
    hs, pts, lists, _, _ = nc.case("soup")
    counts = np.array([len(x) for x in lists])
    many, few, none = np.nonzero(counts > 25)[0], np.nonzero((counts >= 3) & (counts < 25))[0], np.nonzero(counts == 0)[0]
    pick = [few[0], many[1], many[2], many[3], few[1], many[0], many[4], none[0]]
    some, mine = pts[pick], [lists[i] for i in pick]
    # point 0: [70, 2^40): K far above the count, cut at capacity, padded | 1: a decreasing pair, empty | 2: [30, 31), len 1 |
    # 3: [31, 31), len 0 | 4: decreasing | 5: [0, 25), the 25 nearest of more | 6: [25, 28), the 3 nearest | 7: decreasing
    offsets = np.array([70, 2 ** 40, 30, 31, 31, 0, 25, 28, 27], np.uint64)
    total = 100
    for capacity in (total, 85, 20, 0):              # 85 and 20 cut a segment in mid-segment
        buf = nc.sentinel_buffer(total)
        got, _ = irl.near_fill_host(hs.desc, some, offsets, capacity=capacity, hits=buf)
        want = _fill_by_hand(mine, offsets, capacity, total)
        pc.assert_bytes_equal(got, want, f"capacity {capacity}")
        assert np.all(got[capacity:] == np.array(nc.SENTINEL, irl.NEIGHBOUR)), "a record at or past capacity was written"
    # the full lists with a capacity in mid-segment
    full_off, full = nc.packed(mine)
    for capacity in (full.size, full.size - 1, full.size // 2):
        buf = nc.sentinel_buffer(full.size)
        got, _ = irl.near_fill_host(hs.desc, some, full_off, capacity=capacity, hits=buf)
        pc.assert_bytes_equal(got, _fill_by_hand(mine, full_off, capacity, full.size), f"the full lists, capacity {capacity}")


def test_refusals():
    hs = nc.scene("one")
    lib = irl.host_lib()
    pts = pc.points([(0.0, 0.0, 0.0, 1.0)])
    offs = np.zeros(2, np.uint64); offs[1] = 1
    out = np.zeros(1, irl.NEIGHBOUR)
    d, p, o, h = C.byref(hs.desc), pts.ctypes.data, offs.ctypes.data, out.ctypes.data
    for what, args in {"null desc": (None, p, o, 1), "null points": (d, None, o, 1), "null offsets": (d, p, None, 1)}.items():
        assert lib.mi_near_offsets_host(*args, None) == 1, what
        assert b"mi_near_offsets_host" in lib.mi_host_last_error(), what
    for what, args in {"null desc": (None, p, o, h, 1, 1), "null points": (d, None, o, h, 1, 1), "null offsets": (d, p, None, h, 1, 1),
                       "null hits": (d, p, o, None, 1, 1)}.items():
        assert lib.mi_near_fill_host(*args, None) == 1, what
        assert b"mi_near_fill_host" in lib.mi_host_last_error(), what
    assert lib.mi_near_offsets_host(d, None, None, 0, None) == 0 and lib.mi_near_fill_host(d, None, None, None, 0, 0, None) == 0
    lo, hi = (0, 0, 0), (1, 1, 1)
    broken = np.array([pc.compact_node(lo, hi, 5), pc.compact_node(lo, hi, 0, 0), pc.compact_node(lo, hi, 0, 0)])
    with pytest.raises(irl.RaylibError, match="mi_near_offsets_host: .*depth-first"):
        irl.near_offsets_host(pc.with_nodes(hs.desc, broken), pts)
    with pytest.raises(irl.RaylibError, match="mi_near_fill_host: leaf geomID out of range"):
        irl.near_fill_host(pc.with_nodes(hs.desc, np.array([pc.compact_node(lo, hi, 0, 7)])), pts, offs)
