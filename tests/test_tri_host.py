"""Triangle queries on the host (no GPU): mi_tri_query_host / mi_tri_offsets_host / mi_tri_fill_host, the twins the device results
are compared with byte for byte (tests/test_tri_gpu.py), against the checker of tests/tri_cases.py - the contract's text in numpy
binary32 -, against a hand-made catalogue on small integers where every operation is exact, against float64 references on the
pairs they leave a margin for, and at the edges of order, padding and caller-supplied offsets."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import point_cases as pc
import tri_cases as tc

F = np.float32


def _full(desc, tq):
    """(offsets, recs) of the twin's two steps."""
    offsets, _ = irl.tri_offsets_host(desc, tq)
    recs, _ = irl.tri_fill_host(desc, tq, offsets)
    assert recs.size == offsets[-1]
    return offsets, recs


def _listed(desc, q):
    """The (geomID, primID) the twin lists for one query (q0, q1, q2), and its any / count answers checked against the list."""
    tq = tc.tris([q])
    offsets, recs = _full(desc, tq)
    assert irl.tri_query_host(desc, tc.COUNT, tq)[0][0] == recs.size and bool(irl.tri_query_host(desc, tc.ANY, tq)[0][0]) == (recs.size > 0)
    assert np.all(recs["tri"] == 0) and np.all(recs["reserved"] == 0) and np.all(recs["flags"] == 0)
    return [(int(r["geomID"]), int(r["primID"])) for r in recs]


# ------------------------------------------------------------------------------------------------------
# the twin against the checker
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "spheres", "box"])
def test_twin_equals_the_checker(name):
    hs, tq, offsets, recs, counts, anys, v = tc.twin(name)
    ck = tc.TriChecker(hs)
    res = [ck.contacts(t) for t in tq]
    lists = [r[0] for r in res]
    want_counts = np.array([len(x) for x in lists], np.uint64)
    assert offsets.dtype == np.uint64 and offsets[0] == 0 and np.array_equal(np.diff(offsets), want_counts), "offsets are the running total of the counts"
    tc.assert_same((offsets, recs), tc.packed(lists), f"{name}: the full lists")
    assert np.array_equal(counts, want_counts.astype(np.uint32)) and np.array_equal(anys, want_counts > 0)
    walk = (sum(r[1] for r in res), sum(r[2] for r in res))
    assert (v["offsets"]["box_tests"], v["offsets"]["prim_evals"]) == walk, "the count walk's visits"
    assert (v["count"]["box_tests"], v["count"]["prim_evals"]) == walk
    kept = [r for r in res if r[0]]
    assert (v["fill"]["box_tests"], v["fill"]["prim_evals"]) == (sum(r[1] for r in kept), sum(r[2] for r in kept)), "the fill's visits"
    first = [ck.walk(t, first_only=True) for t in tq]
    assert (v["any"]["box_tests"], v["any"]["prim_evals"]) == (sum(r[1] for r in first), sum(r[2] for r in first)), "ANY stops at the first accept"
    assert np.array_equal(recs["tri"], np.repeat(np.arange(tq.size, dtype=np.uint32), want_counts.astype(np.int64)))
    assert np.all(recs["flags"] == 0) and np.all(recs["reserved"] == 0)
    # the special queries: not walked; collapsed ones legal; the overflowing one lists every primitive its bounds reach
    assert want_counts[7] == 0 and want_counts[8] == 0 and res[7][1:] == (0, 0) and res[8][1:] == (0, 0)
    assert res[9][1] > 0 and res[10][1] > 0, "a segment and a point are walked"
    assert want_counts[11] == (len(hs.nodes) + 1) // 2, "a query whose products overflow errs towards listing"
    if len(tc.scene_tris32(hs)):
        assert all(len(lists[i]) >= 1 for i in range(13, 21)), "a scene's own triangle touches at least itself"
    hist = np.bincount(np.minimum(want_counts, 24).astype(np.int64), minlength=25)
    print(f"{name}: queries with 0 / 1-4 / 5+ primitives: {hist[0]} / {hist[1:5].sum()} / {hist[5:].sum()}")
    if name == "soup":
        kinds = {int(hs.geometry[g]["type"]) for g in np.unique(recs["geomID"])}
        assert kinds == {0, 1, 2}, "triangles, the sphere and the disc are all listed somewhere"
        assert hist[0] > 10 and hist[1:5].sum() > 10 and hist[5:].sum() > 10, "the queries span none, a few and several primitives"


# ------------------------------------------------------------------------------------------------------
# the catalogue: small integers, every operation exact, the verdict written by hand
# ------------------------------------------------------------------------------------------------------
T0 = ((0, 0, 0), (4, 0, 0), (0, 4, 0))

CATALOGUE = [
    # (what, the scene's triangle, the query, touching)
    ("shared vertex", T0, ((0, 0, 0), (-2, 0, 3), (0, -2, 3)), True),
    ("shared edge", T0, ((0, 0, 0), (4, 0, 0), (2, 0, 3)), True),
    ("the same triangle", T0, T0, True),
    ("vertex on face", T0, ((1, 1, 0), (1, 1, 3), (2, 1, 3)), True),
    ("edge through interior", T0, ((1, 1, -2), (1, 1, 2), (5, 5, 2)), True),
    ("crossing, no vertex inside the other", T0, ((-1, 1, -1), (3, 1, -1), (1, 1, 3)), True),
    ("coplanar overlapping", T0, ((1, 1, 0), (5, 1, 0), (1, 5, 0)), True),
    ("coplanar, the query inside", T0, ((1, 1, 0), (2, 1, 0), (1, 2, 0)), True),
    ("coplanar, the scene's inside", T0, ((-1, -1, 0), (9, -1, 0), (-1, 9, 0)), True),
    ("coplanar, touching along the hypotenuse", T0, ((4, 0, 0), (0, 4, 0), (4, 4, 0)), True),
    ("coplanar disjoint, bounds meeting", T0, ((3, 3, 0), (5, 3, 0), (3, 5, 0)), False),
    ("parallel planes apart", T0, ((0, 0, 1), (4, 0, 1), (0, 4, 1)), False),
    ("a segment piercing the triangle", T0, ((1, 1, -1), (1, 1, 1), (1, 1, 1)), True),
    ("a segment beside the triangle", T0, ((3, 3, -1), (3, 3, 1), (3, 3, 1)), False),
    ("a point on the triangle", T0, ((1, 1, 0), (1, 1, 0), (1, 1, 0)), True),
    ("a point above the triangle", T0, ((1, 1, 1), (1, 1, 1), (1, 1, 1)), False),
]

# disjoint pairs whose bounds meet and which exactly ONE of the 17 axes separates: ONLY_AXIS[k] is separated by axis k alone
# (tri_cases.AXES[k]): 0, 1 the face normals, 2 .. 10 the edge-edge axes, 11 .. 16 the in-plane axes of coplanar pairs
ONLY_AXIS = {
    0: [[-1, 2, 5], [-1, 0, -1], [5, 0, -2], [-2, 1, 4], [0, 2, -2], [-1, -2, -4]],
    1: [[-2, -2, 0], [5, 3, -1], [1, -3, -4], [1, -2, -2], [4, -4, 1], [2, -1, 2]],
    2: [[3, 1, 0], [2, 0, 5], [-4, 5, -3], [5, 1, 4], [-5, -4, -4], [-1, -5, 3]],
    3: [[-4, -5, -2], [-4, 2, 1], [4, 5, -2], [-4, 5, -4], [-5, 2, 3], [-2, 0, -5]],
    4: [[-4, 5, -2], [1, -1, -2], [4, -2, 5], [1, -2, 4], [-2, -2, 4], [-3, 4, -5]],
    5: [[-3, -4, -2], [3, 1, -1], [-3, -4, 3], [0, -5, -2], [2, 1, 3], [3, -4, 4]],
    6: [[-5, -4, -4], [2, -1, -5], [-1, 5, -2], [4, -2, -4], [-5, 3, 0], [4, 2, -5]],
    7: [[1, -4, 4], [0, 4, 3], [-2, -1, -1], [-3, 3, -1], [2, 0, -1], [2, -4, 1]],
    8: [[5, -5, 4], [-3, 5, -4], [1, 0, -3], [-2, -1, 1], [3, -2, -1], [-5, -3, -2]],
    9: [[-1, 1, -4], [-1, 4, -1], [0, 3, 2], [-4, 1, 5], [-3, 4, 1], [2, -2, -5]],
    10: [[3, 1, 3], [-4, -3, 2], [-3, -5, 1], [5, -2, -3], [2, -3, 3], [-3, -3, 5]],
    11: [[-1, -3, -1], [-3, 4, -3], [-3, 3, -3], [4, 1, 4], [4, 3, 4], [-1, -2, -1]],
    12: [[1, 4, 0], [5, -1, 0], [-2, 3, 0], [-5, -5, 0], [1, 1, 0], [5, -2, 0]],
    13: [[-4, -4, 0], [-2, 3, 0], [4, 3, 0], [5, -5, 0], [4, -5, 0], [-2, -3, 0]],
    14: [[0, -2, 0], [-4, 0, 0], [1, -1, 0], [1, 1, 0], [2, -2, 0], [3, 1, 0]],
    15: [[3, 3, 3], [0, 4, 0], [2, 1, 2], [-3, 0, -3], [0, 2, 0], [3, 0, 3]],
    16: [[-1, -1, -1], [-3, -1, -3], [-1, 1, -1], [-3, -4, -3], [-5, -1, -5], [-4, 4, -4]],
}


def _exact_separators(t, q):
    """The axes that separate, in Python integers."""
    def sub(a, b):
        return tuple(x - y for x, y in zip(a, b))

    def cross(a, v):
        return (a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0])

    def dot(a, b):
        return sum(x * y for x, y in zip(a, b))

    t, q = [tuple(int(x) for x in p) for p in t], [tuple(int(x) for x in p) for p in q]
    u = [sub(p, q[0]) for p in t]
    v = [sub(p, q[0]) for p in q]
    e = [sub(u[1], u[0]), sub(u[2], u[1]), sub(u[0], u[2])]
    f = [v[1], sub(v[2], v[1]), sub((0, 0, 0), v[2])]
    nT, nQ = cross(e[0], e[1]), cross(f[0], f[1])
    axes = [nQ, nT] + [cross(e[i], f[j]) for i in range(3) for j in range(3)] + [cross(nT, e[i]) for i in range(3)] + [cross(nQ, f[j]) for j in range(3)]
    out = []
    for k, x in enumerate(axes):
        pT, pQ = [dot(x, w) for w in u], [dot(x, w) for w in v]
        if min(pT) > max(pQ) or max(pT) < min(pQ):
            out.append(k)
    return out


@pytest.mark.parametrize("what, t, q, touching", CATALOGUE, ids=[c[0] for c in CATALOGUE])
def test_catalogue(what, t, q, touching):
    hs = pc.hand_scene(tris=[t])
    assert _listed(hs.desc, q) == ([(0, 0)] if touching else []), what
    assert tc.tri_touch32(*(np.array(p, F) for p in t), np.array(q, F)) == touching, "the checker"
    assert (not _exact_separators(t, q)) == touching or not tc._meet(np.array(t).min(0), np.array(t).max(0), np.array(q).min(0), np.array(q).max(0))
    if what == "coplanar disjoint, bounds meeting":
        assert set(_exact_separators(t, q)) <= set(range(11, 17)) and _exact_separators(t, q), "separable only by an in-plane axis"
    # the other vertex orders of the query give the same verdict
    for order in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        assert _listed(hs.desc, tuple(q[k] for k in order)) == ([(0, 0)] if touching else []), f"{what}, query order {order}"


@pytest.mark.parametrize("k", range(17), ids=tc.AXES)
def test_every_axis_is_the_only_separator_of_some_pair(k):
    pts = ONLY_AXIS[k]
    t, q = pts[:3], pts[3:]
    assert tc._meet(np.array(t).min(0), np.array(t).max(0), np.array(q).min(0), np.array(q).max(0)), "the bounds meet: the axes decide"
    assert _exact_separators(t, q) == [k], f"only {tc.AXES[k]} separates"
    assert tc.separators32(*(np.array(p, F) for p in t), np.array(q, F)) == [k], "binary32 is exact on these integers"
    hs = pc.hand_scene(tris=[tuple(tuple(p) for p in t)])
    assert _listed(hs.desc, tuple(tuple(p) for p in q)) == [], "separated: not listed"


# ------------------------------------------------------------------------------------------------------
# against float64, on the pairs with margin
# ------------------------------------------------------------------------------------------------------
def _clear_share(gap, scale, meet, what):
    clear = np.abs(gap) > 1e-4 * scale
    left_out = int((~clear & meet).sum())
    share = left_out / max(int(meet.sum()), 1)
    print(f"{what}: {int(meet.sum())} pairs whose bounds meet, {left_out} of them left out ({100 * share:.3f} %)")
    assert share <= 0.01, f"{what}: the margin leaves out {100 * share:.2f} % of the pairs whose bounds meet"
    return clear


def test_triangle_lists_equal_the_float64_reference():
    hs, tq, offsets, recs, _, _, _ = tc.twin("soup")
    Q = np.stack([tq["a"], tq["b"], tq["c"]], 1)
    valid = np.isfinite(Q).all((1, 2)) & (np.abs(Q).max((1, 2)) < 1e20)          # (the overflowing query has no binary64 story to tell)
    Q = Q[valid]
    A, B, Cc, tg, tp = pc.primitives(hs)["tri"]
    T = np.stack([A, B, Cc], 1)
    touch = tc.tri_touch64(Q, T)
    gap = tc.tri_gap64(Q, T)
    clear = _clear_share(gap, tc.pair_scale(Q, T), tc.bounds_meet64(Q, T), "soup triangles")
    assert np.array_equal(touch[clear], (gap < 0)[clear]), "the segment-triangle reference and the float64 SAT agree on every clear pair"
    got = tc.listed(offsets, recs, tq.size)
    index = np.nonzero(valid)[0]
    member = np.zeros(touch.shape, bool)
    for i, qi in enumerate(index):
        for j in range(len(tg)):
            member[i, j] = (int(qi), int(tg[j]), int(tp[j])) in got
    bad = np.nonzero(clear & (member != touch))
    assert bad[0].size == 0, f"{bad[0].size} clear pairs differ from the float64 reference; first: query {index[bad[0][0]]}, triangle {bad[1][0]}, gap {gap[bad][0]}"
    assert (touch & clear).sum() > 100 and (~touch & clear & tc.bounds_meet64(Q, T)).sum() > 100


@pytest.mark.parametrize("name", ["spheres", "soup"])
def test_sphere_lists_equal_the_float64_distance_bounds(name):
    hs, tq, offsets, recs, _, _, _ = tc.twin(name)
    sc, sr, sg = pc.primitives(hs)["sphere"]
    got = tc.listed(offsets, recs, tq.size)
    gaps, scales, meets, members = [], [], [], []
    for i, t in enumerate(tq):
        q = tc.corners(t).astype(np.float64)
        if not np.isfinite(q).all() or np.abs(q).max() > 1e20:
            continue
        for j in range(len(sg)):
            gaps.append(tc.sphere_gap64(q, sc[j], sr[j]))
            scales.append(max(np.abs(q).max(), np.abs(sc[j]).max() + sr[j]))
            meets.append(bool((sc[j] - sr[j] <= q.max(0)).all() and (sc[j] + sr[j] >= q.min(0)).all()))
            members.append((i, int(sg[j]), 0) in got)
    gaps, scales, meets, members = np.array(gaps), np.array(scales), np.array(meets), np.array(members)
    clear = _clear_share(gaps, scales, meets, f"{name} spheres")
    assert np.array_equal(members[clear], (gaps < 0)[clear])
    assert members.any() and (~members & meets).any()


def test_sphere_exact_cases():
    hs = pc.hand_scene(spheres=[(0.0, 0.0, 0.0, 5.0)])
    cases = [("wholly inside", ((1, 0, 0), (0, 1, 0), (0, 0, 1)), False),
             ("wholly outside, bounds meeting", ((4, 4, 4), (6, 4, 4), (4, 6, 4)), False),
             ("piercing", ((0, 0, 0), (10, 0, 0), (0, 10, 0)), True),
             ("tangent at a vertex, from outside", ((3, 4, 0), (6, 8, 0), (3, 4, 5)), True),
             ("tangent at a vertex, from inside", ((3, 4, 0), (0, 0, 0), (1, 0, 0)), True),
             ("a point on the shell", ((0, 0, 5), (0, 0, 5), (0, 0, 5)), True),
             ("a point at the centre", ((0, 0, 0), (0, 0, 0), (0, 0, 0)), False)]
    for what, q, touching in cases:
        assert _listed(hs.desc, q) == ([(0, 0)] if touching else []), what
        assert tc.sphere_touch32((0, 0, 0), 5.0, np.array(q, F)) == touching, what


def test_discs_are_never_missed_and_the_over_listing_is_counted():
    discs = [(0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 0.0), (1.0, 2.0, -1.0, 1.5, 6.0, 0.0, 0.0), (0.3, -0.4, 0.5, 3.0, 0.0, 8.0, 1.0)]
    hs = pc.hand_scene(discs=discs)
    rng = np.random.default_rng(71)
    n = 900
    centre = np.array([[d[4], d[5], d[6]] for d in discs], F)[rng.integers(0, 3, n)]
    size = rng.choice(np.array([0.3, 1.0, 3.0, 8.0], F), (n, 1, 1))
    Q = (centre[:, None, :] + rng.normal(0, 1.5, (n, 1, 3)).astype(F) + size * rng.uniform(-0.5, 0.5, (n, 3, 3)).astype(F)).astype(F)
    tq = tc.tris(list(Q))
    offsets, recs = _full(hs.desc, tq)
    got = tc.listed(offsets, recs, n)
    ck = tc.TriChecker(hs)
    touching = missed = over = listed_n = 0
    for i in range(n):
        want = ck.contacts(tq[i])[0]
        assert sorted((g, p) for (k, g, p) in got if k == i) == want, "the twin is the checker"
        for j, d in enumerate(discs):
            gap = tc.disc_gap64(Q[i], d[:3], d[4:], d[3])
            scale = max(float(np.abs(Q[i]).max()), float(np.abs(np.array(d[4:])).max()) + d[3])
            is_listed = (i, j, 0) in got
            listed_n += is_listed
            if gap < -1e-4 * scale:
                touching += 1
                missed += not is_listed
            elif gap > 1e-4 * scale:
                over += is_listed
    print(f"discs: {listed_n} listed, {touching} clearly touching, {missed} missed, {over} listed without touching ({100 * over / max(listed_n, 1):.1f} % of the listed)")
    assert touching > 100 and missed == 0, "no touching disc is missed"


# ------------------------------------------------------------------------------------------------------
# order, padding, caller-made offsets, capacity
# ------------------------------------------------------------------------------------------------------
def test_first_k_padding_key_order_and_capacity_cuts():
    hs, tq, offsets, recs, counts, _, _ = tc.twin("soup")
    ck = tc.TriChecker(hs)
    lists = [ck.contacts(t)[0] for t in tq]
    for i, x in enumerate(lists):
        assert x == sorted(set(x)), "keys ascend and are unique within a query"
    for k in (1, 3, 8):
        got, v = irl.tri_fill_host(hs.desc, tq, tc.k_offsets(tq.size, k))
        want = np.concatenate([tc.records(x, i, k) for i, x in enumerate(lists)])
        pc.assert_bytes_equal(got, want, f"the first {k}: the smallest keys, padded with the empty record")
    pad = tc.records([], 5, 1)[0]
    assert (int(pad["primID"]), int(pad["geomID"]), int(pad["flags"]), int(pad["tri"]), int(pad["reserved"])) == (irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, 5, 0)
    total = recs.size
    for capacity in (total - 1, total // 2, 0):
        buf = tc.sentinel_buffer(total)
        irl.tri_fill_host(hs.desc, tq, offsets, capacity=capacity, hits=buf)
        assert tc.is_sentinel(buf[capacity:]).all(), "nothing at or past capacity"
        assert buf[:capacity].tobytes() == recs[:capacity].tobytes(), f"capacity {capacity}: the records before it"
    # a decreasing pair is an empty segment, and is not walked
    off = np.array([5, 0, 3], np.uint64)
    buf = tc.sentinel_buffer(8)
    two = tq[[12, 12]]
    _, v = irl.tri_fill_host(hs.desc, two, off, capacity=8, hits=buf)
    want = tc.records(lists[12], 1, 3)
    pc.assert_bytes_equal(buf[0:3], want, "the second query's segment")
    assert tc.is_sentinel(buf[3:]).all() and v["box_tests"] == ck.contacts(tq[12])[1]
    # an empty scene, and n == 0
    empty = pc.hand_scene()
    assert irl.tri_query_host(empty.desc, tc.COUNT, tq)[0].sum() == 0
    assert irl.tri_offsets_host(hs.desc, tq[:0])[0].tolist() == [0]
