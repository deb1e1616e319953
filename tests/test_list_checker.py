"""The crossing-list checker (tests/list_cases.py) and sphere_roots without a GPU, against things they share no code with: another
tree over the same primitives (a list is canonical: it may not depend on the tree), the crossing-count checker, the oracle's own
closest-hit walk, and mi_sphere_roots_host - the definition the kernels run, compiled for the host."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import count_cases as cc
import list_cases as lc
from test_count_checker import _random_sphere_cases

F = np.float32


@pytest.mark.parametrize("name", ["layers", "soup", "mixed"])
def test_lists_do_not_depend_on_the_tree_and_have_the_counted_length(name):
    hs, rays, lists = lc.case(name)
    nodes, _ = irl.build_lbvh(hs.desc)
    assert nodes.tobytes() != np.ascontiguousarray(hs.nodes).tobytes(), "the second tree is the first"
    other = lc.ListChecker(lc.with_nodes(hs, nodes)).lists(rays)
    bad = [i for i in range(rays.size) if lists[i] != other[i]]
    assert not bad, f"{name}: {len(bad)} lists differ between the two trees, first ray {bad[0]}"
    # the same tuples on both trees means the same bytes: the floats compare equal AND carry the same bits
    assert lc.packed(lists)[1].tobytes() == lc.packed(other)[1].tobytes()
    counts = cc.Checker(hs).counts(rays)[0]
    assert np.array_equal(np.array([len(x) for x in lists], np.uint32), counts)
    assert counts.max() >= 2 and (counts == 0).any()
    for i, x in enumerate(lists):
        keys = [lc.key(r) for r in x]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), f"{name}: ray {i} is not strictly sorted by the key"


def test_layers_has_long_lists_exact_ties_and_both_sphere_roots():
    hs, rays, lists = lc.case("layers")
    lens = np.array([len(x) for x in lists])
    assert lens.mean() > 20 and lens.max() > 60
    tied = [x for x in lists if any(a[0] == b[0] for a, b in zip(x, x[1:]))]
    assert len(tied) > 500
    # a tie between the two copies of a quad is ordered by primID
    assert any(a[0] == b[0] and a[1] == b[1] and a[2] < b[2] for x in tied for a, b in zip(x, x[1:]))
    assert any(r[3] == 1 for x in lists for r in x) and any(r[3] == 0 and r[1] >= 1 and r[1] <= 8 for x in lists for r in x)


@pytest.mark.parametrize("name", ["soup-tris", "cube", "box-simple"])
def test_the_front_record_is_the_oracles_closest_hit(name):
    """No sphere in these scenes, so a list's first record is what CompactBvh::intersect finds - t, geomID and primID - and an empty
    list is a miss, for every ray."""
    hs = cc.scene(name)
    n = {"soup-tris": 2500, "cube": 2000, "box-simple": 2000}[name]
    rays = cc.mixed_rays(hs, n, 5)
    lists = lc.ListChecker(hs).lists(rays)
    o = ol.lib()
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    hits = 0
    for i in range(rays.size):
        want = o.o_bvh_intersect(C.byref(hs.desc), C.byref(buf[i]), None)
        if not want.hit:
            assert lists[i] == [], (name, i)
            continue
        hits += 1
        t, g, p, far = lists[i][0]
        assert (F(t).view(np.uint32), g, p, far) == (F(want.t).view(np.uint32), want.geomID, want.primID, 0), (name, i)
    assert hits > n // 10


def test_sphere_roots_host_is_the_restatement_bit_for_bit():
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    for c, radius, o, d, t_min, t_max in _random_sphere_cases(4000, 17):
        r2 = F(radius * radius)
        mask, t0, t1 = irl.sphere_roots_host(c, r2, o, d, t_min, t_max)
        want, w0, w1 = lc.sphere_roots32(c, r2, o, d, t_min, t_max)
        assert mask == want, (c, radius, o, d, t_min, t_max)
        if w0 is not None:
            assert F(t0).view(np.uint32) == w0.view(np.uint32) and F(t1).view(np.uint32) == w1.view(np.uint32)
        else:
            assert np.isnan(t0) and np.isnan(t1)          # a line that misses leaves t as it was
        assert bin(mask).count("1") == irl.sphere_crossings_host(c, r2, o, d, t_min, t_max)
        seen[mask] += 1
    assert min(seen.values()) > 10, seen          # (the near root alone needs t_max between the roots: the rarest of the four)


def test_sphere_roots_host_edges():
    c, r2 = (0.0, 0.0, 0.0), 1.0
    assert irl.sphere_roots_host(c, r2, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0)) == (3, 2.0, 4.0)
    assert irl.sphere_roots_host(c, r2, (0.5, 0.0, 0.0), (1.0, 0.0, 0.0)) == (2, -1.5, 0.5)          # inside: the far root alone
    assert irl.sphere_roots_host(c, r2, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.0, 3.0) == (1, 2.0, 4.0)
    assert irl.sphere_roots_host(c, r2, (-3.0, 1.0, 0.0), (1.0, 0.0, 0.0)) == (3, 3.0, 3.0)          # tangent: both, the same t
    assert irl.sphere_roots_host(c, r2, (-3.0, 2.0, 0.0), (1.0, 0.0, 0.0))[0] == 0
    assert irl.sphere_roots_host(c, r2, (-3.0, 0.0, 0.0), (float("nan"), 0.0, 0.0))[0] == 0
    null = C.POINTER(C.c_float)()
    v = (C.c_float * 3)(0, 0, 0)
    assert irl.host_lib().mi_sphere_roots_host(v, 1.0, v, v, 0.0, 1.0, null) == 0
