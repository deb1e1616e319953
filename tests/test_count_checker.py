"""The crossing-count checker (tests/count_cases.py) and sphere_crossings without a GPU, against things they share no code with:
the oracle's own any-hit walk, the analytic inside of a closed cube and of an icosphere under the default direction - with NO
exception allowed: a wrong parity means a box test dropped a primitive or the checker is wrong, never that a cap was too tight -,
and a binary64 count of a sphere's roots."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import count_cases as cc

F = np.float32


# ------------------------------------------------------------------------------------------------------
# the checker against the oracle's any-hit walk
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "soup", "box-simple", "soup-tris"])
def test_count_positive_where_the_oracle_is_occluded(name):
    """count > 0 exactly where o_bvh_occluded answers 1, for 2 000 mixed rays. box and soup carry spheres: there the two differ by
    design for a ray that starts inside a sphere with the centre behind it (the reference's sphere test gives up, the count sees the
    crossing ahead), and for exactly those rays the count may only say more, never less. box-simple and soup-tris have no sphere:
    no exception of any kind."""
    hs = cc.scene(name)
    rays = cc.mixed_rays(hs, 2000, seed=11)
    counts, boxes, tests = cc.Checker(hs).counts(rays)
    o = ol.lib()
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    occ = np.array([bool(o.o_bvh_occluded(C.byref(hs.desc), C.byref(buf[i]), None)) for i in range(rays.size)])
    assert occ.any() and (~occ).any() and counts.max() >= 2
    by_design = cc.centre_behind_inside_sphere(hs, rays)
    if name in ("box-simple", "soup-tris"):
        assert not by_design.any()
    bad = np.nonzero(((counts > 0) != occ) & ~by_design)[0]
    assert bad.size == 0, f"{name}: {bad.size} rays differ, first {bad[:4]}: counts {counts[bad[:4]]}"
    assert np.all((counts > 0)[by_design] | ~occ[by_design])
    # a ray with t_min > t_max crosses nothing
    empty = rays["tMin"] > rays["tMax"]
    assert empty.any() and not counts[empty].any()


# ------------------------------------------------------------------------------------------------------
# parity against analytic insides
# ------------------------------------------------------------------------------------------------------
def test_cube_parity_is_the_analytic_inside():
    hs = cc.scene("cube")
    assert hs.tris.size == 36
    pos, want = cc.cube_points()
    assert len(pos) == 4096 + 11 ** 3 and want.any() and (~want).any()
    got = cc.Checker(hs).inside(pos)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"cube: {bad.size} wrong parities, first at {pos[bad[:4]]}"


def test_icosphere_parity_is_the_analytic_inside():
    hs = cc.scene("icosphere")
    assert hs.tris.size == 3 * 320
    pos, want = cc.icosphere_points()
    assert want.sum() > 200 and (~want).sum() > 200
    got = cc.Checker(hs).inside(pos)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"icosphere: {bad.size} wrong parities, first at {pos[bad[:4]]}"
    # and the BVH dropped nothing: the same triangle test over every triangle, no boxes
    sub = np.arange(0, len(pos), 8)
    assert np.array_equal(cc.brute_force_parity(hs, pos[sub]), want[sub])


def test_an_axis_direction_sees_no_triangle():
    """Why mi_point_sign refuses a direction with a zero component: the reference's shear divides by the SMALLEST signed component."""
    hs = cc.scene("cube")
    pos = np.random.default_rng(3).uniform(-0.9, 0.9, (64, 3)).astype(F)
    assert not cc.Checker(hs).inside(pos, direction=(1.0, 0.0, 0.0)).any()


# ------------------------------------------------------------------------------------------------------
# sphere_crossings
# ------------------------------------------------------------------------------------------------------
def _random_sphere_cases(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        c = rng.uniform(-5, 5, 3).astype(F)
        radius = F(rng.uniform(0.2, 3.0))
        o = (c + rng.normal(size=3) * radius * rng.uniform(0, 2.5)).astype(F)
        d = rng.normal(size=3); d = (d / np.linalg.norm(d) * 10 ** rng.uniform(-1, 1)).astype(F)
        span = float(radius) * 4 / float(np.linalg.norm(d))
        t_min = F(rng.choice([0.0, rng.uniform(0, span)]))
        t_max = F(rng.choice([np.inf, rng.uniform(0, 2 * span)]))
        yield c, radius, o, d, t_min, t_max


def test_sphere_crossings_host_against_binary64():
    checked = {0: 0, 1: 0, 2: 0}
    scaled = 0
    for c, radius, o, d, t_min, t_max in _random_sphere_cases(4000, 17):
        r2 = F(radius * radius)
        got = irl.sphere_crossings_host(c, r2, o, d, t_min, t_max)
        assert got == cc.sphere_crossings32(c, r2, o, d, t_min, t_max)          # the contract's text, in numpy binary32
        want, roots = cc.sphere_crossings64(c, float(radius), o, d, float(t_min), float(t_max))
        if roots is None:
            continue
        # t is in units of d: a margin of 1e-3 radius in space is 1e-3 radius / |d| in t
        m = 1e-3 * float(radius) / float(np.linalg.norm(d.astype(np.float64)))
        if roots[1] - roots[0] <= m or any(abs(t - b) <= m for t in roots for b in (float(t_min), float(t_max))):
            continue
        assert got == want, (c, radius, o, d, t_min, t_max, got, want)
        checked[want] += 1
        # a direction three times as long, the interval in its units: the same crossings
        assert irl.sphere_crossings_host(c, r2, o, (d * F(3)).astype(F), F(t_min / F(3)), F(t_max / F(3))) == got
        scaled += 1
    assert min(checked.values()) > 100 and scaled > 100, (checked, scaled)


def test_sphere_crossings_host_edges():
    c, r2 = (0.0, 0.0, 0.0), 1.0
    # an origin inside the sphere, the centre behind it: the one crossing ahead (the reference's test answers "miss" here)
    assert irl.sphere_crossings_host(c, r2, (0.5, 0.0, 0.0), (1.0, 0.0, 0.0)) == 1
    assert irl.sphere_crossings_host(c, r2, (0.5, 0.1, -0.2), cc.DEFAULT_DIR) == 1
    # the centre ahead: also one; from outside: two, or none when the sphere lies behind
    assert irl.sphere_crossings_host(c, r2, (-0.5, 0.0, 0.0), (1.0, 0.0, 0.0)) == 1
    assert irl.sphere_crossings_host(c, r2, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0)) == 2
    assert irl.sphere_crossings_host(c, r2, (3.0, 0.0, 0.0), (1.0, 0.0, 0.0)) == 0
    assert irl.sphere_crossings_host(c, r2, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.0, 3.0) == 1          # the interval cuts the far root
    assert irl.sphere_crossings_host(c, r2, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0), 2.5, np.inf) == 1       # ... the near root
    # tangent rays: l2 == radius2 exactly gives td == 0 and t0 == t1: 2; just outside: 0. Never 1: a parity survives
    assert irl.sphere_crossings_host(c, r2, (-3.0, 1.0, 0.0), (1.0, 0.0, 0.0)) == 2
    assert irl.sphere_crossings_host(c, r2, (-3.0, float(np.nextafter(F(1), F(2))), 0.0), (1.0, 0.0, 0.0)) == 0
    rng = np.random.default_rng(23)
    for _ in range(500):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3)); w /= np.linalg.norm(w)
        o = (u + w * rng.uniform(-3, -1)).astype(F)          # on a tangent line of the unit sphere, up to rounding
        assert irl.sphere_crossings_host(c, r2, o, w.astype(F)) in (0, 2)
    # a NaN never counts
    nan = float("nan")
    for args in (((nan, 0, 0), 1.0, (-3, 0, 0), (1, 0, 0)), ((0, 0, 0), nan, (-3, 0, 0), (1, 0, 0)), ((0, 0, 0), 1.0, (-3, nan, 0), (1, 0, 0)),
                 ((0, 0, 0), 1.0, (-3, 0, 0), (1, nan, 0)), ((0, 0, 0), 1.0, (-3, 0, 0), (0, 0, 0))):
        assert irl.sphere_crossings_host(*args) == 0, args
    assert irl.sphere_crossings_host(c, r2, (-3, 0, 0), (1, 0, 0), nan, np.inf) == 0
    assert irl.sphere_crossings_host(c, r2, (-3, 0, 0), (1, 0, 0), 0.0, nan) == 0
