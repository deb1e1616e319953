"""The triangle test without the verdicts its t carries (csrc/tri_math.hpp, POS) and with the error bound's minima as min_abs3, in the
kernels (pytest -m gpu; the arithmetic alone is tests/test_tri_verdict.py). K1w leaves out `det == 0`, `det < 0 & tScaled >= 0`,
`det > 0 & tScaled <= 0` and the `t < inf` of its candidate test, and so does every query family through prim_hit: frames of scenes
made of what those verdicts used to turn away - triangles seen from behind, triangles behind the origin of a ray that enters their
box, zero-area and collinear triangles, a floor the bounce rays start on, and all of them beside sphere and disc lanes - must be the
oracle's byte for byte, with the oracle's node and leaf counters in the instrumented build: on the shared arrays (hot_nodes 0) and on
the private copy (hot_nodes 96), with and without vertex normals (the barycentric builds), under option double_fallback, and in one
NIF-slot render. One query per family that runs the test (closest hit, any hit, count, list), with t_min < 0 and t_max = +inf over
the degenerate and behind-the-origin triangles, against the host checkers of those families."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import count_cases as cc
import list_cases as lc
from test_gpu_parity import _nif_weights, assert_streams_identical, rows_differing
from test_leaf_turn_gpu import _params, _with_normals
from test_query_gpu import assert_bytes_equal, oracle_query

pytestmark = pytest.mark.gpu

HOT = (0, 96)

# The camera stands at the origin and looks down -z.
FRONT = [[-6, -5, -5], [6, -5, -5], [0, 6, -5.5]]                      # fills most of the view
SIDE = [[5, -6, -1], [5, 6, -1], [4, 0, -9]]
FLOOR = [[[-30, -1, 10], [30, -1, 10], [30, -1, -40]], [[-30, -1, 10], [30, -1, -40], [-30, -1, -40]]]
WALL = [[[-30, -1, -12], [30, -1, -12], [0, 40, -12]]]
# A slanted sheet that passes over the camera: its box holds the origin, so every camera ray enters it; the rays that look up cross
# the sheet ahead, the rays that look down cross its plane behind them (t < 0). And a triangle wholly behind the camera.
SHEET = [[-50, -4, 30], [50, -4, 30], [0, 25, -60]]
REAR = [[-3, -2, 5], [3, -2, 5.5], [0, 3, 5]]
# No area: a repeated vertex, three points on a line, one point three times - each with a box the camera rays enter (the point's is
# entered by the rays that pass through it alone).
REPEATED = [[-3, -2, -4], [3, 2, -4.5], [3, 2, -4.5]]
COLLINEAR = [[-3, 2, -3.5], [0, 0, -4], [3, -2, -4.5]]
POINT = [[0.25, 0.25, -3], [0.25, 0.25, -3], [0.25, 0.25, -3]]
SPHERES = [(-2.0, 0.2, -6.0, 1.0), (1.5, -0.3, -3.5, 0.6)]
DISCS = [(0.0, 1.0, 0.0, 2.5, 0.0, -0.95, -4.0), (0.3, 0.2, 1.0, 1.2, -1.0, 1.5, -4.5)]


def _reversed(tris):
    return [[t[0], t[2], t[1]] for t in tris]


def _scene(tris, spheres=(), discs=()):
    p = np.asarray(tris, np.float32).reshape(-1, 3)
    hs = cc.mesh_scene(p, np.arange(len(p), dtype=np.uint16).reshape(-1, 3), spheres, discs)
    m = hs.materials
    m["albedo"]["x"], m["albedo"]["y"], m["albedo"]["z"] = .7, .6, .5
    return hs


def _geometry(name):
    if name == "seen from behind":            # every triangle in the winding that gives det < 0 for a camera ray (asserted by the test)
        return _scene(_reversed([FRONT, SIDE] + FLOOR))
    if name == "behind the origin":
        return _scene([SHEET, REAR, FRONT])
    if name == "no area":
        return _scene([REPEATED, COLLINEAR, POINT, FRONT])
    if name == "floor":
        return _scene(FLOOR + WALL)
    if name == "everything beside spheres and discs":
        return _scene(_reversed([SIDE]) + [SHEET, REAR, REPEATED, COLLINEAR, POINT] + FLOOR + WALL, SPHERES, DISCS)
    raise KeyError(name)


NAMES = ("seen from behind", "behind the origin", "no area", "floor", "everything beside spheres and discs")
CASES = [(n, normals) for n in NAMES for normals in (False, True)]


def _case(name, normals):
    hs = _geometry(name)
    if normals:
        hs = _with_normals(hs)
    return hs, _params(hs.desc, 48, 32, 8)


@pytest.fixture(scope="module")
def oracle_frames():
    """Every case's scene, the oracle's frame of it and the oracle's counters, computed once."""
    out = {}
    for name, normals in CASES:
        hs, d = _case(name, normals)
        want = hs.init_ray_stream()
        first = want.copy()
        st = ol.path_trace_pixel_rng(d, want, 16)
        out[(name, normals)] = (hs, d, first, want, st)
    return out


def _oracle_det_signs(hs, tri):
    """Signs of e0 + e1 + e2 of the oracle's test over the un-jittered camera rays that cross `tri` (read off the barycentrics' common
    sign is not possible - they are e / det - so the edge functions are recomputed here in float64 on the oracle's shear)."""
    first = hs.init_ray_stream()
    r = first["h"]["r"]
    signs = set()
    o = ol.lib()
    for i in range(0, first.size, 7):
        ray = ol.Ray.from_buffer_copy(np.ascontiguousarray(r[i]).tobytes())
        sh = ol.Shear(); o.o_ray_shear(C.byref(ray), C.byref(sh))
        q = []
        for p in np.asarray(tri, np.float64):
            v = [p[sh.ix], p[sh.iy], p[sh.iz]]
            q.append((v[0] + float(sh.sx) * v[2], v[1] + float(sh.sy) * v[2]))
        e = [q[1][0] * q[2][1] - q[1][1] * q[2][0], q[2][0] * q[0][1] - q[2][1] * q[0][0], q[0][0] * q[1][1] - q[0][1] * q[1][0]]
        if all(x < 0 for x in e) or all(x > 0 for x in e):
            signs.add(e[0] > 0)
    return signs


@pytest.mark.parametrize("name,normals", CASES)
def test_frame_and_counters_are_the_oracles(oracle_frames, name, normals):
    hs, d, first, want, st = oracle_frames[(name, normals)]
    assert st.leafTests > 0 and st.casts > st.paths      # (paths that bounce: casts from a surface among them)
    if name == "seen from behind":
        assert _oracle_det_signs(hs, _reversed([FRONT])[0]) == {False}, "the camera rays must see the front triangle with det < 0"
    for hot in HOT:
        what = f"{name}, normals={normals}, hot_nodes={hot}"
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert_streams_identical(got, want, what)
        dev = irl.IpuScene(d).set_option("hot_nodes", hot).set_option("full_stats", 1)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
        c = dev.counters(); dev.close()
        assert_streams_identical(got, want, what + ", instrumented build")
        assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (st.casts, st.nodesVisited, st.leafTests, st.paths), what


@pytest.mark.parametrize("name", ["no area", "floor", "everything beside spheres and discs"])
def test_double_fallback_frames(name):
    """Option double_fallback: the edge functions that are exactly zero (the degenerate triangles', the floor's under a bounce ray
    that starts on it) are recomputed in binary64, on both sides."""
    hs, d = _case(name, False)
    first = hs.init_ray_stream(); want = first.copy()
    with ol.double_fallback():
        st = ol.path_trace_pixel_rng(d, want, 16)
    for hot in HOT:
        dev = irl.IpuScene(d).set_option("hot_nodes", hot).set_option("double_fallback", 1)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert_streams_identical(got, want, f"{name}, double_fallback, hot_nodes={hot}")
    dev = irl.IpuScene(d).set_option("double_fallback", 1).set_option("full_stats", 1)
    got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE)
    c = dev.counters(); dev.close()
    assert_streams_identical(got, want, f"{name}, double_fallback, instrumented build")
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (st.casts, st.nodesVisited, st.leafTests, st.paths)


def test_nif_slot_render():
    """K1w's slot build. What the LEAF turn decides is the hit record - the primitive, its normal, the throughput and the escaped ray's
    direction, which is what the MLP is asked about: the oracle's byte for byte. rgb is the MLP's output in half precision, whose tolerance
    is another test's subject (test_gpu_parity.py::test_config5_monkey_with_nif_environment): here it only has to be finite."""
    rng = np.random.default_rng(8)
    ks, bs, relu = _nif_weights(rng, hidden=64, embed=12, layers=4)
    mean = np.array([-2.35, -2.26, -1.96], np.float32)
    hs, d = _case("everything beside spheres and discs", False)
    nif, keep = ol.make_nif(ks, bs, relu, 12, 3.43, mean, True, half_features=True, half_weights_acts=True)
    first = hs.init_ray_stream(); want = first.copy()
    st = ol.Stats()
    ol.lib().o_path_trace_nif_pixel_rng(C.byref(d), C.byref(nif), 0.0, want.ctypes.data, want.size, 16, C.byref(st))
    assert np.any(want["h"]["flags"] == irl.FLAG_ESCAPED) and np.any(want["h"]["flags"] != irl.FLAG_ESCAPED)
    for hot in HOT:
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        dev.setNif(ks, bs, relu, 12, 3.43, mean, True)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert rows_differing(np.ascontiguousarray(got["h"]), np.ascontiguousarray(want["h"])).size == 0, f"hit records, hot_nodes={hot}"
        assert all(np.all(np.isfinite(got["rgb"][k])) for k in "xyz")


# ---- the query families: every one of them accepts through prim_hit, which took the flag ----------------------------------------------
def _query_scene_and_rays(round_prims, n=1200):
    """The degenerate and the behind-the-origin triangles and both windings of a plain one - beside a sphere and a disc for the
    families whose checkers say what a sphere or a disc gives under a negative t_min (count, list); rays from about the
    camera in every direction - a third of them straight at a vertex of a degenerate triangle or along the sheet's plane - with
    t_min in {-1, -inf, 0} and t_max = +inf."""
    tris = [SHEET, REAR, REPEATED, COLLINEAR, POINT, FRONT] + _reversed([SIDE])
    hs = _scene(tris, SPHERES[:1], DISCS[:1]) if round_prims else _scene(tris)
    rng = np.random.default_rng(29)
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    targets = np.asarray([REPEATED[0], REPEATED[1], COLLINEAR[1], POINT[0], SHEET[2], REAR[0]], np.float32)
    k = np.arange(n)
    aimed = k % 3 == 0
    d[aimed] = targets[k[aimed] % len(targets)] - o[aimed]
    inplane = k % 12 == 1      # origin on the sheet's plane, direction inside it
    a, b, c = np.asarray(SHEET, np.float32)
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    o[inplane] = (a + (b - a) * u[inplane, :1] * np.float32(.5) + (c - a) * u[inplane, 1:] * np.float32(.5)).astype(np.float32)
    d[inplane] = ((b - a) * rng.normal(size=(int(inplane.sum()), 1)) + (c - a) * rng.normal(size=(int(inplane.sum()), 1))).astype(np.float32)
    t_min = np.where(k % 5 == 0, np.float32(0), np.where(k % 5 == 1, np.float32(-np.inf), np.float32(-1))).astype(np.float32)
    rays = qb.make_rays(o, d)
    rays["tMin"] = t_min
    rays["tMax"] = np.float32(np.inf)
    return hs, rays


def test_closest_and_any_hit_queries():
    """Triangles only: under a negative t_min a sphere's or a disc's miss (t = 0) passes t > t_min on both sides, and the closest-hit
    query then reports primID 0 where the oracle reports none - the primitive test's callers are this file's subject, not that."""
    hs, rays = _query_scene_and_rays(False)
    want, occ, _, _ = oracle_query(hs, rays)
    assert (want["primID"] != irl.INVALID_PRIM).mean() > 0.1 and (want["primID"] == irl.INVALID_PRIM).any()
    for k in (0, 1):
        dev = irl.IpuScene(hs.desc).set_option("query_kernel", k)
        assert_bytes_equal(dev.intersect(rays), want, f"closest hit, query_kernel {k}")
        assert np.array_equal(dev.occluded(rays), occ), f"any hit, query_kernel {k}"
        dev.close()


def test_count_and_list_queries():
    hs, rays = _query_scene_and_rays(True)
    lists = lc.ListChecker(hs).lists(rays)
    want = np.array([len(x) for x in lists], np.uint32)
    assert want.max() >= 2 and (want == 0).any()
    assert np.array_equal(want, cc.Checker(hs).counts(rays)[0])
    dev = irl.IpuScene(hs.desc)
    got = dev.count_crossings(rays)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size}/{rays.size} counts differ, first {bad[:4]}: got {got[bad[:4]]} want {want[bad[:4]]}"
    offsets, hits = dev.list_crossings(rays)
    dev.close()
    want_offsets, want_hits = lc.packed(lists)
    assert np.array_equal(offsets, want_offsets)
    assert hits.tobytes() == want_hits.tobytes(), "crossing lists differ from the checker's"
