"""Crossing counts, inside tests and signed distance on the GPU (mi_count_query*, mi_point_sign*): device counts against the
checker of tests/count_cases.py, exactly; against the device's own any-hit answers; inside against analytic answers with no
exception allowed; signed distance against closest_points byte for byte; launch shapes, counters, a live scene, plumbing."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import count_cases as cc

pytestmark = pytest.mark.gpu

F = np.float32
SIGN = np.uint32(0x80000000)


@pytest.fixture(scope="module")
def cases():
    """name -> (host scene, 2 048 mixed rays, the checker's counts, its box tests, its primitive tests), computed once."""
    cache = {}

    def get(name, n=2048):
        if name not in cache:
            hs = cc.scene(name)
            rays = cc.mixed_rays(hs, n, seed=31 + len(name))
            cache[name] = (hs, rays) + cc.Checker(hs).counts(rays)
        return cache[name]
    return get


def _masked(rec):
    """POINT_HIT records with the sign bit of dist and FLAG_INSIDE cleared, as bytes per record."""
    w = rec.copy().view(np.uint32).reshape(rec.size, 8)
    w[:, 0] &= ~SIGN
    w[:, 2] &= ~np.uint32(irl.FLAG_INSIDE << 16)
    return w


def _sign_of(rec):
    return (rec["dist"].view(np.uint32) & SIGN) != 0


# ------------------------------------------------------------------------------------------------------
# counts
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "spheres", "soup", "mixed"])
def test_counts_equal_the_checkers(cases, name):
    hs, rays, want, boxes, tests = cases(name)
    assert want.max() >= 2 and (want == 0).any()
    dev = irl.IpuScene(hs.desc)
    got = dev.count_crossings(rays)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: {bad.size}/{rays.size} counts differ, first {bad[:4]}: got {got[bad[:4]]} want {want[bad[:4]]}"
    c = dev.counters()
    assert c["casts"] == rays.size and c["nodes_visited"] == 0 and c["leaf_tests"] == 0 and c["paths"] == 0
    dev.close()


def test_double_fallback_counts_on_grazing_rays():
    differing = 0
    for seed in range(4):
        hs = cc.grazing_scene(np.random.default_rng(900 + seed), 48)
        rays = cc.grazing_rays(seed)
        res = {}
        for df in (0, 1):
            if df:
                with ol.double_fallback():
                    want = cc.Checker(hs).counts(rays)[0]
            else:
                want = cc.Checker(hs).counts(rays)[0]
            dev = irl.IpuScene(hs.desc).set_option("double_fallback", df)
            got = dev.count_crossings(rays)
            dev.close()
            assert np.array_equal(got, want), f"grazing rays, double_fallback {df}, seed {seed}: {(got != want).sum()} counts differ"
            res[df] = want
        differing += int((res[0] != res[1]).sum())
    assert differing > 0, "the constructed rays never took the binary64 branch to a different count"


@pytest.mark.parametrize("name", ["box", "soup", "box-simple", "soup-tris"])
def test_count_positive_where_the_device_is_occluded(name):
    """Device against device, 50 000 rays, independent of the checker: count > 0 exactly where the any-hit query answers 1. box
    and soup carry spheres; there a ray that starts inside a sphere with the centre behind it differs by design (the reference's
    sphere test gives up, the count sees the crossing ahead) and may only say more; box-simple and soup-tris have no sphere and no
    exception."""
    hs = cc.scene(name)
    rays = cc.mixed_rays(hs, 50000, seed=77)
    dev = irl.IpuScene(hs.desc)
    counts, occ = dev.count_crossings(rays), dev.occluded(rays)
    dev.close()
    by_design = cc.centre_behind_inside_sphere(hs, rays)
    if name in ("box-simple", "soup-tris"):
        assert not by_design.any()
    assert occ.any() and (~occ).any()
    bad = np.nonzero(((counts > 0) != occ) & ~by_design)[0]
    assert bad.size == 0, f"{name}: {bad.size} rays differ, first {bad[:4]}: counts {counts[bad[:4]]}"
    assert np.all((counts > 0)[by_design] | ~occ[by_design])


# ------------------------------------------------------------------------------------------------------
# inside
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_inside_is_the_analytic_answer(name):
    hs = cc.scene(name)
    pos, want = cc.cube_points() if name == "cube" else cc.icosphere_points()
    dev = irl.IpuScene(hs.desc)
    got = dev.inside(cc.points_of(pos))
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    bad = np.nonzero(got.astype(bool) != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} wrong answers, first at {pos[bad[:4]]}"
    # the radius is ignored, a point that is not finite gets 0
    pts = cc.points_of(pos[:64], radius=-1.0)
    pts["radius"][1::2] = np.nan
    assert np.array_equal(dev.inside(pts), got[:64])
    odd = cc.points_of(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, 0]], F))
    assert dev.inside(odd).tolist() == [0, 0, 0, 1]
    # another direction, and the same answers
    assert np.array_equal(dev.inside(cc.points_of(pos), direction=(-0.83, 0.47, -0.31)).astype(bool), want)
    dev.close()


def test_inside_three_spheres():
    hs = cc.scene("three-spheres")
    pos, want = cc.sphere_points(cc.THREE_SPHERES, 3000, seed=9)
    # points whose default ray leaves the sphere with the centre behind them are among them
    d = cc.DEFAULT_DIR.astype(np.float64)
    behind = np.zeros(len(pos), bool)
    for s in cc.THREE_SPHERES:
        f = np.array(s[:3]) - pos.astype(np.float64)
        behind |= ((f * f).sum(1) < s[3] ** 2) & ((f @ d) < 0)
    assert behind.sum() >= 48 and want[behind].all() and (~want).sum() > 500
    dev = irl.IpuScene(hs.desc)
    got = dev.inside(cc.points_of(pos)).astype(bool)
    dev.close()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"three spheres: {bad.size} wrong answers, first at {pos[bad[:4]]}"


# ------------------------------------------------------------------------------------------------------
# signed distance
# ------------------------------------------------------------------------------------------------------
def test_signed_distance_is_closest_points_with_a_sign():
    hs = cc.scene("mixed")
    rng = np.random.default_rng(41)
    pos = rng.uniform(-6, 6, (6000, 3)).astype(F)
    pos[:1500] = rng.uniform(-1.2, 1.2, (1500, 3)).astype(F)                     # in and around the cube
    radius = rng.choice(np.array([np.inf, 0.5, 0.0], F), len(pos), p=[0.6, 0.3, 0.1]).astype(F)
    pts = qb.make_points(pos, radius)
    dev = irl.IpuScene(hs.desc)
    closest, sd, ins = dev.closest_points(pts), dev.signed_distance(pts), dev.inside(pts).astype(bool)
    assert ins.sum() > 300 and (~ins).sum() > 300
    assert np.array_equal(_masked(sd), closest.view(np.uint32).reshape(-1, 8)), "signed distance: not closest_points' bytes"
    assert np.array_equal(_sign_of(sd), ins) and np.array_equal((sd["flags"] & irl.FLAG_INSIDE) != 0, ins)
    assert not _sign_of(closest).any() and not (closest["flags"] & irl.FLAG_INSIDE).any()
    # radius too small: -+ radius as given, ESCAPED kept, the sign and INSIDE all the same
    esc = (closest["flags"] & irl.FLAG_ESCAPED) != 0
    assert (esc & ins).sum() > 20 and (esc & ~ins).sum() > 20
    assert np.array_equal(sd["dist"][esc & ins].view(np.uint32), (-radius[esc & ins]).view(np.uint32))
    assert np.array_equal(sd["dist"][esc & ~ins].view(np.uint32), radius[esc & ~ins].view(np.uint32))
    assert np.all(sd["flags"][esc & ins] == (irl.FLAG_ESCAPED | irl.FLAG_INSIDE)) and np.all(sd["flags"][esc & ~ins] == irl.FLAG_ESCAPED)
    assert np.all(sd["flags"][~esc & ins] == irl.FLAG_INSIDE) and np.all(sd["dist"][~esc & ins] < 0)
    # queries a point query does not walk are not walked for crossings either: "nothing found", byte for byte
    nan = np.nan
    odd = cc.points_of(np.array([[nan, 0, 0], [0, 0, 0], [0, 0, 0], [0.2, np.inf, 0], [0, 0, 0]], F))
    odd["radius"] = [np.inf, -1.0, nan, 1.0, np.inf]
    c2, s2 = dev.closest_points(odd), dev.signed_distance(odd)
    assert s2[:4].tobytes() == c2[:4].tobytes() and np.all(s2["flags"][:4] == irl.FLAG_ESCAPED)
    assert np.all(s2["primID"][:4] == irl.INVALID_PRIM) and s2["dist"][1] == -1.0 and np.isnan(s2["dist"][2])
    assert s2["flags"][4] == irl.FLAG_INSIDE and s2["dist"][4] == -1.0          # the cube's centre, walked: one unit inside
    dev.close()


# ------------------------------------------------------------------------------------------------------
# launch shapes, counters
# ------------------------------------------------------------------------------------------------------
def test_launch_shape_edges_and_an_empty_scene(cases):
    hs, rays, want, boxes, tests = cases("mixed")
    pos = np.random.default_rng(3).uniform(-5, 5, (1024, 3)).astype(F)
    pts = cc.points_of(pos)
    dev = irl.IpuScene(hs.desc)
    ins, sd = dev.inside(pts), dev.signed_distance(pts)
    assert ins.any() and not ins.all()
    for n in (1, 255, 256, 257):
        assert np.array_equal(dev.count_crossings(rays[:n]), want[:n]), n
        assert np.array_equal(dev.inside(pts[:n]), ins[:n]), n
        assert dev.signed_distance(pts[:n]).tobytes() == sd[:n].tobytes(), n
        # a ragged slice: the elements of the larger batch
        assert np.array_equal(dev.count_crossings(rays[333:333 + n]), want[333:333 + n]), n
    assert dev.count_crossings(rays[:0]).size == 0 and dev.inside(pts[:0]).size == 0 and dev.signed_distance(pts[:0]).size == 0
    dev.close()
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = empty.num_spheres = empty.num_discs = 0
    dev = irl.IpuScene(empty)
    assert not dev.count_crossings(rays[:300]).any() and not dev.inside(pts[:300]).any()
    s0 = dev.signed_distance(pts[:300])
    assert s0.tobytes() == dev.closest_points(pts[:300]).tobytes() and np.all(s0["flags"] == irl.FLAG_ESCAPED)
    dev.close()


def test_counters(cases):
    hs, rays, want, boxes, tests = cases("soup")
    chk = cc.Checker(hs)
    sub = rays[:1024]
    _, b, t = chk.counts(sub)
    dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    assert np.array_equal(dev.count_crossings(sub), want[:1024])
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"], c["paths"]) == (1024, b, t, 0)
    # the inside walk: the points it walked are casts, its box and primitive tests are counted
    lo, hi = cc.root_box(hs)
    pos = np.random.default_rng(8).uniform(lo, hi, (512, 3)).astype(F)
    pos[5, 0] = np.nan; pos[77, 2] = np.inf                                   # not walked
    pts = cc.points_of(pos)
    ok = np.isfinite(pos).all(1)
    _, b2, t2 = chk.counts(cc.sign_rays(pts[ok]))
    dev.reset_counters()
    dev.inside(pts)
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (510, b2, t2)
    # signed distance: the point query's box tests and evaluations (mi_point_query counts no casts) plus the walk's
    dev.reset_counters()
    dev.closest_points(pts)
    p = dev.counters()
    assert p["casts"] == 0
    dev.reset_counters()
    dev.signed_distance(pts)
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (510, p["nodes_visited"] + b2, p["leaf_tests"] + t2)
    dev.close()
    dev = irl.IpuScene(hs.desc)
    dev.inside(pts); dev.count_crossings(sub)
    c = dev.counters()
    assert (c["casts"], c["nodes_visited"], c["leaf_tests"]) == (510 + 1024, 0, 0)
    dev.close()


# ------------------------------------------------------------------------------------------------------
# a live scene
# ------------------------------------------------------------------------------------------------------
def test_inside_follows_a_live_scene():
    hs = cc.scene("cube")
    pos, want = cc.cube_points()
    pts = cc.points_of(pos)
    dev = irl.IpuScene(hs.desc)
    assert np.array_equal(dev.inside(pts).astype(bool), want)
    # the cube moved by +2 in x: faces at x = 1 and x = 3 (no input point has a coordinate of exactly 1)
    moved, _ = cc.cube_mesh(shift=(2.0, 0.0, 0.0))
    dev.update_geometry(vertices=moved)
    p64 = pos.astype(np.float64)
    want2 = (np.abs(p64[:, 0] - 2.0) < 1.0) & (np.abs(p64[:, 1:]) < 1.0).all(1)
    assert want2.sum() > 50
    got = dev.inside(pts)
    assert np.array_equal(got.astype(bool), want2)
    sd = dev.signed_distance(pts)
    dev.rebuild_bvh()
    # another tree over the same geometry: the same bytes (a count does not depend on the visit order). Of the signed distance
    # the distance, its sign and the flags: WHICH of two equally near triangles is named is the first in preorder
    assert dev.inside(pts).tobytes() == got.tobytes()
    sd2 = dev.signed_distance(pts)
    assert sd2["dist"].tobytes() == sd["dist"].tobytes() and np.array_equal(sd2["flags"], sd["flags"])
    # other contents: the icosphere's answers
    ico = cc.scene("icosphere")
    dev.set_geometry(ico.desc)
    ipos, iwant = cc.icosphere_points()
    assert np.array_equal(dev.inside(cc.points_of(ipos)).astype(bool), iwant)
    dev.close()


# ------------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------------
def test_torch_sdf_on_a_non_default_stream():
    import torch
    hs = cc.scene("mixed")
    pos = np.random.default_rng(12).uniform(-5, 5, (5000, 3)).astype(F)
    dev = irl.IpuScene(hs.desc)
    for radius in (np.inf, 0.75):
        host = dev.signed_distance(cc.points_of(pos, radius))
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            r = dev.sdf(torch.from_numpy(pos).cuda(), radius)
        st.synchronize()
        assert np.array_equal(r["dist"].cpu().numpy().view(np.uint32), host["dist"].view(np.uint32))
        assert np.array_equal(r["inside"].cpu().numpy(), (host["flags"] & irl.FLAG_INSIDE) != 0) and r["inside"].any()
        assert np.array_equal(r["prim_id"].cpu().numpy().view(np.uint32), host["primID"])
        assert np.array_equal(r["geom_id"].cpu().numpy(), host["geomID"].astype(np.int16).astype(np.int32))
        assert np.array_equal(r["point"].cpu().numpy().view(np.uint32), np.stack([host["point"][c] for c in "xyz"], 1).view(np.uint32))
    # the device entries on raw pointers, a direction given
    t_pts = torch.from_numpy(cc.points_of(pos).view(np.uint8).copy()).cuda()
    out = torch.zeros(len(pos), dtype=torch.uint8, device="cuda")
    d = (-0.83, 0.47, -0.31)
    dev.point_sign_device(irl.SIGN_INSIDE, t_pts.data_ptr(), out.data_ptr(), len(pos), direction=d)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), dev.inside(cc.points_of(pos), direction=d))
    dev.close()


def test_destroy_waits_for_an_enqueued_count_query():
    import torch
    hs = irl.HostScene.builtin("box")
    hs.desc.set_image(512, 512)
    ref = irl.IpuScene(hs.desc)
    prim = qb.primary_rays(hs)
    rays = qb.bounce_rays(prim, ref.intersect(prim), per_hit=2, seed=5)
    want = ref.count_crossings(rays)
    ref.close()
    assert want.max() >= 2
    t_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    out = torch.zeros(rays.size, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    dev = irl.IpuScene(hs.desc)
    dev.count_query_device(t_rays.data_ptr(), out.data_ptr(), rays.size, st.cuda_stream)
    dev.close()
    st.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


def test_host_batches_and_the_variants_build(cases):
    hs, rays, want, boxes, tests = cases("mixed")
    pos = np.random.default_rng(3).uniform(-5, 5, (1024, 3)).astype(F)
    pts = cc.points_of(pos, 1.5)
    dev = irl.IpuScene(hs.desc)
    ins, sd = dev.inside(pts), dev.signed_distance(pts)
    dev.setRayBatch(100)
    assert np.array_equal(dev.count_crossings(rays), want)
    assert np.array_equal(dev.inside(pts), ins) and dev.signed_distance(pts).tobytes() == sd.tobytes()
    dev.close()
    var = irl.IpuScene(hs.desc, variants=True)
    assert np.array_equal(var.count_crossings(rays), want)
    assert np.array_equal(var.inside(pts), ins) and var.signed_distance(pts).tobytes() == sd.tobytes()
    var.close()
