"""geomIDs up to 0xFFFE and primIDs past 65 536 on the device: every query family, the renders, the build variants and the live-scene
entries on tests/id_cases.py's two scenes. Each device result is compared byte for byte with its host twin, the CPU oracle or the
Python checker, and with the closed forms of id_cases (integer arithmetic on the scenes' grids), whose batches assert on the
reference side that they reach the ids they are there for. Then batches of more than 65 536 items, for the item field of the records.

The ray families run on id_cases.ray_scene: for many_geoms its copy moved under the camera, because the reference's disc test sees
a disc only where n . c < 0 (id_cases.mg_vertical) - there rays cross all eight layers, 0xFFFE included. The live-scene tests
also cast the same rays in many_geoms itself, where they cross triangles and spheres alone."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import box_cases as bc
import count_cases as cc
import id_cases as ic
import list_cases as lsc
import near_cases as nc
import oracle_lib as ol
import point_cases as pc
import refit_cases as rc
import tri_cases as tc
from test_query_gpu import oracle_query

pytestmark = pytest.mark.gpu

F = np.float32
TOO_MANY = r"more than 65535 geometries \(geomID is 16 bit\)"

_devs, _memo = {}, {}


@pytest.fixture(scope="module", autouse=True)
def close_devices():
    yield
    for dev in list(_devs.values()) + [v for k, v in _memo.items() if k == "soup-dev"]:
        dev.close()
    _devs.clear(); _memo.clear()


def device(name, rays=False):
    """One IpuScene per scene for the whole module (closed when the module is done); rays: over id_cases.ray_scene."""
    tag = (name, rays and name == "many_geoms")
    if tag not in _devs:
        _devs[tag] = irl.IpuScene((ic.ray_scene(name) if rays else ic.scene(name)).desc)
    return _devs[tag]


def memo(tag, fn):
    if tag not in _memo:
        _memo[tag] = fn()
    return _memo[tag]


def ids(recs):
    return [(int(r["geomID"]), int(r["primID"])) for r in recs]


# ------------------------------------------------------------------------------------------------------
# rays: closest hit, any hit, crossings
# ------------------------------------------------------------------------------------------------------
def _oracle_hits(name):
    return memo(("oracle", name), lambda: oracle_query(ic.ray_scene(name), ic.ray_batch(name)[0]))


def _crossing_lists(name):
    def make():
        ck = ic.ray_checker(lsc.ListChecker, ic.ray_scene(name))
        return ck.lists(ic.ray_batch(name)[0])
    return memo(("lists", name), make)


@pytest.mark.parametrize("name", ic.SCENES)
def test_closest_and_any_hit(name):
    """Both query kernels against the oracle byte for byte; the hit is the first crossing of the closed form: from above a cell of
    many_geoms its layer-7 disc (layer 6 in cell 8191; 0xFFFE in cell 8190), from below its layer-0 triangle, along a row the
    row's first sphere; on long_mesh one of the coincident stack's four ids and each quad's own half from either side, nothing
    through a hole."""
    rays, found, ts = ic.ray_batch(name)
    want, occ, _, _ = _oracle_hits(name)
    first = [(f[0][0], f[0][1]) if f else (irl.INVALID_GEOM, irl.INVALID_PRIM) for f in found]
    # (the reference side first: equal t of the coincident stack leaves the closest hit to the walk's order - any of the four ids)
    for i, f in enumerate(found):
        tied = [(g, p) for (g, p, _), t in zip(f, ts[i]) if t == ts[i][0]]
        assert (int(want["geomID"][i]), int(want["primID"][i])) in (tied or [first[i]]), f"{name}: the oracle's hit of ray {i}"
    if name == "many_geoms":
        assert {0, 1, 8190, 8191, 0xFFFE, 7 * ic.CELLS, 6 * ic.CELLS + 8191} <= set(want["geomID"].tolist())
    else:
        assert (want["primID"][want["geomID"] == 0] >= 65536).any()
    for k in (0, 1):
        dev = device(name, rays=True).set_option("query_kernel", k)
        pc.assert_bytes_equal(dev.intersect(rays), want, f"{name}: closest hit, query_kernel {k}")
        assert np.array_equal(dev.occluded(rays), occ), f"{name}: any hit, query_kernel {k}"
    assert occ.tolist() == [len(f) > 0 for f in found]


@pytest.mark.parametrize("name", ic.SCENES)
def test_crossings(name):
    rays, found, ts = ic.ray_batch(name)
    lists = _crossing_lists(name)
    for i, (mine, f) in enumerate(zip(lists, found)):                        # the checker against the closed form
        assert [(g, p, far) for _, g, p, far in mine] == f, f"{name}: the checker's crossings of ray {i}"
        assert all(abs(float(t) - want) < 1e-4 for (t, _, _, _), want in zip(mine, ts[i]))
    if name == "long_mesh":
        four = [m for m in lists if [p for _, _, p, _ in m] == [0, 65535, 65536, 65537]]
        assert four and all(len(set(float(t) for t, _, _, _ in m)) == 1 for m in four), "four crossings at equal t, by primID across 65 535 | 65 536"
    dev = device(name, rays=True)
    assert dev.count_crossings(rays).tolist() == [len(f) for f in found]
    offsets, hits = dev.list_crossings(rays)
    want_offsets, want = lsc.packed(lists)
    assert np.array_equal(offsets, want_offsets)
    pc.assert_bytes_equal(hits, want, f"{name}: crossing lists")
    for k in (3, 8):
        pc.assert_bytes_equal(dev.first_crossings(rays, k).reshape(-1), lsc.first_k(lists, k).reshape(-1), f"{name}: first {k} crossings")


# ------------------------------------------------------------------------------------------------------
# points
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.SCENES)
def test_points(name):
    hs, dev = ic.scene(name), device(name)
    pts, want, ties = ic.near_batch(name)
    hits, _ = irl.point_query_host(hs.desc, irl.POINT_CLOSEST, pts)
    pc.assert_bytes_equal(dev.closest_points(pts), hits, f"{name}: closest points")
    within, _ = irl.point_query_host(hs.desc, irl.POINT_WITHIN, pts)
    assert np.array_equal(np.asarray(dev.within(pts)).astype(bool), np.asarray(within).astype(bool))
    for i, f in enumerate(want):                                              # the closed form
        if f:
            assert (int(hits[i]["geomID"]), int(hits[i]["primID"])) == (f[0][1], f[0][2]) and abs(float(hits[i]["dist"]) - f[0][0]) <= ic.DIST_TOL
        else:
            assert hits[i]["geomID"] == irl.INVALID_GEOM
    offsets, _ = irl.near_offsets_host(hs.desc, pts)
    recs, _ = irl.near_fill_host(hs.desc, pts, offsets)
    got = dev.neighbours(pts)
    nc.assert_same(got, (offsets, recs), f"{name}: neighbour lists")
    assert np.diff(got[0].astype(np.int64)).tolist() == [len(f) for f in want]
    for i, f in enumerate(want):
        r = got[1][int(got[0][i]):int(got[0][i + 1])]
        assert ids(r) == [(g, p) for _, g, p in f], f"{name}: neighbours of point {i}"
        assert np.all(np.abs(np.sqrt(r["dist2"].astype(np.float64)) - np.array([d for d, _, _ in f])) <= ic.DIST_TOL)
    for i in ties:
        r = got[1][int(got[0][i]):int(got[0][i + 1])]
        assert (r["dist2"] == r["dist2"][-1]).sum() == (2 if name == "many_geoms" else 4), f"{name}: point {i} has no exact tie"
    for k in (1, 2, 4, 5, 12):      # 4 cuts many_geoms' ties between the two ids that differ in bit 15, 1 and 2 long_mesh's four
        twin, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(pts.size, k), capacity=pts.size * k)
        near = dev.k_nearest(pts, k)
        pc.assert_bytes_equal(near.reshape(-1), twin, f"{name}: {k} nearest")
        assert [ids(r[:min(k, len(f))]) for r, f in zip(near.reshape(pts.size, k), want)] == [[(g, p) for _, g, p in f[:k]] for f in want]


def test_ties_across_bit_15_where_the_walk_meets_the_higher_id_first():
    """id_cases.view_tie_batch on the device: the twin's bytes, and the two tied ids ascending in the full lists, the 5 nearest and -
    cut between the two - the 4 nearest, although the walk meets the higher id first."""
    hs = ic.view_scene("many_geoms")
    pts, want = ic.view_tie_batch()
    where = {int(g): i for i, g in enumerate(hs.nodes["geomID"])}
    assert all(where[f[-1][1]] < where[f[-2][1]] for f in want), "the walk no longer meets the higher id first: the test has no teeth"
    dev = irl.IpuScene(hs.desc)
    offsets, _ = irl.near_offsets_host(hs.desc, pts)
    recs, _ = irl.near_fill_host(hs.desc, pts, offsets)
    got = dev.neighbours(pts)
    nc.assert_same(got, (offsets, recs), "tie points of the moved scene")
    assert [ids(got[1][int(got[0][i]):int(got[0][i + 1])]) for i in range(pts.size)] == [[(g, p) for _, g, p in f] for f in want]
    for k in (4, 5):
        twin, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(pts.size, k), capacity=pts.size * k)
        near = dev.k_nearest(pts, k)
        pc.assert_bytes_equal(near.reshape(-1), twin, f"{k} nearest of the tie points")
        assert [ids(r) for r in near.reshape(pts.size, k)] == [[(g, p) for _, g, p in f[:k]] for f in want]
    hit = dev.closest_points(pts)
    pc.assert_bytes_equal(hit, irl.point_query_host(hs.desc, irl.POINT_CLOSEST, pts)[0], "closest points of the tie points")
    dev.close()


@pytest.mark.parametrize("name", ic.SCENES)
def test_inside_and_signed_distance(name):
    """Points at the centres of spheres (many_geoms: layers 3 and 4, ids about 0x7FFF | 0x8000; long_mesh: geometry 1) and the
    neighbour batch's points: inside = the parity of the checker's crossing count along the default direction, signed_distance =
    the twin's closest point with the sign."""
    hs, dev = ic.scene(name), device(name)
    pts = ic.near_batch(name)[0]
    if name == "many_geoms":
        _, sph, _, _, _ = ic.many_geoms_arrays()
        gs = [3 * ic.CELLS + 8191, 4 * ic.CELLS, 4 * ic.CELLS + 1, 2 * ic.PER_KIND - 1]
        centres = np.array([[sph[g - ic.PER_KIND][c] for c in "xyz"] for g in gs], F)
    else:
        centres = np.array([ic.LM_SPHERE[:3]], F)
    pts = np.concatenate([ic.points(centres, 0.5), pts[::5]])
    pos = np.stack([pts[c] for c in "xyz"], 1)
    want = ic.ray_checker(cc.Checker, hs).inside(pos)
    assert want[:len(centres)].all() and not want.all()
    got = np.asarray(dev.inside(pts)).astype(bool)
    assert np.array_equal(got, want)
    closest, _ = irl.point_query_host(hs.desc, irl.POINT_CLOSEST, pts)
    signed = dev.signed_distance(pts)
    closest["dist"] = np.where(want, -closest["dist"], closest["dist"])
    closest["flags"] = np.where(want, closest["flags"] | irl.FLAG_INSIDE, closest["flags"])
    pc.assert_bytes_equal(signed, closest, f"{name}: signed distance")
    if name == "many_geoms":          # (nearest to a sphere's centre is the shell of the layer above or below, 0.05 away, not its own)
        near = signed["geomID"][:len(centres)]
        assert (near >= 0x8000).any() and (near < 0x8000).any() and np.all(signed["flags"][:len(centres)] == irl.FLAG_INSIDE)


# ------------------------------------------------------------------------------------------------------
# boxes and query triangles
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.SCENES)
def test_boxes(name):
    hs, dev = ic.scene(name), device(name)
    bx, found = ic.box_batch(name)
    want = bc.packed(found)                                                   # the closed form, as records
    offsets, _ = irl.box_offsets_host(hs.desc, bx)
    recs, _ = irl.box_fill_host(hs.desc, bx, offsets)
    bc.assert_same((offsets, recs), want, f"{name}: the twin's box lists")
    got = dev.list_overlaps(bx)
    bc.assert_same(got, want, f"{name}: box lists")
    ic.assert_ascending(*got, name)
    assert dev.count_overlaps(bx).tolist() == [len(f) for f in found]
    assert np.asarray(dev.touches(bx)).astype(bool).tolist() == [len(f) > 0 for f in found]
    for k in (1, 3, 4, 5, 7):                     # 4 | 5 cut many_geoms' stacks at bit 15, 1 .. 3 long_mesh's at 65 535 | 65 536
        cut = np.stack([bc.records(f, i, k) for i, f in enumerate(found)])
        pc.assert_bytes_equal(dev.first_overlaps(bx, k).reshape(-1), cut.reshape(-1), f"{name}: first {k} overlaps")
    if name == "many_geoms":
        high = got[1][got[1]["geomID"] >= 0x8000]
        assert set(high["flags"].tolist()) == {0, irl.OVERLAP_CONTAINED}


def test_voxelize_a_block_of_cells():
    """Voxels of 0.125 over the 2 x 2 grid cells from cell 8190 - 128 on (the stacks that end in 0xFFFE - 128 .. 0xFFFE), from
    z = -0.5 to 2: a voxel is set exactly where the box query of the same box touches (the twin); the column about the first
    cell's probe line is set at the height of each of its eight layers; the slices x in 0.625 .. 0.875 of the first cell, where
    nothing reaches (its disc ends at 0.55, the next cell's begins at 0.95), stay empty."""
    hs, dev = ic.many_geoms(), device("many_geoms")
    x, y = ic.cell_xy(8190 - ic.GRID_X)
    origin, dims = (x - 0.125, y - 0.125, -0.5), (16, 16, 20)
    vox = dev.voxelize(origin, 0.125, dims).cpu().numpy()
    i, j, k = np.meshgrid(*(np.arange(d) for d in dims), indexing="ij")
    at = np.stack([i, j, k], -1).reshape(-1, 3)
    lo = (at.astype(F) * F(0.125) + np.array(origin, F)).astype(F)
    hi = ((at + 1).astype(F) * F(0.125) + np.array(origin, F)).astype(F)
    twin, _ = irl.box_query_host(hs.desc, irl.BOX_ANY, qb.make_boxes(lo, hi))
    assert np.array_equal(vox.reshape(-1), np.asarray(twin).astype(bool))
    assert not vox[6:8].any() and vox[2, 2, [4, 6, 14, 16, 18]].all()      # the triangles of layers 0, 1 and the discs of layers 5 .. 7


@pytest.mark.parametrize("name", ic.SCENES)
def test_query_triangles(name):
    hs, dev = ic.scene(name), device(name)
    tq, found = ic.tri_batch(name)
    offsets, _ = irl.tri_offsets_host(hs.desc, tq)
    recs, _ = irl.tri_fill_host(hs.desc, tq, offsets)
    got = dev.list_contacts(tq)
    tc.assert_same(got, (offsets, recs), f"{name}: contact lists")
    assert [ids(got[1][int(got[0][i]):int(got[0][i + 1])]) for i in range(tq.size)] == found
    ic.assert_ascending(*got, name)
    assert dev.count_contacts(tq).tolist() == [len(f) for f in found]
    assert np.asarray(dev.tri_touches(tq)).astype(bool).tolist() == [len(f) > 0 for f in found]
    for k in (3, 5):
        twin, _ = irl.tri_fill_host(hs.desc, tq, bc.k_offsets(tq.size, k), capacity=tq.size * k)
        firsts = dev.first_contacts(tq, k)
        pc.assert_bytes_equal(firsts.reshape(-1), twin, f"{name}: first {k} contacts")
        assert [ids(r[:min(k, len(f))]) for r, f in zip(firsts.reshape(tq.size, k), found)] == [f[:k] for f in found]


# ------------------------------------------------------------------------------------------------------
# renders
# ------------------------------------------------------------------------------------------------------
def render_stream(name):
    """64 x 64 caller-supplied rays from above the scene, pointing down with a spread: over the grid of many_geoms from z = 4, over
    the sheet of long_mesh from z = 6 (a few through its sphere)."""
    hs = ic.scene(name)
    rays = hs.init_ray_stream()
    rng = np.random.default_rng(77)
    n = rays.size
    span = (ic.GRID_X, ic.GRID_Y, 4.0) if name == "many_geoms" else (ic.SIDE - 1, ic.SIDE - 1, 6.0)
    o = np.stack([rng.uniform(0, span[0], n), rng.uniform(0, span[1], n), np.full(n, span[2])], 1)
    if name == "many_geoms":                      # half of them onto the spheres' xy: a cell's sphere covers an eighth of it
        cell = rng.integers(0, ic.CELLS, n // 2)
        o[:n // 2, 0] = cell % ic.GRID_X + 0.25 + rng.uniform(-0.12, 0.12, n // 2)
        o[:n // 2, 1] = cell // ic.GRID_X + 0.25 + rng.uniform(-0.12, 0.12, n // 2)
    d = np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), -np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k, c in enumerate("xyz"):
        rays["h"]["r"]["origin"][c] = o[:, k]
        rays["h"]["r"]["direction"][c] = d[:, k]
    return rays


@pytest.mark.parametrize("name", ic.SCENES)
def test_shadow_trace_of_callers_rays(name):
    """All 84 bytes of every record equal the oracle's, for the default kernel, kernel 0 and hot_nodes on. The oracle's records alone
    meet the conditions first - measured with seed 77: many_geoms 1 652 of 4 096 rays hit, 85 % of the hits have geomID >= 0x8000,
    19 of 19 materials are hit; long_mesh 4 091 of 4 096 rays hit, 51 % of the hits have primID >= 65 536."""
    hs = ic.scene(name)
    desc = irl.SceneDesc.from_buffer_copy(hs.desc)        # (the cached scene's own desc stays as it is)
    desc.samples_per_pixel = 3
    rays = render_stream(name)
    want = rays.copy()
    ol.shadow_trace(desc, want, 8)
    hit = want["h"]["primID"] != irl.INVALID_PRIM
    assert hit.mean() >= 0.25
    if name == "many_geoms":
        assert (want["h"]["geomID"][hit] >= 0x8000).mean() >= 0.25 and len(set(hs.mat_ids[want["h"]["geomID"][hit]].tolist())) >= 12
    else:
        assert (want["h"]["primID"][hit] >= 65536).mean() >= 0.25
    for options in ({}, {"kernel": 0}, {"hot_nodes": 64}):
        dev = irl.IpuScene(desc)
        for key, value in options.items():
            dev.set_option(key, value)
        got = rays.copy()
        dev.run(got, irl.MODE_SHADOW_TRACE)
        dev.close()
        pc.assert_bytes_equal(got, want, f"{name}: shadow trace, options {options}")


@pytest.mark.parametrize("name", ic.SCENES)
def test_path_trace_from_the_camera(name):
    """A path trace makes its own rays at the camera, so it runs on id_cases.view_scene - the same scene moved under the camera -, 64 x
    64 pixels, 3 samples: all 84 bytes equal the oracle's for the default kernel, kernel 0 and hot_nodes on. The oracle's records
    alone, measured: many_geoms 2 190 of 4 096 records end on a hit, 85 % of them with geomID >= 0x8000, 19 of 19 materials;
    long_mesh 4 096 of 4 096, 49 % with primID >= 65 536."""
    hs = ic.view_scene(name)
    desc = irl.SceneDesc.from_buffer_copy(hs.desc)        # (the cached scene's own desc stays as it is)
    desc.set_image(64, 64)
    desc.samples_per_pixel = 3
    rays = np.zeros(64 * 64, irl.TRACE_RESULT)
    irl._check_host(irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size))
    want = rays.copy()
    ol.path_trace_pixel_rng(desc, want, 8)
    hit = want["h"]["primID"] != irl.INVALID_PRIM
    assert hit.mean() >= 0.25 and want["rgb"]["x"].max() > 0
    if name == "many_geoms":
        assert (want["h"]["geomID"][hit] >= 0x8000).mean() >= 0.25 and len(set(hs.mat_ids[want["h"]["geomID"][hit]].tolist())) >= 12
    else:
        assert (want["h"]["primID"][hit] >= 65536).mean() >= 0.25
    for options in ({}, {"kernel": 0}, {"hot_nodes": 64}):
        dev = irl.IpuScene(desc)
        for key, value in options.items():
            dev.set_option(key, value)
        got = rays.copy()
        dev.run(got, irl.MODE_PATH_TRACE)
        dev.close()
        pc.assert_bytes_equal(got, want, f"{name}: path trace, options {options}")


# ------------------------------------------------------------------------------------------------------
# the other builds: one representative batch each
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.SCENES)
def test_variants_full_stats_and_double_fallback(name):
    rays, found, _ = ic.ray_batch(name)
    want = _oracle_hits(name)[0]
    lists = lsc.packed(_crossing_lists(name))
    bx, boxes_found = ic.box_batch(name)
    pts = ic.near_batch(name)[0]
    near = device(name).neighbours(pts)
    for variants, options in ((True, {}), (False, {"full_stats": 1}), (False, {"double_fallback": 1})):
        what = f"{name}: variants {variants}, options {options}"
        dev = irl.IpuScene(ic.ray_scene(name).desc, variants=variants)
        for key, value in options.items():
            dev.set_option(key, value)
        # (no ray of the batch grazes an edge: the binary64 branch of double_fallback decides nothing else here)
        pc.assert_bytes_equal(dev.intersect(rays), want, what)
        got = dev.list_crossings(rays)
        assert np.array_equal(got[0], lists[0])
        pc.assert_bytes_equal(got[1], lists[1], what)
        if name == "many_geoms":                  # the other families on the scene itself
            dev.close()
            dev = irl.IpuScene(ic.scene(name).desc, variants=variants)
            for key, value in options.items():
                dev.set_option(key, value)
        bc.assert_same(dev.list_overlaps(bx), bc.packed(boxes_found), what)
        nc.assert_same(dev.neighbours(pts), near, what)
        dev.close()


# ------------------------------------------------------------------------------------------------------
# live scenes
# ------------------------------------------------------------------------------------------------------
def _all_lists(dev, name):
    return (dev.list_overlaps(ic.box_batch(name)[0]), dev.list_contacts(ic.tri_batch(name)[0]), dev.neighbours(ic.near_batch(name)[0]),
            dev.list_crossings(ic.ray_batch_home(name)[0]), dev.intersect(ic.ray_batch_home(name)[0]))


def _assert_lists_equal(got, want, what):
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g[0], w[0]), what
        pc.assert_bytes_equal(g[1], w[1], what)
    pc.assert_bytes_equal(got[4], want[4], what)


@pytest.mark.parametrize("name", ic.SCENES)
def test_rebuild_keeps_every_list_and_equals_the_twin(name):
    hs = ic.scene(name)
    dev = irl.IpuScene(hs.desc)
    before = _all_lists(dev, name)
    pc.assert_bytes_equal(dev.bvh_nodes(), np.ascontiguousarray(hs.nodes), f"{name}: the uploaded nodes")
    assert np.array_equal(np.array(list(dev.bvh_cost().values())[:3]), np.array(list(irl.bvh_cost(hs.nodes).values())[:3]))
    depth = dev.rebuild_bvh()
    nodes, want_depth = irl.build_lbvh(hs.desc)
    assert depth == want_depth
    pc.assert_bytes_equal(dev.bvh_nodes(), nodes, f"{name}: the rebuilt nodes")
    assert np.array_equal(np.sort(ic.leaf_ids(dev.bvh_nodes())), ic.expected_leaf_ids(name))
    cost, twin = dev.bvh_cost(), irl.bvh_cost(nodes)
    assert [cost[k] for k in ("sum_all", "sum_leaf", "a_root")] == [twin[k] for k in ("sum_all", "sum_leaf", "a_root")]
    # (the closest hit of the coincident stack may name another of the four ids under another tree: compared for many_geoms only)
    after = _all_lists(dev, name)
    _assert_lists_equal(after[:4] + (after[4] if name == "many_geoms" else before[4],), before, f"{name}: after rebuild_bvh")
    dev.close()


@pytest.mark.parametrize("name", ic.SCENES)
def test_update_geometry_equals_the_host_refit_and_a_fresh_scene(name):
    """A jitter of 1e-3: far below every margin of the closed forms, so the lists keep their ids; the nodes equal the host refit's and
    every result equals a fresh scene's over the moved arrays."""
    hs = ic.scene(name)
    verts, sph, dsc = rc.jitter(hs, 5, scale=1e-3)
    moved = rc.Moved(hs, verts=verts, spheres=sph, discs=dsc).refit()
    dev = irl.IpuScene(hs.desc)
    dev.update_geometry(vertices=verts, spheres=sph, discs=dsc if dsc.size else None)
    pc.assert_bytes_equal(dev.bvh_nodes(), moved.nodes, f"{name}: the refitted nodes")
    fresh = irl.IpuScene(moved.desc)
    _assert_lists_equal(_all_lists(dev, name), _all_lists(fresh, name), f"{name}: after update_geometry")
    bx, found = ic.box_batch(name)
    assert [ids(r) for r in np.split(dev.list_overlaps(bx)[1], np.cumsum([len(f) for f in found])[:-1])] == [[(g, p) for g, p, _ in f] for f in found]
    dev.close(); fresh.close()


def test_set_geometry_from_the_soup_to_many_geoms_and_back():
    import torch
    soup, mg = pc.scene("soup"), ic.many_geoms()
    dev = irl.IpuScene(soup.desc)
    soup_boxes = bc.boxes_of("soup", 64)
    first = dev.list_overlaps(soup_boxes)
    lbvh, depth = irl.build_lbvh(mg.desc)
    assert dev.set_geometry(mg.desc) == depth
    pc.assert_bytes_equal(dev.bvh_nodes(), lbvh, "many_geoms' nodes after set_geometry")
    fresh = irl.IpuScene(pc.with_nodes(mg.desc, lbvh))
    want = _all_lists(fresh, "many_geoms")
    _assert_lists_equal(_all_lists(dev, "many_geoms"), want, "after set_geometry")
    bc.assert_same(want[0], bc.packed(ic.box_batch("many_geoms")[1]), "a fresh scene over the LBVH")
    dev.set_geometry(soup.desc)
    bc.assert_same(dev.list_overlaps(soup_boxes), first, "back on the soup")
    tv, sph, dsc, _, _ = ic.many_geoms_arrays()
    t = lambda a, w: torch.from_numpy(np.ascontiguousarray(a).view(F).reshape(-1, w).copy()).cuda()
    idx = torch.from_numpy(np.tile(np.arange(3, dtype=np.int16), (ic.PER_KIND, 1))).cuda()
    assert dev.set_geometry_device(mg.desc, tris=idx, vertices=t(tv, 3), spheres=t(sph, 4), discs=t(dsc, 7)) == depth
    torch.cuda.synchronize()
    pc.assert_bytes_equal(dev.bvh_nodes(), lbvh, "many_geoms' nodes after set_geometry_device")
    _assert_lists_equal(_all_lists(dev, "many_geoms"), want, "after set_geometry_device")
    dev.close(); fresh.close()


def test_scene_from_the_blob_of_65535_geometries():
    """serialise_scene -> IpuScene.from_blob: the scene made from the blob lists what the closed forms say - boxes (ids up to 0xFFFE
    beside MI_OVERLAP_CONTAINED) and neighbours - and casts as the scene made from the desc."""
    hs = ic.many_geoms()
    dev = irl.IpuScene.from_blob(irl.serialise_scene(hs.desc), hs.desc)
    bx, found = ic.box_batch("many_geoms")
    bc.assert_same(dev.list_overlaps(bx), bc.packed(found), "box lists of the scene from the blob")
    pts, want, _ = ic.near_batch("many_geoms")
    got = dev.neighbours(pts)
    assert [ids(got[1][int(got[0][i]):int(got[0][i + 1])]) for i in range(pts.size)] == [[(g, p) for _, g, p in f] for f in want]
    rays = ic.ray_batch_home("many_geoms")[0]
    pc.assert_bytes_equal(dev.intersect(rays), device("many_geoms").intersect(rays), "closest hits of the scene from the blob")
    pc.assert_bytes_equal(dev.bvh_nodes(), np.ascontiguousarray(hs.nodes), "the nodes of the scene from the blob")
    dev.close()


def test_create_and_set_geometry_refuse_65536_geometries_by_name():
    mg = ic.many_geoms()
    ref = np.concatenate([mg.geometry, mg.geometry[ic.PER_KIND:ic.PER_KIND + 1]])
    mat_ids = np.concatenate([mg.mat_ids, [0]]).astype(np.uint32)
    d = irl.SceneDesc.from_buffer_copy(mg.desc)
    d.geometry, d.num_geometry = ref.ctypes.data, len(ref)
    d.mat_ids, d.num_mat_ids = mat_ids.ctypes.data, len(mat_ids)
    with pytest.raises(irl.RaylibError, match=TOO_MANY):
        irl.IpuScene(d)
    dev = device("many_geoms")
    bx, found = ic.box_batch("many_geoms")
    with pytest.raises(irl.RaylibError, match=TOO_MANY):
        dev.set_geometry(d)
    bc.assert_same(dev.list_overlaps(bx), bc.packed(found), "the scene after a refused set_geometry")


# ------------------------------------------------------------------------------------------------------
# item indices past 65 536
# ------------------------------------------------------------------------------------------------------
N_ITEMS = 65537 + 300


def _item_positions():
    """65 837 positions: far outside the soup (a query there touches nothing and ends at the root) but for 150 on either side of
    65 536, which stand on the soup's vertices."""
    hs = pc.scene("soup")
    rng = np.random.default_rng(9)
    pos = rng.uniform(500.0, 600.0, (N_ITEMS, 3)).astype(F)
    verts = np.stack([hs.verts[c] for c in "xyz"], 1).astype(F)
    busy = np.arange(65536 - 150, 65536 + 150)
    pos[busy] = verts[rng.integers(0, len(verts), busy.size)]
    return hs, pos, busy


@pytest.mark.parametrize("family", ["near", "box", "tri", "closest"])
def test_item_indices_past_65536(family):
    """The record's item field is the global index on both sides of 65 536; the bytes equal the twin's and those of the same queries
    run as two batches (the second one's item fields moved up)."""
    hs, pos, busy = _item_positions()
    dev = memo("soup-dev", lambda: irl.IpuScene(hs.desc))
    cut = 65536 - 70
    if family == "closest":
        items = qb.make_points(pos, F(1.5))
        got = dev.closest_points(items)
        twin, _ = irl.point_query_host(hs.desc, irl.POINT_CLOSEST, items)
        pc.assert_bytes_equal(got, twin, "closest points of 65 837 points")
        pc.assert_bytes_equal(np.concatenate([dev.closest_points(items[:cut]), dev.closest_points(items[cut:])]), twin, "as two batches")
        found = got["geomID"] != irl.INVALID_GEOM
        assert found[busy].all() and not found[:busy[0]].any() and not found[busy[-1] + 1:].any()
        return
    if family == "near":
        items, field = qb.make_points(pos, F(1.5)), "point"
        run = dev.neighbours
        twin_offsets, _ = irl.near_offsets_host(hs.desc, items)
        twin = (twin_offsets, irl.near_fill_host(hs.desc, items, twin_offsets)[0])
    elif family == "box":
        items, field = qb.make_boxes(pos - F(0.75), pos + F(0.75)), "box"
        run = dev.list_overlaps
        twin_offsets, _ = irl.box_offsets_host(hs.desc, items)
        twin = (twin_offsets, irl.box_fill_host(hs.desc, items, twin_offsets)[0])
    else:
        items, field = qb.make_tris(pos, pos + np.array([1, 0, 0], F), pos + np.array([0, 1, 0.5], F)), "tri"
        run = dev.list_contacts
        twin_offsets, _ = irl.tri_offsets_host(hs.desc, items)
        twin = (twin_offsets, irl.tri_fill_host(hs.desc, items, twin_offsets)[0])
    offsets, recs = run(items)
    assert np.array_equal(offsets, twin[0])
    pc.assert_bytes_equal(recs, twin[1], f"{family}: lists of 65 837 items")
    want_item = np.repeat(np.arange(N_ITEMS, dtype=np.uint32), np.diff(offsets.astype(np.int64)))
    assert np.array_equal(recs[field], want_item) and (want_item < 65536).sum() >= 100 and (want_item >= 65536).sum() >= 100
    a, b = run(items[:cut]), run(items[cut:])
    second = b[1].copy()
    second[field] += np.uint32(cut)
    assert np.array_equal(offsets, np.concatenate([a[0], b[0][1:] + a[0][-1]]))
    pc.assert_bytes_equal(np.concatenate([a[1], second]), recs, f"{family}: as two batches")


