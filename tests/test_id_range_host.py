"""geomIDs up to 0xFFFE and primIDs past 65 536 on the host (no GPU): the host twins of the point, neighbour, box and triangle families,
the tree builders and the blob on tests/id_cases.py's two scenes, against the Python checkers and against the closed forms of that
module (integer arithmetic on the scenes' grids: a reference that shares no code with the twins, which compile the kernels' headers);
and the limit itself - 65 535 geometries are a scene, 65 536 are refused by name at every entry that takes arrays or a desc."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import box_cases as bc
import id_cases as ic
import list_cases as lsc
import live_cases as lv
import near_cases as nc
import oracle_lib as ol
import point_cases as pc
import tri_cases as tc

F = np.float32
TOO_MANY = r"more than 65535 geometries \(geomID is 16 bit\)"


# ------------------------------------------------------------------------------------------------------
# the scenes and their trees
# ------------------------------------------------------------------------------------------------------
def test_the_scenes_are_the_ones_stated():
    mg, lm = ic.many_geoms(), ic.long_mesh()
    assert mg.desc.num_geometry == 0xFFFF and mg.desc.num_nodes == 2 * 0xFFFF - 1 and mg.desc.num_materials == 19
    ref = mg.geometry
    assert ref["type"].tolist() == [0] * ic.PER_KIND + [1] * ic.PER_KIND + [2] * ic.PER_KIND
    assert np.array_equal(ref["index"], np.tile(np.arange(ic.PER_KIND, dtype=np.uint16), 3))          # no index wrapped
    assert ic.stack(0) == [0, 8192, 16384, 24576, 32768, 40960, 49152, 57344] and ic.stack(8190)[-1] == 0xFFFE and len(ic.stack(8191)) == 7
    assert ic.stack(8191)[3] == 0x7FFF and ic.stack(0)[4] == 0x8000
    m = mg.mat_ids
    g = np.arange(8192, 0xFFFF)
    assert np.all(m[g] != m[g - 8192]) and np.all(m[g[g >= 32768]] != m[g[g >= 32768] - 32768]), "a geomID that loses a bit must change the material"
    assert lm.desc.num_geometry == 2 and lm.desc.num_verts == 65536 and lm.desc.num_tris == 130050 and lm.desc.num_nodes == 2 * 130051 - 1
    t = lm.tris.reshape(-1, 3)
    for p in ic.COPIES:
        assert np.array_equal(t[p], t[0])


@pytest.mark.parametrize("name", ic.SCENES)
def test_every_tree_holds_every_id_once(name):
    """The SAH builder's tree, the LBVH and the refit: every (geomID, primID) in exactly one leaf, no leaf with geomID 0xFFFF (it
    would read as an interior node: the tree would then have fewer leaves than primitives), refit boxes equal to the builder's."""
    hs = ic.scene(name)
    want = ic.expected_leaf_ids(name)
    lbvh, depth = irl.build_lbvh(hs.desc)
    refit = irl.refit_compact_bvh(hs.desc)
    for what, nodes in (("builder", hs.nodes), ("LBVH", lbvh), ("refit", refit)):
        assert len(nodes) == 2 * len(want) - 1, what
        assert np.array_equal(np.sort(ic.leaf_ids(nodes)), want), f"{what}: the leaves are not the scene's primitives, each once"
        assert int((nodes["geomID"] == irl.INVALID_GEOM).sum()) == len(want) - 1, what
    assert refit.tobytes() == np.ascontiguousarray(hs.nodes).tobytes()
    assert 1 <= depth <= 63 + 32 + 1
    # the LBVH is a depth-first BVH2 the twins accept, and it lists what the builder's tree lists
    bx, found = ic.box_batch(name)
    d = pc.with_nodes(hs.desc, lbvh)
    offsets, _ = irl.box_offsets_host(d, bx)
    recs, _ = irl.box_fill_host(d, bx, offsets)
    bc.assert_same((offsets, recs), bc.packed(found), f"{name}: box lists over the LBVH")


@pytest.mark.parametrize("name", ic.SCENES)
def test_canonical_prims_and_cost(name):
    hs = ic.scene(name)
    table = irl.canonical_prims(hs.desc)
    want = ic.expected_leaf_ids(name)
    got = (table["geomID"].astype(np.uint64) << np.uint64(32)) | table["primID"].astype(np.uint64)
    assert np.array_equal(got, want), "the canonical table is not (geomID, primID) ascending, each once"
    if name == "many_geoms":
        assert table["kind"].tolist() == [0] * ic.PER_KIND + [1] * ic.PER_KIND + [2] * ic.PER_KIND
        assert np.array_equal(table["matIndex"], ic.mat_of(np.arange(ic.G)))
        assert np.array_equal(table["a"][ic.PER_KIND:], np.tile(np.arange(ic.PER_KIND, dtype=np.uint32), 2))
    else:
        tris = ic.long_mesh_arrays()[1].astype(np.uint32)
        assert np.array_equal(np.stack([table[k][:-1] for k in "abc"], 1), tris) and np.array_equal(table["triBase"][:-1], 3 * np.arange(ic.LM_TRIS))
    for nodes in (hs.nodes, irl.build_lbvh(hs.desc)[0]):
        cost = irl.bvh_cost(nodes)
        assert lv.bits(cost) == np.array(lv.numpy_cost(nodes), np.float64).tobytes()


# ------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------
def _box_twin(name):
    hs = ic.scene(name)
    bx, found = ic.box_batch(name)
    offsets, _ = irl.box_offsets_host(hs.desc, bx)
    recs, _ = irl.box_fill_host(hs.desc, bx, offsets)
    return hs, bx, found, offsets, recs


@pytest.mark.parametrize("name", ic.SCENES)
def test_box_twin_equals_the_closed_form(name):
    hs, bx, found, offsets, recs = _box_twin(name)
    bc.assert_same((offsets, recs), bc.packed(found), f"{name}: box lists")
    ic.assert_ascending(offsets, recs, name)
    counts, _ = irl.box_query_host(hs.desc, irl.BOX_COUNT, bx)
    anys, _ = irl.box_query_host(hs.desc, irl.BOX_ANY, bx)
    assert counts.tolist() == [len(f) for f in found] and np.asarray(anys).astype(bool).tolist() == [len(f) > 0 for f in found]
    if name == "many_geoms":
        high = recs[recs["geomID"] >= 0x8000]
        assert set(high["flags"].tolist()) == {0, irl.OVERLAP_CONTAINED}, "MI_OVERLAP_CONTAINED keeps its own bit beside bit 15 of a geomID"


@pytest.mark.parametrize("name", ic.SCENES)
@pytest.mark.parametrize("k", [1, 3, 4, 5, 7])
def test_first_overlaps_cut_the_stacks(name, k):
    """The k smallest keys of each list, then the empty record: k = 4 cuts a full stack of many_geoms between 0x6000 + cell and
    0x8000 + cell, k = 5 keeps one id above - the heap's replace-the-root path compares across bit 15 -, and k = 1 .. 3 cut the
    coincident stack of long_mesh at 65 535 | 65 536 and before."""
    hs = ic.scene(name)
    bx, found = ic.box_batch(name)
    recs, _ = irl.box_fill_host(hs.desc, bx, bc.k_offsets(bx.size, k), capacity=bx.size * k)
    want = np.stack([bc.records(f, i, k) for i, f in enumerate(found)])
    pc.assert_bytes_equal(recs.reshape(-1), want.reshape(-1), f"{name}: first {k} overlaps")


@pytest.mark.parametrize("name", ic.SCENES)
def test_box_checker_agrees(name):
    hs = ic.scene(name)
    bx, found = ic.box_batch(name)
    ck = ic.checker(bc.BoxChecker, hs)
    for i in list(range(0, bx.size, 7)) + [3, bx.size - 1]:
        assert ck.overlaps(bx[i])[0] == found[i], f"{name}: box {i}"


# ------------------------------------------------------------------------------------------------------
# query triangles
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.SCENES)
def test_tri_twin_equals_the_closed_form_and_the_checker(name):
    hs = ic.scene(name)
    tq, found = ic.tri_batch(name)
    offsets, _ = irl.tri_offsets_host(hs.desc, tq)
    recs, _ = irl.tri_fill_host(hs.desc, tq, offsets)
    assert np.diff(offsets.astype(np.int64)).tolist() == [len(f) for f in found]
    got = [[(int(r["geomID"]), int(r["primID"])) for r in recs[int(offsets[i]):int(offsets[i + 1])]] for i in range(tq.size)]
    assert got == found
    assert np.array_equal(recs["tri"], np.repeat(np.arange(tq.size, dtype=np.uint32), [len(f) for f in found]))
    ic.assert_ascending(offsets, recs, name)
    counts, _ = irl.tri_query_host(hs.desc, irl.TRI_COUNT, tq)
    assert counts.tolist() == [len(f) for f in found]
    ck = ic.checker(tc.TriChecker, hs)
    for i in (0, 2, 3, tq.size - 1):
        assert [(g, p) for g, p, *_ in ck.contacts(tq[i])[0]] == found[i], f"{name}: query triangle {i}"
    for k in (3, 5):
        firsts, _ = irl.tri_fill_host(hs.desc, tq, bc.k_offsets(tq.size, k), capacity=tq.size * k)
        firsts = firsts.reshape(tq.size, k)
        for i, f in enumerate(found):
            n = min(k, len(f))
            assert [(int(r["geomID"]), int(r["primID"])) for r in firsts[i, :n]] == f[:n] and np.all(firsts[i, n:]["geomID"] == irl.INVALID_GEOM)


# ------------------------------------------------------------------------------------------------------
# points
# ------------------------------------------------------------------------------------------------------
def assert_lists_match(offsets, recs, want, what):
    """Records against [(distance in binary64, geomID, primID)]: the same ids in the same order, the root of dist2 within
    id_cases.DIST_TOL of the binary64 distance."""
    assert np.diff(offsets.astype(np.int64)).tolist() == [len(f) for f in want], f"{what}: list lengths"
    for i, f in enumerate(want):
        r = recs[int(offsets[i]):int(offsets[i + 1])]
        assert [(int(x["geomID"]), int(x["primID"])) for x in r] == [(g, p) for _, g, p in f], f"{what}: point {i}"
        assert np.all(r["point"] == i) and np.all(r["flags"] == 0)
        d = np.array([d for d, _, _ in f])
        assert np.all(np.abs(np.sqrt(r["dist2"].astype(np.float64)) - d) <= ic.DIST_TOL), f"{what}: point {i}"


@pytest.mark.parametrize("name", ic.SCENES)
def test_neighbour_twin_equals_the_closed_form(name):
    hs = ic.scene(name)
    pts, want, ties = ic.near_batch(name)
    offsets, _ = irl.near_offsets_host(hs.desc, pts)
    recs, _ = irl.near_fill_host(hs.desc, pts, offsets)
    assert_lists_match(offsets, recs, want, name)
    for i in ties:                                  # equal dist2, ordered by the ids: across bit 15, across 65 535 | 65 536
        r = recs[int(offsets[i]):int(offsets[i + 1])]
        tied = r[r["dist2"] == (r["dist2"][-1] if name == "many_geoms" else r["dist2"][0])]
        assert len(tied) == (2 if name == "many_geoms" else 4), f"{name}: point {i} has no exact tie"
    for k in (1, 2, 4, 5, 12):      # 4 cuts many_geoms' ties between the two ids that differ in bit 15, 1 and 2 long_mesh's four
        near, _ = irl.near_fill_host(hs.desc, pts, nc.k_offsets(pts.size, k), capacity=pts.size * k)
        near = near.reshape(pts.size, k)
        for i, f in enumerate(want):
            n = min(k, len(f))
            assert [(int(x["geomID"]), int(x["primID"])) for x in near[i, :n]] == [(g, p) for _, g, p in f[:n]], f"{name}: {k} nearest of point {i}"
            assert np.all(near[i, n:]["geomID"] == irl.INVALID_GEOM) and np.all(near[i, n:]["primID"] == irl.INVALID_PRIM)
    ck = ic.checker(nc.NearChecker, hs)
    for i in [0, 5] + ties[:2]:
        mine = nc.records(ck.neighbours(pts[i])[0], i)
        pc.assert_bytes_equal(recs[int(offsets[i]):int(offsets[i + 1])], mine, f"{name}: the checker's list of point {i}")


def test_ties_across_bit_15_where_the_walk_meets_the_higher_id_first():
    """id_cases.view_tie_batch: the two tied ids in ascending order although the walk meets them descending - in the full lists, the
    5 nearest and, cut between the two, the 4 nearest - over the builder's tree and over the LBVH."""
    hs = ic.view_scene("many_geoms")
    pts, want = ic.view_tie_batch()
    for nodes in (hs.nodes, irl.build_lbvh(hs.desc)[0]):
        where = {int(g): i for i, g in enumerate(nodes["geomID"])}
        assert all(where[f[-1][1]] < where[f[-2][1]] for f in want), "the walk no longer meets the higher id first: the test has no teeth"
        d = pc.with_nodes(hs.desc, nodes)
        offsets, _ = irl.near_offsets_host(d, pts)
        recs, _ = irl.near_fill_host(d, pts, offsets)
        assert_lists_match(offsets, recs, want, "tie points of the moved scene")
        for k in (4, 5):
            near, _ = irl.near_fill_host(d, pts, nc.k_offsets(pts.size, k), capacity=pts.size * k)
            for r, f in zip(near.reshape(pts.size, k), want):
                assert [(int(x["geomID"]), int(x["primID"])) for x in r] == [(g, p) for _, g, p in f[:k]], f"{k} nearest of a tie point"


@pytest.mark.parametrize("name", ic.SCENES)
def test_point_twin_equals_the_closed_form(name):
    hs = ic.scene(name)
    pts, want, _ = ic.near_batch(name)
    hits, _ = irl.point_query_host(hs.desc, irl.POINT_CLOSEST, pts)
    within, _ = irl.point_query_host(hs.desc, irl.POINT_WITHIN, pts)
    assert np.asarray(within).astype(bool).tolist() == [len(f) > 0 for f in want]
    for i, f in enumerate(want):
        if not f:
            assert hits[i]["geomID"] == irl.INVALID_GEOM and hits[i]["primID"] == irl.INVALID_PRIM
            continue
        first = [(g, p) for d, g, p in f if d == f[0][0]]           # an exact tie: any of the tied, by the contract the smallest key
        assert (int(hits[i]["geomID"]), int(hits[i]["primID"])) == first[0], f"{name}: point {i}"
        assert abs(float(hits[i]["dist"]) - f[0][0]) <= ic.DIST_TOL


def test_sphere_roots_of_a_high_sphere():
    """mi_sphere_roots_host on the sphere with the largest geomID (43 689) along its cell's probe line: both roots, the bits of the
    numpy restatement, at the heights the closed form states."""
    _, sph, _, _, _ = ic.many_geoms_arrays()
    g = 2 * ic.PER_KIND - 1
    s = sph[g - ic.PER_KIND]
    o, d, found, ts = ic.mg_vertical(g % ic.CELLS, down=True)
    mask, *t = irl.sphere_roots_host((s["x"], s["y"], s["z"]), F(s["radius"]) * F(s["radius"]), o, d)
    m2, t0, t1 = lsc.sphere_roots32((s["x"], s["y"], s["z"]), F(s["radius"]) * F(s["radius"]), o, d, 0.0, np.inf)
    assert mask == m2 == 3 and F(t[0]).tobytes() == F(t0).tobytes() and F(t[1]).tobytes() == F(t1).tobytes()
    mine = [x for x, (gg, _, _) in zip(ts, found) if gg == g]
    assert len(mine) == 2 and abs(t[0] - mine[0]) < 1e-5 and abs(t[1] - mine[1]) < 1e-5


# ------------------------------------------------------------------------------------------------------
# the blob
# ------------------------------------------------------------------------------------------------------
def test_blob_round_trip_with_65535_geometries():
    hs = ic.many_geoms()
    blob = irl.serialise_scene(hs.desc)
    out = irl.deserialise_scene(blob)
    assert out.num_geometry == 0xFFFF and out.num_nodes == hs.desc.num_nodes and out.num_mat_ids == 0xFFFF and out.num_meshes == ic.PER_KIND
    view = lambda ptr, n, dt: np.frombuffer((C.c_uint8 * (n * dt.itemsize)).from_address(C.cast(ptr, C.c_void_p).value), dt)
    assert view(out.geometry, 0xFFFF, irl.GEOM_REF).tobytes() == np.ascontiguousarray(hs.geometry).tobytes()
    assert view(out.bvh_nodes, out.num_nodes, irl.BVH_NODE).tobytes() == np.ascontiguousarray(hs.nodes).tobytes()
    assert view(out.mat_ids, 0xFFFF, np.dtype("<u4")).tobytes() == np.ascontiguousarray(hs.mat_ids).tobytes()


def test_the_reference_reader_walks_the_blob_of_65535_geometries():
    ref = ol.ref_lib()
    if ref is None or not hasattr(ref, "ref_walk_scene_blob"):
        pytest.skip("the reference's own reader (oracle/_ref) is not built here: it needs the reference checkout at build time")
    hs = ic.many_geoms()
    blob = irl.serialise_scene(hs.desc)
    arrays, _, used = ol.ref_walk_scene_blob(blob)
    counts = arrays[1::2]
    assert used == blob.size, "the reference's reader does not consume the blob"
    assert counts[0] == 0xFFFF and counts.count(0xFFFF) >= 2 and hs.desc.num_nodes in counts, "the reference's reader finds other counts"


# ------------------------------------------------------------------------------------------------------
# the limit
# ------------------------------------------------------------------------------------------------------
def test_from_arrays_accepts_65535_geometries():
    hs = irl.HostScene.from_arrays(ic.spheres_desc(0xFFFF))
    assert hs.desc.num_geometry == 0xFFFF and hs.desc.num_nodes == 2 * 0xFFFF - 1
    assert np.array_equal(np.sort(ic.leaf_ids(hs.nodes)), np.arange(0xFFFF, dtype=np.uint64) << np.uint64(32))
    assert np.array_equal(hs.geometry["index"], np.arange(0xFFFF, dtype=np.uint16))


@pytest.mark.parametrize("n", [0x10000, 0x10001])
def test_from_arrays_refuses_more_by_name(n):
    """65 536 spheres used to give a leaf with geomID 0xFFFF - an interior node to every reader -, 65 537 a wrapped mi_geom_ref::index."""
    with pytest.raises(irl.RaylibError, match=TOO_MANY):
        irl.HostScene.from_arrays(ic.spheres_desc(n))
    g = ic.spheres_desc(n)
    out = C.c_void_p()
    assert irl.host_lib().mi_host_scene_from_arrays(C.byref(g), C.byref(out)) != irl.MI_OK and not out.value, "nothing is built"


def test_from_arrays_refuses_a_mix_that_adds_up_to_65536():
    tv, sph, dsc, mats, _ = ic.many_geoms_arrays()
    g = ic.geometry_desc(tv, sph, np.concatenate([dsc, dsc[:1]]), mats, np.zeros(0x10000, np.uint32))
    with pytest.raises(irl.RaylibError, match=TOO_MANY):
        irl.HostScene.from_arrays(g)


def _more(hs, extra):
    """hs's desc with 65 535 + extra geometries: further references (the first spheres again) and material ids; nodes unchanged."""
    ref = np.concatenate([hs.geometry, hs.geometry[ic.PER_KIND:ic.PER_KIND + extra]])
    mat_ids = np.concatenate([hs.mat_ids, [0] * extra]).astype(np.uint32)
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    d.geometry, d.num_geometry = ref.ctypes.data, len(ref)
    d.mat_ids, d.num_mat_ids = mat_ids.ctypes.data, len(mat_ids)
    d._keep = [ref, mat_ids]
    return d


ENTRIES = {
    "mi_build_lbvh_compact": lambda d, q: irl.build_lbvh(d),
    "mi_refit_compact_bvh": lambda d, q: irl.refit_compact_bvh(d),
    "mi_canonical_prims": lambda d, q: irl.canonical_prims(d),
    "mi_point_query_host": lambda d, q: irl.point_query_host(d, irl.POINT_CLOSEST, q["points"]),
    "mi_near_offsets_host": lambda d, q: irl.near_offsets_host(d, q["points"]),
    "mi_near_fill_host": lambda d, q: irl.near_fill_host(d, q["points"], nc.k_offsets(q["points"].size, 1), capacity=q["points"].size),
    "mi_box_query_host": lambda d, q: irl.box_query_host(d, irl.BOX_COUNT, q["boxes"]),
    "mi_box_offsets_host": lambda d, q: irl.box_offsets_host(d, q["boxes"]),
    "mi_box_fill_host": lambda d, q: irl.box_fill_host(d, q["boxes"], bc.k_offsets(q["boxes"].size, 1), capacity=q["boxes"].size),
    "mi_tri_query_host": lambda d, q: irl.tri_query_host(d, irl.TRI_COUNT, q["tris"]),
    "mi_tri_offsets_host": lambda d, q: irl.tri_offsets_host(d, q["tris"]),
    "mi_tri_fill_host": lambda d, q: irl.tri_fill_host(d, q["tris"], bc.k_offsets(q["tris"].size, 1), capacity=q["tris"].size),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_host_entry_refuses_65536_geometries_by_name(entry):
    """Each takes the 65 535 of many_geoms (the tests above) and refuses one and two more with mi_scene_create's words and its own
    name. (mi_scene_serialise, mi_scene_blob_size and mi_leaf_frames are not among them: DESIGN.md section 31.)"""
    hs = ic.many_geoms()
    q = {"points": ic.near_batch("many_geoms")[0][:2], "boxes": ic.box_batch("many_geoms")[0][:2], "tris": ic.tri_batch("many_geoms")[0][:2]}
    ENTRIES[entry](hs.desc, q)
    for extra in (1, 2):
        with pytest.raises(irl.RaylibError, match=entry + ": " + TOO_MANY):
            ENTRIES[entry](_more(hs, extra), q)
