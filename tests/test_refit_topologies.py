"""Geometry updates at their edges, without a GPU: the hand-made topologies of refit_cases.retopologise (that each still hits the
edge of refitTables / refit_top_kernel it is named for), the host refit mi_refit_compact_bvh on them and on a catalogue of extents
where the binary16 encoding can go wrong - against the numpy restatement, byte for byte -, and the refitted BVH against a test
of EVERY primitive: a refit must still find the scene. tests/test_refit_edges_gpu.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import refit_cases as rc


# ------------------------------------------------------------------------------------------------------
# the two restatements agree
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box-simple", "spheres", "soup", "soup-normals"])
def test_per_height_restatement_equals_the_loop(name):
    hs = rc.scene(name)
    rc.assert_nodes_equal(rc.numpy_refit_levels(hs.desc, hs.nodes), rc.numpy_refit(hs.desc, hs.nodes), f"{name}: as built")
    for seed, scale in ((1, 0.25), (2, 7.0)):
        v, s, d = rc.jitter(hs, seed, scale)
        m = rc.Moved(hs, verts=v, spheres=s, discs=d)
        rc.assert_nodes_equal(rc.numpy_refit_levels(m.desc, hs.nodes), rc.numpy_refit(m.desc, hs.nodes), f"{name}: jitter {scale}")


def test_per_height_restatement_on_signed_zeros_and_nans():
    pts = [[[0.0, 1, 1], [-0.0, 2, 2], [1, 3, 3]], [[-0.0, 1, 1], [0.0, 2, 2], [1, 3, 3]], [[np.nan, 1, 1], [2, 2, 2], [5, 3, 3]],
           [[4, np.nan, -0.0], [4, 0.0, 0.0], [4, -0.0, np.nan]]]
    hs = rc.triangles([[[k, 0, 0], [k + 1, 0, 0], [k, 1, 1]] for k in range(len(pts))])
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    v = hs.verts.copy(); v["x"], v["y"], v["z"] = p.T
    m = rc.Moved(hs, verts=v)
    rc.assert_nodes_equal(rc.numpy_refit_levels(m.desc, hs.nodes), rc.numpy_refit(m.desc, hs.nodes), "signed zeros and NaNs")


# ------------------------------------------------------------------------------------------------------
# the shapes, and that each hits its edge
# ------------------------------------------------------------------------------------------------------
def test_shapes_hit_their_edges():
    T = rc.REFIT_TOP_THREADS
    assert T == 1024

    def props(hs, shape, **kw):
        nodes, depth = rc.retopologise(hs, shape, **kw)
        walked, leaves = rc.contract_walk(nodes)
        assert walked == depth
        h = rc.node_heights(nodes)
        levels, top = rc.top_first(h)
        assert levels.sum() == len(nodes) and levels[0] == leaves
        print(f"{shape} {kw}: {len(nodes)} nodes, {len(levels) - 1} heights, level sizes {levels[:4].tolist()} ..., topFirst {top}")
        return nodes, h, levels, top, depth

    big = rc.edge_scene("caterpillar")
    nodes, h, levels, top, depth = props(big, "caterpillar")
    L = (len(nodes) + 1) // 2
    assert L >= 3000 and h[0] == L - 1 and depth == L            # about 3 000 heights ...
    assert (levels[1:] == 1).all() and top == 1                  # ... of one node each, all of them in ONE refit_top_kernel launch
    assert (nodes["geomID"][1::2] != irl.INVALID_GEOM).all()     # the leaf is every interior node's FIRST child (oracle stack: 2)

    nodes, h, levels, top, depth = props(rc.edge_scene("balanced"), "balanced")
    k = int(h[0])
    assert len(nodes) == 2 ** (k + 1) - 1 and levels.tolist() == [2 ** (k - j) for j in range(k + 1)] and depth == k + 1
    assert k == 9 and top == 1                                   # 512 leaves: every level fits the workgroup, no level kernel

    for n, want_top in ((T - 1, 1), (T, 1), (T + 1, 2)):
        nodes, h, levels, top, depth = props(rc.edge_scene("level_of"), "level_of", n=n)
        assert levels[1] == n and top == want_top                # 1023 / 1024: all top, 1025: height 1 goes to refit_level_kernel
        assert levels[0] == 2 * n + 3 and (levels[2:] <= T).all()
    # (the rule admits no level above 1024 nodes to the top kernel, so its stride loop never takes a second turn: a level of
    # exactly 1024, one node per thread, is that kernel's edge, and 1025 the level kernel's)

    nodes, h, levels, top, depth = props(rc.edge_scene("comb"), "comb")
    assert levels[1] == 2048 and top == 2                        # the wide low height runs in refit_level_kernel ...
    assert levels[2] == T                                        # ... the top kernel starts on a level of exactly 1024 ...
    assert h[0] == 300 - 1 + 12 and (levels[12:] == 1).all()     # ... and goes on through hundreds of one-node heights
    inner = np.nonzero(nodes["geomID"] == irl.INVALID_GEOM)[0]
    gap = np.abs(h[inner + 1] - h[nodes["link"][inner]])
    assert gap.max() >= 280                                      # siblings whose heights differ by hundreds

    nodes, h, levels, top, depth = props(rc.edge_scene("one"), "one")
    assert len(nodes) == 1 and levels.tolist() == [1] and top == 1 and depth == 1      # topFirst (1) > H (0): no top kernel at all
    nodes, h, levels, top, depth = props(rc.edge_scene("three"), "three")
    assert len(nodes) == 3 and levels.tolist() == [2, 1] and top == 1 and depth == 2

    # a seeded shuffle hangs the same leaves elsewhere
    a, _ = rc.retopologise(big, "caterpillar", seed=5)
    b, _ = rc.retopologise(big, "caterpillar")
    assert sorted(zip(a["geomID"], a["link"])) == sorted(zip(b["geomID"], b["link"])) and not np.array_equal(a["link"], b["link"])


SHAPES = [("caterpillar", {}), ("balanced", {}), ("level_of", {"n": 1023}), ("level_of", {"n": 1024}), ("level_of", {"n": 1025}),
          ("comb", {}), ("one", {}), ("three", {})]
SMALL_SHAPES = [("caterpillar", {}), ("balanced", {}), ("level_of", {"n": 13}), ("comb", {"n": 16, "tail": 9}), ("one", {}), ("three", {})]


@pytest.mark.parametrize("shape,kw", SHAPES, ids=lambda x: x if isinstance(x, str) else "-".join(str(v) for v in x.values()))
def test_host_refit_on_hand_made_trees_of_a_soup(shape, kw):
    hs = rc.edge_scene(shape)
    nodes, depth = rc.retopologise(hs, shape, seed=3, **kw)
    v, s, d = rc.jitter(hs, 31, 0.75)
    m = rc.with_topology(hs, nodes, depth, verts=v, spheres=s, discs=d)
    got = irl.refit_compact_bvh(m.desc)
    rc.assert_nodes_equal(got, rc.numpy_refit_levels(m.desc, nodes), f"soup {shape} {kw}")
    if len(nodes) <= 6200:
        rc.assert_nodes_equal(got, rc.numpy_refit(m.desc, nodes), f"soup {shape} {kw}: the loop")
    assert not np.array_equal(rc.node_bytes(got), rc.node_bytes(nodes))
    assert np.array_equal(got["link"], nodes["link"]) and np.array_equal(got["geomID"], nodes["geomID"])


@pytest.mark.parametrize("shape,kw", SMALL_SHAPES, ids=lambda x: x if isinstance(x, str) else "-".join(str(v) for v in x.values()))
def test_host_refit_on_hand_made_trees_of_the_box(shape, kw):
    hs = rc.scene("box-simple")                                   # 32 triangles: the shapes at the sizes that fit
    nodes, depth = rc.retopologise(hs, shape, **kw)
    rc.contract_walk(nodes)
    v, s, d = rc.jitter(hs, 32, 5.0)
    m = rc.with_topology(hs, nodes, depth, verts=v)
    got = irl.refit_compact_bvh(m.desc)
    rc.assert_nodes_equal(got, rc.numpy_refit(m.desc, nodes), f"box-simple {shape} {kw}")
    rc.assert_nodes_equal(got, rc.numpy_refit_levels(m.desc, nodes), f"box-simple {shape} {kw}: per height")


# ------------------------------------------------------------------------------------------------------
# the extent catalogue
# ------------------------------------------------------------------------------------------------------
def test_extent_catalogue_on_the_host():
    hs, verts, ext = rc.extent_catalogue()
    assert 2000 <= ext.size <= 20000
    m = rc.Moved(hs, verts=verts)
    got = irl.refit_compact_bvh(m.desc)
    rc.assert_nodes_equal(got, rc.numpy_refit_levels(m.desc, hs.nodes), "extent catalogue")
    rc.assert_nodes_equal(got, rc.numpy_refit(m.desc, hs.nodes), "extent catalogue: the loop")
    # the catalogue is what it says: triangle k's x extent IS probe k (its x minimum is a zero), bit for bit
    leaf = np.nonzero(got["geomID"] != irl.INVALID_GEOM)[0]
    tri = got["link"][leaf].astype(np.int64)
    p = np.stack([verts["x"], verts["y"], verts["z"]], 1).reshape(-1, 3, 3)[tri]
    lo, hi = p.min(1), p.max(1)
    with np.errstate(invalid="ignore"):
        e = (hi - lo).astype(np.float32)
    assert np.array_equal(e[:, 0].view(np.uint32), ext[tri].view(np.uint32))
    for bits in (0x00000000, 0x00000001, 0x33000000, 0x33800000, 0x38800000, 0x477FE000):      # 0, 2^-149, 2^-25, 2^-24, 2^-14, 65504
        for delta in ((0,) if bits in (0, 1, 0x477FE000) else (-1, 0, 1)):
            assert np.uint32(bits + delta) in ext.view(np.uint32), hex(bits + delta)
    assert np.signbit(lo[:, 0]).any() and (~np.signbit(lo[:, 0])).any() and (lo == 0).all(0)[0]
    assert (np.abs(lo[:, 1:]) >= 1e4).any() and ((lo[:, 1:] != 0) & (np.abs(lo[:, 1:]) < 1e-38)).any()
    assert (e[:, 1:] != ext[np.stack([(tri + ext.size // 3) % ext.size, (tri + 2 * (ext.size // 3)) % ext.size], 1)]).any()   # hi - lo rounded
    # independently, from np.float16: every encoded extent is the smallest binary16 that is not below fl(hi - lo)
    enc = np.stack([got["dx"], got["dy"], got["dz"]], 1)[leaf]
    as_f64 = enc.view(np.float16).astype(np.float64)
    assert (enc < 0x7C00).all() and (as_f64 >= e.astype(np.float64)).all()
    below = np.where(enc > 0, enc - 1, enc).astype(np.uint16).view(np.float16).astype(np.float64)
    assert ((enc == 0) & (e == 0) | (enc > 0) & (below < e.astype(np.float64))).all()
    used = {int(b) for b in enc[:, 0]}
    assert 0 in used and 1 in used and 0x0400 in used and 0x0401 in used and 0x7BFF in used
    # the interior boxes stay under 65504, the root's x extent exactly on it
    assert int(got["dx"][0]) == 0x7BFF and float(hi[:, 0].max() - lo[:, 0].min()) == 65504.0


def test_one_ulp_above_a_half_rounds_up_and_the_halfway_point_does_not_decide():
    # (the catalogue's probes one by one, against the oracle's own restatement of precision_utils.hpp:39-47)
    _, _, ext = rc.extent_catalogue()
    o = ol.lib()
    want = np.array([o.o_round_to_half_not_smaller(float(x)) for x in ext], np.uint16)
    assert np.array_equal(rc.half_not_smaller_bits(ext), want)


# ------------------------------------------------------------------------------------------------------
# a refitted BVH still finds the scene
# ------------------------------------------------------------------------------------------------------
def _aimed_rays(hs_desc, nodes, n, seed):
    """Origins round the root box, aimed at points inside it (tMin 0, tMax inf)."""
    rng = np.random.default_rng(seed)
    r = nodes[0]
    lo = np.array([r["min_x"], r["min_y"], r["min_z"]], np.float64)
    size = np.array([r["dx"], r["dy"], r["dz"]], np.uint16).view(np.float16).astype(np.float64)
    c = lo + size / 2
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + u * np.linalg.norm(size) * rng.uniform(0.2, 1.2, (n, 1))
    target = rng.uniform(lo, lo + size, (n, 3))
    d = target - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return qb.make_rays(o.astype(np.float32), d.astype(np.float32))


@pytest.mark.parametrize("name,seed,scale", [("soup", 41, 0.75), ("box-simple", 42, 5.0), ("spheres", 43, 0.5)])
def test_refitted_bvh_finds_what_brute_force_finds(name, seed, scale):
    hs = rc.scene(name)
    v, s, d = rc.jitter(hs, seed, scale)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d).refit()
    assert not np.array_equal(rc.node_bytes(m.nodes), rc.node_bytes(hs.nodes))
    rays = _aimed_rays(m.desc, m.nodes, 300, seed + 100)
    want = rc.brute_force_closest(m.desc, rays)
    o = ol.lib()
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    got = np.array([o.o_bvh_intersect(C.byref(m.desc), C.byref(buf[i]), None).t for i in range(rays.size)], np.float32)
    hits = int(np.isfinite(want).sum())
    print(f"{name}: {hits}/{rays.size} rays hit")
    assert hits >= rays.size // 4
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, f"{name}: {bad.size} rays differ from the brute force; first: ray {rays[bad[0]]} got {got[bad[0]]} want {want[bad[0]]}"
