"""The live loop on the GPU (pytest -m gpu): refit every frame, rebuild when the tree has degraded - decided from the library alone.
mi_scene_bvh_cost equals its host twin bit for bit wherever a scene's nodes come from; option auto_rebuild runs the rebuild from
inside an update exactly when the stated compare says so; and a rebuild leaves the refit's tables ready on the device, so every
update after it equals the host refit under the twin's topology without a host derivation (mi_get_live_stats counts them: 1 when a
scene's first call is an update, 0 when it is a rebuild)."""
import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import live_cases as lc
import rebuild_cases as bc
import refit_cases as rc
import test_refit_gpu as tg

pytestmark = pytest.mark.gpu


def _assert_cost_is_twin(dev, what):
    nodes = dev.bvh_nodes()
    got, want = dev.bvh_cost(), irl.bvh_cost(nodes)
    assert lc.bits(got) == lc.bits(want), f"{what}: device {got}, twin {want}"
    assert got.get("estimate") == want.get("estimate"), what
    return got


# ---- mi_scene_bvh_cost ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 257, 65535, 65537])
def test_cost_equals_twin_at_the_block_edges(n):
    hs = lc.scene_of_nodes(n)
    assert hs.desc.num_nodes == n
    dev = irl.IpuScene(hs.desc)
    fresh = _assert_cost_is_twin(dev, f"{n} nodes, fresh scene")
    st = dev.live_stats()
    assert st["host_derivations"] == 0 and st["updates_applied"] == 0 and st["cost_evaluations"] == 1      # nothing of the update's was built
    dev.update_geometry(vertices=hs.verts.copy())                  # the same positions: the nodes now live on the device
    rc.assert_nodes_equal(dev.bvh_nodes(), hs.nodes, f"{n} nodes: identity update")
    assert dev.live_stats()["host_derivations"] == 1
    counters, nodes = dev.counters(), dev.bvh_nodes()
    first = _assert_cost_is_twin(dev, f"{n} nodes, after an update")
    second = dev.bvh_cost()
    assert lc.bits(first) == lc.bits(second) == lc.bits(fresh), f"{n} nodes: two calls in a row"
    assert dev.counters() == counters
    rc.assert_nodes_equal(dev.bvh_nodes(), nodes, f"{n} nodes: the call changed a node")
    assert dev.live_stats()["cost_evaluations"] == 3
    dev.close()


def test_cost_after_update_and_rebuild_side_stream_blob_and_variants():
    torch = pytest.importorskip("torch")
    hs = rc.scene("soup")
    v, s, d = rc.jitter(hs, 5, 2.0)
    side = torch.cuda.Stream()
    blob = irl.IpuScene.from_blob(irl.serialise_scene(hs.desc), hs.desc)
    for what, dev in (("shipped", irl.IpuScene(hs.desc)), ("variants", irl.IpuScene(hs.desc, variants=True)), ("blob", blob)):
        before = _assert_cost_is_twin(dev, f"{what}: fresh")
        dev.update_geometry(vertices=v, spheres=s, discs=d)
        moved = _assert_cost_is_twin(dev, f"{what}: after an update")
        assert lc.bits(moved) != lc.bits(before)
        dev.rebuild_bvh()
        rebuilt = _assert_cost_is_twin(dev, f"{what}: after a rebuild")
        assert lc.bits(rebuilt) == lc.bits(irl.bvh_cost(bc.rebuilt(hs, verts=v, spheres=s, discs=d).nodes))
        on_side = dev.bvh_cost(side.cuda_stream)
        assert lc.bits(on_side) == lc.bits(rebuilt), f"{what}: side stream"
        dev.close()
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = 0
    empty.num_spheres = empty.num_discs = 0
    assert irl.IpuScene(empty).bvh_cost() == {"sum_all": 0.0, "sum_leaf": 0.0, "a_root": 0.0}


# ---- option auto_rebuild ----------------------------------------------------------------------------------------------------------
def _under(hs, nodes, depth, verts):
    """The host refit of `verts` under the topology `nodes`: what an update that does not rebuild must leave."""
    return rc.with_topology(hs, nodes.copy(), depth, verts=verts).refit()


def _policy_sequence(dev, hs, thrown):
    """jitter, throw, jitter of the thrown, a refused update: the stats after each step."""
    out = []
    dev.update_geometry(vertices=lc.small_jitter(hs.verts, 3)); out.append(dev.live_stats())
    dev.update_geometry(vertices=thrown); out.append(dev.live_stats())
    dev.update_geometry(vertices=lc.small_jitter(thrown, 4)); out.append(dev.live_stats())
    bad = thrown.copy(); bad["x"][:3] = np.nan                     # triangle 0: every point NaN on x
    nodes = dev.bvh_nodes()
    with pytest.raises(irl.RaylibError):
        dev.update_geometry(vertices=bad)
    rc.assert_nodes_equal(dev.bvh_nodes(), nodes, "a refused update changed a node")
    out.append(dev.live_stats())
    return out


def test_auto_rebuild_policy():
    hs, thrown = lc.purpose()
    dev = irl.IpuScene(hs.desc).set_option("auto_rebuild", lc.RATIO)
    twin_dev = irl.IpuScene(hs.desc).set_option("auto_rebuild", lc.RATIO)          # fed the same arrays: stands in for a replica
    depth0 = hs.desc.max_leaf_depth

    j1 = lc.small_jitter(hs.verts, 3)
    dev.update_geometry(vertices=j1)
    st = dev.live_stats()
    assert (st["auto_rebuilds"], st["updates_applied"], st["max_leaf_depth"]) == (0, 1, depth0)
    rc.assert_nodes_equal(dev.bvh_nodes(), _under(hs, hs.nodes, depth0, j1).nodes, "small jitter: the host refit")

    dev.update_geometry(vertices=thrown)
    m = bc.rebuilt(hs, verts=thrown)
    st = dev.live_stats()
    assert (st["auto_rebuilds"], st["rebuilds"], st["updates_applied"]) == (1, 0, 2)
    assert st["max_leaf_depth"] == m.desc.max_leaf_depth
    rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, "the throw: the twin's nodes")
    fresh = irl.IpuScene(m.desc)
    tg._check_queries(dev, fresh, m.desc, tg._rays(m.nodes, 20000, 8), "after the automatic rebuild", oracle_n=1500)
    fresh.close()

    j2 = lc.small_jitter(thrown, 4)
    dev.update_geometry(vertices=j2)
    st = dev.live_stats()
    assert (st["auto_rebuilds"], st["updates_applied"], st["host_derivations"]) == (1, 3, 1)
    after = _under(hs, m.nodes, m.desc.max_leaf_depth, j2)
    rc.assert_nodes_equal(dev.bvh_nodes(), after.nodes, "a further jitter: the host refit under the twin's topology")

    bad = thrown.copy(); bad["x"][:3] = np.nan
    with pytest.raises(irl.RaylibError):
        dev.update_geometry(vertices=bad)
    refused = dev.live_stats()
    assert refused == dict(st, updates_refused=1), "a refused update changes no stat except the refusals"
    rc.assert_nodes_equal(dev.bvh_nodes(), after.nodes, "a refused update changed a node")

    for verts in (j1, thrown, j2):
        twin_dev.update_geometry(vertices=verts)
    rc.assert_nodes_equal(twin_dev.bvh_nodes(), dev.bvh_nodes(), "two scenes fed the same arrays")
    assert twin_dev.live_stats()["auto_rebuilds"] == 1
    dev.close(); twin_dev.close()


def test_auto_rebuild_off_never_rebuilds():
    hs, thrown = lc.purpose()
    dev = irl.IpuScene(hs.desc)
    stats = _policy_sequence(dev, hs, thrown)
    assert [s["auto_rebuilds"] for s in stats] == [0, 0, 0, 0] and [s["rebuilds"] for s in stats] == [0, 0, 0, 0]
    assert [s["updates_applied"] for s in stats] == [1, 2, 3, 3] and stats[-1]["updates_refused"] == 1
    assert stats[-1]["cost_evaluations"] == 0 and stats[-1]["max_leaf_depth"] == hs.desc.max_leaf_depth
    rc.assert_nodes_equal(dev.bvh_nodes(), _under(hs, hs.nodes, hs.desc.max_leaf_depth, lc.small_jitter(thrown, 4)).nodes,
                          "option off: the builder's topology throughout")
    # switched on and off again: "0" is the off value
    dev.set_option("auto_rebuild", 2).set_option("auto_rebuild", 0)
    dev.update_geometry(vertices=thrown)
    assert dev.live_stats()["auto_rebuilds"] == 0
    with pytest.raises(irl.RaylibError):
        dev.set_option("auto_rebuild", 1)
    dev.close()


# ---- a rebuild leaves the refit's tables ready ------------------------------------------------------------------------------------
def _tables_sequence(hs, moves, first_is_rebuild=False, queries=6000):
    """[rebuild ->] update -> rebuild -> update -> rebuild -> update on `moves` (three vertex arrays): after every update the device
    nodes equal the host refit of the moved arrays under the topology before it, and queries equal a fresh scene's."""
    dev = irl.IpuScene(hs.desc)
    nodes, depth = hs.nodes, hs.desc.max_leaf_depth
    current = hs.verts
    derivations = 1
    if first_is_rebuild:
        m = bc.rebuilt(hs)
        assert dev.rebuild_bvh() == m.desc.max_leaf_depth
        nodes, depth = m.nodes, m.desc.max_leaf_depth
        derivations = 0
    for step, verts in enumerate(moves):
        dev.update_geometry(vertices=verts)
        want = _under(hs, nodes, depth, verts)
        rc.assert_nodes_equal(dev.bvh_nodes(), want.nodes, f"update {step}: the host refit under the topology before it")
        assert dev.live_stats()["host_derivations"] == derivations, f"update {step}"
        fresh = irl.IpuScene(want.desc)
        rays = tg._rays(want.nodes, queries, 40 + step)
        tg.assert_bytes_equal(dev.intersect(rays), fresh.intersect(rays), f"update {step}: closest hit")
        assert np.array_equal(dev.occluded(rays), fresh.occluded(rays)), f"update {step}: any hit"
        fresh.close()
        current = verts
        if step < len(moves) - 1:
            m = bc.rebuilt(hs, verts=current)
            assert dev.rebuild_bvh() == m.desc.max_leaf_depth
            rc.assert_nodes_equal(dev.bvh_nodes(), m.nodes, f"rebuild {step}: the twin's nodes")
            nodes, depth = m.nodes, m.desc.max_leaf_depth
    st = dev.live_stats()
    assert st["host_derivations"] == derivations and st["updates_applied"] == len(moves)
    dev.close()
    return st


@pytest.mark.parametrize("first_is_rebuild", [False, True])
def test_tables_after_rebuild_on_a_chain_and_a_tie_cluster(first_is_rebuild):
    hs = lc.chain_scene()
    twin_nodes, twin_depth = bc.twin(hs.desc)
    heights = rc.node_heights(twin_nodes)
    assert heights.max() >= 40 and np.bincount(heights)[1] >= 32          # a chain of at least 40 levels beside the balanced tie tree
    moves = [lc.scaled(hs.verts, f) for f in (1.5, 0.75, 1.25)]           # (scaling keeps the chain and the coincident cluster)
    st = _tables_sequence(hs, moves, first_is_rebuild)
    assert st["rebuilds"] == (3 if first_is_rebuild else 2)


def test_tables_after_rebuild_with_wide_levels():
    hs = rc.soup(9, False, n_tris=6000, n_meshes=2)
    levels, top = rc.top_first(rc.node_heights(bc.twin(hs.desc)[0]))
    assert levels[1] > rc.REFIT_TOP_THREADS and 1 < top <= len(levels) - 1, "both refit_level_kernel and refit_top_kernel must run"
    moves = [rc.jitter(hs, seed, scale)[0] for seed, scale in ((1, 0.3), (2, 1.0), (3, 0.2))]
    _tables_sequence(hs, moves, queries=20000)


def test_tables_after_rebuild_one_primitive_and_an_empty_scene():
    hs = rc.edge_scene("one")
    _tables_sequence(hs, [lc.scaled(hs.verts, f) for f in (2.0, 0.5, 3.0)], queries=2000)
    _tables_sequence(hs, [lc.scaled(hs.verts, f) for f in (2.0, 0.5, 3.0)], first_is_rebuild=True, queries=2000)
    empty = irl.SceneDesc.from_buffer_copy(hs.desc)
    empty.num_geometry = empty.num_meshes = empty.num_tris = empty.num_verts = empty.num_nodes = 0
    dev = irl.IpuScene(empty).set_option("auto_rebuild", 2)
    for _ in range(2):
        dev.update_geometry()
        assert dev.rebuild_bvh() == 0 and len(dev.bvh_nodes()) == 0
    st = dev.live_stats()
    assert (st["updates_applied"], st["auto_rebuilds"], st["rebuilds"], st["host_derivations"]) == (2, 0, 2, 1)
