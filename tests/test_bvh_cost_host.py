"""The tree cost on the CPU: the host twin mi_bvh_cost_compact against a numpy restatement of the same reduction shape (bit for
bit), against math.fsum (within the bound any summation order of non-negative terms keeps), and the direction of the metric on
the auto-rebuild policy's purpose scene - with the margins the GPU tests' ratio rests on."""
import math

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import live_cases as lc
import rebuild_cases as bc
import refit_cases as rc


def _assert_twin_is_numpy(nodes, what, block=None):
    got = irl.bvh_cost(nodes, block)
    want = lc.numpy_cost(nodes, block or lc.COST_BLOCK)
    assert lc.bits(got) == np.array(want, np.float64).tobytes(), f"{what}: twin {got}, numpy {want}"
    return got


@pytest.mark.parametrize("name", ["box", "test_scene.dae", "soup"])
def test_twin_equals_numpy_on_scene_trees(name):
    hs = rc.scene(name)
    _assert_twin_is_numpy(hs.nodes, name)
    _assert_twin_is_numpy(irl.build_lbvh(hs.desc)[0], f"{name}: lbvh")


@pytest.mark.parametrize("shape", ["caterpillar", "balanced", "comb"])
def test_twin_equals_numpy_on_hand_made_topologies(shape):
    nodes, _ = rc.retopologise(rc.edge_scene(shape), shape)
    _assert_twin_is_numpy(nodes, shape)


# node counts are odd: the block edges from both sides of W and W^2
@pytest.mark.parametrize("n", [1, 3, 255, 257, 511, 65535, 65537])
def test_twin_equals_numpy_at_the_block_edges(n):
    assert lc.levels_of(n) == (1 if n <= 256 else 2 if n <= 65536 else 3)
    _assert_twin_is_numpy(lc.synthetic_nodes(n, 100 + n), f"{n} nodes")


def test_block_of_four_reaches_three_levels():
    hs = rc.scene("box")
    assert len(hs.nodes) >= 65 and lc.levels_of(65, 4) == 4 and lc.levels_of(63, 4) == 3
    for n in (63, 65, len(hs.nodes)):
        nodes = hs.nodes[:n] if n == len(hs.nodes) else lc.synthetic_nodes(n, n)
        assert lc.levels_of(n, 4) >= 3
        got4 = _assert_twin_is_numpy(nodes, f"{n} nodes, W = 4", block=4)
        got256 = irl.bvh_cost(nodes)
        # another shape is another rounding, not another sum
        assert got4["a_root"] == got256["a_root"]
        assert abs(got4["sum_all"] - got256["sum_all"]) <= 2 * n * 2.0 ** -53 * got256["sum_all"]
    assert irl.host_lib().mi_bvh_cost_compact_block(hs.nodes.ctypes.data, len(hs.nodes), 3, (irl.C.c_double * 3)()) == 1
    assert irl.host_lib().mi_bvh_cost_compact_block(hs.nodes.ctypes.data, len(hs.nodes), 1, (irl.C.c_double * 3)()) == 1


def _assert_within_fsum(nodes, what):
    """Every term is non-negative, so each partial sum is at most the total and any order of N - 1 rounded additions stays within
    (N - 1) * 2^-53 relative of the exact sum, to first order; 2 N * 2^-53 covers the higher orders."""
    got = irl.bvh_cost(nodes)
    a, leaf = lc.terms(nodes)
    N = len(nodes)
    for key, exact in (("sum_all", math.fsum(a)), ("sum_leaf", math.fsum(a[leaf])), ("a_root", float(a[0]))):
        print(f"{what}: {key} twin {got[key]!r} fsum {exact!r}")
        assert abs(got[key] - exact) <= 2 * N * 2.0 ** -53 * exact, f"{what}: {key}"
    return got


@pytest.mark.parametrize("name", ["box", "soup"])
def test_twin_within_fsum_bound_on_scenes(name):
    _assert_within_fsum(rc.scene(name).nodes, name)


def test_twin_on_extreme_extents():
    n = 1023
    zero = _assert_within_fsum(lc.synthetic_nodes(n, 1, np.zeros((n, 3), np.uint16)), "all zero")
    assert zero["sum_all"] == 0.0 and zero["a_root"] == 0.0 and "estimate" not in zero          # a_root == 0 is legal: raw sums only
    sub = np.random.default_rng(2).integers(1, 0x400, (n, 3)).astype(np.uint16)                 # binary16 subnormals
    got = _assert_within_fsum(lc.synthetic_nodes(n, 2, sub), "subnormals")
    assert got["sum_all"] > 0.0
    big = _assert_within_fsum(lc.synthetic_nodes(n, 3, np.full((n, 3), 0x7BFF, np.uint16)), "65504 on all three axes")
    assert big["a_root"] == 3 * 65504.0 ** 2 and big["sum_all"] == n * big["a_root"] and big["sum_leaf"] == (n + 1) // 2 * big["a_root"]
    one = lc.synthetic_nodes(1, 4, [[0x3C00, 0x4000, 0x4200]])                                  # a single leaf of 1 x 2 x 3
    got = _assert_within_fsum(one, "single leaf")
    assert (got["sum_all"], got["sum_leaf"], got["a_root"]) == (11.0, 11.0, 11.0)
    assert irl.bvh_cost(np.zeros(0, irl.BVH_NODE)) == {"sum_all": 0.0, "sum_leaf": 0.0, "a_root": 0.0}


def test_estimate_is_the_stated_formula():
    c = irl.bvh_cost(rc.scene("box").nodes)
    assert c["estimate"] == lc.estimate(c) and c["box_tests"] == c["sum_all"] / c["a_root"] and c["prim_tests"] == c["sum_leaf"] / c["a_root"]


def test_direction_of_the_metric_on_the_purpose_scene():
    """The refit of the thrown scene must cost more than its LBVH (the oracle counts 2100.7 against 83.2 box tests per cast on
    them, tests/test_rebuild_gpu.py); the policy's test ratio sits between 1 and that with a margin of two on both sides."""
    hs, thrown = lc.purpose()
    base = lc.est_of(hs.nodes)
    m = rc.with_topology(hs, hs.nodes, hs.desc.max_leaf_depth, verts=thrown)
    refit = lc.est_of(irl.refit_compact_bvh(m.desc))
    lbvh_nodes, depth = irl.build_lbvh(m.desc)
    lbvh = lc.est_of(lbvh_nodes)
    print(f"estimate: builder {base:.1f}, thrown refit {refit:.1f}, thrown lbvh {lbvh:.1f}; refit / lbvh {refit / lbvh:.3f}, refit / builder {refit / base:.3f}")
    assert refit > lbvh
    R = lc.RATIO
    assert 1.0 < R and 2 * R < refit / lbvh and 2 * R < refit / base                      # the throw lands above R
    # small jitters stay below it: of the original under the builder's tree, and of the thrown scene under its LBVH
    for seed in (3, 4):
        j = rc.with_topology(hs, hs.nodes, hs.desc.max_leaf_depth, verts=lc.small_jitter(hs.verts, seed))
        assert lc.est_of(irl.refit_compact_bvh(j.desc)) < R / 2 * base
        k = rc.with_topology(hs, lbvh_nodes, depth, verts=lc.small_jitter(thrown, seed))
        assert lc.est_of(irl.refit_compact_bvh(k.desc)) < R / 2 * lbvh
