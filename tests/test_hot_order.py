"""The hot-first order of the private copy of the walk's arrays that plain renders may walk (scene option "hot_nodes";
csrc/hot_order.hpp, exported through the host library as mi_hot_nodes / mi_hot_walk): no GPU needed.

For the built-in scenes and a random soup the order must be a bijection that keeps the root first, every successor of the
private node array must point inside it, and a plain CPU walk of the private array (layout-free protocol: a leaf's record
carries the node that follows) must visit, ray for ray, the same nodes and primitives in the same order as a walk of the
shared preorder array. The same host code also runs inside a small stand-alone program under the address and
undefined-behaviour sanitizers (csrc/host/hot_order_check.cpp; nothing of it is loaded into this interpreter)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from test_gpu_parity import _soup_scene

LEAF = np.uint32(0x80000000)
RAYS = 10_000


def _scene_nodes(name):
    if name == "soup":
        return np.array(_soup_scene(np.random.default_rng(77), 600, False).nodes)
    return np.array(irl.HostScene.builtin(name).nodes)


@pytest.fixture(scope="module", params=["box-simple", "box", "spheres", "soup"])
def tree(request):
    nodes = _scene_nodes(request.param)
    return request.param, nodes, irl.hot_nodes(nodes)


def test_order_is_a_bijection_with_the_root_first(tree):
    name, nodes, h = tree
    n = nodes.size
    assert n > 0 and np.array_equal(np.sort(h["order"]), np.arange(n, dtype=np.uint32)), name
    assert h["order"][0] == 0
    if n > 1 and not (h["preorder"]["hit"][0] & LEAF):
        assert h["order"][1] == 1          # (a cast that starts inside the root's box starts at node 1 in either array)
    # the private array holds the shared array's boxes, moved
    assert np.array_equal(h["hot"]["box"], h["preorder"]["box"][h["order"]])


def test_chains_stand_by_falling_half_area(tree):
    name, nodes, h = tree
    pre, order = h["preorder"], h["order"]
    leaf = (pre["hit"] & LEAF) != 0
    head = np.ones(nodes.size, bool); head[1:] = leaf[:-1]          # the root and every second child start a chain
    # a chain is a run of consecutive preorder indices that ends at a leaf
    inside = ~head[order]
    assert np.array_equal(order[inside], order[np.nonzero(inside)[0] - 1] + 1)
    b = pre["box"].astype(np.float64)
    dx, dy, dz = b[:, 1] - b[:, 0], b[:, 3] - b[:, 2], b[:, 5] - b[:, 4]
    area = dx * dy + dy * dz + dz * dx
    heads = order[head[order]][1:]                                    # (the root's chain stands first whatever its area)
    a = area[heads]
    assert np.all(a[:-1] >= a[1:])
    ties = a[:-1] == a[1:]
    assert np.all(heads[:-1][ties] < heads[1:][ties])


def test_prefix_share_is_a_distribution_over_the_places(tree):
    """share[k - 1]: what the first k places take of a random line's box tests under the surface-area model - the figure the
    default of option hot_nodes is decided from (on where the staged prefix takes 0.9: the box scene, not the Collada scene)."""
    name, nodes, h = tree
    sh = h["share"]
    assert np.all(np.diff(sh) >= 0) and sh[0] > 0 and abs(sh[-1] - 1.0) < 1e-12
    # restated: every node weighs its parent's half-area, the root its own
    pre, n = h["preorder"], nodes.size
    b = pre["box"].astype(np.float64)
    dx, dy, dz = b[:, 1] - b[:, 0], b[:, 3] - b[:, 2], b[:, 5] - b[:, 4]
    area = dx * dy + dy * dz + dz * dx
    interior = np.nonzero((pre["hit"] & LEAF) == 0)[0]
    w = np.zeros(n); w[0] = area[0]
    w[interior + 1] = area[interior]
    w[pre["link"][interior + 1] >> 5] = area[interior]
    want = np.cumsum(w[h["order"]]) / w.sum()
    assert np.allclose(sh, want, rtol=1e-12, atol=0)
    if name == "box":
        assert sh[315] > 0.9 > sh[31]


def test_every_successor_points_inside_the_array(tree):
    name, nodes, h = tree
    n = nodes.size
    hot, link = h["hot"], h["leaf_link"]
    end = np.uint32(n << 5)
    leaf = (hot["hit"] & LEAF) != 0
    assert np.all(hot["link"] <= end) and np.all(hot["link"] % 32 == 0)
    own = (np.arange(n, dtype=np.uint32) << 5)
    assert np.array_equal(hot["hit"][leaf], own[leaf] | LEAF)         # a leaf stops the walk AT itself
    assert np.all(hot["hit"][~leaf] < end) and np.all(hot["hit"][~leaf] % 32 == 0)
    assert np.array_equal(link[leaf], hot["link"][leaf]) and np.all(link[~leaf] == 0)
    # the same tree: successors are the shared array's, renumbered
    place = np.empty(n + 1, np.uint32); place[h["order"]] = np.arange(n, dtype=np.uint32); place[n] = n
    pre = h["preorder"][h["order"]]
    assert np.array_equal(hot["link"], place[pre["link"] >> 5] << 5)
    assert np.array_equal(hot["hit"][~leaf], place[pre["hit"][~leaf] >> 5] << 5)


def test_walks_of_both_arrays_visit_the_same_nodes_in_the_same_order(tree):
    name, nodes, h = tree
    rng = np.random.default_rng(5)
    b = h["preorder"]["box"][0]
    lo, hi = b[0::2].astype(np.float64), b[1::2].astype(np.float64)
    span = hi - lo
    origins = rng.uniform(lo - span, hi + span, (RAYS, 3)).astype(np.float32)
    origins[::3] = rng.uniform(lo, hi, (len(origins[::3]), 3)).astype(np.float32)      # a third starts inside the root's box
    dirs = rng.normal(size=(RAYS, 3)).astype(np.float32)
    dirs[::11, rng.integers(0, 3)] = 0.0                                                # axis-parallel rays: infinite reciprocals
    order = h["order"]
    visited = 0
    for o, d in zip(origins, dirs):
        want = irl.hot_walk(h["preorder"], o, d)
        got = irl.hot_walk(h["hot"], o, d, h["leaf_link"])
        assert got.size == want.size
        assert np.array_equal((got & LEAF) | order[got & ~LEAF], want), (name, o, d)
        visited += want.size
    assert visited > RAYS          # (the rays do walk the tree)


def test_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The order builder, the permutation and the walk in a stand-alone program with its own main, compiled with
    -fsanitize=address,undefined: random trees of 0 .. 1000 primitives, 2000 rays each, both walks compared."""
    root = Path(irl.REPO_ROOT)
    host = root / "ipu_ray_lib_amd" / "csrc" / "host"
    exe = tmp_path / "hot_order_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-I", str(root / "include"), "-o", str(exe), str(host / "hot_order.cpp"), str(host / "hot_order_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "hot_order_check OK" in out.stdout, out.stdout + out.stderr
