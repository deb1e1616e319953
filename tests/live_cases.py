"""Helpers of the live-loop tests (test_bvh_cost_host.py and test_live_abi.py on the CPU, test_live_loop_gpu.py on the GPU): a numpy
restatement of the tree cost in the reduction's shape, synthetic node arrays of a given count, scenes of a given node count, the
purpose scene of the auto-rebuild policy with its moves and the ratio the tests run it at, and geometry whose LBVH has very
unequal heights."""
import functools

import numpy as np

import ipu_ray_lib_amd as irl
import rebuild_cases as bc
import refit_cases as rc

COST_BLOCK = 256              # kCostBlock (ray_math.h)
BOX_TEST, PRIM_TEST = 26.0, 224.0      # kCostBoxTest, kCostPrimTest (ray_math.h): the estimate's weights

# The ratio the policy tests run at. The estimate of the purpose scene's thrown refit is 9.11 x that of its LBVH (the ratio DESIGN.md
# §18 records) and 7.97 x that of the builder's tree, the baseline it is compared against first; jitters of 0.05 move the estimate
# by less than a factor of 1.001. R sits between 1 and those with a clear margin on both sides, and test_bvh_cost_host.py asserts
# it: jittered trees below R / 2 of their baseline, the throw above 2 R of its own.
RATIO = 3.0


def terms(nodes):
    """(a [N] float64, leaf [N] bool): every node's term (ex * ey + ey * ez) + ez * ex from its binary16 extents."""
    ex, ey, ez = (nodes[k].view(np.float16).astype(np.float64) for k in ("dx", "dy", "dz"))
    with np.errstate(all="ignore"):
        a = (ex * ey + ey * ez) + ez * ex
    return a, nodes["geomID"] != irl.INVALID_GEOM


def _reduce_level(v, W):
    """[n, 2] -> [ceil(n / W), 2]: blocks of W consecutive entries (zeros past the end) through strides W / 2 .. 1."""
    blocks = -(-len(v) // W)
    pad = np.zeros((blocks * W, 2), np.float64)
    pad[:len(v)] = v
    pad = pad.reshape(blocks, W, 2)
    s = W // 2
    while s:
        pad[:, :s] = pad[:, :s] + pad[:, s:2 * s]
        s //= 2
    return pad[:, 0].copy()


def numpy_cost(nodes, W=COST_BLOCK):
    """(sum_all, sum_leaf, a_root) in the shape ray_math.h states: level by level until one entry is left, at least once."""
    if len(nodes) == 0:
        return 0.0, 0.0, 0.0
    a, leaf = terms(nodes)
    v = np.stack([a, np.where(leaf, a, 0.0)], 1)
    levels = 0
    while True:
        v = _reduce_level(v, W)
        levels += 1
        if len(v) == 1:
            break
    return float(v[0, 0]), float(v[0, 1]), float(a[0])


def levels_of(n, W=COST_BLOCK):
    k = 0
    while True:
        n = -(-n // W); k += 1
        if n == 1:
            return k


def estimate(cost):
    """(26 * sum_all + 224 * sum_leaf) / a_root from a bvh_cost dict, restated."""
    return (BOX_TEST * cost["sum_all"] + PRIM_TEST * cost["sum_leaf"]) / cost["a_root"]


def bits(cost):
    return np.array([cost["sum_all"], cost["sum_leaf"], cost["a_root"]], np.float64).tobytes()


def synthetic_nodes(n, seed, halves=None):
    """n nodes (n odd) in a caterpillar's layout with seeded binary16 extents (or `halves`, [n, 3] uint16): the cost reads extents
    and geomIDs only."""
    assert n % 2 == 1
    rng = np.random.default_rng(seed)
    nodes = np.zeros(n, irl.BVH_NODE)
    interior = np.arange(n) % 2 == 0
    interior[-1] = False
    nodes["geomID"] = np.where(interior, irl.INVALID_GEOM, 0)
    nodes["link"] = np.where(interior, np.arange(n) + 2, 0)
    h = rng.integers(0, 0x7BFF, (n, 3)).astype(np.uint16) if halves is None else np.asarray(halves, np.uint16)
    nodes["dx"], nodes["dy"], nodes["dz"] = h.T
    return nodes


@functools.lru_cache(maxsize=None)
def scene_of_nodes(n):
    """A host scene whose BVH has exactly n nodes (n odd): (n + 1) / 2 primitives."""
    prims = (n + 1) // 2
    if prims == 1:
        return rc.edge_scene("one")
    if prims == 2:
        return rc.edge_scene("three")
    tris = prims - 2                                            # soup adds a sphere and a disc
    return rc.soup(5000 + n, False, n_tris=tris, n_meshes=max(2, -(-tris // 20000)))


# ---- the policy's purpose scene (tests/test_rebuild_gpu.py's purpose case) -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def purpose():
    """(hs, thrown): the soup of eight meshes and its vertices with every mesh thrown apart."""
    hs = rc.soup(77, False, n_tris=2000, n_meshes=8)
    v = bc.thrown_apart(hs, 1, 30.0)
    v.setflags(write=False)
    return hs, v


def small_jitter(verts, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    v = verts.copy()
    for c in "xyz":
        v[c] += rng.uniform(-scale, scale, v.size).astype(np.float32)
    return v


def est_of(nodes):
    return irl.bvh_cost(nodes)["estimate"]


# ---- geometry whose LBVH has very unequal heights ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_scene(per_axis=19, cluster=64):
    """Small triangles at 1000 * 2^-k, k = 0 .. per_axis - 1, on each of the three axes - every Morton split peels one of them off:
    a chain of more than 40 levels (one axis alone, or any one line, stops at the key's 21 bits per axis) -, plus `cluster`
    coincident triangles (equal keys: the balanced tie tree)."""
    pts = []
    for axis in range(3):
        for k in range(per_axis):
            p = np.zeros(3); p[axis] = 1000.0 * 2.0 ** -k
            q = p * (1 + 2.0 ** -10)
            r = p.copy(); r[(axis + 1) % 3] = p[axis] * 2.0 ** -10
            pts.append([p, q, r])
    for _ in range(cluster):
        pts.append([[700, 700, 700], [701, 700, 700], [700, 701, 700.5]])
    return rc.triangles(np.array(pts, np.float64))


def scaled(verts, f):
    v = verts.copy()
    for c in "xyz":
        v[c] = (v[c] * np.float32(f)).astype(np.float32)
    return v
