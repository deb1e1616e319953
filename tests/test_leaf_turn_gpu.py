"""K1w's primitive-test (LEAF) turn and the single box test that follows it (pytest -m gpu). The turn reads the leaf's record, runs
the test, and the box test behind it decides where the lane goes next - to another primitive, on through the tree, or out of it.
Wherever that hand-over can go wrong the frame must still be the oracle's, byte for byte, and the instrumented build must count the
oracle's box tests and primitive tests: trees in which the node after a leaf is the end of the array at once (0, 1 and 3 nodes), a
soup whose LAST leaf most rays hit, sphere and disc lanes beside triangle lanes, rays with zero and denormal direction components
(the literal box test behind a LEAF turn) - each on the shared arrays (hot_nodes 0) and on the private hot-first copy (hot_nodes 96),
with and without vertex normals - and one NIF-slot render."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
import set_geometry_cases as sg
from test_gpu_parity import _nif_weights, assert_streams_identical, rows_differing

pytestmark = pytest.mark.gpu

HOT = (0, 96)


def _mesh_scene(points, with_normals, seed=3):
    """One mesh of the given triangles ([n, 3, 3]) under three materials' worth of one diffuse grey, built by the host builder;
    with_normals adds seeded unit vertex normals (the barycentric build of the kernel)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.zeros(len(p), dtype=irl.VEC3); v["x"], v["y"], v["z"] = p.T
    tris = np.arange(len(p), dtype=np.uint16).reshape(-1, 3)
    info = np.zeros(1, dtype=irl.MESH_INFO); info[0] = (0, 0, len(tris), len(p))
    nrm = np.zeros(len(p) if with_normals else 0, dtype=irl.VEC3)
    if with_normals:
        nn = np.random.default_rng(seed).normal(size=(len(p), 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nrm["x"], nrm["y"], nrm["z"] = nn.T
    mats = np.zeros(1, dtype=irl.MATERIAL); mats["albedo"]["x"] = .7; mats["albedo"]["y"] = .6; mats["albedo"]["z"] = .5
    mat_ids = np.zeros(1, np.uint32)
    g = irl.SceneDesc()
    g.mesh_info, g.num_meshes = info.ctypes.data, 1
    g.mesh_tris, g.num_tris = tris.ctypes.data, len(tris)
    g.mesh_verts, g.num_verts = v.ctypes.data, len(v)
    g.mesh_normals, g.num_normals = (nrm.ctypes.data if with_normals else None), len(nrm)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, 1
    g.materials, g.num_materials = mats.ctypes.data, 1
    g.fov_radians = 0.9
    hs = irl.HostScene.from_arrays(g)
    hs._keep = [v, tris, info, nrm, mats, mat_ids]
    return hs


def _with_normals(hs, seed=4):
    """hs's geometry again with seeded unit vertex normals (the host builder sees the same primitives: the same tree)."""
    c = sg.Contents(hs.desc)
    n = len(c.a["mesh_verts"])
    nn = np.random.default_rng(seed).normal(size=(n, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    nrm = np.zeros(n, dtype=irl.VEC3); nrm["x"], nrm["y"], nrm["z"] = nn.T
    g = irl.SceneDesc.from_buffer_copy(c.desc)
    g.mesh_normals, g.num_normals = nrm.ctypes.data, n
    g.fov_radians = hs.desc.fov_radians
    out = irl.HostScene.from_arrays(g)
    out._keep = [c, nrm]
    assert out.desc.num_nodes == hs.desc.num_nodes
    return out


FRONT = [[-6, -5, -5], [6, -5, -5], [0, 6, -5.5]]          # fills most of the view
BEHIND = [[-3, -2, -9], [4, -2, -9.5], [0, 3, -9]]


BIG = [[-60, -50, -40], [70, -55, -41], [5, 80, -40]]


def _fraction_hitting(stream, tri):
    """Share of the stream's un-jittered camera rays (from the origin) that cross the triangle (Moeller-Trumbore, float64)."""
    r = stream["h"]["r"]["direction"]
    dirs = np.stack([r["x"], r["y"], r["z"]], 1).astype(np.float64)
    a, b, c = np.asarray(tri, np.float64)
    e1, e2 = b - a, c - a
    pv = np.cross(dirs, e2)
    det = pv @ e1
    u = (pv @ -a) / det
    qv = np.cross(-a, e1)
    v = (dirs @ qv) / det
    t = (qv @ e2) / det
    return float(((u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)).mean())


def last_leaf_soup(with_normals):
    """Sixty small triangles close to the camera, left of the view's centre, and one large triangle far behind them that fills the
    view: the builder puts it last in the walk's order (asserted) and most camera rays cross it (asserted by the test) - their walk
    ends at the final leaf, whose successor is the end of the array."""
    rng = np.random.default_rng(17)
    centres = rng.uniform(-1, 1, (60, 3)) * [3, 4, 1.5] + [-4, 0, -5]
    small = centres[:, None, :] + rng.normal(scale=0.3, size=(60, 3, 3))
    big = np.array([BIG])
    hs = _mesh_scene(np.concatenate([small, big]), with_normals)
    last = hs.nodes[-1]           # (preorder: the array's last node is the walk's last leaf; a leaf's link is its primitive)
    assert int(last["geomID"]) != 0xFFFF and int(last["link"]) == 60, "the large triangle must be the walk's last leaf"
    return hs


def _params(d, w, h, spp):
    d.set_image(w, h); d.samples_per_pixel = spp; d.path_trace = 1
    d.max_path_length, d.roulette_start_depth, d.rng_seed, d.device = 10, 3, 1442, 0
    return d


def _case(name, normals):
    """(host scene, desc ready to render) of a named case."""
    if name == "one node":
        hs = _mesh_scene([FRONT], normals); d = _params(hs.desc, 40, 24, 8)
        assert d.num_nodes == 1
    elif name == "three nodes":
        hs = _mesh_scene([FRONT, BEHIND], normals); d = _params(hs.desc, 40, 24, 8)
        assert d.num_nodes == 3
    elif name == "last leaf":
        hs = last_leaf_soup(normals); d = _params(hs.desc, 72, 40, 8)
    elif name in ("spheres", "box"):
        hs = irl.HostScene.builtin(name)
        if normals:
            hs = _with_normals(hs)
        d = _params(hs.desc, 64, 64, 8)
    elif name == "zero and denormal directions":
        # anti_alias_scale 0 and a field of view of 1e-38 rad: every camera ray is (x, y, -1) with x and y denormal, and zero in the
        # even-sized image's centre row and column - 1 / x overflows, so every cast of the first bounce takes the literal box test
        hs = irl.HostScene.builtin("box")
        if normals:
            hs = _with_normals(hs)
        d = _params(hs.desc, 32, 24, 12)
        d.anti_alias_scale = 0.0; d.fov_radians = 1e-38
    else:
        raise KeyError(name)
    return hs, d


CASES = [(n, False) for n in ("one node", "three nodes", "last leaf", "spheres", "box", "zero and denormal directions")] + \
        [(n, True) for n in ("one node", "three nodes", "last leaf", "box", "zero and denormal directions")]      # (the spheres scene has no mesh)


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


@pytest.mark.parametrize("name,normals", CASES)
def test_frame_and_counters_are_the_oracles(oracle_frames, name, normals):
    hs, d, first, want, st = oracle_frames[(name, normals)]
    if name == "zero and denormal directions":
        dx, dy = first["h"]["r"]["direction"]["x"], first["h"]["r"]["direction"]["y"]
        tiny = np.float32(1.1754944e-38)
        assert np.all(np.abs(dx) < tiny) and np.all(np.abs(dy) < tiny) and np.any(dx == 0) and np.any(dx != 0) and np.any(dy == 0) and np.any(dy != 0)
    if name == "last leaf":
        assert _fraction_hitting(first, BIG) > 0.5
    assert st.leafTests > 0
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


def test_no_node_at_all():
    """The oracle, like the reference, reads node 0 of any tree and cannot render an empty one: the frame is the nested-loop
    kernel's, in which every path escapes at once."""
    empty = sg.hand([])
    d = sg.render_params(irl.SceneDesc.from_buffer_copy(empty.twin()[0]), 40, 8)
    assert d.num_nodes == 0

    def frame(hot, kernel, stats=0):
        dev = irl.IpuScene(d).set_option("hot_nodes", hot).set_option("kernel", kernel).set_option("full_stats", stats)
        got = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
        irl.host_lib().mi_init_ray_stream(C.byref(d), got.ctypes.data, got.size)
        dev.run(got, irl.MODE_PATH_TRACE)
        c = dev.counters(); dev.close()
        return got, c

    want, _ = frame(0, 0)
    assert np.all(want["h"]["flags"] == irl.FLAG_ESCAPED)
    for hot in HOT:
        got, _ = frame(hot, 1)
        assert_streams_identical(got, want, f"empty scene, hot_nodes={hot}")
        got, c = frame(hot, 1, 1)
        assert_streams_identical(got, want, f"empty scene, hot_nodes={hot}, instrumented build")
        assert (c["nodes_visited"], c["leaf_tests"]) == (0, 0) and c["casts"] == c["paths"] > 0


def test_nif_slot_render_of_the_monkey():
    """NIF renders run K1w's slot build on the shared arrays. Hit records are the oracle's byte for byte; rgb carries the MLP's
    stated tolerance (test_gpu_parity.py::test_config5_monkey_with_nif_environment), which is not this turn's."""
    rng = np.random.default_rng(8)
    ks, bs, relu = _nif_weights(rng, hidden=64, embed=12, layers=4)
    mean = np.array([-2.35, -2.26, -1.96], np.float32)
    s = irl.HostScene.builtin("monkey")
    d = _params(s.desc, 64, 64, 8)
    nif, keep = ol.make_nif(ks, bs, relu, 12, 3.43, mean, True, half_features=True, half_weights_acts=True)
    first = s.init_ray_stream(); want = first.copy()
    st = ol.Stats()
    ol.lib().o_path_trace_nif_pixel_rng(C.byref(d), C.byref(nif), 0.0, want.ctypes.data, want.size, 16, C.byref(st))
    w = np.stack([want["rgb"][k] for k in "xyz"], 1)
    for hot in HOT:
        dev = irl.IpuScene(d).set_option("hot_nodes", hot)
        dev.setNif(ks, bs, relu, 12, 3.43, mean, True)
        got = first.copy(); dev.run(got, irl.MODE_PATH_TRACE); dev.close()
        assert rows_differing(np.ascontiguousarray(got["h"]), np.ascontiguousarray(want["h"])).size == 0, f"hit records, hot_nodes={hot}"
        g = np.stack([got["rgb"][k] for k in "xyz"], 1)
        err = np.abs(g - w) / (np.abs(w) + 0.05)
        assert np.quantile(err, 0.995) < 0.03 and err.max() < 0.3, (hot, np.quantile(err, 0.995), err.max())
