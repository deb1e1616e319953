"""Helpers of the BVH rebuild tests (test_rebuild_host.py and test_rebuild_abi.py on the CPU, test_rebuild_gpu.py on the GPU): the
host twin installed into a desc, the canonical primitives of a desc, a numpy / Python restatement of the LBVH (keys, sort, a
top-down radix tree - not Karras' search -, boxes, child order, preorder layout), which primitives every leaf holds, and the
oracle's closest hit with the runner-up test the geometry-level comparisons use."""
import ctypes as C

import numpy as np

import ipu_ray_lib_amd as irl
import refit_cases as rc

ORACLE_STACK = 128            # oracle/ray_oracle.c walks with a stack of this many entries: every test tree needs depth + 1 <= 128


def twin(desc):
    """(nodes, depth) of mi_build_lbvh_compact, the oracle's stack bound asserted."""
    nodes, depth = irl.build_lbvh(desc)
    assert depth + 1 <= ORACLE_STACK, f"twin depth {depth} does not fit the oracle's stack"
    return nodes, depth


def rebuilt(hs, **arrays):
    """A Moved of hs (geometry replaced by `arrays`) hung under the twin's nodes of those arrays: what a fresh scene is created from."""
    m = rc.Moved(hs, **arrays)
    nodes, depth = twin(m.desc)
    m.desc.num_nodes, m.desc.max_leaf_depth = len(nodes), depth
    return m.set_nodes(nodes)


def canonical_prims(desc):
    """(lo [P, 3], hi [P, 3], geomID [P], primID [P]) in canonical order: geometry 0 .. G - 1, inside a mesh triangle 0 .. T - 1."""
    view = irl.HostScene._view
    geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
    info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
    tris = view(None, desc.mesh_tris, 3 * desc.num_tris, np.dtype("<u2")).astype(np.int64)
    verts = view(None, desc.mesh_verts, desc.num_verts, irl.VEC3)
    spheres = view(None, desc.spheres, desc.num_spheres, irl.SPHERE)
    discs = view(None, desc.discs, desc.num_discs, irl.DISC)
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1) if verts.size else np.zeros((0, 3), np.float32)
    lo, hi, gid, pid = [], [], [], []
    inf = np.float32(np.inf)
    for g, ref in enumerate(geometry):
        if ref["type"] == 0:
            m = info[ref["index"]]
            for t in range(int(m["numTriangles"])):
                l, h = np.full(3, inf, np.float32), np.full(3, -inf, np.float32)
                for k in range(3):
                    p = xyz[int(m["firstVertex"]) + tris[3 * (int(m["firstIndex"]) + t) + k]]
                    l, h = np.where(p < l, p, l), np.where(p > h, p, h)
                lo.append(l); hi.append(h); gid.append(g); pid.append(t)
        else:
            q = spheres[ref["index"]] if ref["type"] == 1 else discs[ref["index"]]
            c = np.array([q["x"], q["y"], q["z"]] if ref["type"] == 1 else [q["cx"], q["cy"], q["cz"]], np.float32)
            r = np.float32(q["radius"] if ref["type"] == 1 else q["r"])
            lo.append((c - r).astype(np.float32)); hi.append((c + r).astype(np.float32)); gid.append(g); pid.append(0)
    P = len(lo)
    return (np.array(lo, np.float32).reshape(P, 3), np.array(hi, np.float32).reshape(P, 3), np.array(gid, np.int64), np.array(pid, np.int64))


def _spread(v):
    out = 0
    for b in range(21):
        out |= ((int(v) >> b) & 1) << (3 * b)
    return out


def numpy_keys(lo, hi):
    """The 63-bit Morton keys (Python ints) of the boxes' centroids inside their union, as ray_math.h lbvh_key states them."""
    with np.errstate(all="ignore"):
        c = ((lo + hi).astype(np.float32) * np.float32(.5)).astype(np.float32)
        slo = (lo.min(0) + np.float32(0)).astype(np.float32)
        shi = (hi.max(0) + np.float32(0)).astype(np.float32)
        ext = (shi - slo).astype(np.float32)
        t = ((c - slo).astype(np.float32) / ext).astype(np.float32)
        s = (t * np.float32(2097152)).astype(np.float32)
    q = np.zeros(s.shape, np.int64)
    ok = (ext > 0)[None, :] & (s >= 0)
    q[ok] = np.minimum(s[ok], np.float32(2097151)).astype(np.int64)
    return [(_spread(a) << 2) | (_spread(b) << 1) | _spread(c_) for a, b, c_ in q]


def numpy_lbvh(desc):
    """(nodes, depth): the LBVH of desc restated - the radix tree over the strings (key, sorted position) built TOP DOWN by
    splitting every range at its highest differing bit (the tree Karras' per-node search finds bottom-up), boxes by compare /
    select, the nearer-centre-first child order in float64, the preorder layout, binary16 extents rounded up."""
    lo, hi, gid, pid = canonical_prims(desc)
    P = len(lo)
    if P == 0:
        return np.zeros(0, irl.BVH_NODE), 0
    keys = numpy_keys(lo, hi)
    order = sorted(range(P), key=lambda p: (keys[p], p))
    strings = [(keys[p] << 32) | j for j, p in enumerate(order)]
    rows, boxes = [], []
    depth_max = 0

    def build(a, b):                    # -> a tree ("leaf", j) / ("node", first, second, box) over sorted positions a .. b
        if a == b:
            p = order[a]
            return ("leaf", p, (lo[p], hi[p]))
        bit = (strings[a] ^ strings[b]).bit_length() - 1
        s = a
        while not (strings[s + 1] >> bit) & 1:
            s += 1
        l, r = build(a, s), build(s + 1, b)

        def dist2(box):
            c = ((box[0] + box[1]).astype(np.float32) * np.float32(.5)).astype(np.float32).astype(np.float64)
            return (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if dist2(r[-1]) < dist2(l[-1]):
            l, r = r, l
        blo, bhi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for p in (l[-1][0], l[-1][1], r[-1][0], r[-1][1]):
            blo, bhi = np.where(p < blo, p, blo), np.where(p > bhi, p, bhi)
        return ("node", l, r, (blo, bhi))

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        tree = build(0, P - 1)
    finally:
        sys.setrecursionlimit(old)
    stack = [(tree, 1, None)]
    while stack:
        t, depth, patch = stack.pop()
        if patch is not None:
            rows[patch][1] = len(rows)
        box = t[-1]
        if t[0] == "leaf":
            rows.append([int(gid[t[1]]), int(pid[t[1]])])
            depth_max = max(depth_max, depth)
        else:
            me = len(rows)
            rows.append([irl.INVALID_GEOM, 0])
            stack.append((t[2], depth + 1, me)); stack.append((t[1], depth + 1, None))
        boxes.append(box)
    nodes = np.zeros(len(rows), irl.BVH_NODE)
    nodes["geomID"], nodes["link"] = [r[0] for r in rows], [r[1] for r in rows]
    blo = np.array([b[0] for b in boxes], np.float32); bhi = np.array([b[1] for b in boxes], np.float32)
    nodes["min_x"], nodes["min_y"], nodes["min_z"] = blo.T
    nodes["dx"], nodes["dy"], nodes["dz"] = rc.half_not_smaller_bits((bhi - blo).astype(np.float32)).T
    return nodes, depth_max


def leaf_pairs(nodes):
    """The (geomID, primID) pairs of the leaves, sorted."""
    leaf = nodes["geomID"] != irl.INVALID_GEOM
    return sorted(zip(nodes["geomID"][leaf].tolist(), nodes["link"][leaf].tolist()))


def assert_format(desc, nodes, depth, what):
    """The Format contract: mi_scene_create's preorder rules, every primitive in exactly one leaf, the refit's fixed point."""
    lo, hi, gid, pid = canonical_prims(desc)
    if len(lo) == 0:
        assert len(nodes) == 0 and depth == 0, what
        return
    walked, leaves = rc.contract_walk(nodes)
    assert walked == depth and leaves == len(lo), f"{what}: depth {walked} / {depth}, leaves {leaves} / {len(lo)}"
    assert leaf_pairs(nodes) == sorted(zip(gid.tolist(), pid.tolist())), f"{what}: the leaves are not the primitives, each once"
    d = irl.SceneDesc.from_buffer_copy(desc)
    keep = np.ascontiguousarray(nodes)
    d.bvh_nodes, d.num_nodes = keep.ctypes.data, len(keep)
    rc.assert_nodes_equal(irl.refit_compact_bvh(d), nodes, f"{what}: refit of the twin's nodes")


def oracle_closest(desc, rays):
    """(t, primID, geomID) of the oracle's closest hit per ray on desc's nodes, and its any-hit answers."""
    import oracle_lib as ol
    o = ol.lib()
    buf = (ol.Ray * rays.size).from_buffer(np.ascontiguousarray(rays).copy())
    t = np.zeros(rays.size, np.float32); prim = np.zeros(rays.size, np.int64); geom = np.zeros(rays.size, np.int64)
    occ = np.zeros(rays.size, bool)
    for i in range(rays.size):
        x = o.o_bvh_intersect(C.byref(desc), C.byref(buf[i]), None)
        t[i] = x.t if x.hit else np.inf
        prim[i], geom[i] = (x.primID, x.geomID) if x.hit else (-1, -1)
        occ[i] = bool(o.o_bvh_occluded(C.byref(desc), C.byref(buf[i]), None))
    return t, prim, geom, occ


def seeded_rays(nodes, n, seed):
    """Rays from inside and around the root box towards random points of it, tMin 0 and tMax inf."""
    from ipu_ray_lib_amd import query_batches as qb
    rng = np.random.default_rng(seed)
    r = nodes[0]
    lo = np.array([r["min_x"], r["min_y"], r["min_z"]], np.float32)
    hi = lo + np.array([r["dx"], r["dy"], r["dz"]], np.uint16).view(np.float16).astype(np.float32)
    size = hi - lo
    o = rng.uniform(lo - size / 2, hi + size / 2, (n, 3)).astype(np.float32)
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return qb.make_rays(o, d.astype(np.float32))


def brute_force_two(desc, rays):
    """(best, runner_up): the two smallest accepted t (float32, inf = none) of each ray over EVERY primitive of desc, with the
    oracle's own leaf tests, as refit_cases.brute_force_closest takes the smallest. best == runner_up: two primitives tie in t."""
    import oracle_lib as ol
    o = ol.lib()
    view = irl.HostScene._view
    geometry = view(None, desc.geometry, desc.num_geometry, irl.GEOM_REF)
    info = view(None, desc.mesh_info, desc.num_meshes, irl.MESH_INFO)
    tris = view(None, desc.mesh_tris, 3 * desc.num_tris, np.dtype("<u2")).reshape(-1, 3)
    verts = view(None, desc.mesh_verts, desc.num_verts, irl.VEC3)
    spheres = view(None, desc.spheres, desc.num_spheres, irl.SPHERE)
    discs = view(None, desc.discs, desc.num_discs, irl.DISC)
    tri_list, others = [], []
    for ref in geometry:
        if ref["type"] == 0:
            m = info[ref["index"]]
            for p in range(int(m["numTriangles"])):
                q = [verts[int(m["firstVertex"]) + int(k)] for k in tris[int(m["firstIndex"]) + p]]
                tri_list.append([ol.Vec3(float(v["x"]), float(v["y"]), float(v["z"])) for v in q])
        elif ref["type"] == 1:
            s = spheres[ref["index"]]
            others.append((o.o_sphere_intersect, ol.Sphere(*[float(s[k]) for k in ("x", "y", "z", "radius")])))
        else:
            d = discs[ref["index"]]
            others.append((o.o_disc_intersect, ol.Disc(*[float(d[k]) for k in ("nx", "ny", "nz", "r", "cx", "cy", "cz")])))
    best = np.full(rays.size, np.inf, np.float32); second = np.full(rays.size, np.inf, np.float32)
    bary = (ol.f32 * 3)()
    for i, r in enumerate(rays):
        ray = ol.Ray(ol.Vec3(*[float(r["origin"][k]) for k in "xyz"]), float(r["tMin"]),
                     ol.Vec3(*[float(r["direction"][k]) for k in "xyz"]), float(r["tMax"]))
        sh = ol.Shear(); o.o_ray_shear(C.byref(ray), C.byref(sh))
        ts = []
        for p0, p1, p2 in tri_list:
            t = o.o_intersect_triangle(p0, p1, p2, C.byref(sh), float("inf"), bary)
            if t > 0.0 and t < float("inf") and t > ray.tMin and t < float(r["tMax"]):
                ts.append(t)
        for fn, rec in others:
            t = fn(C.byref(rec), C.byref(ray))
            if t > ray.tMin and t < float(r["tMax"]):
                ts.append(t)
        ts.sort()
        if ts:
            best[i] = ts[0]
        if len(ts) > 1:
            second[i] = ts[1]
    return best, second


def thrown_apart(hs, seed, reach=40.0):
    """hs's vertices with every mesh rotated and shifted on its own (refit_cases.rigid per mesh): large motion, under which a
    refitted tree's boxes overlap."""
    rng = np.random.default_rng(seed)
    v = hs.verts.copy()
    for mesh in range(hs.desc.num_meshes):
        info = hs.mesh_info[mesh]
        a, b = int(info["firstVertex"]), int(info["firstVertex"] + info["numVertices"])
        w = rc.rigid(hs, mesh, float(rng.uniform(0, 3)), rng.uniform(-reach, reach, 3))
        v[a:b] = w[a:b]
    return v


def nodes_visited_per_cast(desc, size=48, spp=4):
    """The oracle's box tests per cast of a size x size x spp path trace on desc's nodes (deterministic, CPU)."""
    import oracle_lib as ol
    d = irl.SceneDesc.from_buffer_copy(desc)
    d.set_image(size, size); d.samples_per_pixel = spp; d.path_trace = 1
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    st = ol.path_trace_pixel_rng(d, rays, 8)
    return st.nodesVisited / st.casts
