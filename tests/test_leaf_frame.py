"""The tangent frame of a diffuse bounce as a constant of the leaf (scene option leaf_frame; csrc/leaf_frame.hpp, csrc/ray_math.h
diffuse_frame): no GPU needed.

1. csrc/host/diffuse_frame_check.cpp, built and run from here: the select forms of diffuse_frame and sample_disc_concentric against the
   two-branch forms they replaced, bit for bit.
2. The records a scene without vertex normals uploads (mi_leaf_frames runs the upload's fill_leaf_frames): every triangle and disc leaf
   holds diffuse_frame of the normal SHADE reads for it - the face normal recomputed here in numpy binary32, the disc's own -, every
   sphere leaf and interior node holds zeros; in the shared (preorder) order, in the private copy of every node and in the joined array
   plain renders walk (the collapsed tree, then every node)."""
import subprocess
from pathlib import Path

import numpy as np

import ipu_ray_lib_amd as irl
import set_geometry_cases as sg


def test_select_forms_equal_the_branch_forms_bit_for_bit(tmp_path):
    root = Path(irl.REPO_ROOT)
    exe = tmp_path / "diffuse_frame_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", str(exe),
                    str(root / "ipu_ray_lib_amd" / "csrc" / "host" / "diffuse_frame_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "diffuse_frame_check OK" in out.stdout, out.stdout + out.stderr


def flat_contents(size=32, spp=16, moved=False, extra=False):
    """A hand-made scene without vertex normals, every material diffuse: triangles with an oblique normal, with normal (0, 0, 1), with
    normal (1, 0, 0) and of zero area, a diffuse sphere and a disc, round a camera at the origin that looks down -z. moved: every vertex,
    the sphere and the disc somewhere else, every normal another one (the zero-area triangle stays one). extra: a second disc and a
    second sphere (other counts, another tree)."""
    tri = np.array([[[-40, -15, -10], [40, -20, -10], [0, -25, -80]],        # oblique (a floor)
                    [[-40, -30, -60], [40, -30, -60], [0, 50, -60]],         # (80, 0, 0) x (40, 80, 0) = (0, 0, 6400): normal (0, 0, 1)
                    [[-20, -30, -70], [-20, 50, -70], [-20, -30, 0]],        # (0, 80, 0) x (0, 0, 70) = (5600, 0, 0): normal (1, 0, 0)
                    [[5, 5, -50], [5, 5, -50], [6, 6, -50]]], np.float32)    # zero area
    sphere = [0.0, -5.0, -45.0, 6.0]
    disc = [-0.8, 0.6, 0.0, 12.0, 20.0, 0.0, -40.0]                          # (nx, ny, nz, r, cx, cy, cz)
    if moved:
        rng = np.random.default_rng(11)
        tri[:3] += rng.uniform(-4, 4, (3, 3, 3)).astype(np.float32)
        tri[3] += np.float32(1.5)
        sphere = [3.0, -7.0, -42.0, 5.0]
        disc = [-0.6, 0.64, 0.48, 10.0, 18.0, 2.0, -38.0]
    verts = np.zeros(12, irl.VEC3)
    verts["x"], verts["y"], verts["z"] = tri.reshape(12, 3).T
    tris = np.arange(12, dtype="<u2").reshape(4, 3)
    info = np.array([(0, 0, 4, 12)], dtype=irl.MESH_INFO)
    geometry = [(0, 0, 0), (0, 1, 0), (0, 2, 0)]
    spheres, discs = [tuple(sphere)], [tuple(disc)]
    if extra:
        geometry += [(1, 2, 0), (1, 1, 0)]
        discs.append((0.0, -0.6, 0.8, 9.0, -8.0, 14.0, -35.0))
        spheres.append((-10.0, -8.0, -38.0, 4.0))
    G = len(geometry)
    geometry = np.array(geometry, dtype=irl.GEOM_REF)
    spheres = np.array(spheres, dtype=irl.SPHERE)
    discs = np.array(discs, dtype=irl.DISC)
    mats = np.zeros(3, irl.MATERIAL)
    for k, (alb, em) in enumerate((((.7, .6, .5), (.5, .4, .3)), ((.8, .8, .3), (0, 0, 0)), ((.4, .6, .9), (1.5, 1.5, 1.5)))):
        mats[k]["albedo"], mats[k]["emission"], mats[k]["type"], mats[k]["ior"], mats[k]["emissive"] = alb, em, 0, 1.5, int(any(em))
    mat_ids = (np.arange(G) % 3).astype(np.uint32)
    d = irl.SceneDesc()
    d.geometry, d.num_geometry = geometry.ctypes.data, G
    d.mesh_info, d.num_meshes = info.ctypes.data, 1
    d.mesh_tris, d.num_tris = tris.ctypes.data, 4
    d.mesh_verts, d.num_verts = verts.ctypes.data, 12
    d.spheres, d.num_spheres = spheres.ctypes.data, len(spheres)
    d.discs, d.num_discs = discs.ctypes.data, len(discs)
    d.mat_ids, d.num_mat_ids = mat_ids.ctypes.data, G
    d.materials, d.num_materials = mats.ctypes.data, 3
    return sg.Contents(d, "flat" + (" moved" if moved else "") + (" extra" if extra else ""), size=size, spp=spp)      # (copies the arrays)


def _f32(a):
    return np.asarray(a, np.float32)


def _face_normal(p0, p1, p2):
    """normalise(cross(p1 - p0, p2 - p0)) as the upload evaluates it: one rounded binary32 operation per step, the same order."""
    a, b = _f32(p1 - p0), _f32(p2 - p0)
    c = _f32([_f32(a[1] * b[2]) - _f32(a[2] * b[1]), _f32(a[2] * b[0]) - _f32(a[0] * b[2]), _f32(a[0] * b[1]) - _f32(a[1] * b[0])])
    with np.errstate(all="ignore"):
        s = np.float32(np.float32(np.float32(c[0] * c[0]) + np.float32(c[1] * c[1])) + np.float32(c[2] * c[2]))
        return _f32(c * np.float32(np.float32(1.0) / np.sqrt(s)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(got, want):
    """Bit for bit; a NaN made on this host stands for any NaN (numpy's and the library's operand order may differ)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


def _expected_normals(c, nodes):
    """Per node: (framed, normal) from the contents' arrays alone."""
    a = c.a
    xyz = np.stack([a["mesh_verts"]["x"], a["mesh_verts"]["y"], a["mesh_verts"]["z"]], 1)
    framed = np.zeros(len(nodes), bool)
    normal = np.zeros((len(nodes), 3), np.float32)
    for i, nd in enumerate(nodes):
        if nd["geomID"] == 0xFFFF:
            continue
        ref = a["geometry"][nd["geomID"]]
        if ref["type"] == 0:
            info = a["mesh_info"][ref["index"]]
            t = a["mesh_tris"].reshape(-1, 3)[int(info["firstIndex"]) + int(nd["primID"])]
            p = xyz[int(info["firstVertex"]) + t.astype(np.int64)]
            normal[i], framed[i] = _face_normal(p[0], p[1], p[2]), True
        elif ref["type"] == 2:
            q = a["discs"][ref["index"]]
            normal[i], framed[i] = (q["nx"], q["ny"], q["nz"]), True
    return framed, normal


def _node_fields(nodes):
    """A leaf's geometry and primitive (BVH_NODE keeps the primitive's index in the word an interior node keeps its second child in)."""
    out = np.zeros(len(nodes), [("geomID", "<u4"), ("primID", "<u4")])
    out["geomID"], out["primID"] = nodes["geomID"], nodes["link"]
    return out


def test_leaf_records_hold_the_frame_of_the_stored_normal_in_every_order():
    for c in (flat_contents(), flat_contents(moved=True, extra=True), sg.named("box")):
        desc, nodes, _ = c.twin()
        n = len(nodes)
        framed, normal = _expected_normals(c, _node_fields(nodes))
        assert framed.sum() >= 4 and (~framed).sum() >= 2
        full = irl.hot_nodes(nodes)
        joined = irl.hot_join(irl.hot_collapse(nodes), full)
        assert joined["place"].size > n or n < 3
        for what, place in (("shared order", None), ("private copy of every node", full["order"]), ("collapsed tree + every node", joined["place"])):
            frames, normals = irl.leaf_frames(desc, place)
            at = np.arange(n) if place is None else place.astype(np.int64)
            assert frames.shape == (at.size, 8)
            assert _same_floats(normals, normal), f"{c.name}, {what}: the normals the frames are built about are not the upload's"
            for k, i in enumerate(at):
                if framed[i]:
                    want = irl.diffuse_frame(normals[i])
                    rec = np.concatenate([want[0], [0.0], want[1], [0.0]]).astype(np.float32)
                    assert np.array_equal(_bits(frames[k]), _bits(rec)), f"{c.name}, {what}: place {k} (node {i}) holds {frames[k]}, want {rec}"
                else:
                    assert not _bits(frames[k]).any(), f"{c.name}, {what}: place {k} (node {i}, no triangle or disc) is not zero"
        # the frame is what it says: orthonormal about a unit normal, xb x yb = n up to rounding
        for i in np.nonzero(framed)[0]:
            if not np.isfinite(normal[i]).all():
                continue
            xb, yb = irl.diffuse_frame(normal[i]).astype(np.float64)
            assert abs(xb @ yb) < 1e-6 and abs(xb @ normal[i]) < 1e-6 and abs(yb @ normal[i]) < 1e-6 and np.allclose(np.cross(xb, yb), normal[i], atol=1e-6)


def test_leaf_frames_refuses_bad_arguments():
    c = flat_contents()
    desc, nodes, _ = c.twin()
    out = np.zeros((4, 8), np.float32)
    lib = irl.host_lib()
    import ctypes as C
    bad = np.array([0, len(nodes)], np.uint32)
    assert lib.mi_leaf_frames(C.byref(desc), bad.ctypes.data, 2, out.ctypes.data, None) != 0, "a place past the node array"
    assert lib.mi_leaf_frames(C.byref(desc), None, len(nodes) + 1, out.ctypes.data, None) != 0, "more places than nodes without a list"
    assert lib.mi_leaf_frames(C.byref(desc), None, 2, None, None) != 0, "no output array"
