"""Geometry updates without a GPU: the mi_geometry_update layout as a C compiler lays it out, the new symbols in both device
libraries and the host library, the update entries' argument rules on a fake scene handle (never dereferenced), and the host
refit mi_refit_compact_bvh - against the builder's own nodes on unchanged geometry, against a numpy restatement on moved
geometry, and on the edge cases that decide a box's bits (signed zeros, NaN coordinates, the largest binary16 extent)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import refit_cases as rc

ROOT = irl.REPO_ROOT

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_raylib.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mi_geometry_update), offsetof(mi_geometry_update, mesh_verts),
         offsetof(mi_geometry_update, num_verts), offsetof(mi_geometry_update, mesh_normals), offsetof(mi_geometry_update, num_normals),
         offsetof(mi_geometry_update, spheres), offsetof(mi_geometry_update, num_spheres), offsetof(mi_geometry_update, discs),
         offsetof(mi_geometry_update, num_discs));
  return 0;
}
"""


def test_geometry_update_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G = irl.GeometryUpdate
    want = [C.sizeof(G)] + [getattr(G, f).offset for f in ("mesh_verts", "num_verts", "mesh_normals", "num_normals", "spheres",
                                                           "num_spheres", "discs", "num_discs")]
    assert got == want


@pytest.mark.parametrize("variants", [False, True])
def test_update_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ("mi_scene_update", "mi_scene_update_device", "mi_scene_get_bvh"):
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_refit_compact_bvh")


@pytest.mark.parametrize("variants", [False, True])
def test_update_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    verts = np.zeros(8, irl.VEC3)
    ok = irl.GeometryUpdate()
    no_array = irl.GeometryUpdate(); no_array.num_verts = 8                       # a count without its array
    no_spheres = irl.GeometryUpdate(); no_spheres.num_spheres = 1
    no_normals = irl.GeometryUpdate(); no_normals.num_normals = 3
    no_discs = irl.GeometryUpdate(); no_discs.num_discs = 2
    ok.mesh_verts, ok.num_verts = verts.ctypes.data, 8
    cases = {"null scene": (None, C.byref(ok)), "null update": (scene, None), "count without array (verts)": (scene, C.byref(no_array)),
             "count without array (spheres)": (scene, C.byref(no_spheres)), "count without array (normals)": (scene, C.byref(no_normals)),
             "count without array (discs)": (scene, C.byref(no_discs))}
    for what, (sc, up) in cases.items():
        assert lib.mi_scene_update(sc, up) == 1, what                     # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        assert b"mi_scene_update" in lib.mi_last_error(), what
        assert lib.mi_scene_update_device(sc, up, None) == 1, what
        assert b"mi_scene_update_device" in lib.mi_last_error(), what
    n = C.c_uint32()
    assert lib.mi_scene_get_bvh(None, None, 0, C.byref(n)) == 1
    assert lib.mi_scene_get_bvh(scene, None, 0, None) == 1
    assert bytes(fake.raw) == bytes(4096)


def test_refit_argument_rules():
    lib = irl.host_lib()
    hs = rc.scene("box-simple")
    out = np.zeros(hs.desc.num_nodes, irl.BVH_NODE)
    assert lib.mi_refit_compact_bvh(None, out.ctypes.data) == 1
    assert lib.mi_refit_compact_bvh(C.byref(hs.desc), None) == 1
    bad = rc.Moved(hs, nodes=hs.nodes.copy())
    bad.nodes["link"][0] = 0                                        # the root's second child before its first
    assert lib.mi_refit_compact_bvh(C.byref(bad.desc), out.ctypes.data) == 1
    assert b"depth-first" in lib.mi_host_last_error()


IDENTITY = ["box-simple", "box", "spheres", "test_scene.dae", "monkey_bust.glb", "soup", "soup-normals"]


@pytest.mark.parametrize("name", IDENTITY)
def test_identity_refit_is_the_builders_nodes(name):
    hs = rc.scene(name)
    rc.assert_nodes_equal(irl.refit_compact_bvh(hs.desc), hs.nodes, f"{name}: identity refit")


@pytest.mark.parametrize("name", ["box-simple", "spheres", "soup", "soup-normals"])
def test_refit_of_moved_geometry_matches_numpy(name):
    hs = rc.scene(name)
    for seed, scale in ((1, 0.25), (2, 7.0)):
        v, s, d = rc.jitter(hs, seed, scale)
        m = rc.Moved(hs, verts=v, spheres=s, discs=d)
        got = irl.refit_compact_bvh(m.desc)
        rc.assert_nodes_equal(got, rc.numpy_refit(m.desc, hs.nodes), f"{name}: jitter {scale}")
        assert not np.array_equal(rc.node_bytes(got), rc.node_bytes(hs.nodes))
        # the topology is kept: links and geomIDs are the builder's
        assert np.array_equal(got["link"], hs.nodes["link"]) and np.array_equal(got["geomID"], hs.nodes["geomID"])


def test_refit_of_a_rigid_move_matches_numpy():
    hs = rc.scene("box")
    m = rc.Moved(hs, verts=rc.rigid(hs, 6, 0.7, (30.0, -5.0, 12.0)))
    rc.assert_nodes_equal(irl.refit_compact_bvh(m.desc), rc.numpy_refit(m.desc, hs.nodes), "box: monkey bust moved")


def _one_triangle_refit(points):
    hs = rc.triangles([[[0, 0, 0], [1, 0, 0], [0, 1, 1]]])
    v = hs.verts.copy()
    p = np.asarray(points, np.float32)
    v["x"], v["y"], v["z"] = p.T
    m = rc.Moved(hs, verts=v)
    out = np.zeros(1, irl.BVH_NODE)
    status = irl.host_lib().mi_refit_compact_bvh(C.byref(m.desc), out.ctypes.data)
    return status, out[0], m, hs


def _bits(f):
    return int(np.array(f, np.float32).view(np.uint32))


def test_refit_signed_zeros_keep_the_first_vertex():
    # Bounds::grow: "p < lo ? p : lo" - -0.0 < +0.0 is false, so the first zero seen stays (fminf would pick -0.0 either way)
    st, n, m, hs = _one_triangle_refit([[0.0, 1, 1], [-0.0, 2, 2], [1, 3, 3]])
    assert st == 0 and _bits(n["min_x"]) == 0x00000000
    st, n, m, hs = _one_triangle_refit([[-0.0, 1, 1], [0.0, 2, 2], [1, 3, 3]])
    assert st == 0 and _bits(n["min_x"]) == 0x80000000
    rc.assert_nodes_equal(np.array([n]), rc.numpy_refit(m.desc, hs.nodes), "signed zeros")


def test_refit_nan_coordinate_is_ignored():
    st, n, m, hs = _one_triangle_refit([[np.nan, 1, 1], [2, 2, 2], [5, 3, 3]])
    assert st == 0
    assert n["min_x"] == 2.0 and np.float16(np.array(n["dx"], np.uint16).view(np.float16)) == 3.0
    rc.assert_nodes_equal(np.array([n]), rc.numpy_refit(m.desc, hs.nodes), "one NaN coordinate")


def test_refit_all_nan_axis_is_refused():
    st, n, m, hs = _one_triangle_refit([[np.nan, 1, 1], [np.nan, 2, 2], [np.nan, 3, 3]])
    assert st == 1 and b"not finite" in irl.host_lib().mi_host_last_error()


def test_refit_largest_half_extent():
    st, n, m, hs = _one_triangle_refit([[0, 0, 0], [65504, 0, 0], [0, 1, 1]])
    assert st == 0 and int(n["dx"]) == 0x7BFF
    above = float(np.nextafter(np.float32(65504), np.float32(np.inf)))
    st, n, m, hs = _one_triangle_refit([[0, 0, 0], [above, 0, 0], [0, 1, 1]])
    assert st == 4 and b"Cannot compress BVH bounds into fp16" in irl.host_lib().mi_host_last_error()      # MI_ERR_IO, the builder's message
