"""The canonical primitive table on the CPU: mi_canonical_prims (the host twin of the kernel that writes the table for
mi_scene_set_geometry*, through the same search and record code, csrc/canon_prims.hpp) against rebuild_cases.canonical_prims - the
plain double loop over geometries and triangles - on the named scenes and on hand-made tables that put geometries without
triangles first, last and in a row, primitive counts round 256 and a 12-step search."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import set_geometry_cases as sg


def _assert_table(c, what):
    table = irl.canonical_prims(c.desc)
    lo, hi, gid, pid = sg.canon_reference(c)
    assert table.size == len(lo) == c.num_prims, f"{what}: {table.size} records, {len(lo)} primitives"
    glo, ghi, ggid, gpid = sg.canon_boxes(c, table)
    assert np.array_equal(ggid, gid) and np.array_equal(gpid, pid), f"{what}: (geomID, primID)"
    assert np.array_equal(glo.view(np.uint32), lo.view(np.uint32)) and np.array_equal(ghi.view(np.uint32), hi.view(np.uint32)), f"{what}: boxes"
    # the rest of the record: the material of its geometry, a triangle's place in the index list and its absolute vertices
    assert np.array_equal(table["matIndex"], c.a["mat_ids"][table["geomID"]]), f"{what}: matIndex"
    geometry, info = c.a["geometry"], c.a["mesh_info"]
    assert np.array_equal(table["kind"], geometry["type"][table["geomID"]]), f"{what}: kind"
    tri = table["kind"] == 0
    m = info[geometry["index"][table["geomID"][tri]]]
    base = 3 * (m["firstIndex"].astype(np.int64) + table["primID"][tri])
    assert np.array_equal(table["triBase"][tri], base), f"{what}: triBase"
    flat = c.a["mesh_tris"].reshape(-1).astype(np.int64)
    for k, f in enumerate("abc"):
        assert np.array_equal(table[f][tri], m["firstVertex"] + flat[base + k]), f"{what}: vertex {f}"
    assert not table["triBase"][~tri].any() and not table["b"][~tri].any() and not table["c"][~tri].any()
    return table


@pytest.mark.parametrize("name", ["box", "spheres", "test_scene.dae", "soup-normals"])
def test_named_scenes(name):
    _assert_table(sg.named(name), name)


@pytest.mark.parametrize("label", list(sg.HAND_MADE))
def test_hand_made_tables(label):
    c = sg.hand(sg.HAND_MADE[label])
    table = _assert_table(c, label)
    if label == "empty scene":
        assert table.size == 0
    if label == "3000 single-sphere geometries":
        assert np.array_equal(table["geomID"], np.arange(3000)) and np.array_equal(table["a"], np.arange(3000))
    if label.endswith("primitives"):
        assert table.size == int(label.split()[0])


def test_from_arrays_scene_with_empty_meshes():
    """The same through mi_host_scene_from_arrays: the packed scene of a desc with a mesh without triangles."""
    c = sg.hand(sg.HAND_MADE["two empty meshes in a row"])
    hs = irl.HostScene.from_arrays(c.desc)
    _assert_table(sg.Contents(hs.desc), "from_arrays")


def _refused(desc, words):
    n = C.c_uint32(77)
    out = np.zeros(4096, irl.CANON_PRIM)
    rc = irl.host_lib().mi_canonical_prims(C.byref(desc), out.ctypes.data, out.size, C.byref(n))
    msg = irl.host_lib().mi_host_last_error().decode()
    assert rc == 1 and words in msg and msg.startswith("mi_canonical_prims: "), (rc, msg)


def test_refusals_use_the_create_words():
    c = sg.hand(sg.HAND_MADE["empty mesh first"])
    m = int(c.a["geometry"]["index"][1])                                   # geometry 1: a mesh with triangles
    c.a["mesh_tris"][3 * (int(c.a["mesh_info"][m]["firstIndex"]) + 2) + 1] = c.a["mesh_info"][m]["numVertices"]
    _refused(c.desc, "triangle vertex index out of range")
    c = sg.hand(sg.HAND_MADE["empty mesh first"])
    c.a["geometry"]["index"][2] = 1                                         # the one sphere is sphere 0
    _refused(c.desc, "geometry index out of range")
    c = sg.hand(sg.HAND_MADE["empty mesh first"])
    c.a["mat_ids"][3] = 3                                                   # three materials
    _refused(c.desc, "material index out of range")
    c = sg.hand(sg.HAND_MADE["empty mesh first"])
    c.desc.mesh_verts = None
    _refused(c.desc, "mesh arrays are null")
    c = sg.hand(sg.HAND_MADE["empty mesh first"])
    c.a["geometry"]["type"][0] = 3
    _refused(c.desc, "unknown geometry type")


def test_count_only_and_capacity():
    c = sg.named("box")
    n = C.c_uint32()
    assert irl.host_lib().mi_canonical_prims(C.byref(c.desc), None, 0, C.byref(n)) == 0 and n.value == c.num_prims
    out = np.zeros(3, irl.CANON_PRIM)
    assert irl.host_lib().mi_canonical_prims(C.byref(c.desc), out.ctypes.data, out.size, C.byref(n)) == 1
    assert "capacity" in irl.host_lib().mi_host_last_error().decode() and not out.view(np.uint32).any()
    assert irl.host_lib().mi_canonical_prims(None, None, 0, C.byref(n)) == 1
