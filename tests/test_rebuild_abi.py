"""The BVH rebuild without a GPU: the new symbols in both device libraries and the host library, and the argument rules that
touch neither a scene nor a device."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import refit_cases as rc


@pytest.mark.parametrize("variants", [False, True])
def test_rebuild_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ("mi_scene_rebuild", "mi_get_rebuild_timing"):
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_build_lbvh_compact")
    assert hasattr(irl.IpuScene, "rebuild_bvh") and hasattr(irl, "build_lbvh")


@pytest.mark.parametrize("variants", [False, True])
def test_rebuild_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    depth = C.c_uint32(77)
    assert lib.mi_scene_rebuild(None, None, C.byref(depth)) == 1           # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
    assert b"mi_scene_rebuild" in lib.mi_last_error() and depth.value == 77
    assert lib.mi_scene_rebuild(None, None, None) == 1
    fake = C.create_string_buffer(65536)                                   # stands in for a scene: never read
    out = (C.c_double * 6)()
    assert lib.mi_get_rebuild_timing(None, out) == 1 and b"mi_get_rebuild_timing" in lib.mi_last_error()
    assert lib.mi_get_rebuild_timing(C.cast(fake, C.c_void_p), None) == 1
    assert bytes(fake.raw) == bytes(65536)


def test_twin_argument_rules():
    lib = irl.host_lib()
    hs = rc.scene("box-simple")
    out = np.zeros(hs.desc.num_nodes, irl.BVH_NODE)
    n, depth = C.c_uint32(), C.c_uint32()
    assert lib.mi_build_lbvh_compact(None, out.ctypes.data, C.byref(n), C.byref(depth)) == 1
    assert lib.mi_build_lbvh_compact(C.byref(hs.desc), None, C.byref(n), C.byref(depth)) == 1
    assert lib.mi_build_lbvh_compact(C.byref(hs.desc), out.ctypes.data, None, C.byref(depth)) == 1
    assert lib.mi_build_lbvh_compact(C.byref(hs.desc), out.ctypes.data, C.byref(n), None) == 1
    assert b"mi_build_lbvh_compact" in lib.mi_host_last_error()
    bad = irl.SceneDesc.from_buffer_copy(hs.desc)
    geometry = hs._view(hs.desc.geometry, hs.desc.num_geometry, irl.GEOM_REF).copy()
    geometry["index"][0] = 999
    bad.geometry = geometry.ctypes.data
    assert lib.mi_build_lbvh_compact(C.byref(bad), out.ctypes.data, C.byref(n), C.byref(depth)) == 1
    assert b"geometry index out of range" in lib.mi_host_last_error()
    assert lib.mi_build_lbvh_compact(C.byref(hs.desc), out.ctypes.data, C.byref(n), C.byref(depth)) == 0
    assert n.value == hs.desc.num_nodes and depth.value >= 2
