"""The live-loop entries without a GPU: the new symbols in both device libraries and the host library, and the refusals that
touch neither a scene nor a device - on a fake scene handle that must never be read or written."""
import ctypes as C

import numpy as np
import pytest

import ipu_ray_lib_amd as irl


@pytest.mark.parametrize("variants", [False, True])
def test_live_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ("mi_scene_bvh_cost", "mi_get_live_stats"):
        assert hasattr(lib, name), name
    for name in ("mi_bvh_cost_compact", "mi_bvh_cost_compact_block", "mi_bvh_cost_estimate"):
        assert hasattr(irl.host_lib(), name), name


@pytest.mark.parametrize("variants", [False, True])
def test_live_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(1 << 16)               # stands in for a scene: the rules below must never touch it
    scene = C.cast(fake, C.c_void_p)
    out = (C.c_double * 3)()
    stats = (C.c_uint64 * 8)()
    assert lib.mi_scene_bvh_cost(None, None, out) == 1 and b"mi_scene_bvh_cost" in lib.mi_last_error()
    assert lib.mi_scene_bvh_cost(scene, None, None) == 1 and b"mi_scene_bvh_cost" in lib.mi_last_error()
    assert lib.mi_get_live_stats(None, stats) == 1 and b"mi_get_live_stats" in lib.mi_last_error()
    assert lib.mi_get_live_stats(scene, None) == 1
    # auto_rebuild: "0" or a decimal ratio above 1 - anything else is refused, as other keys refuse bad values
    for bad in (b"1", b"0.5", b"-2", b"abc", b"nan", b"", b"inf", b"1.0", b"2x", b"0x2", b" 2"):
        assert lib.mi_scene_set_option(scene, b"auto_rebuild", bad) == 1, bad
        assert b"auto_rebuild" in lib.mi_last_error(), bad
    assert lib.mi_scene_set_option(None, b"auto_rebuild", b"2") == 1
    assert bytes(fake.raw) == bytes(1 << 16)


def test_host_twin_argument_rules():
    lib = irl.host_lib()
    nodes = np.zeros(3, irl.BVH_NODE)
    out = (C.c_double * 3)()
    assert lib.mi_bvh_cost_compact(nodes.ctypes.data, 3, None) == 1
    assert lib.mi_bvh_cost_compact(None, 3, out) == 1
    assert lib.mi_bvh_cost_compact(None, 0, out) == 0 and list(out) == [0.0, 0.0, 0.0]        # an empty scene is legal
