"""mi_scene_set_geometry* without a GPU: the mi_scene_geometry layout as a C compiler lays it out, the new symbols in both device
libraries and the host library, and the two refusals that are made before anything is read - a null scene, and a null struct
beside a fake scene handle that must stay untouched. Nothing here opens a device."""
import ctypes as C
import shutil
import subprocess

import pytest

import ipu_ray_lib_amd as irl

ROOT = irl.REPO_ROOT
FIELDS = [name for name, _ in irl.SceneGeometry._fields_]

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_raylib.h"
int main(void) {
  printf("%zu", sizeof(mi_scene_geometry));
""" + "".join(f'  printf(" %zu", offsetof(mi_scene_geometry, {f}));\n' for f in FIELDS) + r"""
  printf("\n");
  return 0;
}
"""


def test_scene_geometry_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G = irl.SceneGeometry
    assert got == [C.sizeof(G)] + [getattr(G, f).offset for f in FIELDS]
    assert C.sizeof(G) == 9 * 16


@pytest.mark.parametrize("variants", [False, True])
def test_set_geometry_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ("mi_scene_set_geometry", "mi_scene_set_geometry_device"):
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_canonical_prims")


@pytest.mark.parametrize("variants", [False, True])
def test_null_arguments_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(8192)                  # stands in for a scene: the rules below must never read or write it
    scene = C.cast(fake, C.c_void_p)
    g = irl.SceneGeometry()
    depth = C.c_uint32(4242)
    for what, (sc, arrays) in {"null scene": (None, C.byref(g)), "null struct": (scene, None), "both null": (None, None)}.items():
        assert lib.mi_scene_set_geometry(sc, arrays, C.byref(depth)) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        assert lib.mi_last_error().startswith(b"mi_scene_set_geometry: "), what
        assert lib.mi_scene_set_geometry_device(sc, arrays, None, C.byref(depth)) == 1, what
        assert lib.mi_last_error().startswith(b"mi_scene_set_geometry_device: "), what
        assert lib.mi_scene_set_geometry(sc, arrays, None) == 1, what                  # (the depth pointer may be NULL)
    assert depth.value == 4242
    assert bytes(fake.raw) == bytes(8192)


def test_from_desc_takes_the_nine_arrays():
    hs = irl.HostScene.builtin("box-simple")
    g = irl.SceneGeometry.from_desc(hs.desc)
    for name in FIELDS:
        assert getattr(g, name) == getattr(hs.desc, name), name
    stats = ("updates_applied", "updates_refused", "rebuilds", "auto_rebuilds", "host_derivations", "cost_evaluations", "max_leaf_depth",
             "geometry_sets")
    import inspect
    assert all(s in inspect.getsource(irl.IpuScene.live_stats) for s in stats)
