"""Point-query C ABI without a GPU: the mi_point / mi_point_hit layouts as a C compiler lays them out from include/mi_raylib.h,
the POINT / POINT_HIT dtypes beside them, the entry points exported by both device libraries and the host library, and the
argument rules - checked before anything touches a scene or a device (a fake scene handle is never dereferenced)."""
import ctypes as C
import shutil
import subprocess

import pytest

import ipu_ray_lib_amd as irl

ROOT = irl.REPO_ROOT

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_scene_host.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(mi_point), offsetof(mi_point, x), offsetof(mi_point, y),
         offsetof(mi_point, z), offsetof(mi_point, radius), sizeof(mi_point_hit), offsetof(mi_point_hit, dist),
         offsetof(mi_point_hit, prim_id), offsetof(mi_point_hit, geom_id), offsetof(mi_point_hit, flags), offsetof(mi_point_hit, point),
         offsetof(mi_point_hit, b1), offsetof(mi_point_hit, b2), MI_POINT_CLOSEST, MI_POINT_WITHIN);
  return (int)(sizeof(&mi_point_query) + sizeof(&mi_point_query_device) + sizeof(&mi_point_query_host)) * 0;
}
"""


def test_point_layouts_and_dtypes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12, 32, 0, 4, 8, 10, 12, 24, 28, 0, 1]
    p, h = irl.POINT, irl.POINT_HIT
    assert p.itemsize == 16 and [p.fields[f][1] for f in ("x", "y", "z", "radius")] == got[1:5]
    assert h.itemsize == 32 and [h.fields[f][1] for f in ("dist", "primID", "geomID", "flags", "point", "b1", "b2")] == got[6:13]
    assert (irl.POINT_CLOSEST, irl.POINT_WITHIN) == (0, 1)
    from ipu_ray_lib_amd import query_batches as qb
    assert qb.POINT is p and qb.POINT_HIT is h and qb.RAY is irl.RAY


@pytest.mark.parametrize("variants", [False, True])
def test_point_query_symbols_exported(variants):
    lib = irl.device_lib(variants)
    assert hasattr(lib, "mi_point_query") and hasattr(lib, "mi_point_query_device")
    assert hasattr(irl.host_lib(), "mi_point_query_host")


@pytest.mark.parametrize("variants", [False, True])
def test_point_query_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    pts = irl.aligned_bytes(64 * 16)
    out = irl.aligned_bytes(64 * 32)
    p, o = pts.ctypes.data, out.ctypes.data
    bad = {
        "null scene": (None, 0, p, o, 4),
        "null points": (scene, 0, None, o, 4),
        "null out": (scene, 1, p, None, 4),
        "unknown kind": (scene, 2, p, o, 4),
        "negative kind": (scene, -1, p, o, 4),
        "misaligned points": (scene, 0, p + 4, o, 4),
        "misaligned points, within": (scene, 1, p + 8, o, 4),
        "misaligned closest out": (scene, 0, p, o + 8, 4),
        "too many points": (scene, 0, p, o, 0xFFBFFFFF + 1),
        "too many points, within": (scene, 1, p, o, 0xFFBFFFFF + 1),
    }
    words = {"null scene": b"null scene", "null points": b"null buffer", "null out": b"null buffer", "unknown kind": b"unknown query kind",
             "negative kind": b"unknown query kind", "misaligned points": b"16-byte aligned", "misaligned points, within": b"16-byte aligned",
             "misaligned closest out": b"16-byte aligned", "too many points": b"more points than one launch indexes",
             "too many points, within": b"more points than one launch indexes"}
    for what, (sc, kind, pp, op, n) in bad.items():
        assert lib.mi_point_query_device(sc, kind, pp, op, n, None) == 1, what          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_point_query_device" in err and words[what] in err, (what, err)
        if not what.startswith("too many points"):      # (the host entry applies the limit per batch, which needs the scene)
            assert lib.mi_point_query(sc, kind, pp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_point_query:" in err and words[what] in err, (what, err)
    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_point_query_device(scene, 0, None, None, 0, None) == 0
    assert lib.mi_point_query(scene, 1, None, None, 0) == 0
    assert lib.mi_point_query_device(scene, 7, p, o, 0, None) == 1          # (an unknown kind is refused all the same)
    assert bytes(fake.raw) == bytes(4096)
