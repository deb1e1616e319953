"""Neighbour-list C ABI without a GPU: the record as a C99 compiler reads it from include/mi_raylib.h, the entry points exported by
both device libraries and the host library, and the argument rules - checked before anything touches a scene or a device (a fake
scene handle is never dereferenced)."""
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
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_neighbour), offsetof(mi_neighbour, dist2), offsetof(mi_neighbour, primID),
         offsetof(mi_neighbour, geomID), offsetof(mi_neighbour, flags), offsetof(mi_neighbour, point));
  return (int)(sizeof(&mi_near_offsets) + sizeof(&mi_near_offsets_device) + sizeof(&mi_near_fill) + sizeof(&mi_near_fill_device) +
               sizeof(&mi_near_offsets_host) + sizeof(&mi_near_fill_host)) * 0;
}
"""

ENTRIES = ("mi_near_offsets", "mi_near_offsets_device", "mi_near_fill", "mi_near_fill_device")


def test_neighbour_record_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 10, 12]
    d = irl.NEIGHBOUR
    assert d.itemsize == 16 and [d.fields[k][1] for k in ("dist2", "primID", "geomID", "flags", "point")] == [0, 4, 8, 10, 12]


@pytest.mark.parametrize("variants", [False, True])
def test_near_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in ("mi_near_offsets_host", "mi_near_fill_host"):
        assert hasattr(irl.host_lib(), name), name
    for name in ("near_offsets", "near_fill", "neighbours", "k_nearest", "near_offsets_device", "near_fill_device", "ball_query", "knn"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.near_offsets_host) and callable(irl.near_fill_host)


@pytest.mark.parametrize("variants", [False, True])
def test_near_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    pts = irl.aligned_bytes(64 * 16)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    p, o, h = pts.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def offsets_entries(sc, pp, op, n, words, what, host=True):
        assert lib.mi_near_offsets_device(sc, pp, op, n, None) == 1, what          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_near_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_near_offsets(sc, pp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_near_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, pp, op, hp, n, words, what, host=True):
        assert lib.mi_near_fill_device(sc, pp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_near_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_near_fill(sc, pp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_near_fill:" in err and words in err, (what, err)

    offsets_entries(None, p, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null points")
    offsets_entries(scene, p, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, p + 8, o, 4, b"points must be 16-byte aligned", "misaligned points")
    offsets_entries(scene, p + 4, o, 4, b"points must be 16-byte aligned", "misaligned points by 4")
    offsets_entries(scene, p, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, p, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, p, o, big, b"more points than one launch indexes", "too many points", host=False)

    fill_entries(None, p, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null points")
    fill_entries(scene, p, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, p, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, p + 8, o, h, 4, b"points must be 16-byte aligned", "misaligned points")
    fill_entries(scene, p, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, p, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, p, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, p, o, h, big, b"more points than one launch indexes", "too many points", host=False)

    # offsets need 8-byte alignment only
    assert lib.mi_near_offsets_device(None, p, o + 8, 4, None) == 1 and b"null scene" in lib.mi_last_error()
    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_near_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_near_offsets(scene, None, None, 0) == 0
    assert lib.mi_near_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_near_fill(scene, p + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not offs.any() and not hits.any()
