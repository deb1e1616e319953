"""Crossing-list C ABI without a GPU: the record and its flag as a C99 compiler reads them from include/mi_raylib.h, the entry points
exported by both device libraries and the host library, and the argument rules - checked before anything touches a scene or a
device (a fake scene handle is never dereferenced)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import ipu_ray_lib_amd as irl

ROOT = irl.REPO_ROOT

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_scene_host.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d %zu\n", sizeof(mi_crossing), offsetof(mi_crossing, t), offsetof(mi_crossing, primID),
         offsetof(mi_crossing, geomID), offsetof(mi_crossing, flags), offsetof(mi_crossing, ray), (int)MI_CROSS_FAR, sizeof(MI_CROSS_FAR));
  return (int)(sizeof(&mi_list_offsets) + sizeof(&mi_list_offsets_device) + sizeof(&mi_list_fill) + sizeof(&mi_list_fill_device) +
               sizeof(&mi_sphere_roots_host)) * 0;
}
"""

ENTRIES = ("mi_list_offsets", "mi_list_offsets_device", "mi_list_fill", "mi_list_fill_device")


def test_crossing_record_layout_and_constants(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 10, 12, 8, 2]
    d = irl.CROSSING
    assert d.itemsize == 16 and [d.fields[k][1] for k in ("t", "primID", "geomID", "flags", "ray")] == [0, 4, 8, 10, 12]
    assert irl.CROSS_FAR == 8 and irl.CROSS_FAR & (irl.FLAG_ERROR | irl.FLAG_ESCAPED | irl.FLAG_INSIDE) == 0


@pytest.mark.parametrize("variants", [False, True])
def test_list_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_sphere_roots_host")
    for name in ("list_crossings", "first_crossings", "list_offsets_device", "list_fill_device", "cast_all", "cast_first"):
        assert hasattr(irl.IpuScene, name), name


@pytest.mark.parametrize("variants", [False, True])
def test_list_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    rays = irl.aligned_bytes(64 * 32)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    r, o, h = rays.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def offsets_entries(sc, rp, op, n, words, what, host=True):
        assert lib.mi_list_offsets_device(sc, rp, op, n, None) == 1, what          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_list_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_list_offsets(sc, rp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_list_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, rp, op, hp, n, words, what, host=True):
        assert lib.mi_list_fill_device(sc, rp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_list_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_list_fill(sc, rp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_list_fill:" in err and words in err, (what, err)

    offsets_entries(None, r, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null rays")
    offsets_entries(scene, r, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, r + 8, o, 4, b"rays must be 16-byte aligned", "misaligned rays")
    offsets_entries(scene, r + 4, o, 4, b"rays must be 16-byte aligned", "misaligned rays by 4")
    offsets_entries(scene, r, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, r, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, r, o, big, b"more rays than one launch indexes", "too many rays", host=False)

    fill_entries(None, r, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null rays")
    fill_entries(scene, r, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, r, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, r + 8, o, h, 4, b"rays must be 16-byte aligned", "misaligned rays")
    fill_entries(scene, r, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, r, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, r, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, r, o, h, big, b"more rays than one launch indexes", "too many rays", host=False)

    # offsets need 8-byte alignment only
    assert lib.mi_list_offsets_device(None, r, o + 8, 4, None) == 1 and b"null scene" in lib.mi_last_error()
    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_list_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_list_offsets(scene, None, None, 0) == 0
    assert lib.mi_list_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_list_fill(scene, r + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not offs.any() and not hits.any()
