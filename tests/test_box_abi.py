"""Box-query C ABI without a GPU: the box and the record as a C99 compiler reads them from include/mi_raylib.h, the entry points
exported by both device libraries and the host library, and the argument rules - checked before anything touches a scene or a
device (a fake scene handle is never dereferenced)."""
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
  printf("%zu %zu %zu %zu %zu\n", sizeof(mi_box), offsetof(mi_box, lo), offsetof(mi_box, reserved0), offsetof(mi_box, hi),
         offsetof(mi_box, reserved1));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_overlap), offsetof(mi_overlap, primID), offsetof(mi_overlap, geomID),
         offsetof(mi_overlap, flags), offsetof(mi_overlap, box), offsetof(mi_overlap, reserved));
  printf("%d %d %d\n", (int)MI_OVERLAP_CONTAINED, (int)MI_BOX_ANY, (int)MI_BOX_COUNT);
  return (int)(sizeof(&mi_box_query) + sizeof(&mi_box_query_device) + sizeof(&mi_box_offsets) + sizeof(&mi_box_offsets_device) +
               sizeof(&mi_box_fill) + sizeof(&mi_box_fill_device) + sizeof(&mi_box_query_host) + sizeof(&mi_box_offsets_host) +
               sizeof(&mi_box_fill_host)) * 0;
}
"""

ENTRIES = ("mi_box_query", "mi_box_query_device", "mi_box_offsets", "mi_box_offsets_device", "mi_box_fill", "mi_box_fill_device")
TWINS = ("mi_box_query_host", "mi_box_offsets_host", "mi_box_fill_host")


def test_box_and_overlap_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 12, 16, 28, 16, 0, 4, 6, 8, 12, 16, 0, 1]
    b, o = irl.BOX, irl.OVERLAP
    assert b.itemsize == 32 and [b.fields[k][1] for k in ("lo", "reserved0", "hi", "reserved1")] == [0, 12, 16, 28]
    assert o.itemsize == 16 and [o.fields[k][1] for k in ("primID", "geomID", "flags", "box", "reserved")] == [0, 4, 6, 8, 12]
    assert (irl.OVERLAP_CONTAINED, irl.BOX_ANY, irl.BOX_COUNT) == (16, 0, 1)


@pytest.mark.parametrize("variants", [False, True])
def test_box_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in TWINS:
        assert hasattr(irl.host_lib(), name), name
    for name in ("touches", "count_overlaps", "list_overlaps", "first_overlaps", "box_offsets", "box_fill", "box_query_device",
                 "box_offsets_device", "box_fill_device", "box_any", "box_count", "box_list", "voxelize"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.box_query_host) and callable(irl.box_offsets_host) and callable(irl.box_fill_host)
    from ipu_ray_lib_amd import query_batches as qb
    assert callable(qb.make_boxes)


@pytest.mark.parametrize("variants", [False, True])
def test_box_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    bxs = irl.aligned_bytes(64 * 32)
    outs = irl.aligned_bytes(64 * 4)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    b, u, o, h = bxs.ctypes.data, outs.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def query_entries(sc, kind, bp, up, n, words, what, host=True):
        assert lib.mi_box_query_device(sc, kind, bp, up, n, None) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_box_query_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_box_query(sc, kind, bp, up, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_box_query:" in err and words in err, (what, err)

    def offsets_entries(sc, bp, op, n, words, what, host=True):
        assert lib.mi_box_offsets_device(sc, bp, op, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_box_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_box_offsets(sc, bp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_box_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, bp, op, hp, n, words, what, host=True):
        assert lib.mi_box_fill_device(sc, bp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_box_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_box_fill(sc, bp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_box_fill:" in err and words in err, (what, err)

    for kind in (irl.BOX_ANY, irl.BOX_COUNT):
        query_entries(None, kind, b, u, 4, b"null scene", "null scene")
        query_entries(scene, kind, None, u, 4, b"null buffer", "null boxes")
        query_entries(scene, kind, b, None, 4, b"null buffer", "null out")
        query_entries(scene, kind, b + 8, u, 4, b"boxes must be 16-byte aligned", "misaligned boxes")
        query_entries(scene, kind, b + 4, u, 4, b"boxes must be 16-byte aligned", "misaligned boxes by 4")
        query_entries(scene, kind, b, u, big, b"more boxes than one launch indexes", "too many boxes", host=False)
    query_entries(scene, 2, b, u, 4, b"unknown box kind", "unknown kind")
    query_entries(scene, -1, b, u, 4, b"unknown box kind", "unknown kind")
    query_entries(scene, 2, None, None, 0, b"unknown box kind", "an unknown kind comes before n == 0")
    query_entries(scene, irl.BOX_COUNT, b, u + 2, 4, b"counts must be 4-byte aligned", "misaligned counts")
    query_entries(scene, irl.BOX_COUNT, b, u + 1, 4, b"counts must be 4-byte aligned", "misaligned counts by 1")
    # the bytes of BOX_ANY lie anywhere: an odd address passes the buffer rules (what is refused here is the scene)
    assert lib.mi_box_query_device(None, irl.BOX_ANY, b, u + 1, 4, None) == 1 and b"null scene" in lib.mi_last_error()

    offsets_entries(None, b, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null boxes")
    offsets_entries(scene, b, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, b + 8, o, 4, b"boxes must be 16-byte aligned", "misaligned boxes")
    offsets_entries(scene, b, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, b, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, b, o, big, b"more boxes than one launch indexes", "too many boxes", host=False)

    fill_entries(None, b, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null boxes")
    fill_entries(scene, b, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, b, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, b + 8, o, h, 4, b"boxes must be 16-byte aligned", "misaligned boxes")
    fill_entries(scene, b, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, b, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, b, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, b, o, h, big, b"more boxes than one launch indexes", "too many boxes", host=False)

    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_box_query_device(scene, irl.BOX_ANY, None, None, 0, None) == 0
    assert lib.mi_box_query(scene, irl.BOX_COUNT, None, None, 0) == 0
    assert lib.mi_box_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_box_offsets(scene, None, None, 0) == 0
    assert lib.mi_box_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_box_fill(scene, b + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not outs.any() and not offs.any() and not hits.any()


def test_box_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    assert host.mi_box_query_host(None, irl.BOX_ANY, p, p, 1, None) == 1 and b"mi_box_query_host" in host.mi_host_last_error()
    assert host.mi_box_query_host(C.byref(desc), 7, p, p, 1, None) == 1 and b"unknown box kind" in host.mi_host_last_error()
    assert host.mi_box_query_host(C.byref(desc), irl.BOX_ANY, None, p, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_box_offsets_host(None, p, p, 1, None) == 1 and b"mi_box_offsets_host" in host.mi_host_last_error()
    assert host.mi_box_offsets_host(C.byref(desc), p, None, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_box_fill_host(None, p, p, p, 1, 1, None) == 1 and b"mi_box_fill_host" in host.mi_host_last_error()
    assert host.mi_box_fill_host(C.byref(desc), p, p, None, 1, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_box_query_host(C.byref(desc), irl.BOX_COUNT, None, None, 0, None) == 0
