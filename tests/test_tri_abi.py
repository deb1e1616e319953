"""Triangle-query C ABI without a GPU: the triangle and the record as a C99 and a C++ compiler read them from
include/mi_raylib.h, the entry points exported by both device libraries and the host library, and the argument rules - checked
before anything touches a scene or a device (a fake scene handle is never dereferenced)."""
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
  printf("%zu %zu %zu %zu\n", sizeof(mi_tri), offsetof(mi_tri, a), offsetof(mi_tri, b), offsetof(mi_tri, c));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_contact), offsetof(mi_contact, primID), offsetof(mi_contact, geomID),
         offsetof(mi_contact, flags), offsetof(mi_contact, tri), offsetof(mi_contact, reserved));
  printf("%d %d\n", (int)MI_TRI_ANY, (int)MI_TRI_COUNT);
  return (int)(sizeof(&mi_tri_query) + sizeof(&mi_tri_query_device) + sizeof(&mi_tri_offsets) + sizeof(&mi_tri_offsets_device) +
               sizeof(&mi_tri_fill) + sizeof(&mi_tri_fill_device) + sizeof(&mi_tri_query_host) + sizeof(&mi_tri_offsets_host) +
               sizeof(&mi_tri_fill_host)) * 0;
}
"""

ENTRIES = ("mi_tri_query", "mi_tri_query_device", "mi_tri_offsets", "mi_tri_offsets_device", "mi_tri_fill", "mi_tri_fill_device")
TWINS = ("mi_tri_query_host", "mi_tri_offsets_host", "mi_tri_fill_host")


@pytest.mark.parametrize("language", ["c", "c++"])
def test_tri_and_contact_layout(tmp_path, language):
    cc = (shutil.which("gcc") or shutil.which("cc")) if language == "c" else (shutil.which("g++") or shutil.which("c++"))
    assert cc is not None, f"no {language} compiler"
    src = tmp_path / ("layout.c" if language == "c" else "layout.cpp")
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    std = ["-std=c99", "-pedantic-errors"] if language == "c" else ["-std=c++17"]
    subprocess.run([cc, *std, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [36, 0, 12, 24, 16, 0, 4, 6, 8, 12, 0, 1]
    t, c = irl.TRI, irl.CONTACT
    assert t.itemsize == 36 and [t.fields[k][1] for k in ("a", "b", "c")] == [0, 12, 24]
    assert c.itemsize == 16 and [c.fields[k][1] for k in ("primID", "geomID", "flags", "tri", "reserved")] == [0, 4, 6, 8, 12]
    assert (irl.TRI_ANY, irl.TRI_COUNT) == (0, 1)


def test_a_float_array_is_a_batch():
    import numpy as np
    from ipu_ray_lib_amd import query_batches as qb
    v = np.arange(15, dtype=np.float32).reshape(5, 3)
    f = np.array([[0, 1, 2], [4, 2, 3]])
    a = qb.make_tris(v, f)
    b = qb.make_tris(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert a.dtype == irl.TRI and a.shape == (2,) and a.tobytes() == b.tobytes() == v[f].tobytes()


@pytest.mark.parametrize("variants", [False, True])
def test_tri_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in TWINS:
        assert hasattr(irl.host_lib(), name), name
    for name in ("tri_touches", "count_contacts", "list_contacts", "first_contacts", "tri_offsets", "tri_fill", "tri_query_device",
                 "tri_offsets_device", "tri_fill_device", "tri_any", "tri_count", "tri_list", "mesh_contacts", "collides"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.tri_query_host) and callable(irl.tri_offsets_host) and callable(irl.tri_fill_host)


@pytest.mark.parametrize("variants", [False, True])
def test_tri_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    trs = irl.aligned_bytes(64 * 36 + 16)
    outs = irl.aligned_bytes(64 * 4)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    t, u, o, h = trs.ctypes.data, outs.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def query_entries(sc, kind, tp, up, n, words, what, host=True):
        assert lib.mi_tri_query_device(sc, kind, tp, up, n, None) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_tri_query_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_tri_query(sc, kind, tp, up, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_tri_query:" in err and words in err, (what, err)

    def offsets_entries(sc, tp, op, n, words, what, host=True):
        assert lib.mi_tri_offsets_device(sc, tp, op, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_tri_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_tri_offsets(sc, tp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_tri_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, tp, op, hp, n, words, what, host=True):
        assert lib.mi_tri_fill_device(sc, tp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_tri_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_tri_fill(sc, tp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_tri_fill:" in err and words in err, (what, err)

    for kind in (irl.TRI_ANY, irl.TRI_COUNT):
        query_entries(None, kind, t, u, 4, b"null scene", "null scene")
        query_entries(scene, kind, None, u, 4, b"null buffer", "null triangles")
        query_entries(scene, kind, t, None, 4, b"null buffer", "null out")
        query_entries(scene, kind, t + 2, u, 4, b"triangles must be 4-byte aligned", "misaligned triangles by 2")
        query_entries(scene, kind, t + 1, u, 4, b"triangles must be 4-byte aligned", "misaligned triangles by 1")
        query_entries(scene, kind, t, u, big, b"more triangles than one launch indexes", "too many triangles", host=False)
    query_entries(scene, 2, t, u, 4, b"unknown triangle kind", "unknown kind")
    query_entries(scene, -1, t, u, 4, b"unknown triangle kind", "unknown kind")
    query_entries(scene, 2, None, None, 0, b"unknown triangle kind", "an unknown kind comes before n == 0")
    query_entries(scene, irl.TRI_COUNT, t, u + 2, 4, b"counts must be 4-byte aligned", "misaligned counts")
    query_entries(scene, irl.TRI_COUNT, t, u + 1, 4, b"counts must be 4-byte aligned", "misaligned counts by 1")
    # the bytes of TRI_ANY lie anywhere, and triangles at a 4-byte aligned address pass (what is refused here is the scene)
    assert lib.mi_tri_query_device(None, irl.TRI_ANY, t + 4, u + 1, 4, None) == 1 and b"null scene" in lib.mi_last_error()

    offsets_entries(None, t, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null triangles")
    offsets_entries(scene, t, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, t + 2, o, 4, b"triangles must be 4-byte aligned", "misaligned triangles")
    offsets_entries(scene, t, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, t, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, t, o, big, b"more triangles than one launch indexes", "too many triangles", host=False)

    fill_entries(None, t, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null triangles")
    fill_entries(scene, t, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, t, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, t + 2, o, h, 4, b"triangles must be 4-byte aligned", "misaligned triangles")
    fill_entries(scene, t, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, t, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, t, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, t, o, h, big, b"more triangles than one launch indexes", "too many triangles", host=False)

    # n == 0 is a no-op, whatever the buffers: wild pointers are never read
    wild = 0xDEAD0001
    assert lib.mi_tri_query_device(scene, irl.TRI_ANY, None, None, 0, None) == 0
    assert lib.mi_tri_query(scene, irl.TRI_COUNT, wild, wild, 0) == 0
    assert lib.mi_tri_offsets_device(scene, wild, wild, 0, None) == 0
    assert lib.mi_tri_offsets(scene, None, None, 0) == 0
    assert lib.mi_tri_fill_device(scene, wild, wild, wild, 0, 0, None) == 0
    assert lib.mi_tri_fill(scene, t + 1, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not outs.any() and not offs.any() and not hits.any()


def test_tri_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    assert host.mi_tri_query_host(None, irl.TRI_ANY, p, p, 1, None) == 1 and b"mi_tri_query_host" in host.mi_host_last_error()
    assert host.mi_tri_query_host(C.byref(desc), 7, p, p, 1, None) == 1 and b"unknown triangle kind" in host.mi_host_last_error()
    assert host.mi_tri_query_host(C.byref(desc), irl.TRI_ANY, None, p, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_tri_offsets_host(None, p, p, 1, None) == 1 and b"mi_tri_offsets_host" in host.mi_host_last_error()
    assert host.mi_tri_offsets_host(C.byref(desc), p, None, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_tri_fill_host(None, p, p, p, 1, 1, None) == 1 and b"mi_tri_fill_host" in host.mi_host_last_error()
    assert host.mi_tri_fill_host(C.byref(desc), p, p, None, 1, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_tri_query_host(C.byref(desc), irl.TRI_COUNT, None, None, 0, None) == 0
