"""Capsule-query C ABI without a GPU: mi_capsule as a C99 and a C++17 compiler read it from include/mi_raylib.h, the entry points
exported by both device libraries and the host library, the argument rules - checked before anything touches a scene or a
device (a fake scene handle is never dereferenced) - and make_capsules."""
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
  printf("%zu %zu %zu %zu %zu\n", sizeof(mi_capsule), offsetof(mi_capsule, a), offsetof(mi_capsule, radius), offsetof(mi_capsule, b),
         offsetof(mi_capsule, reserved));
  printf("%d %d\n", (int)MI_CAPSULE_ANY, (int)MI_CAPSULE_COUNT);
  return (int)(sizeof(&mi_capsule_query) + sizeof(&mi_capsule_query_device) + sizeof(&mi_capsule_offsets) + sizeof(&mi_capsule_offsets_device) +
               sizeof(&mi_capsule_fill) + sizeof(&mi_capsule_fill_device) + sizeof(&mi_capsule_query_host) + sizeof(&mi_capsule_offsets_host) +
               sizeof(&mi_capsule_fill_host) + sizeof(&mi_capsule_meets_bounds_host)) * 0;
}
"""

ENTRIES = ("mi_capsule_query", "mi_capsule_query_device", "mi_capsule_offsets", "mi_capsule_offsets_device", "mi_capsule_fill", "mi_capsule_fill_device")
TWINS = ("mi_capsule_query_host", "mi_capsule_offsets_host", "mi_capsule_fill_host")


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_capsule_layout(tmp_path, compiler, std, suffix):
    cc = shutil.which(compiler)
    assert cc is not None, f"no {compiler}"
    src = tmp_path / ("layout" + suffix)
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, std, "-pedantic-errors", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 12, 16, 28, 0, 1]
    b = irl.CAPSULE
    assert b.itemsize == 32 and [b.fields[k][1] for k in ("a", "radius", "b", "reserved")] == [0, 12, 16, 28]
    assert (irl.CAPSULE_ANY, irl.CAPSULE_COUNT) == (0, 1)


@pytest.mark.parametrize("variants", [False, True])
def test_capsule_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in TWINS:
        assert hasattr(irl.host_lib(), name), name
    for name in ("capsule_touches", "count_capsule_overlaps", "list_capsule_overlaps", "first_capsule_overlaps", "capsule_offsets", "capsule_fill",
                 "capsule_query_device", "capsule_offsets_device", "capsule_fill_device", "capsule_any", "capsule_count", "capsule_list"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.capsule_query_host) and callable(irl.capsule_offsets_host) and callable(irl.capsule_fill_host) and callable(irl.capsule_meets_bounds_host)
    assert hasattr(irl.host_lib(), "mi_capsule_meets_bounds_host")
    from ipu_ray_lib_amd import query_batches as qb
    assert callable(qb.make_capsules) and irl.CAPSULE.itemsize == 32


@pytest.mark.parametrize("variants", [False, True])
def test_capsule_argument_rules_need_no_device(variants):
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
        assert lib.mi_capsule_query_device(sc, kind, bp, up, n, None) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_capsule_query_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_capsule_query(sc, kind, bp, up, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_capsule_query:" in err and words in err, (what, err)

    def offsets_entries(sc, bp, op, n, words, what, host=True):
        assert lib.mi_capsule_offsets_device(sc, bp, op, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_capsule_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_capsule_offsets(sc, bp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_capsule_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, bp, op, hp, n, words, what, host=True):
        assert lib.mi_capsule_fill_device(sc, bp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_capsule_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_capsule_fill(sc, bp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_capsule_fill:" in err and words in err, (what, err)

    for kind in (irl.CAPSULE_ANY, irl.CAPSULE_COUNT):
        query_entries(None, kind, b, u, 4, b"null scene", "null scene")
        query_entries(scene, kind, None, u, 4, b"null buffer", "null capsules")
        query_entries(scene, kind, b, None, 4, b"null buffer", "null out")
        query_entries(scene, kind, b + 8, u, 4, b"capsules must be 16-byte aligned", "misaligned capsules")
        query_entries(scene, kind, b + 4, u, 4, b"capsules must be 16-byte aligned", "misaligned capsules by 4")
        query_entries(scene, kind, b, u, big, b"more capsules than one launch indexes", "too many capsules", host=False)
    query_entries(scene, 2, b, u, 4, b"unknown capsule kind", "unknown kind")
    query_entries(scene, -1, b, u, 4, b"unknown capsule kind", "unknown kind")
    query_entries(scene, 2, None, None, 0, b"unknown capsule kind", "an unknown kind comes before n == 0")
    query_entries(scene, irl.CAPSULE_COUNT, b, u + 2, 4, b"counts must be 4-byte aligned", "misaligned counts")
    query_entries(scene, irl.CAPSULE_COUNT, b, u + 1, 4, b"counts must be 4-byte aligned", "misaligned counts by 1")
    # the bytes of CAPSULE_ANY lie anywhere: an odd address passes the buffer rules (what is refused here is the scene)
    assert lib.mi_capsule_query_device(None, irl.CAPSULE_ANY, b, u + 1, 4, None) == 1 and b"null scene" in lib.mi_last_error()

    offsets_entries(None, b, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null capsules")
    offsets_entries(scene, b, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, b + 8, o, 4, b"capsules must be 16-byte aligned", "misaligned capsules")
    offsets_entries(scene, b, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, b, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, b, o, big, b"more capsules than one launch indexes", "too many capsules", host=False)

    fill_entries(None, b, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null capsules")
    fill_entries(scene, b, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, b, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, b + 8, o, h, 4, b"capsules must be 16-byte aligned", "misaligned capsules")
    fill_entries(scene, b, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, b, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, b, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, b, o, h, big, b"more capsules than one launch indexes", "too many capsules", host=False)

    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_capsule_query_device(scene, irl.CAPSULE_ANY, None, None, 0, None) == 0
    assert lib.mi_capsule_query(scene, irl.CAPSULE_COUNT, None, None, 0) == 0
    assert lib.mi_capsule_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_capsule_offsets(scene, None, None, 0) == 0
    assert lib.mi_capsule_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_capsule_fill(scene, b + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not outs.any() and not offs.any() and not hits.any()


def test_capsule_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    assert host.mi_capsule_query_host(None, irl.CAPSULE_ANY, p, p, 1, None) == 1 and b"mi_capsule_query_host" in host.mi_host_last_error()
    assert host.mi_capsule_query_host(C.byref(desc), 7, p, p, 1, None) == 1 and b"unknown capsule kind" in host.mi_host_last_error()
    assert host.mi_capsule_query_host(C.byref(desc), irl.CAPSULE_ANY, None, p, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_capsule_offsets_host(None, p, p, 1, None) == 1 and b"mi_capsule_offsets_host" in host.mi_host_last_error()
    assert host.mi_capsule_offsets_host(C.byref(desc), p, None, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_capsule_fill_host(None, p, p, p, 1, 1, None) == 1 and b"mi_capsule_fill_host" in host.mi_host_last_error()
    assert host.mi_capsule_fill_host(C.byref(desc), p, p, None, 1, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_capsule_query_host(C.byref(desc), irl.CAPSULE_COUNT, None, None, 0, None) == 0


def test_n_zero_with_wild_pointers():
    """n == 0 reads and writes nothing, on the device entries (a scene handle that is never read) and on the twins."""
    wild = 0xDEAD0001                                    # odd, unmapped
    fake = C.create_string_buffer(4096)
    scene = C.cast(fake, C.c_void_p)
    for variants in (False, True):
        lib = irl.device_lib(variants)
        assert lib.mi_capsule_query_device(scene, irl.CAPSULE_ANY, wild, wild, 0, None) == 0
        assert lib.mi_capsule_query(scene, irl.CAPSULE_COUNT, wild, wild, 0) == 0
        assert lib.mi_capsule_offsets_device(scene, wild, wild, 0, None) == 0
        assert lib.mi_capsule_offsets(scene, wild, wild, 0) == 0
        assert lib.mi_capsule_fill_device(scene, wild, wild, wild, 5, 0, None) == 0
        assert lib.mi_capsule_fill(scene, wild, wild, wild, 5, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    host = irl.host_lib()
    desc = irl.SceneDesc()
    assert host.mi_capsule_query_host(C.byref(desc), irl.CAPSULE_ANY, wild, wild, 0, None) == 0
    assert host.mi_capsule_fill_host(C.byref(desc), wild, wild, wild, 5, 0, None) == 0
    visits = (C.c_uint64 * 2)(7, 7)
    assert host.mi_capsule_query_host(C.byref(desc), irl.CAPSULE_COUNT, wild, wild, 0, visits) == 0 and list(visits) == [0, 0]


def test_make_capsules():
    import numpy as np
    from ipu_ray_lib_amd import query_batches as qb
    rng = np.random.default_rng(7)
    n = 9
    a, b = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    r = rng.uniform(0, 2, n)
    one = qb.make_capsules(a, b, 0.75)                            # float64 in, a scalar radius
    assert one.dtype == irl.CAPSULE and one.shape == (n,) and one.flags["C_CONTIGUOUS"] and one.strides == (32,)
    assert np.array_equal(one["a"], a.astype(np.float32)) and np.array_equal(one["b"], b.astype(np.float32))
    assert np.all(one["radius"] == np.float32(0.75)) and not one["reserved"].any()
    many = qb.make_capsules(a.astype(np.float32), b.astype(np.float32), r)      # an array radius
    assert np.array_equal(many["radius"], r.astype(np.float32)) and many["a"].tobytes() == one["a"].tobytes()
    # strided and transposed inputs are taken by value
    wide = rng.normal(size=(n, 6))
    got = qb.make_capsules(wide[:, :3], wide[:, 3:], r[::-1])
    assert np.array_equal(got["a"], wide[:, :3].astype(np.float32)) and np.array_equal(got["b"], wide[:, 3:].astype(np.float32))
    assert np.array_equal(got["radius"], r[::-1].astype(np.float32))
    got = qb.make_capsules(a.T.copy().T, b, r)
    assert got.tobytes() == qb.make_capsules(a, b, r).tobytes()
    # the record is what the C header lays out: a, radius, b, reserved as eight words
    words = many.view(np.float32).reshape(n, 8)
    assert np.array_equal(words[:, 0:3], many["a"]) and np.array_equal(words[:, 3], many["radius"]) and np.array_equal(words[:, 4:7], many["b"])
    assert not many.view(np.uint32).reshape(n, 8)[:, 7].any()
    # aligned_bytes gives the 16-byte alignment the device entries ask for
    buf = irl.aligned_bytes(many.nbytes).view(irl.CAPSULE)
    buf[:] = many
    assert buf.ctypes.data % 16 == 0 and buf.tobytes() == many.tobytes()
    assert qb.make_capsules(np.zeros((0, 3)), np.zeros((0, 3)), 1.0).shape == (0,)
    for bad in ((a, b[:-1], 1.0), (a, b, r[:-1]), (a, b, np.ones((n, 1)))):
        with pytest.raises(ValueError, match="make_capsules"):
            qb.make_capsules(*bad)
