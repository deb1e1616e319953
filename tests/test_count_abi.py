"""Crossing-count and point-sign C ABI without a GPU: the constants as a C compiler reads them from include/mi_raylib.h, the entry
points exported by both device libraries and the host library, and the argument rules - checked before anything touches a scene
or a device (a fake scene handle is never dereferenced)."""
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
  printf("%d %d %d %zu %zu %zu %zu\n", (int)MI_FLAG_INSIDE, MI_SIGN_INSIDE, MI_SIGN_DISTANCE, sizeof(MI_FLAG_INSIDE), sizeof(mi_ray),
         sizeof(mi_point), sizeof(mi_point_hit));
  return (int)(sizeof(&mi_count_query) + sizeof(&mi_count_query_device) + sizeof(&mi_point_sign) + sizeof(&mi_point_sign_device) +
               sizeof(&mi_sphere_crossings_host)) * 0;
}
"""


def test_sign_constants_and_layouts(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [4, 0, 1, 2, 32, 16, 32]
    assert (irl.FLAG_INSIDE, irl.SIGN_INSIDE, irl.SIGN_DISTANCE) == (4, 0, 1)
    assert irl.FLAG_INSIDE & (irl.FLAG_ERROR | irl.FLAG_ESCAPED) == 0
    d = np.array(irl.DEFAULT_INSIDE_DIR, np.float32)
    assert d.tolist() == [1.0, float(np.float32(0.70710678)), float(np.float32(0.57735027))]
    assert abs(float(d.sum()) - 1.0) > 0.5 and len(set(d.tolist())) == 3 and np.all(d > 0)


@pytest.mark.parametrize("variants", [False, True])
def test_count_and_sign_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ("mi_count_query", "mi_count_query_device", "mi_point_sign", "mi_point_sign_device"):
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_sphere_crossings_host")


@pytest.mark.parametrize("variants", [False, True])
def test_count_query_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    rays = irl.aligned_bytes(64 * 32)
    out = irl.aligned_bytes(64 * 4)
    r, o = rays.ctypes.data, out.ctypes.data
    bad = {
        "null scene": ((None, r, o, 4), b"null scene"),
        "null rays": ((scene, None, o, 4), b"null buffer"),
        "null counts": ((scene, r, None, 4), b"null buffer"),
        "misaligned rays": ((scene, r + 8, o, 4), b"rays must be 16-byte aligned"),
        "misaligned rays by 4": ((scene, r + 4, o, 4), b"rays must be 16-byte aligned"),
        "misaligned counts": ((scene, r, o + 2, 4), b"counts must be 4-byte aligned"),
        "misaligned counts by 1": ((scene, r, o + 1, 4), b"counts must be 4-byte aligned"),
        "too many rays": ((scene, r, o, 0xFFBFFFFF + 1), b"more rays than one launch indexes"),
    }
    for what, ((sc, rp, op, n), words) in bad.items():
        assert lib.mi_count_query_device(sc, rp, op, n, None) == 1, what          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_count_query_device" in err and words in err, (what, err)
        if what != "too many rays":      # (the host entry applies the limit per batch, which needs the scene)
            assert lib.mi_count_query(sc, rp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_count_query:" in err and words in err, (what, err)
    # counts need 4-byte alignment only
    assert lib.mi_count_query_device(None, r, o + 4, 4, None) == 1 and b"null scene" in lib.mi_last_error()
    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_count_query_device(scene, None, None, 0, None) == 0
    assert lib.mi_count_query(scene, None, None, 0) == 0
    assert lib.mi_count_query_device(scene, r + 4, o + 1, 0, None) == 0
    assert bytes(fake.raw) == bytes(4096)


@pytest.mark.parametrize("variants", [False, True])
def test_point_sign_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)
    scene = C.cast(fake, C.c_void_p)
    pts = irl.aligned_bytes(64 * 16)
    out = irl.aligned_bytes(64 * 32)
    p, o = pts.ctypes.data, out.ctypes.data

    def vec(*x):
        return (C.c_float * 3)(*x)
    ok = vec(0.3, -0.4, 0.5)
    nan, inf = float("nan"), float("inf")
    bad = {
        "null scene": ((None, 0, p, o, None, 4), b"null scene"),
        "null points": ((scene, 0, None, o, None, 4), b"null buffer"),
        "null out": ((scene, 1, p, None, ok, 4), b"null buffer"),
        "unknown kind": ((scene, 2, p, o, None, 4), b"unknown sign kind"),
        "kind 7": ((scene, 7, p, o, ok, 4), b"unknown sign kind"),
        "negative kind": ((scene, -1, p, o, None, 4), b"unknown sign kind"),
        "misaligned points": ((scene, 0, p + 4, o, None, 4), b"16-byte aligned"),
        "misaligned points, distance": ((scene, 1, p + 8, o, None, 4), b"16-byte aligned"),
        "misaligned distance out": ((scene, 1, p, o + 8, None, 4), b"16-byte aligned"),
        "too many points": ((scene, 0, p, o, None, 0xFFBFFFFF + 1), b"more points than one launch indexes"),
        "too many points, distance": ((scene, 1, p, o, ok, 0xFFBFFFFF + 1), b"more points than one launch indexes"),
    }
    for k, comp in enumerate((0.0, -0.0, nan, inf, -inf)):
        for axis in range(3):
            d = [1.0, 0.70710678, 0.57735027]
            d[axis] = comp
            bad[f"direction component {axis} = {comp!r}"] = ((scene, k % 2, p, o, vec(*d), 4), b"direction component is zero, NaN or infinite")
    bad["an axis direction"] = ((scene, 0, p, o, vec(1.0, 0.0, 0.0), 4), b"direction component is zero, NaN or infinite")
    for what, ((sc, kind, pp, op, dp, n), words) in bad.items():
        assert lib.mi_point_sign_device(sc, kind, pp, op, dp, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_point_sign_device" in err and words in err, (what, err)
        if not what.startswith("too many points"):      # (the host entry applies the limit per batch, which needs the scene)
            assert lib.mi_point_sign(sc, kind, pp, op, dp, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_point_sign:" in err and words in err, (what, err)
    # n == 0 is a no-op, whatever the buffers; an unknown kind or a refused direction is refused all the same
    assert lib.mi_point_sign_device(scene, 0, None, None, None, 0, None) == 0
    assert lib.mi_point_sign(scene, 1, None, None, ok, 0) == 0
    assert lib.mi_point_sign_device(scene, 7, p, o, None, 0, None) == 1
    assert lib.mi_point_sign(scene, 0, p, o, vec(0.0, 1.0, 1.0), 0) == 1
    # a zero, NaN or infinite direction component is refused before n == 0 is looked at, null buffers or not
    for comp in (0.0, -0.0, nan, inf, -inf):
        for axis in range(3):
            d = [1.0, 0.70710678, 0.57735027]
            d[axis] = comp
            for kind in (0, 1):
                assert lib.mi_point_sign_device(scene, kind, None, None, vec(*d), 0, None) == 1, (comp, axis, kind)
                err = lib.mi_last_error()
                assert b"mi_point_sign_device" in err and b"direction component is zero, NaN or infinite" in err, (comp, axis, kind, err)
                assert lib.mi_point_sign(scene, kind, None, None, vec(*d), 0) == 1, (comp, axis, kind)
                err = lib.mi_last_error()
                assert b"mi_point_sign:" in err and b"direction component is zero, NaN or infinite" in err, (comp, axis, kind, err)
    # the bytes of MI_SIGN_INSIDE need no alignment: an odd out pointer passes the rules (n == 0, so nothing is launched)
    assert lib.mi_point_sign_device(scene, 0, p, o + 1, ok, 0, None) == 0
    assert bytes(fake.raw) == bytes(4096)
