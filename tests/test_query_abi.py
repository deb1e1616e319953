"""Ray-query C ABI without a GPU: the mi_query_hit layout as a C compiler lays it out from include/mi_raylib.h, the
QUERY_HIT dtype beside it, the two entry points exported by both device libraries, and the argument rules - checked before
anything touches a scene or a device (a fake scene handle is never dereferenced)."""
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
#include "mi_raylib.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(mi_query_hit), offsetof(mi_query_hit, t), offsetof(mi_query_hit, prim_id),
         offsetof(mi_query_hit, geom_id), offsetof(mi_query_hit, flags), offsetof(mi_query_hit, normal), offsetof(mi_query_hit, b1),
         offsetof(mi_query_hit, b2), MI_QUERY_CLOSEST, MI_QUERY_ANY);
  return 0;
}
"""


def test_query_hit_layout_and_dtype(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 4, 8, 10, 12, 24, 28, 0, 1]
    q = irl.QUERY_HIT
    assert q.itemsize == 32
    assert [q.fields[f][1] for f in ("t", "primID", "geomID", "flags", "normal", "b1", "b2")] == got[1:8]
    assert (irl.QUERY_CLOSEST, irl.QUERY_ANY) == (0, 1)


@pytest.mark.parametrize("variants", [False, True])
def test_query_symbols_exported(variants):
    lib = irl.device_lib(variants)
    assert hasattr(lib, "mi_query") and hasattr(lib, "mi_query_device")


@pytest.mark.parametrize("variants", [False, True])
def test_query_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    rays = irl.aligned_bytes(64 * 32)
    out = irl.aligned_bytes(64 * 32)
    r, o = rays.ctypes.data, out.ctypes.data
    bad = {
        "null scene": ((None, 0, r, o, 4), b"null scene"),
        "null rays": ((scene, 0, None, o, 4), b"null buffer"),
        "null out": ((scene, 1, r, None, 4), b"null buffer"),
        "unknown kind": ((scene, 2, r, o, 4), b"unknown query kind"),
        "negative kind": ((scene, -1, r, o, 4), b"unknown query kind"),
        "misaligned rays": ((scene, 0, r + 4, o, 4), b"16-byte aligned"),
        "misaligned out": ((scene, 1, r, o + 8, 4), b"16-byte aligned"),
        "too many rays": ((scene, 0, r, o, 0xFFBFFFFF + 1), b"more rays than one launch indexes"),
    }
    for what, ((sc, kind, rp, op, n), words) in bad.items():
        assert lib.mi_query_device(sc, kind, rp, op, n, None) == 1, what          # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_query_device" in err and words in err, (what, err)
        if what != "too many rays":      # (the host entry applies the limit per batch, which needs the scene)
            assert lib.mi_query(sc, kind, rp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_query:" in err and words in err, (what, err)
    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_query_device(scene, 0, None, None, 0, None) == 0
    assert lib.mi_query(scene, 1, None, None, 0) == 0
    assert lib.mi_query_device(scene, 7, r, o, 0, None) == 1          # (an unknown kind is refused all the same)
    assert bytes(fake.raw) == bytes(4096)
