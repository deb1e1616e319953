"""Oriented-box-query C ABI without a GPU: mi_obox as a C99 and a C++17 compiler read it from include/mi_raylib.h, the entry points
exported by both device libraries and the host library, the argument rules - checked before anything touches a scene or a
device (a fake scene handle is never dereferenced) - and make_oboxes."""
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
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_obox), offsetof(mi_obox, centre), offsetof(mi_obox, reserved0), offsetof(mi_obox, half),
         offsetof(mi_obox, reserved1), offsetof(mi_obox, quat));
  printf("%d %d\n", (int)MI_OBOX_ANY, (int)MI_OBOX_COUNT);
  return (int)(sizeof(&mi_obox_query) + sizeof(&mi_obox_query_device) + sizeof(&mi_obox_offsets) + sizeof(&mi_obox_offsets_device) +
               sizeof(&mi_obox_fill) + sizeof(&mi_obox_fill_device) + sizeof(&mi_obox_query_host) + sizeof(&mi_obox_offsets_host) +
               sizeof(&mi_obox_fill_host) + sizeof(&mi_obox_meets_bounds_host)) * 0;
}
"""

ENTRIES = ("mi_obox_query", "mi_obox_query_device", "mi_obox_offsets", "mi_obox_offsets_device", "mi_obox_fill", "mi_obox_fill_device")
TWINS = ("mi_obox_query_host", "mi_obox_offsets_host", "mi_obox_fill_host")


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_obox_layout(tmp_path, compiler, std, suffix):
    cc = shutil.which(compiler)
    assert cc is not None, f"no {compiler}"
    src = tmp_path / ("layout" + suffix)
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, std, "-pedantic-errors", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [48, 0, 12, 16, 28, 32, 0, 1]
    b = irl.OBOX
    assert b.itemsize == 48 and [b.fields[k][1] for k in ("centre", "reserved0", "half", "reserved1", "quat")] == [0, 12, 16, 28, 32]
    assert (irl.OBOX_ANY, irl.OBOX_COUNT) == (0, 1)


@pytest.mark.parametrize("variants", [False, True])
def test_obox_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in TWINS:
        assert hasattr(irl.host_lib(), name), name
    for name in ("obox_touches", "count_obox_overlaps", "list_obox_overlaps", "first_obox_overlaps", "obox_offsets", "obox_fill",
                 "obox_query_device", "obox_offsets_device", "obox_fill_device", "obox_any", "obox_count", "obox_list"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.obox_query_host) and callable(irl.obox_offsets_host) and callable(irl.obox_fill_host)
    from ipu_ray_lib_amd import query_batches as qb
    assert callable(qb.make_oboxes) and irl.OBOX.itemsize == 48


@pytest.mark.parametrize("variants", [False, True])
def test_obox_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    bxs = irl.aligned_bytes(64 * 48)
    outs = irl.aligned_bytes(64 * 4)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    b, u, o, h = bxs.ctypes.data, outs.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def query_entries(sc, kind, bp, up, n, words, what, host=True):
        assert lib.mi_obox_query_device(sc, kind, bp, up, n, None) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_obox_query_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_obox_query(sc, kind, bp, up, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_obox_query:" in err and words in err, (what, err)

    def offsets_entries(sc, bp, op, n, words, what, host=True):
        assert lib.mi_obox_offsets_device(sc, bp, op, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_obox_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_obox_offsets(sc, bp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_obox_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, bp, op, hp, n, words, what, host=True):
        assert lib.mi_obox_fill_device(sc, bp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_obox_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_obox_fill(sc, bp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_obox_fill:" in err and words in err, (what, err)

    for kind in (irl.OBOX_ANY, irl.OBOX_COUNT):
        query_entries(None, kind, b, u, 4, b"null scene", "null scene")
        query_entries(scene, kind, None, u, 4, b"null buffer", "null oriented boxes")
        query_entries(scene, kind, b, None, 4, b"null buffer", "null out")
        query_entries(scene, kind, b + 8, u, 4, b"oriented boxes must be 16-byte aligned", "misaligned oriented boxes")
        query_entries(scene, kind, b + 4, u, 4, b"oriented boxes must be 16-byte aligned", "misaligned oriented boxes by 4")
        query_entries(scene, kind, b, u, big, b"more oriented boxes than one launch indexes", "too many oriented boxes", host=False)
    query_entries(scene, 2, b, u, 4, b"unknown oriented-box kind", "unknown kind")
    query_entries(scene, -1, b, u, 4, b"unknown oriented-box kind", "unknown kind")
    query_entries(scene, 2, None, None, 0, b"unknown oriented-box kind", "an unknown kind comes before n == 0")
    query_entries(scene, irl.OBOX_COUNT, b, u + 2, 4, b"counts must be 4-byte aligned", "misaligned counts")
    query_entries(scene, irl.OBOX_COUNT, b, u + 1, 4, b"counts must be 4-byte aligned", "misaligned counts by 1")
    # the bytes of OBOX_ANY lie anywhere: an odd address passes the buffer rules (what is refused here is the scene)
    assert lib.mi_obox_query_device(None, irl.OBOX_ANY, b, u + 1, 4, None) == 1 and b"null scene" in lib.mi_last_error()

    offsets_entries(None, b, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null oriented boxes")
    offsets_entries(scene, b, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, b + 8, o, 4, b"oriented boxes must be 16-byte aligned", "misaligned oriented boxes")
    offsets_entries(scene, b, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, b, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, b, o, big, b"more oriented boxes than one launch indexes", "too many oriented boxes", host=False)

    fill_entries(None, b, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null oriented boxes")
    fill_entries(scene, b, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, b, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, b + 8, o, h, 4, b"oriented boxes must be 16-byte aligned", "misaligned oriented boxes")
    fill_entries(scene, b, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, b, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, b, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, b, o, h, big, b"more oriented boxes than one launch indexes", "too many oriented boxes", host=False)

    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_obox_query_device(scene, irl.OBOX_ANY, None, None, 0, None) == 0
    assert lib.mi_obox_query(scene, irl.OBOX_COUNT, None, None, 0) == 0
    assert lib.mi_obox_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_obox_offsets(scene, None, None, 0) == 0
    assert lib.mi_obox_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_obox_fill(scene, b + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not outs.any() and not offs.any() and not hits.any()


def test_obox_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    assert host.mi_obox_query_host(None, irl.OBOX_ANY, p, p, 1, None) == 1 and b"mi_obox_query_host" in host.mi_host_last_error()
    assert host.mi_obox_query_host(C.byref(desc), 7, p, p, 1, None) == 1 and b"unknown oriented-box kind" in host.mi_host_last_error()
    assert host.mi_obox_query_host(C.byref(desc), irl.OBOX_ANY, None, p, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_obox_offsets_host(None, p, p, 1, None) == 1 and b"mi_obox_offsets_host" in host.mi_host_last_error()
    assert host.mi_obox_offsets_host(C.byref(desc), p, None, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_obox_fill_host(None, p, p, p, 1, 1, None) == 1 and b"mi_obox_fill_host" in host.mi_host_last_error()
    assert host.mi_obox_fill_host(C.byref(desc), p, p, None, 1, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_obox_query_host(C.byref(desc), irl.OBOX_COUNT, None, None, 0, None) == 0


def test_make_oboxes_takes_a_quaternion_or_its_matrix():
    import numpy as np
    from ipu_ray_lib_amd import query_batches as qb
    import point_cases as pc
    hs = pc.scene("soup")
    rng = np.random.default_rng(5)
    n = 40
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    # the matrix of the same rotation: its COLUMNS are the box's axes U, V, W of the contract
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    lo, hi = pc.root_box(hs.nodes)
    centre = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    half = rng.uniform(2.0, 12.0, (n, 3)).astype(np.float32)
    a = qb.make_oboxes(centre, half, quat=q)
    b = qb.make_oboxes(centre, half, matrix=R)
    assert a.dtype == irl.OBOX and b.dtype == irl.OBOX and a.size == n
    back = qb.matrix_to_quat(R)                                    # float64: the conversion itself, before make_oboxes rounds it to float32
    sign = np.sign((back * q).sum(1))[:, None]
    assert np.abs(back * sign - q).max() < 1e-12, "the matrix gives the quaternion back, up to sign, to what float64 gives"
    b["quat"] *= sign.astype(np.float32)      # (q and -q are one rotation; the same sign gives the same float32 frame)
    assert b["quat"].tobytes() == a["quat"].tobytes(), "rounded to float32 the two are the same quaternions"
    la, _ = irl.obox_offsets_host(hs.desc, a)
    lb, _ = irl.obox_offsets_host(hs.desc, b)
    ra, _ = irl.obox_fill_host(hs.desc, a, la)
    rb, _ = irl.obox_fill_host(hs.desc, b, lb)
    assert la[-1] > 200, "the boxes list something"
    assert np.array_equal(la, lb) and ra.tobytes() == rb.tobytes(), "a quaternion and the matrix of the same rotation give the same lists"
    # exact by construction: the cube rotations whose quaternion is exact in binary32 - the identity, the three half turns (one
    # component +-1) and the eight third turns (four components +-1/2). Their integer matrices convert to exactly those quaternions,
    # up to sign, and list what the unnormalised {0, +-1} quaternion lists, byte for byte, on a scene of small integers.
    import obox_cases as oc
    dy = oc.dyadic_scene()
    exact = [(qi, oc.matrix64(qi)) for qi, _ in oc.cube_rotations() if sum(abs(v) for v in qi) in (1, 4)]
    assert len(exact) == 12
    qs = np.array([qi for qi, _ in exact], np.float64)
    Rs = np.rint(np.array([m for _, m in exact]))
    conv = qb.matrix_to_quat(Rs)
    unit = qs / np.linalg.norm(qs, axis=1, keepdims=True)
    assert all(np.array_equal(c, u) or np.array_equal(c, -u) for c, u in zip(conv, unit)), "the conversion of an exact rotation is exact"
    cen = np.tile(np.array([0.5, -1.0, 0.5], np.float32), (12, 1))
    hlf = np.tile(np.array([3.0, 1.5, 5.0], np.float32), (12, 1))
    want = oc.full(dy.desc, qb.make_oboxes(cen, hlf, quat=qs))
    got = oc.full(dy.desc, qb.make_oboxes(cen, hlf, matrix=Rs))
    assert want[0][-1] > 50 and np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), "the exact rotations"
    for bad in ({}, {"quat": q, "matrix": R}):
        with pytest.raises(ValueError, match="exactly one of quat and matrix"):
            qb.make_oboxes(centre, half, **bad)
