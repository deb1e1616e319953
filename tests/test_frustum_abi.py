"""Frustum-query C ABI without a GPU: mi_frustum as a C99 and a C++17 compiler read it from include/mi_raylib.h, the entry points
exported by both device libraries and the host library, the argument rules - checked before anything touches a scene or a
device (a fake scene handle is never dereferenced) - and make_frusta: planes from a view-projection matrix, from a camera, and tiles."""
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
  mi_frustum f;
  printf("%zu %zu %zu %zu %zu\n", sizeof(mi_frustum), offsetof(mi_frustum, planes), sizeof(f.planes[0]), sizeof(f.planes[0][0]),
         sizeof(f.planes) / sizeof(f.planes[0]));
  printf("%d %d\n", (int)MI_FRUSTUM_ANY, (int)MI_FRUSTUM_COUNT);
  return (int)(sizeof(&mi_frustum_query) + sizeof(&mi_frustum_query_device) + sizeof(&mi_frustum_offsets) + sizeof(&mi_frustum_offsets_device) +
               sizeof(&mi_frustum_fill) + sizeof(&mi_frustum_fill_device) + sizeof(&mi_frustum_query_host) + sizeof(&mi_frustum_offsets_host) +
               sizeof(&mi_frustum_fill_host) + sizeof(&mi_frustum_meets_bounds_host)) * 0;
}
"""

ENTRIES = ("mi_frustum_query", "mi_frustum_query_device", "mi_frustum_offsets", "mi_frustum_offsets_device", "mi_frustum_fill", "mi_frustum_fill_device")
TWINS = ("mi_frustum_query_host", "mi_frustum_offsets_host", "mi_frustum_fill_host")


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_frustum_layout(tmp_path, compiler, std, suffix):
    cc = shutil.which(compiler)
    assert cc is not None, f"no {compiler}"
    src = tmp_path / ("layout" + suffix)
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, std, "-pedantic-errors", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [96, 0, 16, 4, 6, 0, 1]
    b = irl.FRUSTUM
    assert b.itemsize == 96 and b.fields["planes"][1] == 0 and b["planes"].shape == (6, 4)
    assert (irl.FRUSTUM_ANY, irl.FRUSTUM_COUNT) == (0, 1)


@pytest.mark.parametrize("variants", [False, True])
def test_frustum_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in TWINS:
        assert hasattr(irl.host_lib(), name), name
    for name in ("frustum_touches", "count_frustum_overlaps", "list_frustum_overlaps", "first_frustum_overlaps", "frustum_offsets", "frustum_fill",
                 "frustum_query_device", "frustum_offsets_device", "frustum_fill_device", "frustum_any", "frustum_count", "frustum_list", "cull"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.frustum_query_host) and callable(irl.frustum_offsets_host) and callable(irl.frustum_fill_host) and callable(irl.frustum_meets_bounds_host)
    assert hasattr(irl.host_lib(), "mi_frustum_meets_bounds_host")
    from ipu_ray_lib_amd import query_batches as qb
    assert callable(qb.make_frusta) and callable(qb.camera_view_proj) and irl.FRUSTUM.itemsize == 96


@pytest.mark.parametrize("variants", [False, True])
def test_frustum_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    bxs = irl.aligned_bytes(64 * 96)
    outs = irl.aligned_bytes(64 * 4)
    offs = irl.aligned_bytes(65 * 8)
    hits = irl.aligned_bytes(64 * 16)
    b, u, o, h = bxs.ctypes.data, outs.ctypes.data, offs.ctypes.data, hits.ctypes.data
    big = 0xFFBFFFFF + 1

    def query_entries(sc, kind, bp, up, n, words, what, host=True):
        assert lib.mi_frustum_query_device(sc, kind, bp, up, n, None) == 1, what        # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert b"mi_frustum_query_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_frustum_query(sc, kind, bp, up, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_frustum_query:" in err and words in err, (what, err)

    def offsets_entries(sc, bp, op, n, words, what, host=True):
        assert lib.mi_frustum_offsets_device(sc, bp, op, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_frustum_offsets_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_frustum_offsets(sc, bp, op, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_frustum_offsets:" in err and words in err, (what, err)

    def fill_entries(sc, bp, op, hp, n, words, what, host=True):
        assert lib.mi_frustum_fill_device(sc, bp, op, hp, 64, n, None) == 1, what
        err = lib.mi_last_error()
        assert b"mi_frustum_fill_device" in err and words in err, (what, err)
        if host:
            assert lib.mi_frustum_fill(sc, bp, op, hp, 64, n) == 1, what
            err = lib.mi_last_error()
            assert b"mi_frustum_fill:" in err and words in err, (what, err)

    for kind in (irl.FRUSTUM_ANY, irl.FRUSTUM_COUNT):
        query_entries(None, kind, b, u, 4, b"null scene", "null scene")
        query_entries(scene, kind, None, u, 4, b"null buffer", "null frusta")
        query_entries(scene, kind, b, None, 4, b"null buffer", "null out")
        query_entries(scene, kind, b + 8, u, 4, b"frusta must be 16-byte aligned", "misaligned frusta")
        query_entries(scene, kind, b + 4, u, 4, b"frusta must be 16-byte aligned", "misaligned frusta by 4")
        query_entries(scene, kind, b, u, big, b"more frusta than one launch indexes", "too many frusta", host=False)
    query_entries(scene, 2, b, u, 4, b"unknown frustum kind", "unknown kind")
    query_entries(scene, -1, b, u, 4, b"unknown frustum kind", "unknown kind")
    query_entries(scene, 2, None, None, 0, b"unknown frustum kind", "an unknown kind comes before n == 0")
    query_entries(scene, irl.FRUSTUM_COUNT, b, u + 2, 4, b"counts must be 4-byte aligned", "misaligned counts")
    query_entries(scene, irl.FRUSTUM_COUNT, b, u + 1, 4, b"counts must be 4-byte aligned", "misaligned counts by 1")
    # the bytes of FRUSTUM_ANY lie anywhere: an odd address passes the buffer rules (what is refused here is the scene)
    assert lib.mi_frustum_query_device(None, irl.FRUSTUM_ANY, b, u + 1, 4, None) == 1 and b"null scene" in lib.mi_last_error()

    offsets_entries(None, b, o, 4, b"null scene", "null scene")
    offsets_entries(scene, None, o, 4, b"null buffer", "null frusta")
    offsets_entries(scene, b, None, 4, b"null buffer", "null offsets")
    offsets_entries(scene, b + 8, o, 4, b"frusta must be 16-byte aligned", "misaligned frusta")
    offsets_entries(scene, b, o + 4, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    offsets_entries(scene, b, o + 1, 4, b"offsets must be 8-byte aligned", "misaligned offsets by 1")
    # (the host entries apply the limit per batch, which needs the scene)
    offsets_entries(scene, b, o, big, b"more frusta than one launch indexes", "too many frusta", host=False)

    fill_entries(None, b, o, h, 4, b"null scene", "null scene")
    fill_entries(scene, None, o, h, 4, b"null buffer", "null frusta")
    fill_entries(scene, b, None, h, 4, b"null buffer", "null offsets")
    fill_entries(scene, b, o, None, 4, b"null buffer", "null hits")
    fill_entries(scene, b + 8, o, h, 4, b"frusta must be 16-byte aligned", "misaligned frusta")
    fill_entries(scene, b, o + 4, h, 4, b"offsets must be 8-byte aligned", "misaligned offsets")
    fill_entries(scene, b, o, h + 8, 4, b"hits must be 16-byte aligned", "misaligned hits")
    fill_entries(scene, b, o, h + 4, 4, b"hits must be 16-byte aligned", "misaligned hits by 4")
    fill_entries(scene, b, o, h, big, b"more frusta than one launch indexes", "too many frusta", host=False)

    # n == 0 is a no-op, whatever the buffers
    assert lib.mi_frustum_query_device(scene, irl.FRUSTUM_ANY, None, None, 0, None) == 0
    assert lib.mi_frustum_query(scene, irl.FRUSTUM_COUNT, None, None, 0) == 0
    assert lib.mi_frustum_offsets_device(scene, None, None, 0, None) == 0
    assert lib.mi_frustum_offsets(scene, None, None, 0) == 0
    assert lib.mi_frustum_fill_device(scene, None, None, None, 0, 0, None) == 0
    assert lib.mi_frustum_fill(scene, b + 4, o + 1, h + 2, 7, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    assert not outs.any() and not offs.any() and not hits.any()


def test_frustum_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    assert host.mi_frustum_query_host(None, irl.FRUSTUM_ANY, p, p, 1, None) == 1 and b"mi_frustum_query_host" in host.mi_host_last_error()
    assert host.mi_frustum_query_host(C.byref(desc), 7, p, p, 1, None) == 1 and b"unknown frustum kind" in host.mi_host_last_error()
    assert host.mi_frustum_query_host(C.byref(desc), irl.FRUSTUM_ANY, None, p, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_frustum_offsets_host(None, p, p, 1, None) == 1 and b"mi_frustum_offsets_host" in host.mi_host_last_error()
    assert host.mi_frustum_offsets_host(C.byref(desc), p, None, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_frustum_fill_host(None, p, p, p, 1, 1, None) == 1 and b"mi_frustum_fill_host" in host.mi_host_last_error()
    assert host.mi_frustum_fill_host(C.byref(desc), p, p, None, 1, 1, None) == 1 and b"null buffer" in host.mi_host_last_error()
    assert host.mi_frustum_query_host(C.byref(desc), irl.FRUSTUM_COUNT, None, None, 0, None) == 0


def test_n_zero_with_wild_pointers():
    """n == 0 reads and writes nothing, on the device entries (a scene handle that is never read) and on the twins."""
    wild = 0xDEAD0001                                    # odd, unmapped
    fake = C.create_string_buffer(4096)
    scene = C.cast(fake, C.c_void_p)
    for variants in (False, True):
        lib = irl.device_lib(variants)
        assert lib.mi_frustum_query_device(scene, irl.FRUSTUM_ANY, wild, wild, 0, None) == 0
        assert lib.mi_frustum_query(scene, irl.FRUSTUM_COUNT, wild, wild, 0) == 0
        assert lib.mi_frustum_offsets_device(scene, wild, wild, 0, None) == 0
        assert lib.mi_frustum_offsets(scene, wild, wild, 0) == 0
        assert lib.mi_frustum_fill_device(scene, wild, wild, wild, 5, 0, None) == 0
        assert lib.mi_frustum_fill(scene, wild, wild, wild, 5, 0) == 0
    assert bytes(fake.raw) == bytes(4096)
    host = irl.host_lib()
    desc = irl.SceneDesc()
    assert host.mi_frustum_query_host(C.byref(desc), irl.FRUSTUM_ANY, wild, wild, 0, None) == 0
    assert host.mi_frustum_fill_host(C.byref(desc), wild, wild, wild, 5, 0, None) == 0
    visits = (C.c_uint64 * 2)(7, 7)
    assert host.mi_frustum_query_host(C.byref(desc), irl.FRUSTUM_COUNT, wild, wild, 0, visits) == 0 and list(visits) == [0, 0]


# ------------------------------------------------------------------------------------------------------
# make_frusta
# ------------------------------------------------------------------------------------------------------
def _camera(depth, far=40.0):
    from ipu_ray_lib_amd import query_batches as qb
    return dict(eye=(1.0, 2.0, -3.0), forward=(0.3, -0.2, 1.0), up=(0.1, 1.0, 0.0), fovy=np.radians(50.0), aspect=1.6, near=0.5, far=far), qb


def test_make_frusta_planes_form():
    from ipu_ray_lib_amd import query_batches as qb
    rng = np.random.default_rng(11)
    pl = rng.normal(size=(5, 6, 4))
    fr = qb.make_frusta(planes=pl)
    assert fr.dtype == irl.FRUSTUM and fr.shape == (5,) and fr.strides == (96,) and np.array_equal(fr["planes"], pl.astype(np.float32))
    assert fr.view(np.float32).reshape(5, 24).tobytes() == pl.astype(np.float32).tobytes(), "nx, ny, nz, d plane by plane, as the C header lays it out"
    assert qb.make_frusta(planes=pl[0]).shape == (1,) and qb.make_frusta(planes=np.zeros((0, 6, 4))).shape == (0,)
    buf = irl.aligned_bytes(fr.nbytes).view(irl.FRUSTUM)
    buf[:] = fr
    assert buf.ctypes.data % 16 == 0 and buf.tobytes() == fr.tobytes()
    for bad in (dict(planes=pl[:, :5]), dict(planes=pl, tiles=(2, 2)), dict(), dict(view_proj=np.eye(4), depth="xx"), dict(view_proj=np.eye(3)),
                dict(view_proj=np.eye(4), tiles=(0, 2))):
        with pytest.raises(ValueError, match="make_frusta"):
            qb.make_frusta(**bad)


@pytest.mark.parametrize("depth", ["zo", "no"])
def test_inside_the_planes_is_inside_the_clip_cube(depth):
    """For seeded points, "every plane made from view_proj holds" equals "the projected point lies in the clip cube": -w <= x, y <= w
    and 0 <= z <= w ("zo") or -w <= z <= w ("no"). The planes ARE those six inequalities, row by row, so in binary64 the two agree
    on every point; the float32 planes are the float64 ones rounded once."""
    cam, qb = _camera(depth)
    m = qb.camera_view_proj(depth=depth, **cam)
    fr = qb.make_frusta(view_proj=m, depth=depth)
    want = np.stack([m[3] + m[0], m[3] - m[0], m[3] + m[1], m[3] - m[1], m[2] if depth == "zo" else m[3] + m[2], m[3] - m[2]])
    assert np.array_equal(fr["planes"][0], want.astype(np.float32)), "float64, not normalised, rounded once"
    rng = np.random.default_rng(13)
    pts = np.concatenate([rng.uniform(-30, 30, (4000, 3)), np.array(cam["eye"]) + rng.normal(size=(4000, 3)) * 2.0])
    clip = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ m.T
    x, y, z, w = clip.T
    in_cube = (-w <= x) & (x <= w) & (-w <= y) & (y <= w) & ((0 <= z) if depth == "zo" else (-w <= z)) & (z <= w)
    s = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ want.T
    assert np.array_equal((s >= 0).all(1), in_cube) and 200 < in_cube.sum() < len(pts) - 200
    # a batch of matrices
    both = qb.make_frusta(view_proj=np.stack([m, 2.0 * m]), depth=depth)
    assert both.shape == (2,) and np.array_equal(both["planes"][1], (2.0 * want).astype(np.float32))


def test_the_camera_form_and_its_matrix_list_the_same_bytes():
    import box_cases as bc
    hs = bc.scene("soup")
    for depth in ("zo", "no"):
        cam, qb = _camera(depth, far=4000.0)
        cam["eye"], cam["near"] = (0.0, 0.0, -900.0), 1.0
        a = qb.make_frusta(depth=depth, **cam)
        b = qb.make_frusta(view_proj=qb.camera_view_proj(depth=depth, **cam), depth=depth)
        assert a.tobytes() == b.tobytes()
        la, lb = (irl.frustum_fill_host(hs.desc, f, irl.frustum_offsets_host(hs.desc, f)[0])[0] for f in (a, b))
        assert la.size > 0 and la.tobytes() == lb.tobytes()
        # far = inf: the far plane is absent, and the list is the limit matrix's
        cam["far"] = np.inf
        a = qb.make_frusta(depth=depth, **cam)
        b = qb.make_frusta(view_proj=qb.camera_view_proj(depth=depth, **cam), depth=depth)
        assert not a["planes"][0, 5].any() and np.array_equal(a["planes"][0, :5], b["planes"][0, :5])
        la, lb = (irl.frustum_fill_host(hs.desc, f, irl.frustum_offsets_host(hs.desc, f)[0])[0] for f in (a, b))
        assert la.size > 0 and la.tobytes() == lb.tobytes()


def test_tiles_jointly_list_the_parents_set():
    """tiles=(4, 4): 16 sub-frusta in row-major order whose shared planes are each other's negation bit for bit and whose outer
    planes are the parent's. Every triangle the parent lists is listed by a tile and the reverse: a point of the triangle in the
    parent lies in some tile, and a tile is a subset of the parent. (A sphere or a disc is tested conservatively, plane by plane,
    so a tile may list one that the parent's planes reject; the soup's triangles are what is compared.)"""
    import box_cases as bc
    hs = bc.scene("soup")
    cam, qb = _camera("zo", far=4000.0)
    import point_cases as pc
    lo, hi = (x.astype(np.float64) for x in pc.root_box(hs.nodes))
    size = float((hi - lo).max())
    cam.update(eye=0.5 * (lo + hi) - np.array([0.1, 0.2, 1.5]) * size, forward=(0.05, 0.1, 1.0), near=1e-3 * size, far=10 * size, fovy=np.radians(30.0))
    parent = qb.make_frusta(**cam)
    tiles = qb.make_frusta(tiles=(4, 4), **cam)
    assert tiles.shape == (16,)
    P, T = parent["planes"][0], tiles["planes"].reshape(4, 4, 6, 4)                    # [row, column]
    assert np.array_equal(T[:, 0, 0], np.tile(P[0], (4, 1))) and np.array_equal(T[:, 3, 1], np.tile(P[1], (4, 1))), "the outer columns keep the parent's sides"
    assert np.array_equal(T[0, :, 2], np.tile(P[2], (4, 1))) and np.array_equal(T[3, :, 3], np.tile(P[3], (4, 1))), "the outer rows too"
    assert np.array_equal(T[:, :3, 1], -T[:, 1:, 0]) and np.array_equal(T[:3, :, 3], -T[1:, :, 2]), "neighbours share their plane up to the sign"
    assert np.array_equal(T[..., 4:, :], np.broadcast_to(P[4:], (4, 4, 2, 4)))

    def tris(fr):
        off, _ = irl.frustum_offsets_host(hs.desc, fr)
        recs, _ = irl.frustum_fill_host(hs.desc, fr, off)
        keep = np.array([int(hs.geometry[g]["type"]) == 0 for g in recs["geomID"]], bool)
        return {(int(r["geomID"]), int(r["primID"])) for r in recs[keep]}, np.diff(off)

    whole, _ = tris(parent)
    parts, per_tile = tris(tiles)
    assert parts == whole and 20 < len(whole) < 590 and (per_tile > 0).sum() >= 4 and per_tile.max() < len(whole)
