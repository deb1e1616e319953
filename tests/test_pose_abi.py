"""Rigid-pose C ABI without a GPU: mi_pose as a C99 and a C++17 compiler read it from include/mi_raylib.h, the entry points exported
by both device libraries and the host library, the argument rules that are checked before anything touches a scene or a device (a
fake scene handle is never dereferenced), the twin's rules, and make_poses."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb

ROOT = irl.REPO_ROOT

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_scene_host.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(mi_pose), offsetof(mi_pose, quat), offsetof(mi_pose, translation), offsetof(mi_pose, scale));
  return (int)(sizeof(&mi_scene_set_poses) + sizeof(&mi_scene_set_poses_device) + sizeof(&mi_scene_get_poses) + sizeof(&mi_scene_bake_poses) +
               sizeof(&mi_get_pose_timing) + sizeof(&mi_pose_geometry_host)) * 0;
}
"""

ENTRIES = ("mi_scene_set_poses", "mi_scene_set_poses_device", "mi_scene_get_poses", "mi_scene_bake_poses", "mi_get_pose_timing")


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_pose_layout(tmp_path, compiler, std, suffix):
    cc = shutil.which(compiler)
    assert cc is not None, f"no {compiler}"
    src = tmp_path / ("layout" + suffix)
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, std, "-pedantic-errors", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 16, 28]
    p = irl.POSE
    assert p.itemsize == 32 and [p.fields[k][1] for k in ("quat", "translation", "scale")] == [0, 16, 28]


@pytest.mark.parametrize("variants", [False, True])
def test_pose_symbols_exported(variants):
    lib = irl.device_lib(variants)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert hasattr(irl.host_lib(), "mi_pose_geometry_host")
    for name in ("set_poses", "set_poses_device", "poses", "bake_poses", "pose", "pose_timing"):
        assert hasattr(irl.IpuScene, name), name
    assert callable(irl.pose_geometry_host) and callable(qb.make_poses)


@pytest.mark.parametrize("variants", [False, True])
def test_pose_argument_rules_need_no_device(variants):
    lib = irl.device_lib(variants)
    fake = C.create_string_buffer(4096)                  # stands in for a scene: the rules below must never read it
    scene = C.cast(fake, C.c_void_p)
    poses = irl.aligned_bytes(4 * 32)
    p = poses.ctypes.data
    n = C.c_uint32(7)
    out2 = (C.c_double * 2)(3.0, 3.0)

    def words(rc, entry, what):
        assert rc == 1, (entry, what)                   # MI_ERR_INVALID_ARG, not MI_ERR_DEVICE
        err = lib.mi_last_error()
        assert entry in err and what in err, (entry, what, err)

    words(lib.mi_scene_set_poses(None, p, 4), b"mi_scene_set_poses:", b"null scene")
    words(lib.mi_scene_set_poses_device(None, p, 4, None), b"mi_scene_set_poses_device:", b"null scene")
    words(lib.mi_scene_set_poses(None, None, 0), b"mi_scene_set_poses:", b"null scene")
    words(lib.mi_scene_set_poses(scene, None, 4), b"mi_scene_set_poses:", b"null poses")
    words(lib.mi_scene_set_poses_device(scene, None, 4, None), b"mi_scene_set_poses_device:", b"null poses")
    words(lib.mi_scene_get_poses(None, p, 4, C.byref(n)), b"mi_scene_get_poses", b"null argument")
    words(lib.mi_scene_get_poses(scene, p, 4, None), b"mi_scene_get_poses", b"null argument")
    words(lib.mi_scene_bake_poses(None), b"mi_scene_bake_poses", b"null scene")
    words(lib.mi_get_pose_timing(None, out2), b"mi_get_pose_timing", b"null argument")
    words(lib.mi_get_pose_timing(scene, None), b"mi_get_pose_timing", b"null argument")
    assert bytes(fake.raw) == bytes(4096) and not poses.any() and n.value == 7 and list(out2) == [3.0, 3.0]


def test_pose_twin_argument_rules():
    host = irl.host_lib()
    desc = irl.SceneDesc()
    buf = irl.aligned_bytes(256)
    p = buf.ctypes.data
    wild = 0xDEAD0000

    def words(rc, what):
        assert rc == 1
        err = host.mi_host_last_error()
        assert b"mi_pose_geometry_host" in err and what in err, (what, err)

    words(host.mi_pose_geometry_host(None, p, 0, p, p, p, p), b"null scene description")
    words(host.mi_pose_geometry_host(C.byref(desc), None, 1, p, p, p, p), b"null poses")
    words(host.mi_pose_geometry_host(C.byref(desc), p, 1, p, p, p, p), b"num_geometry differs")
    # zero geometries: a no-op that reads no pointer
    assert host.mi_pose_geometry_host(C.byref(desc), wild, 0, wild, wild, wild, wild) == 0
    assert host.mi_pose_geometry_host(C.byref(desc), None, 0, None, None, None, None) == 0
    # a scene of vertices no geometry owns: they are copied, the poses still unread
    v = np.zeros(3, irl.VEC3); v["x"] = (1.0, -0.0, 3.0)
    info = np.zeros(1, irl.MESH_INFO); info[0] = (0, 0, 0, 3)
    desc.mesh_verts, desc.num_verts, desc.mesh_info, desc.num_meshes = v.ctypes.data, 3, info.ctypes.data, 1
    out = np.zeros(3, irl.VEC3)
    assert host.mi_pose_geometry_host(C.byref(desc), wild, 0, out.ctypes.data, None, None, None) == 0
    assert out.tobytes() == v.tobytes()
    words(host.mi_pose_geometry_host(C.byref(desc), wild, 0, None, None, None, None), b"null buffer")
    # an invalid pose and a reference to nothing, by name
    geom = np.zeros(1, irl.GEOM_REF)
    desc.geometry, desc.num_geometry = geom.ctypes.data, 1
    bad = qb.make_poses(1, scale=0.0)
    words(host.mi_pose_geometry_host(C.byref(desc), bad.ctypes.data, 1, out.ctypes.data, None, None, None), b"pose 0 is not valid")
    geom["type"] = 1
    ok = qb.make_poses(1)
    words(host.mi_pose_geometry_host(C.byref(desc), ok.ctypes.data, 1, out.ctypes.data, None, None, None), b"geometry 0 references nothing")


def test_make_poses_takes_a_quaternion_or_its_matrix():
    import pose_cases as po
    import refit_cases as rc
    rng = np.random.default_rng(5)
    n = 40
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    # the matrix of the same rotation: its COLUMNS are the frame's U, V, W of the contract
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    t = rng.uniform(-5, 5, (n, 3))
    s = rng.uniform(0.5, 2.0, n)
    a = qb.make_poses(n, quat=q, translation=t, scale=s)
    b = qb.make_poses(n, matrix=R, translation=t, scale=s)
    assert a.dtype == irl.POSE and b.dtype == irl.POSE and a.size == n
    sign = np.sign((qb.matrix_to_quat(R) * q).sum(1))[:, None].astype(np.float32)
    b["quat"] *= sign                     # (q and -q are one rotation; the same sign gives the same float32 frame)
    assert a.tobytes() == b.tobytes(), "rounded to float32 the two are the same poses"
    # missing parts are the identity's
    ident = qb.make_poses(3)
    assert ident.tobytes() == np.tile(po.pose_row(po.IDENTITY), 3).tobytes()
    assert po.PoseChecker.identity(ident).all() and po.PoseChecker.valid(ident).all()
    only_t = qb.make_poses(2, translation=[[1, 2, 3], [4, 5, 6]])
    assert only_t["quat"].tolist() == [[0, 0, 0, 1]] * 2 and only_t["scale"].tolist() == [1, 1] and only_t["translation"][1].tolist() == [4, 5, 6]
    with pytest.raises(ValueError, match="at most one of quat and matrix"):
        qb.make_poses(n, quat=q, matrix=R)
    # and the twin moves a scene alike under both
    hs = rc.scene("soup")
    G = hs.desc.num_geometry
    po.assert_arrays_equal(irl.pose_geometry_host(hs.desc, b[:G].copy()), irl.pose_geometry_host(hs.desc, a[:G].copy()), "matrix and quaternion")
