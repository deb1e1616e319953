"""Rigid-pose timing (mi_scene_set_poses_device) against the ways to say the same thing with mi_scene_update*: the box scene,
test_scene.dae and a ~1 M-triangle random soup. Per scene, medians of wall times:
  a  set_poses_device                                  the feature: 32 bytes per geometry cross the bus
  b  update_geometry_device on arrays already there    the floor: the feature contains it
  c  torch poses the vertices on the device, then b    what a caller does today
  d  update_geometry from host arrays                  the host route: 12 bytes per vertex cross the bus
and the pose pass alone (HIP events, scene option refit_timing: mi_get_pose_timing), a device-to-device copy of the same vertex
array timed in the same run (torch's copy_ of a contiguous tensor is a hipMemcpyAsync), and the bytes sent per frame.
Usage: python3 tools/bench_pose.py [--reps 20] [--soup-tris 1048576]"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch  # noqa: E402

import ipu_ray_lib_amd as irl  # noqa: E402
from ipu_ray_lib_amd import query_batches as qb  # noqa: E402
import pose_cases as po  # noqa: E402
import refit_cases as rc  # noqa: E402


def small_poses(G, seed):
    """A few degrees about a random axis, a small shift, scale within 1 %: the frame-to-frame motion of rigid bodies."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(G, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = np.radians(rng.uniform(1, 5, G)) / 2
    q = np.concatenate([axis * np.sin(half)[:, None], np.cos(half)[:, None]], 1)
    return qb.make_poses(G, quat=q, translation=rng.uniform(-0.5, 0.5, (G, 3)), scale=rng.uniform(0.99, 1.01, G))


def torch_pose(verts, owner, q, t, s):
    """What a caller writes today: the unit quaternion's matrix, then s R p + t per vertex, in float32 on the device."""
    q = q / q.norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    return (torch.bmm(R[owner], verts.unsqueeze(2)).squeeze(2) * s[owner].unsqueeze(1) + t[owner]).contiguous()


def median_wall(fn, reps):
    walls = []
    for i in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(walls))


def bench(name, hs, reps):
    d = hs.desc
    G, V, S, D = d.num_geometry, (d.num_verts if d.num_meshes else 0), d.num_spheres, d.num_discs
    sets = [small_poses(G, 200 + r) for r in range(2)]
    arrays = [irl.pose_geometry_host(d, p) for p in sets]
    as_t = lambda a, w: torch.from_numpy(a.view(np.float32).reshape(-1, w).copy()).cuda() if a.size else None
    tens = [dict(vertices=as_t(a["vertices"], 3), normals=as_t(a["normals"], 3), spheres=as_t(a["spheres"], 4), discs=as_t(a["discs"], 7)) for a in arrays]
    t_poses = [torch.from_numpy(p.view(np.float32).reshape(-1, 8).copy()).cuda() for p in sets]
    stream = torch.cuda.current_stream().cuda_stream

    # a: the feature
    dev = irl.IpuScene(d).set_option("refit_timing", 1)
    dev.set_poses_device(t_poses[0].data_ptr(), G, stream)      # the first call: tables, snapshot, owners
    passes = []

    def pose(i):
        dev.set_poses_device(t_poses[i % 2].data_ptr(), G, stream)
        passes.append(dev.pose_timing())
    a = median_wall(pose, reps)
    pass_ms, after_ms = np.median(np.array(passes), 0)
    rc.assert_nodes_equal(dev.bvh_nodes(), po.with_arrays(hs, arrays[(reps - 1) % 2]).nodes, f"{name}: the posed scene")
    dev.close()

    # b: the floor; c: torch poses the vertices, then the same update; d: the host route
    dev = irl.IpuScene(d)
    dev.update_geometry_device(**tens[0])
    b = median_wall(lambda i: dev.update_geometry_device(**tens[i % 2]), reps)
    c = float("nan")
    if V:
        rest = as_t(po.arrays_of(d)["vertices"], 3)
        owner = torch.from_numpy(po.PoseChecker(d).derive_owners()["vertices"]).cuda()
        assert int(owner.max()) < G, "every vertex of these scenes has an owner"
        parts = [tuple(torch.from_numpy(np.ascontiguousarray(p[f])).cuda() for f in ("quat", "translation", "scale")) for p in sets]

        def today(i):
            q, t, s = parts[i % 2]
            dev.update_geometry_device(vertices=torch_pose(rest, owner, q, t, s), normals=tens[i % 2]["normals"], spheres=tens[i % 2]["spheres"],
                                       discs=tens[i % 2]["discs"])
        today(0)
        c = median_wall(today, reps)
    host = [po.update_args(x) for x in arrays]
    dd = median_wall(lambda i: dev.update_geometry(**host[i % 2]), max(3, reps // 4))
    dev.close()

    # the copy of the same vertex array, device to device, by events
    copy_ms = float("nan")
    if V:
        src, dst = tens[0]["vertices"], torch.empty_like(tens[0]["vertices"])
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        copy_ms = float(np.median(times))
    sent_d = 12 * V + (12 * d.num_normals) + 16 * S + 28 * D
    print(f"{name:16s} G {G:4d}  vertices {V:8d} | a set_poses_device {a:.3f} ms (pose pass {pass_ms:.3f}, after it {after_ms:.3f})"
          f" | b update_geometry_device {b:.3f} ms | c torch + update {c:.3f} ms | d update_geometry (host) {dd:.3f} ms"
          f" | D2D copy of the vertices {copy_ms:.3f} ms (pose pass / copy {pass_ms / copy_ms:.2f})"
          f" | bytes sent per frame: a {32 * G}, b 0, c {32 * G}, d {sent_d}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    a = ap.parse_args()
    bench("box", rc.scene("box"), a.reps)
    bench("test_scene.dae", rc.scene("test_scene.dae"), a.reps)
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
    t0 = time.perf_counter()
    soup = rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0)
    print(f"(soup of {a.soup_tris} triangles built on the host in {time.perf_counter() - t0:.1f} s)", flush=True)
    bench("soup", soup, a.reps)


if __name__ == "__main__":
    main()
