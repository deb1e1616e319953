"""The live loop's timing (refit every frame, rebuild when the tree has degraded): the box scene, test_scene.dae and a ~1 M-triangle
random soup (bench_refit.py's three). Medians, in bench_rebuild.py's style.
Per scene: the wall time of mi_scene_bvh_cost; the wall time of the first update after a rebuild against a steady-state update -
the step that used to read every node back and derive the refit's tables on one host thread. Then a 60-frame throw of the soup
(every mesh drifting away from the others a little more each frame) with option auto_rebuild off and on: per-frame update wall
time, closest-hit query rate on a fixed ray batch, and the frames that rebuilt.
The update timing needs nothing this tool's library added, so the same file runs against an older build of the package
(--package-root): entries that build lacks are reported as absent, not faked.
Usage: python3 tools/bench_animate.py [--reps 20] [--soup-tris 1048576] [--frames 60] [--ratio 2.0] [--package-root DIR]"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def bench(name, hs, reps, irl, rc, torch):
    sync = torch.cuda.synchronize
    v, s, d = rc.jitter(hs, 100, 0.3)
    w, _, _ = rc.jitter(hs, 101, 0.3)
    dev = irl.IpuScene(hs.desc)
    first_ever = wall(lambda: dev.update_geometry(vertices=v, spheres=s, discs=d), sync)      # builds the tables (host derivation)
    dev.rebuild_bvh(0)
    steady, after = [], []
    for k in range(reps):
        dev.rebuild_bvh(0)
        after.append(wall(lambda: dev.update_geometry(vertices=w if k % 2 else v), sync))      # the first update after a rebuild
        steady.append(wall(lambda: dev.update_geometry(vertices=v if k % 2 else w), sync))     # and one more on the same topology
    line = (f"{name:16s} nodes {hs.desc.num_nodes:8d} | first update ever {first_ever:.3f} ms | update after a rebuild "
            f"{np.median(after):.3f} ms  steady-state update {np.median(steady):.3f} ms")
    if hasattr(dev, "bvh_cost"):
        cost = [wall(lambda: dev.bvh_cost(0), sync) for _ in range(reps + 1)][1:]
        c = dev.bvh_cost(0)
        line += (f" | bvh_cost {np.median(cost):.3f} ms (box tests {c.get('box_tests', 0):.2f}, primitive tests {c.get('prim_tests', 0):.3f}, "
                 f"estimate {c.get('estimate', 0):.1f}) | host derivations {dev.live_stats()['host_derivations']}")
    else:
        line += " | bvh_cost: not in this build"
    print(line, flush=True)
    dev.close()


def drift(hs, rc, frames, reach):
    """Per-mesh unit directions; frame f shifts mesh m by f / frames * reach * direction[m]."""
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(hs.desc.num_meshes, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    first = hs.mesh_info["firstVertex"].astype(np.int64); count = hs.mesh_info["numVertices"].astype(np.int64)
    per_vertex = np.repeat(dirs, count, axis=0).astype(np.float32)
    assert first[0] == 0 and per_vertex.shape[0] == hs.verts.size
    base = np.stack([hs.verts["x"], hs.verts["y"], hs.verts["z"]], 1)
    return lambda f: (base + np.float32(reach * f / frames) * per_vertex).astype(np.float32)


def throw(hs, frames, ratio, irl, rc, torch, n_rays=1 << 20):
    sync = torch.cuda.synchronize
    at = drift(hs, rc, frames, 150.0)
    sys.path.insert(0, str(ROOT / "tests"))
    import test_refit_gpu as tg
    for mode in ("off", "on"):
        dev = irl.IpuScene(hs.desc)
        if mode == "on":
            if not hasattr(dev, "live_stats"):
                print("throw, auto_rebuild on: not in this build", flush=True)
                break
            dev.set_option("auto_rebuild", ratio)
        upd, rate, rebuilt_at, seen = [], [], [], 0
        for f in range(1, frames + 1):
            verts = torch.from_numpy(at(f)).cuda()
            upd.append(wall(lambda: dev.update_geometry_device(vertices=verts), sync))
            if mode == "on":
                n = dev.live_stats()["auto_rebuilds"]
                if n != seen:
                    rebuilt_at.append(f); seen = n
            rays = tg._rays(dev.bvh_nodes(), n_rays, 1) if f == 1 else rays                   # a fixed batch, aimed at the first frame's box
            rate.append(n_rays / wall(lambda: dev.intersect(rays), sync) * 1e-3)
        u = np.array(upd)
        print(f"throw, auto_rebuild {mode:3s}: update median {np.median(u):.3f} ms  max {u.max():.3f} ms | closest-hit (host entry, copies included) "
              f"first frame {rate[0]:.2f} Mrays/s  last frame {rate[-1]:.2f} Mrays/s  median {np.median(rate):.2f} | rebuilt at frames {rebuilt_at}", flush=True)
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--no-throw", action="store_true")
    ap.add_argument("--package-root", default=str(ROOT), help="directory holding the ipu_ray_lib_amd package to measure")
    a = ap.parse_args()
    sys.path[:0] = [a.package_root, str(ROOT / "tests")]
    import torch
    import ipu_ray_lib_amd as irl
    import refit_cases as rc
    print(f"package: {Path(irl.__file__).parent}  ({irl.device_lib().mi_version().decode()})", flush=True)
    bench("box", rc.scene("box"), a.reps, irl, rc, torch)
    bench("test_scene.dae", rc.scene("test_scene.dae"), a.reps, irl, rc, torch)
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
    soup = rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0)
    bench("soup", soup, a.reps, irl, rc, torch)
    if not a.no_throw:
        throw(soup, a.frames, a.ratio, irl, rc, torch)


if __name__ == "__main__":
    main()
