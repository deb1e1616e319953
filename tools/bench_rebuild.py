"""BVH rebuild timing (mi_scene_rebuild): the box scene, test_scene.dae and a ~1 M-triangle random soup (bench_refit.py's three).
Per scene: the rebuild's pass times (HIP events, scene option rebuild_timing) and wall time (medians), the alternative a caller had
before - the host SAH build of the moved arrays + mi_scene_create - and the host twin's time; then the cost side: box tests and
primitive tests per cast of the builder's tree and of the LBVH from the CPU oracle's counters, and ms per frame of one box-scene
render on each tree.
The host SAH build runs with the builder's default settings for the two small scenes; for the soup it runs with MI_BVH_REINSERT=0
(as bench_refit.py builds it: with reinsertion the 1 M-triangle build takes minutes), so the soup's alternative is a lower bound.
Usage: python3 tools/bench_rebuild.py [--reps 20] [--soup-tris 1048576] [--no-gpu]"""
import argparse
import ctypes as C
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import ipu_ray_lib_amd as irl  # noqa: E402
import oracle_lib as ol  # noqa: E402
import refit_cases as rc  # noqa: E402
import rebuild_cases as bc  # noqa: E402

PASSES = ("boxes+keys", "sort", "hierarchy+depths", "level boxes", "preorder", "scatter")


def tests_per_cast(desc, size=160, spp=8):
    d = irl.SceneDesc.from_buffer_copy(desc)
    d.set_image(size, size); d.samples_per_pixel = spp; d.path_trace = 1
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    st = ol.path_trace_pixel_rng(d, rays, 8)
    return st.nodesVisited / st.casts, st.leafTests / st.casts


def frame_ms(desc, reps=5):
    d = irl.SceneDesc.from_buffer_copy(desc)
    d.set_image(720, 720); d.samples_per_pixel = 32; d.path_trace = 1
    sc = irl.IpuScene(d)
    rays = np.zeros(d.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(d), rays.ctypes.data, rays.size)
    times = []
    for _ in range(reps + 1):
        sc.run(rays.copy(), irl.MODE_PATH_TRACE)
        times.append(sc.getTraceTimeSecs() * 1e3)
    sc.close()
    return float(np.median(times[1:]))


def bench(name, hs, reps, gpu, quality):
    v, s, d = rc.jitter(hs, 100, 0.3)
    m = rc.Moved(hs, verts=v, spheres=s, discs=d)
    t0 = time.perf_counter(); built = irl.HostScene.from_arrays(m.desc); sah = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); nodes, depth = irl.build_lbvh(m.desc); twin = (time.perf_counter() - t0) * 1e3
    line = f"{name:16s} nodes {hs.desc.num_nodes:8d} depth {depth:3d} | host SAH build {sah:.1f} ms  twin {twin:.1f} ms"
    if gpu:
        import torch
        dev = irl.IpuScene(hs.desc).set_option("rebuild_timing", 1)
        dev.update_geometry(vertices=v, spheres=s, discs=d)
        dev.rebuild_bvh(0)                                         # the first rebuild builds the tables
        passes, walls = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev.rebuild_bvh(0)
            walls.append((time.perf_counter() - t0) * 1e3)
            passes.append(dev.rebuild_timing())
        p = np.median(np.array(passes), 0)
        wall = float(np.median(walls))
        t0 = time.perf_counter(); fresh = irl.IpuScene(built.desc); torch.cuda.synchronize(); create = (time.perf_counter() - t0) * 1e3
        fresh.close(); dev.close()
        line += (f"  create {create:.1f} ms  SAH+create {sah + create:.1f} ms | rebuild " + "  ".join(f"{k} {x:.3f}" for k, x in zip(PASSES, p)) +
                 f"  passes {p.sum():.3f} ms  wall {wall:.3f} ms  -> {(sah + create) / wall:.0f}x")
    print(line, flush=True)
    if quality:
        reb = rc.Moved(hs, verts=v, spheres=s, discs=d).set_nodes(nodes)
        reb.desc.max_leaf_depth = depth
        a, b = tests_per_cast(built.desc), tests_per_cast(reb.desc)
        q = f"{'':16s} per cast: builder's tree {a[0]:.2f} box tests, {a[1]:.3f} primitive tests | LBVH {b[0]:.2f}, {b[1]:.3f}"
        if gpu and name == "box":
            q += f" | 720x720x32 spp frame: builder's tree {frame_ms(built.desc):.2f} ms, LBVH {frame_ms(reb.desc):.2f} ms"
        print(q, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--no-gpu", action="store_true", help="host times and the oracle's counters only")
    a = ap.parse_args()
    bench("box", rc.scene("box"), a.reps, not a.no_gpu, True)
    bench("test_scene.dae", rc.scene("test_scene.dae"), a.reps, not a.no_gpu, True)
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
    soup = rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0)
    bench("soup", soup, a.reps, not a.no_gpu, False)


if __name__ == "__main__":
    main()
