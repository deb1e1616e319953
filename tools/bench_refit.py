"""Geometry update + BVH refit timing (mi_scene_update_device): the box scene, test_scene.dae and a ~1 M-triangle random soup.
Per scene: the device update's pass times (HIP events, scene option refit_timing), its wall time, the effective bandwidth of the
passes, and for comparison the host refit (mi_refit_compact_bvh) and mi_scene_create from the moved arrays.
Usage: python3 tools/bench_refit.py [--reps 20] [--soup-tris 1048576]"""
import argparse
import ctypes as C
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch  # noqa: E402

import ipu_ray_lib_amd as irl  # noqa: E402
import refit_cases as rc  # noqa: E402


def bytes_moved(hs):
    """HBM bytes the four passes read and write (a lower bound: every record once)."""
    n = hs.desc.num_nodes
    leaves = (n + 1) // 2
    b = leaves * (16 + 4 + 36 + 24 + 48)            # pass 1: prim table, order, three vertices, box, compact node read + write
    b += (n - leaves) * (16 + 4 + 48 + 24 + 48)     # pass 2: table, order, two child boxes, own box, compact node read + write
    b += n * (24 + 16 + 64) + leaves * (36 + 128 + 128)   # pass 4: compact node, table, GNode r/w; leaves: vertices, GLeaf r/w, GLeafRot
    return b


def bench(name, hs, reps):
    dev = irl.IpuScene(hs.desc).set_option("refit_timing", 1)
    frames = []
    for r in range(2):
        v, s, d = rc.jitter(hs, 100 + r, 0.3)
        frames.append((v, s, d))
    tens = [(torch.from_numpy(np.stack([v["x"], v["y"], v["z"]], 1).copy()).cuda(),
             torch.from_numpy(s.view(np.float32).reshape(-1, 4).copy()).cuda() if s.size else None,
             torch.from_numpy(d.view(np.float32).reshape(-1, 7).copy()).cuda() if d.size else None) for v, s, d in frames]
    dev.update_geometry_device(*tens[0][:1], spheres=tens[0][1], discs=tens[0][2])      # first update: builds the tables
    passes, walls = [], []
    lib = irl.device_lib()
    lib.mi_get_refit_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    for i in range(reps):
        tv, ts, td = tens[i % 2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.update_geometry_device(vertices=tv, spheres=ts, discs=td)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = (C.c_double * 3)()
        lib.mi_get_refit_timing(dev._h, ms)
        passes.append(list(ms))
    p = np.median(np.array(passes), 0)
    wall = float(np.median(walls))
    kern = float(p.sum())
    # the alternatives: host refit of the moved arrays, and mi_scene_create from them (+ the refit)
    v, s, d = frames[0]
    m = rc.Moved(hs, verts=v, spheres=s, discs=d)
    t0 = time.perf_counter(); m.refit(); host_refit = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); fresh = irl.IpuScene(m.desc); torch.cuda.synchronize(); create = (time.perf_counter() - t0) * 1e3
    fresh.close(); dev.close()
    gbs = bytes_moved(hs) / (kern * 1e-3) / 1e9
    print(f"{name:16s} nodes {hs.desc.num_nodes:8d} | leaf {p[0]:.3f} ms  interior {p[1]:.3f} ms  write {p[2]:.3f} ms  kernels {kern:.3f} ms"
          f" ({gbs:.0f} GB/s)  update wall {wall:.3f} ms | host refit {host_refit:.1f} ms  create {create:.1f} ms"
          f"  refit+create {host_refit + create:.1f} ms  -> {(host_refit + create) / wall:.0f}x", flush=True)


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
