"""New contents for a live scene (mi_scene_set_geometry_device) against what a caller had before: the box scene, test_scene.dae
and a ~1 M-triangle random soup (bench_rebuild.py's three). Per scene the call alternates between TWO contents of different size -
the scene itself and a cut of it (the first half of every mesh's triangles) - so that the scene's buffers both grow and are
reused, with the data plane already on the device (torch tensors). Reported: the median wall time of the call towards the large
and towards the small contents, and - in the same run, on the same arrays - the alternative: scene.close() + irl.build_lbvh(desc) +
IpuScene(desc), the host twin of the same tree followed by a create.
Usage: python3 tools/bench_set_geometry.py [--reps 20] [--soup-tris 1048576]"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import ipu_ray_lib_amd as irl  # noqa: E402
import refit_cases as rc  # noqa: E402
import set_geometry_cases as sg  # noqa: E402


def cut(c):
    """c's contents with the second half of every mesh's triangles left out (the arrays stay; the meshes shrink)."""
    out = sg.Contents(c.desc, c.name + " cut", int(c.desc.image_width), int(c.desc.samples_per_pixel))
    out.a["mesh_info"]["numTriangles"] = (out.a["mesh_info"]["numTriangles"] + 1) // 2
    return out


def bench(name, hs, reps):
    import torch
    big = sg.Contents(hs.desc, name)
    small = cut(big)
    tb, ts = big.tensors(), small.tensors()
    dev = irl.IpuScene.from_geometry(small.desc)
    stream = torch.cuda.current_stream().cuda_stream
    dev.set_geometry_device(big.desc, stream=stream, **tb); dev.set_geometry_device(small.desc, stream=stream, **ts)      # warm
    grow, shrink = [], []
    for _ in range(reps):
        for c, t, into in ((big, tb, grow), (small, ts, shrink)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev.set_geometry_device(c.desc, stream=stream, **t)
            into.append((time.perf_counter() - t0) * 1e3)
    # the alternative, on the large contents: destroy, build the same tree on the host, create
    old = []
    for _ in range(max(1, min(reps, 3))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.close()
        nodes, depth = irl.build_lbvh(big.desc)
        d = irl.SceneDesc.from_buffer_copy(big.desc)
        d.bvh_nodes, d.num_nodes, d.max_leaf_depth = nodes.ctypes.data, len(nodes), depth
        dev = irl.IpuScene(d)
        torch.cuda.synchronize()
        old.append((time.perf_counter() - t0) * 1e3)
    dev.close()
    g, s, o = float(np.median(grow)), float(np.median(shrink)), float(np.median(old))
    print(f"{name:16s} primitives {small.num_prims:8d} <-> {big.num_prims:8d} | set_geometry_device to the large {g:.3f} ms  to the small {s:.3f} ms"
          f" | close + build_lbvh + create (large) {o:.1f} ms  -> {o / g:.0f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    a = ap.parse_args()
    bench("box", rc.scene("box"), a.reps)
    bench("test_scene.dae", rc.scene("test_scene.dae"), a.reps)
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup's fixture builds in seconds
    bench("soup", rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0), a.reps)


if __name__ == "__main__":
    main()
