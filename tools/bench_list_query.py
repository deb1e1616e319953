#!/usr/bin/env python3
"""Throughput of crossing lists (mi_list_offsets_device, mi_list_fill_device) beside the queries they extend, on the scenes and ray
batches of tools/bench_sign_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup; primary, bounce and shadow rays
built on each):
  offsets           the count walk + the prefix sum, beside count_crossings on the SAME rays;
  fill              the walk + the sorted insertion and the stores, into a buffer sized from those offsets;
  first_crossings   the fill with offsets 4 i (the first four crossings of every ray, padded), beside the closest-hit query;
  work              box tests and primitive tests per ray from a separate full_stats run;
  lengths           the mean and the maximum list length of the batch.
No target is set: the figures are what DESIGN.md section 22 quotes.

    python3 tools/bench_list_query.py [--size 1024] [--seconds 0.3] [--soup-tris 1048576] [--json out]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]
import ipu_ray_lib_amd as irl  # noqa: E402
from ipu_ray_lib_amd import query_batches as qb  # noqa: E402
import refit_cases as rc  # noqa: E402
from bench_sign_query import timed  # noqa: E402

K = 4


def bench(name, hs, size, seconds, torch, table):
    hs.desc.set_image(size, size)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    prim = qb.primary_rays(hs)
    hits = dev.intersect(prim)
    batches = {"primary": prim, "bounce": qb.bounce_rays(prim, hits, 1, seed=1), "shadow": qb.shadow_rays(prim, hits)}
    for bname, rays in batches.items():
        n = rays.size
        if n == 0:
            continue
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_offk = torch.arange(n + 1, dtype=torch.int64, device="cuda") * K
        r, o, off, offk = d_rays.data_ptr(), d_out.data_ptr(), d_off.data_ptr(), d_offk.data_ptr()
        dev.list_offsets_device(r, off, n, stream)
        lens = (d_off[1:] - d_off[:-1])
        total, longest = int(d_off[-1].item()), int(lens.max().item())
        d_hits = torch.empty((max(total, n * K, 1), 4), dtype=torch.int32, device="cuda")
        h = d_hits.data_ptr()
        launches = {
            "closest hit": lambda s: s.query_device(irl.QUERY_CLOSEST, r, o, n, stream),
            "count_crossings": lambda s: s.count_query_device(r, o, n, stream),
            "offsets": lambda s: s.list_offsets_device(r, off, n, stream),
            "fill": lambda s: s.list_fill_device(r, off, h, total, n, stream),
            f"first_crossings(k = {K})": lambda s: s.list_fill_device(r, offk, h, n * K, n, stream),
        }
        for label, go in launches.items():
            stats.reset_counters()
            go(stats)
            c = stats.counters()
            timed(torch, lambda: go(dev), 0.02)          # warm-up
            rate = n / timed(torch, lambda: go(dev), seconds)
            row = {"scene": name, "batch": bname, "what": label, "n": n, "per_s": rate, "box_tests": c["nodes_visited"] / n,
                   "prim_tests": c["leaf_tests"] / n, "mean_length": total / n, "max_length": longest}
            table.append(row)
            print(f"{name:<15} {bname:<8} n={n:>8}  {label:<24} {rate:.3e} rays/s   box tests {row['box_tests']:8.2f}  "
                  f"primitive tests {row['prim_tests']:7.2f} per ray   list length mean {total / n:.2f} max {longest}", flush=True)
        del d_rays, d_out, d_off, d_offk, d_hits
    torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024, help="the camera image the ray batches are built from is size x size")
    ap.add_argument("--seconds", type=float, default=0.3, help="timed time per launch kind and batch")
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--scenes", nargs="*", default=["box", "test_scene.dae", "soup"])
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    table = []
    for name in a.scenes:
        if name == "soup":
            os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
            t0 = time.perf_counter()
            hs = rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0)
            print(f"(soup of {a.soup_tris} triangles built on the host in {time.perf_counter() - t0:.1f} s)", flush=True)
        else:
            hs = rc.scene(name)
        bench(name, hs, a.size, a.seconds, torch, table)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"size": a.size, "k": K, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
