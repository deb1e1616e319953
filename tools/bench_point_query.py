#!/usr/bin/env python3
"""Point-query throughput (mi_point_query_device): the box scene, test_scene.dae and a ~1 M-triangle random soup (bench_refit.py's
three), each with three point sets:
  (a) uniform      2^22 points uniform in the root box, radius +inf
  (b) uniform 1 %  the same points at a radius of 1 % of the root box's diagonal
  (c) surface      points 1e-3 off the surface: the first hits of the scene's camera rays moved along the hit normal, radius +inf
Per set and kind (CLOSEST, WITHIN): HIP-event time over >= --seconds of repeated queries, points/s; box tests and primitive
evaluations per point from a separate full_stats run. A record, not a gate.

    python tools/bench_point_query.py [--points 4194304] [--size 1440] [--seconds 0.5] [--soup-tris 1048576] [--json out]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ipu_ray_lib_amd as irl  # noqa: E402
from ipu_ray_lib_amd import query_batches as qb  # noqa: E402
import refit_cases as rc  # noqa: E402


def time_queries(torch, dev, kind, d_pts, d_out, n, seconds):
    """Seconds per query, HIP events round a run of back-to-back queries lasting >= `seconds`."""
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream().cuda_stream
        a.record()
        for _ in range(reps):
            dev.point_query_device(kind, d_pts, d_out, n, stream)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= seconds * 1e3:
            return ms * 1e-3 / reps
        reps = max(reps * 2, int(reps * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def bench(name, hs, args, torch, table):
    hs.desc.set_image(args.size, args.size)
    dev = irl.IpuScene(hs.desc)
    stats_dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    n0 = hs.nodes[0]
    lo = np.array([n0["min_x"], n0["min_y"], n0["min_z"]], np.float32)
    hi = lo + np.array([n0["dx"], n0["dy"], n0["dz"]], np.uint16).view(np.float16).astype(np.float32)
    diag = float(np.linalg.norm(hi - lo))
    pos = np.random.default_rng(1).uniform(lo, hi, (args.points, 3)).astype(np.float32)
    rays = qb.primary_rays(hs)
    _, p, nrm = qb.hit_points(rays, dev.intersect(rays))
    sets = {"uniform": qb.make_points(pos, np.inf), "uniform 1 %": qb.make_points(pos, 0.01 * diag),
            "surface": qb.make_points((p + nrm * np.float32(1e-3)).astype(np.float32), np.inf)}
    for sname, pts in sets.items():
        n = pts.size
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        for kind, kname in ((irl.POINT_CLOSEST, "closest"), (irl.POINT_WITHIN, "within")):
            stats_dev.reset_counters()
            stats_dev.point_query_device(kind, d_pts.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
            c = stats_dev.counters()
            found = int(d_out[:n].count_nonzero()) if kind == irl.POINT_WITHIN else None
            time_queries(torch, dev, kind, d_pts.data_ptr(), d_out.data_ptr(), n, 0.05)      # warm-up
            rate = n / time_queries(torch, dev, kind, d_pts.data_ptr(), d_out.data_ptr(), n, args.seconds)
            row = {"scene": name, "nodes": int(hs.desc.num_nodes), "set": sname, "kind": kname, "points": n, "points_per_s": rate,
                   "box_tests_per_point": c["nodes_visited"] / n, "prim_evals_per_point": c["leaf_tests"] / n}
            if found is not None:
                row["within_fraction"] = found / n
            table.append(row)
            print(f"{name:<15} nodes {hs.desc.num_nodes:>8}  {sname:<12} {kname:<8} n={n:>8}  {rate:.3e} points/s  box tests/point "
                  f"{row['box_tests_per_point']:8.2f}  primitive evaluations/point {row['prim_evals_per_point']:7.2f}"
                  + (f"  within {found / n:.3f}" if found is not None else ""), flush=True)
        del d_pts, d_out
        torch.cuda.empty_cache()
    dev.close(); stats_dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--size", type=int, default=1440, help="the camera's image size for the surface set")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed query time per set and kind")
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    table = []
    bench("box", rc.scene("box"), args, torch, table)
    bench("test_scene.dae", rc.scene("test_scene.dae"), args, torch, table)
    os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
    bench("soup", rc.soup(7, False, n_tris=args.soup_tris, n_meshes=max(1, args.soup_tris // 16384), spread=200.0), args, torch, table)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps({"rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
