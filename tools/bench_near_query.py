#!/usr/bin/env python3
"""Throughput of neighbour lists (mi_near_offsets_device, mi_near_fill_device) beside the point query they extend, on the scenes of
tools/bench_list_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup), for points uniform in the root box:
  offsets           the count walk + the prefix sum, at a radius of --radius (default 0.5 %) of the root box's diagonal;
  fill              the walk + the sorted insertion and the stores, into a buffer sized from those offsets;
  lengths           the histogram of the list lengths of that batch (0, 1-3, 4-15, 16-63, 64+), their mean and maximum;
  k_nearest         the fill with offsets K i at radius = +inf for K = 1, 8, 32, beside closest_points on the SAME points;
  work              box tests and primitive evaluations per point from a separate full_stats run.
No target is set: the figures are what DESIGN.md section 23 quotes.

    python3 tools/bench_near_query.py [--points 1048576] [--radius 0.005] [--seconds 0.3] [--soup-tris 1048576] [--json out]
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

KS = (1, 8, 32)
BINS = ((0, 0), (1, 3), (4, 15), (16, 63), (64, None))


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    n0 = hs.nodes[0]
    lo = np.array([n0["min_x"], n0["min_y"], n0["min_z"]], np.float32)
    hi = lo + np.array([n0["dx"], n0["dy"], n0["dz"]], np.uint16).view(np.float16).astype(np.float32)
    diag = float(np.linalg.norm(hi - lo))
    n = a.points
    pos = np.random.default_rng(1).uniform(lo, hi, (n, 3)).astype(np.float32)
    d_ball = torch.from_numpy(qb.make_points(pos, a.radius * diag).view(np.uint8).copy()).cuda()
    d_far = torch.from_numpy(qb.make_points(pos, np.inf).view(np.uint8).copy()).cuda()
    d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ball, far, o, off = d_ball.data_ptr(), d_far.data_ptr(), d_out.data_ptr(), d_off.data_ptr()
    dev.near_offsets_device(ball, off, n, stream)
    lens = d_off[1:] - d_off[:-1]
    total, longest = int(d_off[-1].item()), int(lens.max().item())
    hist = {f"{b0}" if b0 == b1 else (f"{b0}+" if b1 is None else f"{b0}-{b1}"):
            int(((lens >= b0) & (lens <= (b1 if b1 is not None else longest))).sum().item()) / n for b0, b1 in BINS}
    print(f"{name:<15} n={n}  radius {a.radius:g} of the diagonal: list length mean {total / n:.2f} max {longest}, shares "
          + ", ".join(f"{k}: {v:.3f}" for k, v in hist.items()), flush=True)
    d_hits = torch.empty((max(total, n * max(KS), 1), 4), dtype=torch.int32, device="cuda")
    h = d_hits.data_ptr()
    d_offk = {k: torch.arange(n + 1, dtype=torch.int64, device="cuda") * k for k in KS}
    launches = {
        "offsets": lambda s: s.near_offsets_device(ball, off, n, stream),
        "fill": lambda s: s.near_fill_device(ball, off, h, total, n, stream),
        "closest_points (radius inf)": lambda s: s.point_query_device(irl.POINT_CLOSEST, far, o, n, stream),
    }
    for k in KS:
        launches[f"k_nearest(k = {k}, radius inf)"] = lambda s, k=k: s.near_fill_device(far, d_offk[k].data_ptr(), h, n * k, n, stream)
    for label, go in launches.items():
        stats.reset_counters()
        go(stats)
        c = stats.counters()
        timed(torch, lambda: go(dev), 0.02)          # warm-up
        rate = n / timed(torch, lambda: go(dev), a.seconds)
        row = {"scene": name, "nodes": int(hs.desc.num_nodes), "what": label, "n": n, "per_s": rate, "box_tests": c["nodes_visited"] / n,
               "prim_evals": c["leaf_tests"] / n}
        if label in ("offsets", "fill"):
            row.update({"radius_of_diagonal": a.radius, "mean_length": total / n, "max_length": longest, "length_shares": hist})
        table.append(row)
        print(f"{name:<15} nodes {hs.desc.num_nodes:>8}  {label:<34} {rate:.3e} points/s   box tests {row['box_tests']:9.2f}  "
              f"primitive evaluations {row['prim_evals']:8.2f} per point", flush=True)
    del d_ball, d_far, d_out, d_off, d_hits, d_offk
    torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--radius", type=float, default=0.005, help="the radius of the full lists, as a share of the root box's diagonal")
    ap.add_argument("--seconds", type=float, default=0.3, help="timed time per launch kind")
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
        bench(name, hs, a, torch, table)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"points": a.points, "ks": list(KS), "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
