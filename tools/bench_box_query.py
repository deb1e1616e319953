#!/usr/bin/env python3
"""Throughput of box queries (mi_box_query_device, mi_box_offsets_device, mi_box_fill_device) on the scenes of
tools/bench_near_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup), for cubes centred uniformly in the root
box, at three cell sizes per scene - a tiny one that holds about no primitive, and the two of a geometric sweep whose mean counts
come closest to 8 and 200:
  any / count       MI_BOX_ANY, MI_BOX_COUNT;
  offsets           the count walk + the prefix sum;
  fill              the walk + the heap in the segment + the in-place sort, into a buffer sized from those offsets;
  near_offsets      mi_near_offsets_device on the circumscribed balls of the same cubes, and how many neighbours they list: what a
                    caller without box queries pays, and over-reports, today;
  work              box tests and primitive tests per box from a separate full_stats run;
  voxelize          one 256^3 voxelisation of the scene's root box (IpuScene.voxelize: the cell boxes built with torch + MI_BOX_ANY).
No target is set: the figures are what DESIGN.md section 25 quotes.

    python3 tools/bench_box_query.py [--boxes 262144] [--seconds 0.3] [--soup-tris 1048576] [--grid 256] [--json out]
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

TARGETS = (8.0, 200.0)


def cubes(torch, pos, half):
    return torch.from_numpy(qb.make_boxes(pos - np.float32(half), pos + np.float32(half)).view(np.uint8).copy()).cuda()


def mean_count(torch, dev, pos, half, stream):
    d_bx = cubes(torch, pos, half)
    d_cnt = torch.zeros(len(pos), dtype=torch.int32, device="cuda")
    dev.box_query_device(irl.BOX_COUNT, d_bx.data_ptr(), d_cnt.data_ptr(), len(pos), stream)
    return float(d_cnt.double().mean().item())


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    n0 = hs.nodes[0]
    lo = np.array([n0["min_x"], n0["min_y"], n0["min_z"]], np.float32)
    hi = lo + np.array([n0["dx"], n0["dy"], n0["dz"]], np.uint16).view(np.float16).astype(np.float32)
    diag = float(np.linalg.norm(hi - lo))
    n = a.boxes
    pos = np.random.default_rng(1).uniform(lo, hi, (n, 3)).astype(np.float32)
    # the cell sizes: a sweep of half sizes on a sample of the boxes
    sweep = [diag * 2.0 ** (-k / 2.0) for k in range(6, 28)]
    means = [mean_count(torch, dev, pos[:4096], h, stream) for h in sweep]
    halves = [("~0", diag * 1e-5)] + [(f"~{t:g}", sweep[int(np.argmin([abs(np.log((m + 1e-9) / t)) for m in means]))]) for t in TARGETS]
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    for tag, half in halves:
        d_bx = cubes(torch, pos, half)
        d_balls = torch.from_numpy(qb.make_points(pos, np.float32(half) * np.float32(np.sqrt(3.0))).view(np.uint8).copy()).cuda()
        bx, balls, off, o = d_bx.data_ptr(), d_balls.data_ptr(), d_off.data_ptr(), d_out.data_ptr()
        dev.near_offsets_device(balls, off, n, stream)
        ball_total = int(d_off[-1].item())
        dev.box_offsets_device(bx, off, n, stream)
        total = int(d_off[-1].item())
        longest = int((d_off[1:] - d_off[:-1]).max().item())
        d_hits = torch.empty((max(total, 1), 4), dtype=torch.int32, device="cuda")
        d_boff = d_off.clone()
        launches = {
            "any": lambda s: s.box_query_device(irl.BOX_ANY, bx, o, n, stream),
            "count": lambda s: s.box_query_device(irl.BOX_COUNT, bx, o, n, stream),
            "offsets": lambda s: s.box_offsets_device(bx, off, n, stream),
            "fill": lambda s: s.box_fill_device(bx, d_boff.data_ptr(), d_hits.data_ptr(), total, n, stream),
            "near_offsets (circumscribed balls)": lambda s: s.near_offsets_device(balls, off, n, stream),
        }
        for label, go in launches.items():
            stats.reset_counters()
            go(stats)
            c = stats.counters()
            timed(torch, lambda: go(dev), 0.02)          # warm-up
            rate = n / timed(torch, lambda: go(dev), a.seconds)
            row = {"scene": name, "nodes": int(hs.desc.num_nodes), "cell": tag, "half_of_diagonal": half / diag, "what": label, "n": n,
                   "per_s": rate, "box_tests": c["nodes_visited"] / n, "prim_tests": c["leaf_tests"] / n, "mean_count": total / n,
                   "max_count": longest, "mean_ball_count": ball_total / n}
            table.append(row)
            print(f"{name:<15} cell {tag:<5} (mean {total / n:8.2f}, max {longest:6d}; the ball lists {ball_total / n:8.2f})  {label:<36} "
                  f"{rate:.3e} boxes/s   box tests {row['box_tests']:9.2f}  primitive tests {row['prim_tests']:8.2f} per box", flush=True)
        del d_bx, d_balls, d_hits, d_boff
        torch.cuda.empty_cache()
    if a.grid:
        g = a.grid
        cell = (hi - lo) / np.float32(g)
        dev.voxelize(tuple(float(x) for x in lo), tuple(float(x) for x in cell), (8, 8, 8))          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = dev.voxelize(tuple(float(x) for x in lo), tuple(float(x) for x in cell), (g, g, g))
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        filled = int(grid.sum().item())
        table.append({"scene": name, "what": f"voxelize {g}^3", "seconds": secs, "cells_set": filled})
        print(f"{name:<15} voxelize {g}^3: {secs * 1e3:.1f} ms wall, {filled} cells set", flush=True)
        del grid
        torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 18)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed time per launch kind")
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=256, help="cells per axis of the voxelisation (0: none)")
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
        Path(a.json).write_text(json.dumps({"boxes": a.boxes, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
