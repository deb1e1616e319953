#!/usr/bin/env python3
"""Throughput of crossing counts, inside tests and signed distance (mi_count_query_device, mi_point_sign_device) beside the queries
they extend, on the box scene, test_scene.dae and a ~1 M-triangle random soup (bench_rebuild.py's three):
  rays    tools/bench_query.py's batches (primary, bounce, shadow) built on each scene: rays/s of count_crossings beside the
          closest-hit and the any-hit query on the SAME rays;
  points  the bounce rays' origins pushed off their surfaces by up to a hundredth of the root box's diagonal along the rays, and
          as many uniform points of the root box: points/s of inside and signed_distance beside closest_points on the same points;
  work    box tests and primitive tests per query from a separate full_stats run.
The count walk cannot prune, so it is expected to cost more than a closest-hit cast: no target is set, the figures are what
DESIGN.md section 21 quotes.

    python3 tools/bench_sign_query.py [--size 1024] [--seconds 0.3] [--soup-tris 1048576] [--json out]
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


def timed(torch, launch, seconds):
    """Seconds per call, HIP events round a run of back-to-back calls lasting >= `seconds`."""
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= seconds * 1e3:
            return ms * 1e-3 / reps
        reps = max(reps * 2, int(reps * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def bench(name, hs, size, seconds, torch, table):
    hs.desc.set_image(size, size)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    prim = qb.primary_rays(hs)
    hits = dev.intersect(prim)
    bounce = qb.bounce_rays(prim, hits, 1, seed=1)
    batches = {"primary": prim, "bounce": bounce, "shadow": qb.shadow_rays(prim, hits)}

    def row(what, batch, n, launches):
        """launches: {label: (callable on a scene, unit)}; each timed on `dev`, its work counted once on `stats`."""
        for label, go in launches.items():
            stats.reset_counters()
            go(stats)
            c = stats.counters()
            timed(torch, lambda: go(dev), 0.02)          # warm-up
            rate = n / timed(torch, lambda: go(dev), seconds)
            r = {"scene": name, "batch": batch, "what": label, "n": n, "per_s": rate, "box_tests": c["nodes_visited"] / n,
                 "prim_tests": c["leaf_tests"] / n}
            table.append(r)
            print(f"{name:<15} {batch:<8} n={n:>8}  {label:<16} {rate:.3e} {what}/s   box tests {r['box_tests']:8.2f}  "
                  f"primitive tests {r['prim_tests']:7.2f} per query", flush=True)

    for bname, rays in batches.items():
        n = rays.size
        if n == 0:
            continue
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        r, o = d_rays.data_ptr(), d_out.data_ptr()
        row("rays", bname, n, {
            "closest hit": lambda s: s.query_device(irl.QUERY_CLOSEST, r, o, n, stream),
            "any hit": lambda s: s.query_device(irl.QUERY_ANY, r, o, n, stream),
            "count_crossings": lambda s: s.count_query_device(r, o, n, stream),
        })
        del d_rays, d_out
    # points: near the surfaces (where an SDF is sampled) and anywhere in the root box
    nd = hs.nodes[0]
    lo = np.array([nd["min_x"], nd["min_y"], nd["min_z"]], np.float32)
    hi = lo + np.array([nd["dx"], nd["dy"], nd["dz"]], np.uint16).view(np.float16).astype(np.float32)
    rng = np.random.default_rng(2)
    o3 = np.stack([bounce["origin"][c] for c in "xyz"], 1)
    d3 = np.stack([bounce["direction"][c] for c in "xyz"], 1)
    near = (o3 + d3 * (rng.uniform(-1, 1, (len(o3), 1)) * 0.01 * np.linalg.norm(hi - lo))).astype(np.float32)
    sets = {"near": near, "uniform": rng.uniform(lo, hi, (max(len(near), 1 << 16), 3)).astype(np.float32)}
    for pname, pos in sets.items():
        n = len(pos)
        if n == 0:
            continue
        d_pts = torch.from_numpy(qb.make_points(pos).view(np.uint8).copy()).cuda()
        d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        p, o = d_pts.data_ptr(), d_out.data_ptr()
        row("points", pname, n, {
            "closest_points": lambda s: s.point_query_device(irl.POINT_CLOSEST, p, o, n, stream),
            "inside": lambda s: s.point_sign_device(irl.SIGN_INSIDE, p, o, n, None, stream),
            "signed_distance": lambda s: s.point_sign_device(irl.SIGN_DISTANCE, p, o, n, None, stream),
        })
        del d_pts, d_out
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
        Path(a.json).write_text(json.dumps({"size": a.size, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
