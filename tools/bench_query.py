#!/usr/bin/env python3
"""Ray-query throughput (mi_query_device) of the two query kernels - query_kernel 0 (one thread per ray) and 1 (K4) - on BASELINE
config 2's scene (box, 1440^2) with three batches built on the host (ipu_ray_lib_amd/query_batches.py, no oracle):
  (a) primary   the camera rays, closest hit
  (b) bounce    cosine-distributed diffuse bounce rays from their first hits, closest hit
  (c) shadow    any-hit rays from those hits to the reference's light (18, 257, -1060)
Per batch and kernel: HIP-event time over >= --seconds of repeated queries, the two kernels alternating round by round, rays/s
(= casts/s: one cast per ray) with the spread over rounds; nodes visited and primitive tests per ray from a separate full_stats
run; and the fraction of the node-gather roof that tools/gather_probe.py measures (L1 path, tree-shaped walk, 64 active lanes,
8 workgroups per CU: K4's occupancy), as casts/s x (nodes + 1.5 x leaf tests) per ray / the probe's lane-gathers per second.

    python tools/bench_query.py [--size 1440] [--seconds 0.5] [--rounds 5] [--tune leafAt,dbl,maxExtra,burst,keep8 ...] [--json out]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import ipu_ray_lib_amd as irl  # noqa: E402
from ipu_ray_lib_amd import query_batches as qb  # noqa: E402


def time_queries(torch, dev, kind, d_rays, d_out, n, seconds):
    """Seconds per query, HIP events round a run of back-to-back queries lasting >= `seconds`."""
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream().cuda_stream
        a.record()
        for _ in range(reps):
            dev.query_device(kind, d_rays, d_out, n, stream)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= seconds * 1e3:
            return ms * 1e-3 / reps
        reps = max(reps * 2, int(reps * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1440)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed query time per kernel, batch and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tune", nargs="*", default=[], help="extra K4 weight sets to time beside the default (query_tune)")
    ap.add_argument("--no-roof", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch

    hs = irl.HostScene.builtin("box")
    hs.desc.set_image(args.size, args.size)
    dev = irl.IpuScene(hs.desc)
    prim = qb.primary_rays(hs)
    hits = dev.intersect(prim)
    batches = {"primary": (irl.QUERY_CLOSEST, prim), "bounce": (irl.QUERY_CLOSEST, qb.bounce_rays(prim, hits, 1, seed=1)),
               "shadow": (irl.QUERY_ANY, qb.shadow_rays(prim, hits))}
    stats_dev = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    roof = None
    if not args.no_roof:
        import gather_probe
        lib = gather_probe.build()
        nodes = gather_probe.device_nodes(hs)
        _, roof = gather_probe.measure(lib, nodes, 0, 1, 64, 8)
        print(f"node-gather roof (gather_probe: L1, tree-shaped, 64 lanes, 8 wg/CU): {roof:.3e} lane-gathers/s", flush=True)
    configs = [("0", {"query_kernel": 0}), ("1", {"query_kernel": 1})] + [(f"1 tune={t}", {"query_kernel": 1, "query_tune": t}) for t in args.tune]
    table = []
    for bname, (kind, rays) in batches.items():
        n = rays.size
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        stats_dev.reset_counters()
        stats_dev.query_device(kind, d_rays.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        c = stats_dev.counters()
        V, T = c["nodes_visited"] / n, c["leaf_tests"] / n
        per = {name: [] for name, _ in configs}
        for name, opts in configs:            # warm-up
            for k, v in opts.items():
                dev.set_option(k, v)
            time_queries(torch, dev, kind, d_rays.data_ptr(), d_out.data_ptr(), n, 0.05)
        for _ in range(args.rounds):
            for name, opts in configs:
                for k, v in opts.items():
                    dev.set_option(k, v)
                per[name].append(n / time_queries(torch, dev, kind, d_rays.data_ptr(), d_out.data_ptr(), n, args.seconds / args.rounds))
        for name, rates in per.items():
            r = np.array(rates)
            row = {"batch": bname, "kind": "any" if kind == irl.QUERY_ANY else "closest", "rays": n, "query_kernel": name,
                   "rays_per_s": float(np.median(r)), "casts_per_s": float(np.median(r)), "spread": [float(r.min()), float(r.max())],
                   "nodes_per_ray": V, "leaf_tests_per_ray": T}
            if roof:
                row["gather_roof_frac"] = float(np.median(r)) * (V + 1.5 * T) / roof
            table.append(row)
            print(f"{bname:<8} {row['kind']:<8} n={n:>8}  query_kernel {name:<24} {row['rays_per_s']:.3e} rays/s (= casts/s)  "
                  f"spread {r.min():.3e} .. {r.max():.3e}  nodes/ray {V:6.2f}  leaf tests/ray {T:5.2f}"
                  + (f"  gather-roof frac {row['gather_roof_frac']:.3f}" if roof else ""), flush=True)
        del d_rays, d_out
        torch.cuda.empty_cache()
    dev.reset_counters()
    dev.close(); stats_dev.close()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps({"scene": "box", "size": args.size, "roof_lane_gathers_per_s": roof, "rows": table,
                                               "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
