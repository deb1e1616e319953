#!/usr/bin/env python3
"""Throughput of oriented-box queries (mi_obox_query_device, mi_obox_offsets_device, mi_obox_fill_device) on the scenes of
tools/bench_box_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup): oriented boxes with centres uniform in the
root box and orientations uniform, at that tool's three cell sizes (a tiny one, and the two whose cubes hold about 8 and about 200
primitives), each in the aspects 1:1:1 (half extents h, h, h) and 1:1:8 (h, h, 8 h):
  any / count       MI_OBOX_ANY, MI_OBOX_COUNT;
  offsets           the count walk + the prefix sum;
  fill              the walk + the heap in the segment + the in-place sort, into a buffer sized from those offsets;
each beside the box query of the same kind on the same boxes' WORLD BOUNDS - what a caller without oriented-box queries runs today
before filtering on the host - with the mean counts on both sides: how much shorter the lists are;
  work              box tests and primitive tests per query on both sides from a separate full_stats run: what the three slabs per
                    node save in visits, to set against what they cost in rate.
No target is set: the figures are what DESIGN.md section 34 quotes.

    python3 tools/bench_obox_query.py [--oboxes 262144] [--seconds 0.3] [--soup-tris 1048576] [--json out]
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
import point_cases as pc  # noqa: E402
import refit_cases as rc  # noqa: E402
from bench_sign_query import timed  # noqa: E402
from bench_box_query import TARGETS, mean_count  # noqa: E402

ASPECTS = (("1:1:1", 1.0), ("1:1:8", 8.0))
MAX_RECORDS = 1 << 30      # a fill whose buffer would hold more records than this (16 GiB) is not timed


def world_bounds(centre, half, quat):
    """The axis-aligned bounds of the oriented boxes, as a caller computes them today: |R| half about the centre (float64, rounded
    outwards by one float32 step so that they hold the box whatever the rounding)."""
    q = quat.astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    ext = np.einsum("nij,nj->ni", np.abs(R), half.astype(np.float64))
    lo = np.nextafter((centre - ext).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter((centre + ext).astype(np.float32), np.float32(np.inf))
    return lo, hi


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    lo, hi = pc.root_box(hs.nodes)
    diag = float(np.linalg.norm(hi - lo))
    n = a.oboxes
    rng = np.random.default_rng(1)
    pos = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    quat = rng.normal(size=(n, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    # the cell sizes of bench_box_query.py: a sweep of half sizes on a sample of axis-aligned cubes
    sweep = [diag * 2.0 ** (-k / 2.0) for k in range(6, 28)]
    means = [mean_count(torch, dev, pos[:4096], h, stream) for h in sweep]
    halves = [("~0", diag * 1e-5)] + [(f"~{t:g}", sweep[int(np.argmin([abs(np.log((m + 1e-9) / t)) for m in means]))]) for t in TARGETS]
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    for tag, h in halves:
        for aspect, stretch in ASPECTS:
            half = np.tile(np.array([h, h, h * stretch], np.float32), (n, 1))
            d_ob = torch.from_numpy(qb.make_oboxes(pos, half, quat=quat).view(np.uint8).copy()).cuda()
            d_bx = torch.from_numpy(qb.make_boxes(*world_bounds(pos, half, quat)).view(np.uint8).copy()).cuda()
            ob, bx, off, o = d_ob.data_ptr(), d_bx.data_ptr(), d_off.data_ptr(), d_out.data_ptr()
            dev.box_offsets_device(bx, off, n, stream)
            d_boff = d_off.clone()
            box_total = int(d_boff[-1].item())
            dev.obox_offsets_device(ob, off, n, stream)
            d_ooff = d_off.clone()
            total = int(d_ooff[-1].item())
            longest = int((d_ooff[1:] - d_ooff[:-1]).max().item())
            fills = box_total <= MAX_RECORDS
            d_hits = torch.empty((max(box_total if fills else total, total, 1), 4), dtype=torch.int32, device="cuda")
            launches = {
                "obox any": lambda s: s.obox_query_device(irl.OBOX_ANY, ob, o, n, stream),
                "box any": lambda s: s.box_query_device(irl.BOX_ANY, bx, o, n, stream),
                "obox count": lambda s: s.obox_query_device(irl.OBOX_COUNT, ob, o, n, stream),
                "box count": lambda s: s.box_query_device(irl.BOX_COUNT, bx, o, n, stream),
                "obox offsets": lambda s: s.obox_offsets_device(ob, off, n, stream),
                "box offsets": lambda s: s.box_offsets_device(bx, off, n, stream),
                "obox fill": lambda s: s.obox_fill_device(ob, d_ooff.data_ptr(), d_hits.data_ptr(), total, n, stream),
            }
            if fills:
                launches["box fill"] = lambda s: s.box_fill_device(bx, d_boff.data_ptr(), d_hits.data_ptr(), box_total, n, stream)
            for label, go in launches.items():
                stats.reset_counters()
                go(stats)
                c = stats.counters()
                timed(torch, lambda: go(dev), 0.02)          # warm-up
                rate = n / timed(torch, lambda: go(dev), a.seconds)
                row = {"scene": name, "nodes": int(hs.desc.num_nodes), "cell": tag, "half_of_diagonal": h / diag, "aspect": aspect, "what": label,
                       "n": n, "per_s": rate, "box_tests": c["nodes_visited"] / n, "prim_tests": c["leaf_tests"] / n, "mean_count": total / n,
                       "max_count": longest, "mean_bounds_count": box_total / n}
                table.append(row)
                print(f"{name:<15} cell {tag:<5} {aspect} (mean {total / n:9.3f}, max {longest:6d}; its world bounds list {box_total / n:10.3f})  {label:<13} "
                      f"{rate:.3e} queries/s   box tests {row['box_tests']:9.2f}  primitive tests {row['prim_tests']:9.2f} per query", flush=True)
            del d_ob, d_bx, d_hits, d_boff, d_ooff
            torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oboxes", type=int, default=1 << 18)
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
        if a.json:      # (after every scene: a run cut short keeps what it measured)
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps({"oboxes": a.oboxes, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
