#!/usr/bin/env python3
"""Throughput of capsule queries (mi_capsule_query_device, mi_capsule_offsets_device, mi_capsule_fill_device) on the scenes of
tools/bench_box_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup): capsules with centres uniform in the root
box and directions uniform, the radius at that tool's three cell sizes (a tiny one, and the two whose cubes hold about 8 and about
200 primitives), each at length : radius 0:1 (a ball), 4:1 and 16:1:
  any / count       MI_CAPSULE_ANY, MI_CAPSULE_COUNT;
  offsets           the count walk + the prefix sum;
  fill              the walk + the heap in the segment + the in-place sort, into a buffer sized from those offsets;
each beside what a caller without capsule queries runs today before filtering on the host:
  box ...           mi_box_* on the capsule's WORLD BOUNDS;
  obox ...          mi_obox_* on the CIRCUMSCRIBED oriented box - half extents (r, r, |d| / 2 + r) about the midpoint, a quaternion
                    that turns z onto d -
with the mean list lengths of the three: how much shorter the capsule's lists are;
  work              box tests and primitive tests per query on all sides from a separate full_stats run: what the four axes per
                    node save in visits, to set against what they and the longer primitive test cost in rate.
No target is set: the figures are what DESIGN.md section 36 quotes.

    python3 tools/bench_capsule_query.py [--capsules 262144] [--seconds 0.3] [--soup-tris 1048576] [--json out]
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

RATIOS = (("0:1", 0.0), ("4:1", 4.0), ("16:1", 16.0))      # length : radius
MAX_RECORDS = 1 << 30      # a fill whose buffer would hold more records than this (16 GiB) is not timed


def world_bounds(a, b, radius):
    """The axis-aligned bounds of the capsules, as a caller computes them today (rounded outwards by one float32 step)."""
    lo = np.nextafter((np.minimum(a, b) - radius).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter((np.maximum(a, b) + radius).astype(np.float32), np.float32(np.inf))
    return lo, hi


def circumscribed(a, b, radius):
    """The oriented box about each capsule: half extents (r, r, |d| / 2 + r) about the midpoint, and the quaternion of the shortest
    turn of z onto d - (z x u, 1 + z.u) = (-u.y, u.x, 0, 1 + u.z), which need not be unit; a half turn about x where u = -z, and the
    identity for a ball."""
    d = (b - a).astype(np.float64)
    ln = np.linalg.norm(d, axis=1)
    u = np.where(ln[:, None] > 0, d / np.where(ln > 0, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    quat = np.stack([-u[:, 1], u[:, 0], np.zeros(len(u)), 1.0 + u[:, 2]], 1)
    quat[1.0 + u[:, 2] < 1e-6] = (1.0, 0.0, 0.0, 0.0)
    half = np.stack([radius, radius, ln / 2 + radius], 1) * (1 + 2.0 ** -20)      # (a hair outwards: the frame is rounded)
    return qb.make_oboxes(((a.astype(np.float64) + b) / 2).astype(np.float32), half.astype(np.float32), quat=quat.astype(np.float32))


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    lo, hi = pc.root_box(hs.nodes)
    diag = float(np.linalg.norm(hi - lo))
    n = a.capsules
    rng = np.random.default_rng(1)
    pos = rng.uniform(lo, hi, (n, 3))
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    # the cell sizes of bench_box_query.py: a sweep of half sizes on a sample of axis-aligned cubes
    sweep = [diag * 2.0 ** (-k / 2.0) for k in range(6, 28)]
    means = [mean_count(torch, dev, pos[:4096].astype(np.float32), h, stream) for h in sweep]
    radii = [("~0", diag * 1e-5)] + [(f"~{t:g}", sweep[int(np.argmin([abs(np.log((m + 1e-9) / t)) for m in means]))]) for t in TARGETS]
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    for tag, r in radii:
        for ratio, stretch in RATIOS:
            ea, eb = (pos - dirs * (0.5 * stretch * r)).astype(np.float32), (pos + dirs * (0.5 * stretch * r)).astype(np.float32)
            radius = np.full(n, r, np.float32)
            d_cp, d_bx, d_ob = up(qb.make_capsules(ea, eb, radius)), up(qb.make_boxes(*world_bounds(ea, eb, radius[:, None]))), up(circumscribed(ea, eb, radius))
            cp, bx, ob, off, o = d_cp.data_ptr(), d_bx.data_ptr(), d_ob.data_ptr(), d_off.data_ptr(), d_out.data_ptr()
            dev.box_offsets_device(bx, off, n, stream)
            d_boff = d_off.clone()
            box_total = int(d_boff[-1].item())
            dev.obox_offsets_device(ob, off, n, stream)
            d_ooff = d_off.clone()
            obox_total = int(d_ooff[-1].item())
            dev.capsule_offsets_device(cp, off, n, stream)
            d_coff = d_off.clone()
            total = int(d_coff[-1].item())
            longest = int((d_coff[1:] - d_coff[:-1]).max().item())
            fills = box_total <= MAX_RECORDS
            d_hits = torch.empty((max(box_total if fills else obox_total, obox_total, total, 1), 4), dtype=torch.int32, device="cuda")
            launches = {
                "capsule any": lambda s: s.capsule_query_device(irl.CAPSULE_ANY, cp, o, n, stream),
                "obox any": lambda s: s.obox_query_device(irl.OBOX_ANY, ob, o, n, stream),
                "box any": lambda s: s.box_query_device(irl.BOX_ANY, bx, o, n, stream),
                "capsule count": lambda s: s.capsule_query_device(irl.CAPSULE_COUNT, cp, o, n, stream),
                "obox count": lambda s: s.obox_query_device(irl.OBOX_COUNT, ob, o, n, stream),
                "box count": lambda s: s.box_query_device(irl.BOX_COUNT, bx, o, n, stream),
                "capsule offsets": lambda s: s.capsule_offsets_device(cp, off, n, stream),
                "obox offsets": lambda s: s.obox_offsets_device(ob, off, n, stream),
                "box offsets": lambda s: s.box_offsets_device(bx, off, n, stream),
                "capsule fill": lambda s: s.capsule_fill_device(cp, d_coff.data_ptr(), d_hits.data_ptr(), total, n, stream),
                "obox fill": lambda s: s.obox_fill_device(ob, d_ooff.data_ptr(), d_hits.data_ptr(), obox_total, n, stream),
            }
            if fills:
                launches["box fill"] = lambda s: s.box_fill_device(bx, d_boff.data_ptr(), d_hits.data_ptr(), box_total, n, stream)
            for label, go in launches.items():
                stats.reset_counters()
                go(stats)
                c = stats.counters()
                timed(torch, lambda: go(dev), 0.02)          # warm-up
                rate = n / timed(torch, lambda: go(dev), a.seconds)
                row = {"scene": name, "nodes": int(hs.desc.num_nodes), "cell": tag, "radius_of_diagonal": r / diag, "length_to_radius": ratio, "what": label,
                       "n": n, "per_s": rate, "box_tests": c["nodes_visited"] / n, "prim_tests": c["leaf_tests"] / n, "mean_count": total / n,
                       "max_count": longest, "mean_obox_count": obox_total / n, "mean_bounds_count": box_total / n}
                table.append(row)
                print(f"{name:<15} cell {tag:<5} {ratio:<4} (mean {total / n:9.3f}, max {longest:6d}; its box lists {obox_total / n:10.3f}, its world bounds "
                      f"{box_total / n:10.3f})  {label:<15} {rate:.3e} queries/s   box tests {row['box_tests']:9.2f}  primitive tests {row['prim_tests']:9.2f} per query",
                      flush=True)
            del d_cp, d_bx, d_ob, d_hits, d_boff, d_ooff, d_coff
            torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capsules", type=int, default=1 << 18)
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
            Path(a.json).write_text(json.dumps({"capsules": a.capsules, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
