#!/usr/bin/env python3
"""Throughput of triangle queries (mi_tri_query_device, mi_tri_offsets_device, mi_tri_fill_device) on the scenes of
tools/bench_box_query.py (the box scene, test_scene.dae and a ~1 M-triangle random soup), for query triangles centred uniformly in
the root box, at two sizes per scene (edges of about 1/256 and 1/32 of the root box's diagonal):
  any / count       MI_TRI_ANY, MI_TRI_COUNT;
  offsets           the count walk + the prefix sum;
  fill              the walk + the heap in the segment + the in-place sort, into a buffer sized from those offsets;
each beside the box query of the same kind on the same triangles' bounding boxes - the same walk with a cheaper test at the leaves,
and what a caller without triangle queries runs today before filtering on the host - with the mean contacts per triangle beside
the mean overlaps per box: the filtering the caller no longer does;
  work              box tests and primitive tests per query from a separate full_stats run;
  mesh              monkey_bust.glb against a copy of itself displaced by a tenth of its extent, through IpuScene.mesh_contacts.
No target is set: the figures are what DESIGN.md section 30 quotes.

    python3 tools/bench_tri_query.py [--tris 262144] [--seconds 0.3] [--soup-tris 1048576] [--json out]
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

SIZES = (("1/256", 1.0 / 256.0), ("1/32", 1.0 / 32.0))


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    lo, hi = pc.root_box(hs.nodes)
    diag = float(np.linalg.norm(hi - lo))
    n = a.tris
    rng = np.random.default_rng(1)
    pos = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    shape = rng.uniform(-0.5, 0.5, (n, 3, 3)).astype(np.float32)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    for tag, share in SIZES:
        q = (pos[:, None, :] + np.float32(share * diag) * shape).astype(np.float32)
        d_tq = torch.from_numpy(q).cuda()
        d_bx = torch.from_numpy(qb.make_boxes(q.min(1), q.max(1)).view(np.uint8).copy()).cuda()
        tq, bx, off, o = d_tq.data_ptr(), d_bx.data_ptr(), d_off.data_ptr(), d_out.data_ptr()
        dev.box_offsets_device(bx, off, n, stream)
        d_boff = d_off.clone()
        box_total = int(d_boff[-1].item())
        dev.tri_offsets_device(tq, off, n, stream)
        d_toff = d_off.clone()
        total = int(d_toff[-1].item())
        longest = int((d_toff[1:] - d_toff[:-1]).max().item())
        d_hits = torch.empty((max(box_total, total, 1), 4), dtype=torch.int32, device="cuda")
        launches = {
            "tri any": lambda s: s.tri_query_device(irl.TRI_ANY, tq, o, n, stream),
            "box any": lambda s: s.box_query_device(irl.BOX_ANY, bx, o, n, stream),
            "tri count": lambda s: s.tri_query_device(irl.TRI_COUNT, tq, o, n, stream),
            "box count": lambda s: s.box_query_device(irl.BOX_COUNT, bx, o, n, stream),
            "tri offsets": lambda s: s.tri_offsets_device(tq, off, n, stream),
            "box offsets": lambda s: s.box_offsets_device(bx, off, n, stream),
            "tri fill": lambda s: s.tri_fill_device(tq, d_toff.data_ptr(), d_hits.data_ptr(), total, n, stream),
            "box fill": lambda s: s.box_fill_device(bx, d_boff.data_ptr(), d_hits.data_ptr(), box_total, n, stream),
        }
        for label, go in launches.items():
            stats.reset_counters()
            go(stats)
            c = stats.counters()
            timed(torch, lambda: go(dev), 0.02)          # warm-up
            rate = n / timed(torch, lambda: go(dev), a.seconds)
            row = {"scene": name, "nodes": int(hs.desc.num_nodes), "edge_of_diagonal": tag, "what": label, "n": n, "per_s": rate,
                   "box_tests": c["nodes_visited"] / n, "prim_tests": c["leaf_tests"] / n, "mean_contacts": total / n, "max_contacts": longest,
                   "mean_box_overlaps": box_total / n}
            table.append(row)
            print(f"{name:<15} edge {tag:<6} (contacts {total / n:8.3f} per triangle, max {longest:5d}; its box lists {box_total / n:8.3f})  {label:<12} "
                  f"{rate:.3e} queries/s   box tests {row['box_tests']:9.2f}  primitive tests {row['prim_tests']:8.2f} per query", flush=True)
        del d_tq, d_bx, d_hits, d_boff, d_toff
        torch.cuda.empty_cache()
    dev.close(); stats.close()


def mesh_against_mesh(torch, table):
    hs = rc.scene("monkey_bust.glb")
    hs.desc.set_image(64, 64)
    A, B, Cc, _, _ = pc.primitives(hs)["tri"]
    own = np.stack([A, B, Cc], 1).astype(np.float32)
    extent = own.reshape(-1, 3).max(0) - own.reshape(-1, 3).min(0)
    verts = torch.from_numpy((own.reshape(-1, 3) + np.float32(0.1) * extent).astype(np.float32)).cuda()
    faces = torch.arange(len(verts), dtype=torch.int64, device="cuda").reshape(-1, 3)
    dev = irl.IpuScene(hs.desc)
    dev.mesh_contacts(verts, faces)                  # warm-up: the same call (kernel load, torch's allocator and index kernels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = dev.mesh_contacts(verts, faces)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    hit = dev.collides(verts, faces)
    table.append({"scene": "monkey_bust.glb", "what": "mesh_contacts, a copy displaced by a tenth of its extent", "faces": int(len(faces)),
                  "seconds": secs, "contacts": int(rows.shape[0]), "collides": hit})
    print(f"monkey_bust.glb against a copy displaced by a tenth of its extent: {len(faces)} faces, {rows.shape[0]} contacts in {secs * 1e3:.2f} ms wall "
          f"(offsets, one read-back, fill, unpack); collides = {hit}", flush=True)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1 << 18)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed time per launch kind")
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--scenes", nargs="*", default=["box", "test_scene.dae", "soup"])
    ap.add_argument("--no-mesh", action="store_true")
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
    if not a.no_mesh:
        mesh_against_mesh(torch, table)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"tris": a.tris, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
