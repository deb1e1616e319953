#!/usr/bin/env python3
"""Throughput of frustum queries (mi_frustum_query_device, mi_frustum_offsets_device, mi_frustum_fill_device) on the scenes of
tools/bench_box_query.py (the box scene and test_scene.dae; --scenes soup adds the ~1 M-triangle random soup):
  tiles             the scene camera's view volume (the eye and the axis of the scene's own primary rays, its field of view) split
                    into 16 x 16, 64 x 64 and 256 x 256 sub-frusta: what a tiled or clustered light list asks;
  seeded            262 144 cameras with positions uniform in the root box and uniform directions, 60 degrees wide, their far plane at
                    that tool's three cell sizes (a tiny one, and the two whose cubes hold about 8 and about 200 primitives);
each timed as
  any / count       MI_FRUSTUM_ANY, MI_FRUSTUM_COUNT;
  offsets           the count walk + the prefix sum;
  fill              the walk + the heap in the segment + the in-place sort, into a buffer sized from those offsets;
beside what a caller without frustum queries runs today before filtering on the host:
  box ...           mi_box_* on each frustum's WORLD BOUNDS, computed in float64 from its eight corners;
with the mean list lengths of the two, and
  work              box tests and primitive tests per query on both sides from a separate full_stats run: the plane-only node test
                    admits boxes that miss a frustum only past its edges; what that costs shows in the visits.
No target is set: the figures are what DESIGN.md section 37 quotes.

    python3 tools/bench_frustum_query.py [--frusta 262144] [--seconds 0.3] [--scenes box test_scene.dae] [--json out]
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

MAX_RECORDS = 1 << 28      # a fill whose buffer would hold more records than this (4 GiB) is not timed


def tile_bounds(m, tx, ty):
    """The world bounds of the tx ty tiles of the view-projection matrix m ("zo"), in make_frusta's row-major order: each tile's
    eight corners - the clip-space corners brought back through the inverse matrix - in float64, rounded outwards by one float32
    step. What a caller computes today."""
    inv = np.linalg.inv(m)
    col, row = np.tile(np.arange(tx), ty), np.repeat(np.arange(ty), tx)
    lo, hi = np.full((tx * ty, 3), np.inf), np.full((tx * ty, 3), -np.inf)
    for cx in (col, col + 1):
        for cy in (row, row + 1):
            for z in (0.0, 1.0):
                clip = np.stack([-1.0 + 2.0 * cx / tx, -1.0 + 2.0 * cy / ty, np.full(len(col), z), np.ones(len(col))], 1)
                w = clip @ inv.T
                p = w[:, :3] / w[:, 3:4]
                lo, hi = np.minimum(lo, p), np.maximum(hi, p)
    return np.nextafter(lo.astype(np.float32), np.float32(-np.inf)), np.nextafter(hi.astype(np.float32), np.float32(np.inf))


def scene_camera(hs, diag):
    """The view-projection matrix of the scene's own camera: the eye and the mean direction of its primary rays, its field of view,
    the near plane at a thousandth of the root box's diagonal and the far plane beyond it."""
    rays = qb.primary_rays(hs)
    eye, d = qb._vec(rays, "origin")[0].astype(np.float64), qb._vec(rays, "direction").astype(np.float64)
    fwd = d.mean(0)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 * np.linalg.norm(fwd) else np.array([1.0, 0.0, 0.0])
    return qb.camera_view_proj(eye, fwd, up, float(hs.desc.fov_radians), 1.0, 1e-3 * diag, 2.0 * diag, "zo")


def bench(name, hs, a, torch, table):
    hs.desc.set_image(64, 64)
    dev = irl.IpuScene(hs.desc)
    stats = irl.IpuScene(hs.desc).set_option("full_stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    lo, hi = pc.root_box(hs.nodes)
    diag = float(np.linalg.norm(hi - lo))
    sets = []
    cam = scene_camera(hs, diag)
    for t in (16, 64, 256):
        sets.append((f"tiles {t}x{t}", qb.make_frusta(view_proj=cam, tiles=(t, t)), tile_bounds(cam, t, t)))
    n = a.frusta
    rng = np.random.default_rng(1)
    pos = rng.uniform(lo, hi, (n, 3))
    dirs = rng.normal(size=(n, 3))
    ups = rng.normal(size=(n, 3))
    # camera_view_proj for all of them at once: the view matrices, and one projection per cell size (60 degrees, square, "zo")
    fw = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rt = np.cross(fw, ups)
    rt /= np.linalg.norm(rt, axis=1, keepdims=True)
    view = np.zeros((n, 4, 4))
    view[:, 0, :3], view[:, 1, :3], view[:, 2, :3], view[:, 3, 3] = rt, np.cross(rt, fw), fw, 1.0
    view[:, :3, 3] = -np.einsum("nij,nj->ni", view[:, :3, :3], pos)
    t = np.tan(np.radians(30.0))
    proj = lambda nr, fa: np.array([[1 / t, 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, fa / (fa - nr), -fa * nr / (fa - nr)], [0, 0, 1.0, 0]])      # noqa: E731
    sweep = [diag * 2.0 ** (-k / 2.0) for k in range(6, 28)]
    means = [mean_count(torch, dev, pos[:4096].astype(np.float32), h, stream) for h in sweep]
    cells = [("~0", diag * 1e-5)] + [(f"~{t:g}", sweep[int(np.argmin([abs(np.log((m + 1e-9) / t)) for m in means]))]) for t in TARGETS]
    for tag, h in cells:
        mats = proj(0.05 * h, 2.0 * h) @ view
        blo, bhi = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        inv = np.linalg.inv(mats)
        clo, chi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
        for x in (-1.0, 1.0):
            for y in (-1.0, 1.0):
                for z in (0.0, 1.0):
                    w = inv @ np.array([x, y, z, 1.0])
                    p = w[:, :3] / w[:, 3:4]
                    clo, chi = np.minimum(clo, p), np.maximum(chi, p)
        blo[:], bhi[:] = np.nextafter(clo.astype(np.float32), np.float32(-np.inf)), np.nextafter(chi.astype(np.float32), np.float32(np.inf))
        sets.append((f"seeded, far {tag}", qb.make_frusta(view_proj=mats), (blo, bhi)))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    for tag, fr, (blo, bhi) in sets:
        n = fr.size
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
        d_fr, d_bx = up(fr), up(qb.make_boxes(blo, bhi))
        f, bx, off, o = d_fr.data_ptr(), d_bx.data_ptr(), d_off.data_ptr(), d_out.data_ptr()
        dev.box_offsets_device(bx, off, n, stream)
        d_boff = d_off.clone()
        box_total = int(d_boff[-1].item())
        dev.frustum_offsets_device(f, off, n, stream)
        d_foff = d_off.clone()
        total = int(d_foff[-1].item())
        longest = int((d_foff[1:] - d_foff[:-1]).max().item())
        fills, box_fills = total <= MAX_RECORDS, box_total <= MAX_RECORDS
        d_hits = torch.empty((max(total if fills else 1, box_total if box_fills else 1, 1), 4), dtype=torch.int32, device="cuda")
        launches = {
            "frustum any": lambda s: s.frustum_query_device(irl.FRUSTUM_ANY, f, o, n, stream),
            "box any": lambda s: s.box_query_device(irl.BOX_ANY, bx, o, n, stream),
            "frustum count": lambda s: s.frustum_query_device(irl.FRUSTUM_COUNT, f, o, n, stream),
            "box count": lambda s: s.box_query_device(irl.BOX_COUNT, bx, o, n, stream),
            "frustum offsets": lambda s: s.frustum_offsets_device(f, off, n, stream),
            "box offsets": lambda s: s.box_offsets_device(bx, off, n, stream),
        }
        if fills:
            launches["frustum fill"] = lambda s: s.frustum_fill_device(f, d_foff.data_ptr(), d_hits.data_ptr(), total, n, stream)
        if box_fills:
            launches["box fill"] = lambda s: s.box_fill_device(bx, d_boff.data_ptr(), d_hits.data_ptr(), box_total, n, stream)
        for label, go in launches.items():
            stats.reset_counters()
            go(stats)
            c = stats.counters()
            timed(torch, lambda: go(dev), 0.02)          # warm-up
            rate = n / timed(torch, lambda: go(dev), a.seconds)
            row = {"scene": name, "nodes": int(hs.desc.num_nodes), "set": tag, "what": label, "n": n, "per_s": rate,
                   "box_tests": c["nodes_visited"] / n, "prim_tests": c["leaf_tests"] / n, "mean_count": total / n, "max_count": longest,
                   "mean_bounds_count": box_total / n}
            table.append(row)
            print(f"{name:<15} {tag:<18} n {n:7d} (mean {total / n:10.3f}, max {longest:7d}; its world bounds {box_total / n:10.3f})  {label:<16} "
                  f"{rate:.3e} queries/s   box tests {row['box_tests']:9.2f}  primitive tests {row['prim_tests']:9.2f} per query", flush=True)
        del d_fr, d_bx, d_hits, d_boff, d_foff
        torch.cuda.empty_cache()
    dev.close(); stats.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frusta", type=int, default=1 << 18)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed time per launch kind")
    ap.add_argument("--soup-tris", type=int, default=1 << 20)
    ap.add_argument("--scenes", nargs="*", default=["box", "test_scene.dae"])
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    table = []
    for name in a.scenes:
        if name == "soup":
            os.environ["MI_BVH_REINSERT"] = "0"          # the plain sweep tree: the soup builds in seconds
            hs = rc.soup(7, False, n_tris=a.soup_tris, n_meshes=max(1, a.soup_tris // 16384), spread=200.0)
        else:
            hs = rc.scene(name)
        bench(name, hs, a, torch, table)
        if a.json:      # (after every scene: a run cut short keeps what it measured)
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps({"frusta": a.frusta, "rows": table, "when": time.strftime("%Y-%m-%d %H:%M:%S")}, indent=1))


if __name__ == "__main__":
    main()
