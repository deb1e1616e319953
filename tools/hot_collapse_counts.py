"""Box tests per cast of the collapsed walk (csrc/hot_order.hpp) against the full tree's, counted on the host: no GPU.

python tools/hot_collapse_counts.py [--rays N]

Rays: the scene's camera rays (a regular sub-sample) and two generations of cosine-distributed bounce rays from their hit points, hits
from the CPU oracle's closest-hit walk - the casts a path tracer makes inside the scene. The host walk tests boxes only, so each cast
is counted twice: with the segment [0, inf) (no primitive has shortened the ray: an upper bound) and with [0, t] of the hit the oracle
finds (the ray as short as it ever gets: a lower bound). A real cast lies between the two. Per theta it prints the nodes deleted, the
interior nodes only the containment rule keeps, and the box tests per cast of both trees; every pair of walks must reach the same
leaves in the same order."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ipu_ray_lib_amd as irl                      # noqa: E402
from ipu_ray_lib_amd import query_batches as qb    # noqa: E402
import oracle_lib                                  # noqa: E402

LEAF = np.uint32(0x80000000)


def closest_hits(scene, rays):
    o = oracle_lib.lib()
    buf = (oracle_lib.Ray * rays.size).from_buffer(rays.copy())
    hits = np.zeros(rays.size, irl.QUERY_HIT)
    hits["primID"] = qb.INVALID_PRIM
    for i in range(rays.size):
        h = o.o_bvh_intersect(C.byref(scene.desc), C.byref(buf[i]), None)
        if h.hit:
            hits["primID"][i], hits["t"][i] = h.primID, h.t
            hits["normal"]["x"][i], hits["normal"]["y"][i], hits["normal"]["z"][i] = h.normal.x, h.normal.y, h.normal.z
    return hits


def casts_of(scene, n):
    prim = qb.primary_rays(scene)
    prim = np.ascontiguousarray(prim[:: max(1, prim.size // n)][:n])
    rays, hits = [prim], [closest_hits(scene, prim)]
    for gen in range(2):
        nxt = np.ascontiguousarray(qb.bounce_rays(rays[-1], hits[-1], 1, seed=gen + 1))
        if not nxt.size:
            break
        rays.append(nxt); hits.append(closest_hits(scene, nxt))
    return np.concatenate(rays), np.concatenate(hits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1500, help="camera rays per scene (each gives up to two bounce rays)")
    args = ap.parse_args()
    scenes = [("box", irl.HostScene.builtin("box")),
              ("test_scene.dae", irl.HostScene.import_file(ROOT / "assets" / "test_scene.dae", True)),
              ("monkey", irl.HostScene.builtin("monkey"))]
    for name, scene in scenes:
        nodes = np.array(scene.nodes)
        rays, hits = casts_of(scene, args.rays)
        org = np.stack([rays["origin"][c] for c in "xyz"], 1)
        drc = np.stack([rays["direction"][c] for c in "xyz"], 1)
        tfar = np.where(hits["primID"] != qb.INVALID_PRIM, hits["t"], np.float32(np.inf)).astype(np.float32)
        print(f"== {name}: {nodes.size} nodes, {rays.size} casts ({int((hits['primID'] != qb.INVALID_PRIM).sum())} hit)")
        for theta in (0.5, 0.6, 0.75):
            c = irl.hot_collapse(nodes, theta)
            full = np.zeros(2, np.int64); thin = np.zeros(2, np.int64)
            for o, d, t in zip(org, drc, tfar):
                for k, far in enumerate((np.inf, t)):
                    a, na = irl.hot_walk_count(c["preorder"], o, d, None, far)
                    b, nb = irl.hot_walk_count(c["collapsed"], o, d, None, far)
                    la, lb = a[(a & LEAF) != 0] & ~LEAF, c["from"][b[(b & LEAF) != 0] & ~LEAF]
                    assert np.array_equal(la, lb), (name, theta, o, d, far)
                    full[k] += na; thin[k] += nb
            n = rays.size
            print(f"theta {theta:4.2f}: {nodes.size - c['hot'].size:5d} deleted, {c['blocked']:5d} kept by containment alone | box tests per cast, "
                  f"[0, inf): {full[0] / n:6.2f} -> {thin[0] / n:6.2f} ({100 * (thin[0] / full[0] - 1):+5.1f} %) | "
                  f"[0, t_hit]: {full[1] / n:6.2f} -> {thin[1] / n:6.2f} ({100 * (thin[1] / full[1] - 1):+5.1f} %)", flush=True)


if __name__ == "__main__":
    main()
