#!/usr/bin/env python3
"""Generates tests/golden/ref_live_vectors.npz: what the REFERENCE's own code answered to the inputs of the two tests that
used to call it live (tests/test_oracle_pins.py::test_oracle_against_live_reference_dense and
tests/test_scene_blob.py::test_real_scene_blobs_against_the_live_reference_deserialiser), stored as DATA so that those tests
hold on a checkout without the reference. Needs oracle/_ref/libref_l0.so (`make -C oracle ref REF=<reference checkout>`)
and the built host library. No reference source text is stored.

  dense_sincos_x / _s / _c        20 000 arguments in [-30, 30] (default_rng(7)) and the reference's sincos of each
  dense_diffuse_n / _u / _out     5 000 unit normals and (u1, u2) pairs (the same generator, continued) and the
                                  reference's sample_diffuse of each
  blob_<scene>_sha256             the product writer's blob of the scene (box; assets/test_scene.dae with normals)
  blob_<scene>_walk / _scalars / _used   the reference's Deserialiser<16> walking that blob
"""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import oracle_lib  # noqa: E402

f32 = C.c_float
OUT = Path(__file__).resolve().parent / "ref_live_vectors.npz"


def scenes(irl):
    return {"box": irl.HostScene.builtin("box"),
            "test_scene": irl.HostScene.import_file(ROOT / "assets" / "test_scene.dae", load_normals=True)}


def main():
    import ipu_ray_lib_amd as irl
    r = oracle_lib.ref_lib()
    if r is None or not hasattr(r, "ref_walk_scene_blob"):
        raise SystemExit("oracle/_ref/libref_l0.so missing: run `make -C oracle ref REF=<reference checkout>` first")
    out = {}
    rng = np.random.default_rng(7)
    xs = rng.uniform(-30, 30, 20000).astype(np.float32)
    s = np.zeros_like(xs); c = np.zeros_like(xs)
    for i, x in enumerate(xs):
        a, b = f32(), f32()
        r.ref_sincos(float(x), C.byref(a), C.byref(b))
        s[i], c[i] = a.value, b.value
    out.update(dense_sincos_x=xs, dense_sincos_s=s, dense_sincos_c=c)
    ns = np.zeros((5000, 3), np.float32); us = np.zeros((5000, 2), np.float32); res = np.zeros((5000, 3), np.float32)
    for i in range(5000):
        n = rng.normal(size=3); n /= np.linalg.norm(n); n = n.astype(np.float32)
        u = rng.random(2).astype(np.float32)
        o = (f32 * 3)()
        r.ref_sample_diffuse((f32 * 3)(*[float(x) for x in n]), float(u[0]), float(u[1]), o)
        ns[i], us[i], res[i] = n, u, list(o)
    out.update(dense_diffuse_n=ns, dense_diffuse_u=us, dense_diffuse_out=res)
    for name, sc in scenes(irl).items():
        blob = irl.serialise_scene(sc.desc)
        walk, scal, used = oracle_lib.ref_walk_scene_blob(blob)
        out[f"blob_{name}_sha256"] = np.frombuffer(hashlib.sha256(blob.tobytes()).digest(), np.uint8)
        out[f"blob_{name}_walk"] = np.array(walk, np.int64)
        out[f"blob_{name}_scalars"] = np.array(scal, np.uint32)
        out[f"blob_{name}_used"] = np.array(used, np.int64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
