"""ipu_ray_lib_amd — MI355X-native ray/path-trace hot path behind the reference's IpuScene surface.

Python here is plumbing only: ctypes bindings over the two C-ABI shared libraries

* ``libmi_scene_host.so``  (include/mi_scene_host.h) — CPU-side scene construction, BVH build,
  ray-stream initialisation: the callers' side of the hot path;
* ``libmi_raylib.so``      (include/mi_raylib.h)     — the gfx950 HIP kernels (shadow trace,
  path trace, NIF MLP) and nothing else.

There is NO CPU fallback for the device library: :func:`device_lib` raises if it is missing.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import inspect
import os
import sys
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
DEFAULT_MESH = REPO_ROOT / "assets" / "monkey_bust.glb"

# --------------------------------------------------------------------------------------------
# POD layouts (== include/mi_raylib.h == the reference's structs)
# --------------------------------------------------------------------------------------------
VEC3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
RAY = np.dtype([("origin", VEC3), ("tMin", "<f4"), ("direction", VEC3), ("tMax", "<f4")])
HIT = np.dtype([("r", RAY), ("primID", "<u4"), ("normal", VEC3), ("throughput", VEC3),
                ("geomID", "<u2"), ("flags", "<u2")])
TRACE_RESULT = np.dtype([("rgb", VEC3), ("u", "<f4"), ("v", "<f4"), ("h", HIT)])
BVH_NODE = np.dtype([("min_x", "<f4"), ("min_y", "<f4"), ("min_z", "<f4"), ("link", "<u4"),
                     ("dx", "<u2"), ("dy", "<u2"), ("dz", "<u2"), ("geomID", "<u2")])
MATERIAL = np.dtype([("albedo", VEC3), ("ior", "<f4"), ("emission", VEC3), ("type", "<i4"),
                     ("emissive", "u1"), ("pad", "u1", (3,))])
MESH_INFO = np.dtype([("firstIndex", "<u4"), ("firstVertex", "<u4"), ("numTriangles", "<u4"), ("numVertices", "<u4")])
GEOM_REF = np.dtype([("index", "<u2"), ("type", "u1"), ("pad", "u1")])
SPHERE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("radius", "<f4")])
DISC = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("r", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4")])

# mi_query_hit: the result of a closest-hit ray query (IpuScene.intersect / query_device)
QUERY_HIT = np.dtype([("t", "<f4"), ("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("normal", VEC3),
                      ("b1", "<f4"), ("b2", "<f4")])

# mi_point / mi_point_hit: a point query and its closest-primitive result (IpuScene.closest_points / point_query_device)
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("radius", "<f4")])
POINT_HIT = np.dtype([("dist", "<f4"), ("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("point", VEC3),
                      ("b1", "<f4"), ("b2", "<f4")])

# mi_crossing: one record of a crossing list (IpuScene.list_crossings / first_crossings / list_fill_device)
CROSSING = np.dtype([("t", "<f4"), ("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("ray", "<u4")])

# mi_neighbour: one record of a neighbour list (IpuScene.neighbours / k_nearest / near_fill_device)
NEIGHBOUR = np.dtype([("dist2", "<f4"), ("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("point", "<u4")])

# mi_box / mi_overlap: a box query and one record of its list (IpuScene.touches / count_overlaps / list_overlaps / box_fill_device)
BOX = np.dtype([("lo", "<f4", (3,)), ("reserved0", "<u4"), ("hi", "<f4", (3,)), ("reserved1", "<u4")])
OVERLAP = np.dtype([("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("box", "<u4"), ("reserved", "<u4")])

# mi_tri / mi_contact: a triangle query - a float32 [n, 3, 3] array viewed as records - and one record of its list (IpuScene.tri_touches /
# count_contacts / list_contacts / tri_fill_device)
TRI = np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3,)), ("c", "<f4", (3,))])
CONTACT = np.dtype([("primID", "<u4"), ("geomID", "<u2"), ("flags", "<u2"), ("tri", "<u4"), ("reserved", "<u4")])

# mi_obox: an oriented-box query - centre, half extents, a quaternion x, y, z, w that need not be unit; its list holds OVERLAP records
# (IpuScene.obox_touches / count_obox_overlaps / list_obox_overlaps / obox_fill_device)
OBOX = np.dtype([("centre", "<f4", (3,)), ("reserved0", "<u4"), ("half", "<f4", (3,)), ("reserved1", "<u4"), ("quat", "<f4", (4,))])

# mi_capsule: a capsule query - the segment [a, b] and a radius; its list holds OVERLAP records
# (IpuScene.capsule_touches / count_capsule_overlaps / list_capsule_overlaps / capsule_fill_device)
CAPSULE = np.dtype([("a", "<f4", (3,)), ("radius", "<f4"), ("b", "<f4", (3,)), ("reserved", "<u4")])

# mi_pose: the rigid pose of one geometry - a quaternion x, y, z, w that need not be unit, a translation, a uniform scale
# (IpuScene.set_poses / poses / pose; query_batches.make_poses)
POSE = np.dtype([("quat", "<f4", (4,)), ("translation", "<f4", (3,)), ("scale", "<f4")])

# mi_frustum: a frustum query - six planes nx, ny, nz, d, normals inward, a plane of four zeros absent; its list holds OVERLAP records
# (IpuScene.frustum_touches / count_frustum_overlaps / list_frustum_overlaps / frustum_fill_device; query_batches.make_frusta)
FRUSTUM = np.dtype([("planes", "<f4", (6, 4))])

assert CROSSING.itemsize == 16 and NEIGHBOUR.itemsize == 16
assert OBOX.itemsize == 48 and POSE.itemsize == 32 and CAPSULE.itemsize == 32
assert FRUSTUM.itemsize == 96
assert TRI.itemsize == 36 and CONTACT.itemsize == 16
assert BOX.itemsize == 32 and OVERLAP.itemsize == 16
assert TRACE_RESULT.itemsize == 84 and HIT.itemsize == 64 and RAY.itemsize == 32 and QUERY_HIT.itemsize == 32
assert POINT.itemsize == 16 and POINT_HIT.itemsize == 32
assert BVH_NODE.itemsize == 24 and MATERIAL.itemsize == 36 and MESH_INFO.itemsize == 16 and GEOM_REF.itemsize == 4

FLAG_ERROR, FLAG_ESCAPED, FLAG_INSIDE = 1, 2, 4
CROSS_FAR = 8      # MI_CROSS_FAR: a crossing record's flag for a sphere's far root
INVALID_GEOM, INVALID_PRIM = 0xFFFF, 0xFFFFFFFF
MODE_SHADOW_TRACE, MODE_PATH_TRACE = 0, 1
QUERY_CLOSEST, QUERY_ANY = 0, 1
POINT_CLOSEST, POINT_WITHIN = 0, 1
BOX_ANY, BOX_COUNT = 0, 1
TRI_ANY, TRI_COUNT = 0, 1
OBOX_ANY, OBOX_COUNT = 0, 1
CAPSULE_ANY, CAPSULE_COUNT = 0, 1
FRUSTUM_ANY, FRUSTUM_COUNT = 0, 1
OVERLAP_CONTAINED = 16      # MI_OVERLAP_CONTAINED: the primitive's own bounds lie inside the box
SIGN_INSIDE, SIGN_DISTANCE = 0, 1
# the ray direction of an inside test when none is given (mi_point_sign: no zero component, off the diagonals of axis-aligned boxes)
DEFAULT_INSIDE_DIR = (1.0, 0.70710678, 0.57735027)

MI_OK = 0


class SceneDesc(C.Structure):
    """mi_scene_desc (include/mi_raylib.h); the CPU oracle's ``oscene`` has the same layout."""
    _fields_ = [
        ("geometry", C.c_void_p), ("num_geometry", C.c_uint32),
        ("mesh_info", C.c_void_p), ("num_meshes", C.c_uint32),
        ("mesh_tris", C.c_void_p), ("num_tris", C.c_uint32),
        ("mesh_verts", C.c_void_p), ("num_verts", C.c_uint32),
        ("mesh_normals", C.c_void_p), ("num_normals", C.c_uint32),
        ("mat_ids", C.c_void_p), ("num_mat_ids", C.c_uint32),
        ("materials", C.c_void_p), ("num_materials", C.c_uint32),
        ("bvh_nodes", C.c_void_p), ("num_nodes", C.c_uint32),
        ("max_leaf_depth", C.c_uint32),
        ("spheres", C.c_void_p), ("num_spheres", C.c_uint32),
        ("discs", C.c_void_p), ("num_discs", C.c_uint32),
        ("image_width", C.c_float), ("image_height", C.c_float),
        ("fov_radians", C.c_float), ("anti_alias_scale", C.c_float),
        ("max_path_length", C.c_uint32), ("roulette_start_depth", C.c_uint32),
        ("samples_per_pixel", C.c_uint32),
        ("rng_seed", C.c_uint64),
        ("window_w", C.c_int32), ("window_h", C.c_int32), ("window_c", C.c_int32), ("window_r", C.c_int32),
        ("path_trace", C.c_int32),
        ("device", C.c_int32),
    ]

    def set_image(self, width: int, height: int, crop=None):
        """--width/--height/--crop of the reference CLI (trace.cpp:475-479)."""
        self.image_width, self.image_height = float(width), float(height)
        if crop is None:
            crop = (width, height, 0, 0)
        self.window_w, self.window_h, self.window_c, self.window_r = crop
        return self

    @property
    def num_rays(self) -> int:
        return int(self.window_w) * int(self.window_h)


class GeometryUpdate(C.Structure):
    """mi_geometry_update (include/mi_raylib.h): new positions for a live scene's primitives; NULL = keep."""
    _fields_ = [("mesh_verts", C.c_void_p), ("num_verts", C.c_uint32),
                ("mesh_normals", C.c_void_p), ("num_normals", C.c_uint32),
                ("spheres", C.c_void_p), ("num_spheres", C.c_uint32),
                ("discs", C.c_void_p), ("num_discs", C.c_uint32)]


class SceneGeometry(C.Structure):
    """mi_scene_geometry (include/mi_raylib.h): new contents for a live scene. Control plane (geometry, mesh_info, mat_ids,
    materials) in host memory; data plane in host memory for mi_scene_set_geometry, device memory for ..._device."""
    _fields_ = [("geometry", C.c_void_p), ("num_geometry", C.c_uint32),
                ("mesh_info", C.c_void_p), ("num_meshes", C.c_uint32),
                ("mat_ids", C.c_void_p), ("num_mat_ids", C.c_uint32),
                ("materials", C.c_void_p), ("num_materials", C.c_uint32),
                ("mesh_tris", C.c_void_p), ("num_tris", C.c_uint32),
                ("mesh_verts", C.c_void_p), ("num_verts", C.c_uint32),
                ("mesh_normals", C.c_void_p), ("num_normals", C.c_uint32),
                ("spheres", C.c_void_p), ("num_spheres", C.c_uint32),
                ("discs", C.c_void_p), ("num_discs", C.c_uint32)]

    @classmethod
    def from_desc(cls, desc: "SceneDesc") -> "SceneGeometry":
        """The nine arrays of a SceneDesc (its nodes and render parameters are not part of a scene's contents)."""
        g = cls()
        for name, _ in cls._fields_:
            setattr(g, name, getattr(desc, name))
        return g


# a canonical primitive (mi_canonical_prims, include/mi_scene_host.h): kind 0 = triangle (a, b, c = absolute vertex indices), 1 = sphere,
# 2 = disc (a = its index)
CANON_PRIM = np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("kind", "<u4"), ("geomID", "<u4"), ("primID", "<u4"),
                       ("triBase", "<u4"), ("matIndex", "<u4")])
assert CANON_PRIM.itemsize == 32


class NifDesc(C.Structure):
    """mi_nif_desc (include/mi_scene_host.h)."""
    _fields_ = [("num_layers", C.c_uint32), ("kernels", C.POINTER(C.POINTER(C.c_float))),
                ("biases", C.POINTER(C.POINTER(C.c_float))), ("rows", C.POINTER(C.c_uint32)),
                ("cols", C.POINTER(C.c_uint32)), ("relu", C.POINTER(C.c_uint8)),
                ("embedding_dimension", C.c_uint32), ("hidden_size", C.c_uint32), ("max_value", C.c_float),
                ("mean", C.c_float * 3), ("log_tonemap", C.c_int32), ("weights_are_half", C.c_int32),
                ("name", C.c_char_p), ("source", C.c_char_p)]


class RaylibError(RuntimeError):
    pass


_host = None
_device = {}


def _load(path: Path) -> C.CDLL:
    if not path.exists():
        raise RaylibError(f"{path.name} is not built (run `python -c 'import __graft_entry__ as g; g.build()'` at the repo root)")
    return C.CDLL(str(path))


def host_lib() -> C.CDLL:
    """libmi_scene_host.so — CPU-only scene plumbing."""
    global _host
    if _host is None:
        # (MI_SCENE_HOST_LIB: another build of the same library, e.g. the AddressSanitizer / UBSan build of tools/sanitize_host.sh)
        lib = _load(Path(os.environ["MI_SCENE_HOST_LIB"]) if os.environ.get("MI_SCENE_HOST_LIB") else PKG_DIR / "libmi_scene_host.so")
        lib.mi_host_last_error.restype = C.c_char_p
        lib.mi_host_scene_builtin.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        lib.mi_host_scene_import.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.mi_host_scene_from_arrays.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.mi_host_scene_fill_desc.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
        lib.mi_host_scene_destroy.argtypes = [C.c_void_p]
        lib.mi_host_scene_destroy.restype = None
        lib.mi_build_compact_bvh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.mi_refit_compact_bvh.argtypes = [C.POINTER(SceneDesc), C.c_void_p]
        lib.mi_build_lbvh_compact.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.mi_canonical_prims.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.mi_point_query_host.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        lib.mi_near_offsets_host.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        lib.mi_near_fill_host.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
        for fam in _TOUCH_FAMILIES:
            getattr(lib, fam.c("query_host")).argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
            getattr(lib, fam.c("offsets_host")).argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
            getattr(lib, fam.c("fill_host")).argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
            if fam.bounds_twin:
                getattr(lib, fam.c("meets_bounds_host")).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mi_pose_geometry_host.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mi_sphere_crossings_host.argtypes = [C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float]
        lib.mi_sphere_crossings_host.restype = C.c_uint32
        lib.mi_sphere_roots_host.argtypes = [C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float)]
        lib.mi_sphere_roots_host.restype = C.c_uint32
        lib.mi_hot_nodes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mi_hot_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]
        lib.mi_hot_walk.restype = C.c_uint32
        lib.mi_hot_share.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.mi_hot_collapse.argtypes = [C.c_void_p, C.c_uint32, C.c_double] + [C.c_void_p] * 8 + [C.POINTER(C.c_uint32)]
        lib.mi_hot_join.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.mi_hot_cast_is_literal.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_hot_walk_count.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        lib.mi_hot_walk_count.restype = C.c_uint32
        lib.mi_diffuse_frame.argtypes = [C.POINTER(C.c_float)] * 3
        lib.mi_diffuse_frame.restype = None
        lib.mi_leaf_frames.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.mi_bvh_cost_compact.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]
        lib.mi_bvh_cost_compact_block.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        lib.mi_bvh_cost_estimate.argtypes = [C.POINTER(C.c_double)]
        lib.mi_bvh_cost_estimate.restype = C.c_double
        lib.mi_init_ray_stream.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_size_t]
        lib.mi_scale_rgb.argtypes = [C.c_void_p, C.c_size_t, C.c_float]
        lib.mi_scale_rgb.restype = None
        lib.mi_scene_blob_size.argtypes = [C.POINTER(SceneDesc)]
        lib.mi_scene_blob_size.restype = C.c_size_t
        lib.mi_scene_serialise.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.mi_scene_deserialise.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(SceneDesc), C.POINTER(C.c_size_t)]
        lib.mi_blob_padding.argtypes = [C.c_uint32, C.c_size_t, C.c_uint32]
        lib.mi_blob_padding.restype = C.c_uint32
        lib.mi_shard_band_rays.argtypes = [C.c_size_t, C.c_uint32]
        lib.mi_shard_band_rays.restype = C.c_size_t
        lib.mi_shard_count.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32]
        lib.mi_shard_count.restype = C.c_size_t
        lib.mi_shard_stream_index.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
        lib.mi_shard_frame_index.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.mi_host_nif_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.mi_host_nif_describe.argtypes = [C.c_void_p, C.POINTER(NifDesc)]
        lib.mi_host_nif_destroy.argtypes = [C.c_void_p]
        lib.mi_host_nif_destroy.restype = None
        lib.mi_host_nif_last_error.restype = C.c_char_p
        _host = lib
    return _host


def device_lib(variants: bool = False) -> C.CDLL:
    """libmi_raylib.so — the HIP kernels. Raises (never falls back) when it is not built.
    variants=True: libmi_raylib_variants.so, the test build of the same sources with -DMI_RAYLIB_VARIANTS=1, which also
    carries the kernel families that were measured and not made the default (options kernel 2 / 3, spec, waves, tune, pool_*)."""
    global _device
    if variants not in _device:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same SONAME as the
        # system one libmi_raylib.so links to). Importing torch FIRST makes both resolve to the same
        # already-loaded runtime; the other order leaves torch unable to see the GPU afterwards.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # (MI_RAYLIB_LIB: another build of the same library, for A/B timing of two builds on one box)
        if variants:
            # (MI_RAYLIB_VARIANTS_LIB: another build of the variants library, e.g. the timing-only builds of tools/k3r_knockouts.sh)
            lib = _load(Path(os.environ["MI_RAYLIB_VARIANTS_LIB"]) if os.environ.get("MI_RAYLIB_VARIANTS_LIB") else PKG_DIR / "libmi_raylib_variants.so")
        else:
            lib = _load(Path(os.environ["MI_RAYLIB_LIB"]) if os.environ.get("MI_RAYLIB_LIB") else PKG_DIR / "libmi_raylib.so")
        lib.mi_last_error.restype = C.c_char_p
        lib.mi_version.restype = C.c_char_p
        lib.mi_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.mi_scene_create_from_blob.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.mi_scene_destroy.argtypes = [C.c_void_p]
        lib.mi_scene_destroy.restype = None
        lib.mi_render.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.mi_render_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_trace_time_secs.argtypes = [C.c_void_p]
        lib.mi_trace_time_secs.restype = C.c_double
        lib.mi_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_reset_counters.argtypes = [C.c_void_p]
        lib.mi_get_phase_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_scene_set_nif.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_int32]
        lib.mi_scene_set_hdri_rotation.argtypes = [C.c_void_p, C.c_float]
        lib.mi_scene_set_max_nif_batch.argtypes = [C.c_void_p, C.c_size_t]
        lib.mi_scene_set_ray_batch.argtypes = [C.c_void_p, C.c_size_t]
        lib.mi_nif_infer_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_scene_update.argtypes = [C.c_void_p, C.POINTER(GeometryUpdate)]
        lib.mi_scene_update_device.argtypes = [C.c_void_p, C.POINTER(GeometryUpdate), C.c_void_p]
        lib.mi_scene_rebuild.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.mi_scene_set_geometry.argtypes = [C.c_void_p, C.POINTER(SceneGeometry), C.POINTER(C.c_uint32)]
        lib.mi_scene_set_geometry_device.argtypes = [C.c_void_p, C.POINTER(SceneGeometry), C.c_void_p, C.POINTER(C.c_uint32)]
        lib.mi_get_rebuild_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.mi_scene_get_bvh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.mi_scene_bvh_cost.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.mi_get_live_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_query_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_point_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_point_query_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_count_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_count_query_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_list_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_list_offsets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_list_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        lib.mi_list_fill_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        lib.mi_near_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_near_offsets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mi_near_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        lib.mi_near_fill_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        for fam in _TOUCH_FAMILIES:
            getattr(lib, fam.c("query")).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
            getattr(lib, fam.c("query_device")).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, fam.c("offsets")).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            getattr(lib, fam.c("offsets_device")).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, fam.c("fill")).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
            getattr(lib, fam.c("fill_device")).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        lib.mi_scene_set_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.mi_scene_set_poses_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.mi_scene_get_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.mi_scene_bake_poses.argtypes = [C.c_void_p]
        lib.mi_get_pose_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.mi_point_sign.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_size_t]
        lib.mi_point_sign_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_void_p]
        lib.mi_group_create.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.mi_group_destroy.argtypes = [C.c_void_p]
        lib.mi_group_destroy.restype = None
        lib.mi_group_size.argtypes = [C.c_void_p]
        lib.mi_group_size.restype = C.c_uint32
        lib.mi_group_scene.argtypes = [C.c_void_p, C.c_uint32]
        lib.mi_group_scene.restype = C.c_void_p
        lib.mi_group_set_ray_batch.argtypes = [C.c_void_p, C.c_size_t]
        lib.mi_group_render.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.mi_group_trace_time_secs.argtypes = [C.c_void_p]
        lib.mi_group_trace_time_secs.restype = C.c_double
        lib.mi_group_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_group_last_transfer.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_group_last_gather_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.mi_group_devices.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.mi_group_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_group_trace.argtypes = [C.c_void_p, C.c_int]
        lib.mi_group_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mi_group_gathered_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_uint32]
        lib.mi_group_reset_counters.argtypes = [C.c_void_p]
        lib.mi_get_pool_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_get_hot_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_debug_launch_progress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.mi_scene_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        lib.mi_get_nif_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.mi_get_nif_clock.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _device[variants] = lib
    return _device[variants]


def _check_host(status: int):
    if status != MI_OK:
        raise RaylibError(f"host scene call failed ({status}): {host_lib().mi_host_last_error().decode()}")


def _check_dev(status: int):
    if status != MI_OK:
        raise RaylibError(f"mi_raylib call failed ({status}): {device_lib().mi_last_error().decode()}")


class HostScene:
    """Scene arrays + CompactBVH built on the host (buildSceneDescription + buildSceneData,
    reference src/app_utils.cpp:252-371). ``desc`` is the SceneRef analogue handed to renderers."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self.desc = SceneDesc()
        _check_host(host_lib().mi_host_scene_fill_desc(self._h, C.byref(self.desc)))

    @classmethod
    def builtin(cls, name: str = "box", mesh_file: os.PathLike | str | None = None) -> "HostScene":
        mesh = str(mesh_file if mesh_file is not None else DEFAULT_MESH)
        h = C.c_void_p()
        _check_host(host_lib().mi_host_scene_builtin(name.encode(), mesh.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def import_file(cls, path, load_normals: bool = False) -> "HostScene":
        """importScene(): --mesh-file / --load-normals of the reference CLI."""
        h = C.c_void_p()
        _check_host(host_lib().mi_host_scene_import(str(path).encode(), 1 if load_normals else 0, C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, geometry_desc: SceneDesc) -> "HostScene":
        h = C.c_void_p()
        _check_host(host_lib().mi_host_scene_from_arrays(C.byref(geometry_desc), C.byref(h)))
        return cls(h)

    def _view(self, ptr, count, dtype):
        if not ptr or not count:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (count * dtype.itemsize)).from_address(ptr)
        buf._scene = self          # a view keeps its scene alive: `HostScene.builtin(...).nodes` must not read freed memory
        return np.frombuffer(buf, dtype=dtype, count=count)

    @property
    def nodes(self):
        return self._view(self.desc.bvh_nodes, self.desc.num_nodes, BVH_NODE)

    @property
    def verts(self):
        return self._view(self.desc.mesh_verts, self.desc.num_verts, VEC3)

    @property
    def tris(self):
        return self._view(self.desc.mesh_tris, self.desc.num_tris * 3, np.dtype("<u2")).reshape(-1, 3)

    @property
    def mesh_info(self):
        return self._view(self.desc.mesh_info, self.desc.num_meshes, MESH_INFO)

    @property
    def geometry(self):
        return self._view(self.desc.geometry, self.desc.num_geometry, GEOM_REF)

    @property
    def materials(self):
        return self._view(self.desc.materials, self.desc.num_materials, MATERIAL)

    @property
    def mat_ids(self):
        return self._view(self.desc.mat_ids, self.desc.num_mat_ids, np.dtype("<u4"))

    @property
    def spheres(self):
        return self._view(self.desc.spheres, self.desc.num_spheres, SPHERE)

    @property
    def discs(self):
        return self._view(self.desc.discs, self.desc.num_discs, DISC)

    def init_ray_stream(self) -> np.ndarray:
        """initPerspectiveRayStream (no jitter) + zeroRgb for the desc's window."""
        rays = np.zeros(self.desc.num_rays, dtype=TRACE_RESULT)
        _check_host(host_lib().mi_init_ray_stream(C.byref(self.desc), rays.ctypes.data, rays.size))
        return rays

    def close(self):
        if self._h:
            host_lib().mi_host_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def aligned_bytes(n: int, align: int = 16) -> np.ndarray:
    """A writable uint8 array of n bytes whose first byte is `align`-aligned."""
    raw = np.zeros(n + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n]


def _aligned_copy(a: np.ndarray) -> np.ndarray:
    """A C-contiguous copy of `a` at a 16-byte aligned address (the query entries' buffer rule)."""
    out = aligned_bytes(a.size * a.dtype.itemsize).view(a.dtype)
    out[...] = a.reshape(-1)
    return out


def refit_compact_bvh(desc: SceneDesc) -> np.ndarray:
    """mi_refit_compact_bvh: desc's BVH topology with every box recomputed from desc's arrays (a BVH_NODE array). The host reference
    of IpuScene.update_geometry; raises RaylibError where mi_scene_update refuses (a box that is not finite, an extent above 65504)."""
    out = np.zeros(desc.num_nodes, dtype=BVH_NODE)
    _check_host(host_lib().mi_refit_compact_bvh(C.byref(desc), out.ctypes.data))
    return out


def build_lbvh(desc: SceneDesc):
    """mi_build_lbvh_compact: (nodes, max leaf depth) of the LBVH over desc's primitives, from desc's geometry arrays (desc's own
    nodes are ignored). The host twin of IpuScene.rebuild_bvh; raises RaylibError where mi_scene_rebuild refuses."""
    geometry = HostScene._view(None, desc.geometry, desc.num_geometry, GEOM_REF)
    info = HostScene._view(None, desc.mesh_info, desc.num_meshes, MESH_INFO)
    prims = sum(int(info[g["index"]]["numTriangles"]) if g["type"] == 0 and g["index"] < info.size else 1 for g in geometry)
    out = np.zeros(max(2 * prims - 1, 1), dtype=BVH_NODE)
    n, depth = C.c_uint32(), C.c_uint32()
    _check_host(host_lib().mi_build_lbvh_compact(C.byref(desc), out.ctypes.data, C.byref(n), C.byref(depth)))
    return out[:n.value].copy(), depth.value


def canonical_prims(desc: SceneDesc) -> np.ndarray:
    """mi_canonical_prims: desc's primitives in canonical order (geometry 0 .. G - 1, inside a mesh triangle 0 .. T - 1), a
    CANON_PRIM array - the table the LBVH builds sort, from the code the device kernel of IpuScene.set_geometry runs. Raises
    RaylibError, with mi_scene_create's words, where the arrays are not a scene."""
    n = C.c_uint32()
    _check_host(host_lib().mi_canonical_prims(C.byref(desc), None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=CANON_PRIM)
    _check_host(host_lib().mi_canonical_prims(C.byref(desc), out.ctypes.data if n.value else None, n.value, C.byref(n)))
    return out


def _cost_dict(out) -> dict:
    """{sum_all, sum_leaf, a_root} and, where a_root > 0, the figures normalised by it: the expected box tests and primitive tests
    of a random line through the root box, and the estimate the auto-rebuild policy compares (mi_bvh_cost_estimate)."""
    d = {"sum_all": out[0], "sum_leaf": out[1], "a_root": out[2]}
    if out[2] > 0:
        d["box_tests"] = out[0] / out[2]
        d["prim_tests"] = out[1] / out[2]
        d["estimate"] = host_lib().mi_bvh_cost_estimate(out)
    return d


def bvh_cost(nodes: np.ndarray, block: int | None = None) -> dict:
    """mi_bvh_cost_compact: the surface-area cost of a tree of compact nodes (a BVH_NODE array), the host twin of
    IpuScene.bvh_cost - the same three doubles bit for bit. `block`: another block width of the reduction (a power of two)."""
    nodes = np.ascontiguousarray(nodes, dtype=BVH_NODE)
    out = (C.c_double * 3)()
    if block is None:
        _check_host(host_lib().mi_bvh_cost_compact(nodes.ctypes.data, nodes.size, out))
    else:
        _check_host(host_lib().mi_bvh_cost_compact_block(nodes.ctypes.data, nodes.size, block, out))
    return _cost_dict(out)


def point_query_host(desc: SceneDesc, kind: int, points: np.ndarray):
    """mi_point_query_host: the host twin of IpuScene.closest_points / .within on desc's arrays and nodes - the same bytes.
    Returns (out, visits): a POINT_HIT array (POINT_CLOSEST) or a bool array (POINT_WITHIN), and {"box_tests", "prim_evals"}
    summed over the points (what the device counts as nodes visited / leaf tests under option full_stats)."""
    assert points.dtype == POINT and points.ndim == 1
    src = np.ascontiguousarray(points)
    out = np.zeros(src.size, np.uint8) if kind == POINT_WITHIN else np.zeros(src.size, POINT_HIT)
    visits = (C.c_uint64 * 2)()
    _check_host(host_lib().mi_point_query_host(C.byref(desc), int(kind), src.ctypes.data if src.size else None,
                                               out.ctypes.data if src.size else None, src.size, visits))
    return (out.view(np.bool_) if kind == POINT_WITHIN else out), {"box_tests": int(visits[0]), "prim_evals": int(visits[1])}


def near_offsets_host(desc: SceneDesc, points: np.ndarray):
    """mi_near_offsets_host: the host twin of IpuScene.near_offsets on desc's arrays and nodes - the same uint64 offsets. Returns
    (offsets, visits), visits as point_query_host's."""
    assert points.dtype == POINT and points.ndim == 1
    src = np.ascontiguousarray(points)
    offsets = np.zeros(src.size + 1, np.uint64)
    visits = (C.c_uint64 * 2)()
    _check_host(host_lib().mi_near_offsets_host(C.byref(desc), src.ctypes.data if src.size else None, offsets.ctypes.data, src.size, visits))
    return offsets, {"box_tests": int(visits[0]), "prim_evals": int(visits[1])}


def near_fill_host(desc: SceneDesc, points: np.ndarray, offsets: np.ndarray, capacity: int | None = None, hits: np.ndarray | None = None):
    """mi_near_fill_host: the host twin of IpuScene.near_fill - the same bytes. Returns (recs, visits): recs is `hits` (a NEIGHBOUR
    array the fill writes into, e.g. one of sentinels) or a fresh zeroed array as long as the offsets reach (at least `capacity`);
    nothing at or past `capacity` (None: recs.size) is written."""
    assert points.dtype == POINT and points.ndim == 1
    src = np.ascontiguousarray(points)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    assert offsets.ndim == 1 and offsets.size == src.size + 1
    if hits is None:
        size = int(offsets.max()) if capacity is None else int(capacity)
        hits = np.zeros(max(size, 1), NEIGHBOUR)[:size]
    assert hits.dtype == NEIGHBOUR and hits.flags["C_CONTIGUOUS"]
    capacity = hits.size if capacity is None else int(capacity)
    assert 0 <= capacity <= hits.size
    visits = (C.c_uint64 * 2)()
    base = hits.ctypes.data if hits.size else np.zeros(1, NEIGHBOUR).ctypes.data
    _check_host(host_lib().mi_near_fill_host(C.byref(desc), src.ctypes.data if src.size else None, offsets.ctypes.data, base, capacity, src.size, visits))
    return hits, {"box_tests": int(visits[0]), "prim_evals": int(visits[1])}


# --------------------------------------------------------------------------------------------
# The touch families (every primitive that touches a caller-supplied item - the rows below say which items): one row each. From
# the rows come the argtypes of both libraries, the module-level host twins and the nine IpuScene methods of a family - one
# implementation per kind of method, bound under the family's public names, which are not regular, with a docstring from one
# template. The same list on the C side is TouchFamilies of csrc/query_drivers.hpp.
# --------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class _TouchFamily:
    prefix: str           # the C entries are mi_<prefix>_query, mi_<prefix>_offsets_device, ...; <PREFIX> is the item's dtype here
    item: np.dtype
    record: np.dtype      # OVERLAP or CONTACT
    arg: str              # what the Python entries call a batch: boxes, tris, ...
    one: str              # the nouns of messages and docstrings
    noun: str
    any: str              # the public method names
    count: str
    list: str
    first: str
    contained: str = ""   # what a list's docstring says of the records' flags
    bounds_twin: bool = False

    def c(self, entry: str) -> str:
        return f"mi_{self.prefix}_{entry}"

    def words(self) -> dict:
        """What the docstring templates are formatted with."""
        ITEM, REC = self.prefix.upper(), "CONTACT" if self.record is CONTACT else "OVERLAP"
        a = lambda w: ("an " if w[0] in "AEIOU" else "a ") + w      # noqa: E731
        return dict(dataclasses.asdict(self), p=self.prefix, ITEM=ITEM, REC=REC, a_ITEM=a(ITEM), a_REC=a(REC), adj=self.one.replace(" ", "-"))


_INSIDE = ", flags = OVERLAP_CONTAINED where the primitive lies inside the {one} (a triangle: exactly; mi_raylib.h)"
_TOUCH_FAMILIES = (
    _TouchFamily("box", BOX, OVERLAP, "boxes", "box", "boxes", "touches", "count_overlaps", "list_overlaps", "first_overlaps",
                 contained=", flags = OVERLAP_CONTAINED where the primitive's own bounds lie inside the box"),
    _TouchFamily("tri", TRI, CONTACT, "tris", "triangle", "triangles", "tri_touches", "count_contacts", "list_contacts", "first_contacts"),
    _TouchFamily("obox", OBOX, OVERLAP, "oboxes", "oriented box", "oriented boxes", "obox_touches", "count_obox_overlaps", "list_obox_overlaps",
                 "first_obox_overlaps", contained=_INSIDE.format(one="oriented box"), bounds_twin=True),
    _TouchFamily("capsule", CAPSULE, OVERLAP, "capsules", "capsule", "capsules", "capsule_touches", "count_capsule_overlaps", "list_capsule_overlaps",
                 "first_capsule_overlaps", contained=_INSIDE.format(one="capsule"), bounds_twin=True),
    _TouchFamily("frustum", FRUSTUM, OVERLAP, "frusta", "frustum", "frusta", "frustum_touches", "count_frustum_overlaps", "list_frustum_overlaps",
                 "first_frustum_overlaps", contained=_INSIDE.format(one="frustum"), bounds_twin=True),
)
assert all((globals()[f.prefix.upper() + "_ANY"], globals()[f.prefix.upper() + "_COUNT"]) == (0, 1) for f in _TOUCH_FAMILIES), "one kind numbering"
_TOUCH_ANY, _TOUCH_COUNT = 0, 1


def _bound(impl, fam: _TouchFamily, name: str, doc: str, qualname: str = ""):
    """impl(fam, ...) as the public function `name`: impl's signature without `fam` and with its arguments `items`, `d_items` and
    `item` under the family's own names (boxes, d_frusta, capsule), by which a caller may also pass them; `doc` is formatted with
    the family's words."""
    own = {"items": fam.arg, "d_items": "d_" + fam.arg, "item": fam.prefix}
    sig = inspect.signature(impl)
    sig = sig.replace(parameters=[q.replace(name=own.get(q.name, q.name)) for q in list(sig.parameters.values())[1:]])

    def call(*args, **kwargs):
        if kwargs:                                   # (the family's names are the signature's, not impl's)
            bound = sig.bind(*args, **kwargs)
            args, kwargs = bound.args, bound.kwargs
        return impl(fam, *args, **kwargs)

    call.__name__, call.__qualname__, call.__signature__, call.__doc__ = name, qualname + name, sig, doc.format(**fam.words())
    return call


def _visits(visits) -> dict:
    return {"box_tests": int(visits[0]), "prim_evals": int(visits[1])}


def _touch_query_host(fam, desc: SceneDesc, kind: int, items: np.ndarray):
    assert items.dtype == fam.item and items.ndim == 1
    src = np.ascontiguousarray(items)
    out = np.zeros(src.size, np.uint8 if kind == _TOUCH_ANY else np.uint32)
    visits = (C.c_uint64 * 2)()
    _check_host(getattr(host_lib(), fam.c("query_host"))(C.byref(desc), int(kind), src.ctypes.data if src.size else None,
                                                         out.ctypes.data if src.size else None, src.size, visits))
    return (out.view(np.bool_) if kind == _TOUCH_ANY else out), _visits(visits)


def _touch_offsets_host(fam, desc: SceneDesc, items: np.ndarray):
    assert items.dtype == fam.item and items.ndim == 1
    src = np.ascontiguousarray(items)
    offsets = np.zeros(src.size + 1, np.uint64)
    visits = (C.c_uint64 * 2)()
    _check_host(getattr(host_lib(), fam.c("offsets_host"))(C.byref(desc), src.ctypes.data if src.size else None, offsets.ctypes.data, src.size, visits))
    return offsets, _visits(visits)


def _touch_fill_host(fam, desc: SceneDesc, items: np.ndarray, offsets: np.ndarray, capacity: int | None = None, hits: np.ndarray | None = None):
    assert items.dtype == fam.item and items.ndim == 1
    src = np.ascontiguousarray(items)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    assert offsets.ndim == 1 and offsets.size == src.size + 1
    if hits is None:
        size = int(offsets.max()) if capacity is None else int(capacity)
        hits = np.zeros(max(size, 1), fam.record)[:size]
    assert hits.dtype == fam.record and hits.flags["C_CONTIGUOUS"]
    capacity = hits.size if capacity is None else int(capacity)
    assert 0 <= capacity <= hits.size
    visits = (C.c_uint64 * 2)()
    base = hits.ctypes.data if hits.size else np.zeros(1, fam.record).ctypes.data
    _check_host(getattr(host_lib(), fam.c("fill_host"))(C.byref(desc), src.ctypes.data if src.size else None, offsets.ctypes.data, base, capacity, src.size, visits))
    return hits, _visits(visits)


def _touch_meets_bounds_host(fam, item: np.ndarray, mn, mx) -> bool:
    q = np.ascontiguousarray(item, fam.item).reshape(1)
    lo, hi = np.ascontiguousarray(mn, np.float32).reshape(3), np.ascontiguousarray(mx, np.float32).reshape(3)
    return bool(getattr(host_lib(), fam.c("meets_bounds_host"))(q.ctypes.data, lo.ctypes.data, hi.ctypes.data))


_TOUCH_TWINS = (        # suffix of the public name, implementation, docstring
    ("query_host", _touch_query_host,
     """mi_{p}_query_host: the host twin of IpuScene.{any} / .{count} on desc's arrays and nodes - the same bytes. Returns
    (out, visits): a bool array ({ITEM}_ANY) or a uint32 array ({ITEM}_COUNT), and {{"box_tests", "prim_evals"}} summed over the
    {noun} (what the device counts as nodes visited / leaf tests under option full_stats)."""),
    ("offsets_host", _touch_offsets_host,
     """mi_{p}_offsets_host: the host twin of IpuScene.{p}_offsets - the same uint64 offsets. Returns (offsets, visits)."""),
    ("fill_host", _touch_fill_host,
     """mi_{p}_fill_host: the host twin of IpuScene.{p}_fill - the same bytes. Returns (recs, visits): recs is `hits` ({a_REC}
    array the fill writes into, e.g. one of sentinels) or a fresh zeroed array as long as the offsets reach (at least `capacity`);
    nothing at or past `capacity` (None: recs.size) is written."""),
    ("meets_bounds_host", _touch_meets_bounds_host,
     """mi_{p}_meets_bounds_host: {p}_meets_bounds of the {adj} queries on its own - whether the bounds [mn, mx] (three floats
    each) meet the one {ITEM} record `{p}`; False for a query that is not valid."""),
)
for _fam in _TOUCH_FAMILIES:
    for _suffix, _impl, _doc in _TOUCH_TWINS:
        if _impl is not _touch_meets_bounds_host or _fam.bounds_twin:
            globals()[f"{_fam.prefix}_{_suffix}"] = _bound(_impl, _fam, f"{_fam.prefix}_{_suffix}", _doc)


def pose_geometry_host(desc: SceneDesc, poses: np.ndarray) -> dict:
    """mi_pose_geometry_host: the host twin of the pose pass of IpuScene.set_poses - desc's geometry as the rest geometry, one POSE per
    geometry entry. Returns {"vertices": VEC3 [num_verts], "normals": VEC3 [num_normals], "spheres": SPHERE [...], "discs": DISC [...]}:
    the arrays the device hands to its refit, byte for byte."""
    assert poses.dtype == POSE and poses.ndim == 1
    src = np.ascontiguousarray(poses)
    out = {"vertices": np.zeros(desc.num_verts if desc.num_meshes else 0, VEC3), "normals": np.zeros(desc.num_normals, VEC3),
           "spheres": np.zeros(desc.num_spheres, SPHERE), "discs": np.zeros(desc.num_discs, DISC)}
    ptr = [a.ctypes.data if a.size else None for a in out.values()]
    _check_host(host_lib().mi_pose_geometry_host(C.byref(desc), src.ctypes.data if src.size else None, src.size, *ptr))
    return out


DEVICE_NODE = np.dtype([("box", "<f4", (6,)), ("link", "<u4"), ("hit", "<u4")])     # the 32-byte device node: min/max per axis, two byte-offset successors


def hot_nodes(nodes: np.ndarray) -> dict:
    """mi_hot_nodes: for a BVH_NODE array, the device's preorder node array, the hot-first order of the private copy plain renders
    may walk (option hot_nodes; order[k] = preorder index of the node at place k), that copy's node array and the successor each of
    its leaves' records carries - {"preorder", "order", "hot", "leaf_link"}, from the functions the upload runs (csrc/hot_order.hpp)."""
    nodes = np.ascontiguousarray(nodes, dtype=BVH_NODE)
    n = nodes.size
    out = {"preorder": np.zeros(n, DEVICE_NODE), "order": np.zeros(n, np.uint32), "hot": np.zeros(n, DEVICE_NODE), "leaf_link": np.zeros(n, np.uint32)}
    _check_host(host_lib().mi_hot_nodes(nodes.ctypes.data if n else None, n, *[out[k].ctypes.data if n else None for k in ("preorder", "order", "hot", "leaf_link")]))
    out["share"] = np.zeros(n, np.float64)      # share[k - 1]: what the first k places take of a random line's box tests (mi_hot_share)
    _check_host(host_lib().mi_hot_share(out["preorder"].ctypes.data if n else None, n, out["order"].ctypes.data if n else None, out["share"].ctypes.data if n else None))
    return out


def hot_walk(device_nodes: np.ndarray, origin, direction, leaf_link: np.ndarray | None = None) -> np.ndarray:
    """mi_hot_walk: the entries of the stackless, box-tests-only walk of a DEVICE_NODE array for one ray (node indices; bit 31 marks
    the primitive test of a leaf whose box was hit). leaf_link = None: the shared array's protocol, else the private array's."""
    assert device_nodes.dtype == DEVICE_NODE and device_nodes.flags.c_contiguous
    o, d = ((C.c_float * 3)(*[float(np.float32(x)) for x in v]) for v in (origin, direction))
    link = None if leaf_link is None else np.ascontiguousarray(leaf_link, np.uint32)
    cap = 4 * device_nodes.size + 4
    visits = np.zeros(cap, np.uint32)
    status = C.c_int(0)
    cnt = host_lib().mi_hot_walk(device_nodes.ctypes.data, device_nodes.size, None if link is None else link.ctypes.data, o, d, visits.ctypes.data, cap, C.byref(status))
    _check_host(status.value)
    return visits[:min(cnt, cap)].copy()


def hot_collapse(nodes: np.ndarray, theta: float = -1.0) -> dict:
    """mi_hot_collapse: the collapsed tree plain renders walk where the private copy is on (csrc/hot_order.hpp) - {"preorder", "keep"}
    over the BVH_NODE array's nodes, and over the survivors {"from" (preorder index of survivor j), "collapsed" (the survivors as a
    preorder array of their own), "order", "hot", "leaf_link", "share"}; "blocked": the interior nodes only the containment rule keeps.
    theta < 0: the device library's constant."""
    nodes = np.ascontiguousarray(nodes, dtype=BVH_NODE)
    n = nodes.size
    out = {"preorder": np.zeros(n, DEVICE_NODE), "keep": np.zeros(n, np.uint8), "from": np.zeros(n, np.uint32), "collapsed": np.zeros(n, DEVICE_NODE),
           "order": np.zeros(n, np.uint32), "hot": np.zeros(n, DEVICE_NODE), "leaf_link": np.zeros(n, np.uint32), "share": np.zeros(n, np.float64)}
    counts = (C.c_uint32 * 2)()
    _check_host(host_lib().mi_hot_collapse(nodes.ctypes.data if n else None, n, float(theta),
                                           *[out[k].ctypes.data if n else None for k in ("preorder", "keep", "from", "collapsed", "order", "hot", "leaf_link", "share")], counts))
    m = int(counts[0])
    for k in ("from", "collapsed", "order", "hot", "leaf_link", "share"):
        out[k] = out[k][:m].copy()
    out["blocked"] = int(counts[1])
    return out


def hot_join(collapse: dict, full: dict) -> dict:
    """mi_hot_join: the node array plain renders walk where the private copy is on - hot_collapse's tree, then hot_nodes' (every node) -
    {"nodes", "leaf_link", "exact_start" (where a cast on the literal box test starts), "place" (preorder index of the node at place k)}."""
    m, n = collapse["hot"].size, full["hot"].size
    out = {"nodes": np.zeros(m + n, DEVICE_NODE), "leaf_link": np.zeros(m + n, np.uint32)}
    start = C.c_uint32(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    _check_host(host_lib().mi_hot_join(ptr(collapse["hot"]), ptr(collapse["leaf_link"]), m, ptr(full["hot"]), ptr(full["leaf_link"]), n, ptr(out["nodes"]), ptr(out["leaf_link"]),
                                       C.byref(start)))
    out["exact_start"] = int(start.value)
    out["place"] = np.concatenate([collapse["from"][collapse["order"]], full["order"]]).astype(np.uint32)
    return out


def diffuse_frame(normal) -> np.ndarray:
    """mi_diffuse_frame: the tangent frame (xb, yb) a diffuse bounce builds about `normal`, as a (2, 3) float32 array."""
    n = (C.c_float * 3)(*[float(np.float32(x)) for x in normal])
    xb, yb = (C.c_float * 3)(), (C.c_float * 3)()
    host_lib().mi_diffuse_frame(n, xb, yb)
    return np.array([list(xb), list(yb)], np.float32)


def leaf_frames(desc: SceneDesc, place: np.ndarray | None = None):
    """mi_leaf_frames: the per-leaf frame records of a scene without vertex normals (option leaf_frame) - (frames, normals): frames[k] =
    the eight floats {xb, 0, yb, 0} of the node at place[k] (None: the shared, preorder array), normals[i] = the normal node i's frame
    is built about (zeros for sphere leaves and interior nodes). place = hot_nodes(...)["order"] or hot_join(...)["place"]: the records
    of a private copy."""
    n = int(desc.num_nodes)
    at = None if place is None else np.ascontiguousarray(place, np.uint32)
    count = n if at is None else at.size
    frames, normals = np.zeros((count, 8), np.float32), np.zeros((n, 3), np.float32)
    _check_host(host_lib().mi_leaf_frames(C.byref(desc), None if at is None or not count else at.ctypes.data, count, frames.ctypes.data if count else None, normals.ctypes.data if n else None))
    return frames, normals


def hot_cast_is_literal(origin, direction) -> bool:
    """mi_hot_cast_is_literal: whether K1w runs the literal box test for this cast (and starts it in the region of every node)."""
    o, d = ((C.c_float * 3)(*[float(np.float32(x)) for x in v]) for v in (origin, direction))
    return bool(host_lib().mi_hot_cast_is_literal(o, d))


def hot_walk_count(device_nodes: np.ndarray, origin, direction, leaf_link: np.ndarray | None = None, t_max: float = float("inf"), start: int = 0):
    """mi_hot_walk_count: hot_walk from node `start` for the segment [0, t_max] with the far slab product scaled as the kernels scale it -
    (entries, number of box tests)."""
    assert device_nodes.dtype == DEVICE_NODE and device_nodes.flags.c_contiguous
    o, d = ((C.c_float * 3)(*[float(np.float32(x)) for x in v]) for v in (origin, direction))
    link = None if leaf_link is None else np.ascontiguousarray(leaf_link, np.uint32)
    cap = 4 * device_nodes.size + 4
    visits = np.zeros(cap, np.uint32)
    status, tests = C.c_int(0), C.c_uint32(0)
    cnt = host_lib().mi_hot_walk_count(device_nodes.ctypes.data, device_nodes.size, None if link is None else link.ctypes.data, int(start), o, d, C.c_float(float(np.float32(t_max))),
                                       visits.ctypes.data, cap, C.byref(tests), C.byref(status))
    _check_host(status.value)
    return visits[:min(cnt, cap)].copy(), int(tests.value)


def sphere_crossings_host(centre, radius2, origin, direction, t_min=0.0, t_max=float("inf")) -> int:
    """mi_sphere_crossings_host: how often the ray crosses the sphere's shell with t_min < t < t_max (0, 1 or 2), from the
    definition the crossing-count kernels run (csrc/cross_math.hpp) - the part of IpuScene.count_crossings with no reference
    counterpart. centre, origin, direction: three numbers each, taken as binary32; radius2: the squared radius."""
    c, o, d = ((C.c_float * 3)(*[float(np.float32(x)) for x in v]) for v in (centre, origin, direction))
    return int(host_lib().mi_sphere_crossings_host(c, C.c_float(float(np.float32(radius2))), o, d, C.c_float(float(np.float32(t_min))),
                                                   C.c_float(float(np.float32(t_max)))))


def sphere_roots_host(centre, radius2, origin, direction, t_min=0.0, t_max=float("inf")):
    """mi_sphere_roots_host: the crossings sphere_crossings_host counts, with their t, as a crossing list reports them. Returns
    (mask, t0, t1): bit 0 of mask = the near root t0 is accepted, bit 1 = the far root t1 is (the one marked CROSS_FAR); t0 and t1
    are binary32 values as Python floats, NaN when the line misses the sphere."""
    c, o, d = ((C.c_float * 3)(*[float(np.float32(x)) for x in v]) for v in (centre, origin, direction))
    t = (C.c_float * 2)(float("nan"), float("nan"))
    mask = int(host_lib().mi_sphere_roots_host(c, C.c_float(float(np.float32(radius2))), o, d, C.c_float(float(np.float32(t_min))),
                                               C.c_float(float(np.float32(t_max))), t))
    return mask, float(t[0]), float(t[1])


def _geometry_array(a, dtype, width):
    """A C-contiguous `dtype` array from a `dtype` array or an [n, width] float32 array (None stays None)."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype != dtype:
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"expected a {dtype} array or an [n, {width}] float32 array, got shape {a.shape}")
        return a.view(dtype).reshape(-1)
    return np.ascontiguousarray(a).reshape(-1)


def serialise_scene(desc: SceneDesc) -> np.ndarray:
    """Serialiser<16> << SceneRef (src/IpuScene.cpp:51-53): the scene as one 16-byte-aligned byte stream."""
    lib = host_lib()
    n = lib.mi_scene_blob_size(C.byref(desc))
    out = aligned_bytes(n)
    written = C.c_size_t()
    _check_host(lib.mi_scene_serialise(C.byref(desc), out.ctypes.data, n, C.byref(written)))
    assert written.value == n
    return out


def deserialise_scene(blob: np.ndarray, into: SceneDesc | None = None) -> SceneDesc:
    """Deserialiser<16> >> SceneRef: array views INTO `blob` (keep it alive) + the eight scalars."""
    d = into if into is not None else SceneDesc()
    used = C.c_size_t()
    _check_host(host_lib().mi_scene_deserialise(blob.ctypes.data, blob.size, C.byref(d), C.byref(used)))
    d._blob = blob        # keep-alive
    d._blob_bytes_used = used.value
    return d


class NifAssets:
    """NIF model read from an 'assets.extra' directory: nif_metadata.txt + converted.hdf5 (Keras H5) or
    nif_weights.bin — what IpuScene::loadNifModel reads (src/IpuScene.cpp:174-187). Arrays are copies."""

    def __init__(self, asset_path):
        lib = host_lib()
        h = C.c_void_p()
        if lib.mi_host_nif_load(os.fspath(asset_path).encode(), C.byref(h)) != 0:
            raise RaylibError(lib.mi_host_nif_last_error().decode())
        try:
            d = NifDesc()
            if lib.mi_host_nif_describe(h, C.byref(d)) != 0:
                raise RaylibError(lib.mi_host_nif_last_error().decode())
            self.kernels, self.biases, self.relu = [], [], []
            for i in range(d.num_layers):
                r, c = int(d.rows[i]), int(d.cols[i])
                self.kernels.append(np.ctypeslib.as_array(d.kernels[i], shape=(r, c)).copy())
                self.biases.append(np.ctypeslib.as_array(d.biases[i], shape=(c,)).copy() if d.biases[i] else None)
                self.relu.append(bool(d.relu[i]))
            self.embedding_dimension = int(d.embedding_dimension)
            self.hidden_size = int(d.hidden_size)
            self.max_value = float(d.max_value)
            self.mean = np.array(list(d.mean), dtype=np.float32)
            self.log_tonemap = bool(d.log_tonemap)
            self.weights_are_half = bool(d.weights_are_half)
            self.name = d.name.decode()
            self.source = d.source.decode()
        finally:
            lib.mi_host_nif_destroy(h)


class IpuScene:
    """Mirror of the reference's ``IpuScene`` driver object (include/IpuScene.hpp:22-56) over the
    C ABI: construct from a scene description, optionally load a NIF, ``run`` a ray stream."""

    def __init__(self, desc: SceneDesc, variants: bool = False):
        self._lib = device_lib(variants)
        self._h = C.c_void_p()
        self.desc = desc
        self._check(self._lib.mi_scene_create(C.byref(desc), C.byref(self._h)))

    def _check(self, status: int):
        if status != MI_OK:
            raise RaylibError(f"mi_raylib call failed ({status}): {self._lib.mi_last_error().decode()}")

    # -- reference API names -------------------------------------------------------------
    @classmethod
    def from_blob(cls, blob: np.ndarray, extras: SceneDesc, variants: bool = False) -> "IpuScene":
        """Scene from the reference's serialised byte stream + the fields that are not part of it."""
        self = cls.__new__(cls)
        self._lib = device_lib(variants)
        self._h = C.c_void_p()
        self.desc = extras
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self._lib.mi_scene_create_from_blob(b.ctypes.data, b.size, C.byref(extras), C.byref(self._h)))
        return self

    @classmethod
    def from_geometry(cls, desc: SceneDesc, variants: bool = False) -> "IpuScene":
        """A scene without a host-built BVH: an empty scene with desc's render parameters, then set_geometry(desc) - the BVH is
        the LBVH of desc's arrays, built on the device (desc's own nodes are ignored)."""
        empty = SceneDesc.from_buffer_copy(desc)
        for name, _ in SceneGeometry._fields_:
            setattr(empty, name, 0)
        empty.bvh_nodes, empty.num_nodes, empty.max_leaf_depth = None, 0, 0
        self = cls(empty, variants)
        self.desc = desc
        self.set_geometry(desc)
        return self

    def setHdriRotation(self, degrees: float):
        self._check(self._lib.mi_scene_set_hdri_rotation(self._h, float(degrees)))

    def setMaxNifBatchSize(self, rays_per_batch: int):
        self._check(self._lib.mi_scene_set_max_nif_batch(self._h, int(rays_per_batch)))

    def setRayBatch(self, rays_per_batch: int):
        self._check(self._lib.mi_scene_set_ray_batch(self._h, int(rays_per_batch)))

    def set_option(self, key: str, value) -> "IpuScene":
        """Kernel selection / tuning of THIS scene (mi_scene_set_option); never changes a result bit."""
        self._check(self._lib.mi_scene_set_option(self._h, key.encode(), str(value).encode()))
        return self

    def getTraceTimeSecs(self) -> float:
        return float(self._lib.mi_trace_time_secs(self._h))

    def loadNifModel(self, asset_path) -> bool:
        """IpuScene::loadNifModel (src/IpuScene.cpp:174-187): log and return False on any failure."""
        try:
            a = NifAssets(asset_path)
            self.setNif(a.kernels, a.biases, a.relu, a.embedding_dimension, a.max_value, a.mean, a.log_tonemap)
            return True
        except RaylibError as e:
            print(f"[error] {e}", file=sys.stderr)
            return False

    def setNif(self, kernels, biases, relu, embedding_dimension, max_value, mean, log_tonemap=True):
        """Weights as arrays (what loadNifModel ends up calling)."""
        n = len(kernels)
        ks = [np.ascontiguousarray(k, dtype=np.float32) for k in kernels]
        bs = [None if b is None else np.ascontiguousarray(b, dtype=np.float32) for b in biases]
        kp = (C.c_void_p * n)(*[k.ctypes.data for k in ks])
        bp = (C.c_void_p * n)(*[(b.ctypes.data if b is not None else None) for b in bs])
        rows = np.array([k.shape[0] for k in ks], dtype=np.uint32)
        cols = np.array([k.shape[1] for k in ks], dtype=np.uint32)
        rl = np.array([1 if r else 0 for r in relu], dtype=np.uint8)
        mean_a = np.ascontiguousarray(mean, dtype=np.float32)
        self._check(self._lib.mi_scene_set_nif(self._h, n, kp, bp, rows.ctypes.data, cols.ctypes.data, rl.ctypes.data,
                                              int(embedding_dimension), float(max_value), mean_a.ctypes.data,
                                              1 if log_tonemap else 0))

    def run(self, rays: np.ndarray, mode: int | None = None, callback=None) -> np.ndarray:
        """GraphManager().run(ipuScene): trace the HOST ray stream in place. `callback(batch_index, first, count)`
        mirrors IpuScene::RayCallbackFn (one call per finished ray batch, see setRayBatch)."""
        assert rays.dtype == TRACE_RESULT and rays.flags["C_CONTIGUOUS"]
        if mode is None:
            mode = MODE_PATH_TRACE if self.desc.path_trace else MODE_SHADOW_TRACE
        cb = None
        if callback is not None:
            base = rays.ctypes.data
            proto = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t)
            cb = proto(lambda user, idx, ptr, cnt: callback(idx, (ptr - base) // TRACE_RESULT.itemsize, cnt))
        self._check(self._lib.mi_render(self._h, mode, rays.ctypes.data, rays.size, cb, None))
        return rays

    def run_device(self, d_rays_ptr: int, n: int, mode: int, stream: int = 0):
        """Trace a DEVICE-resident ray stream (e.g. a torch uint8 tensor's data_ptr) asynchronously."""
        self._check(self._lib.mi_render_device(self._h, mode, C.c_void_p(d_rays_ptr), n, C.c_void_p(stream)))

    # -- what the query wrappers below share ---------------------------------------------------------------------------------------
    @staticmethod
    def _source(arr: np.ndarray, dtype) -> np.ndarray:
        """A 1-d `dtype` array as the host entries take it: contiguous, at a 16-byte aligned address (a copy where it is not)."""
        assert arr.dtype == dtype and arr.ndim == 1
        return arr if (arr.flags["C_CONTIGUOUS"] and arr.ctypes.data % 16 == 0) else _aligned_copy(arr)

    @staticmethod
    def _torch_rays(what, origins, directions, t_min, t_max):
        import torch
        o = origins.to(torch.float32)
        d = directions.to(torch.float32)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape or not o.is_cuda or d.device != o.device:
            raise ValueError(f"{what}: origins and directions must be [N, 3] tensors on one GPU")
        n = o.shape[0]

        def column(x):
            return torch.as_tensor(x, dtype=torch.float32, device=o.device).expand(n).reshape(n, 1)

        return torch.cat([o, column(t_min), d, column(t_max)], dim=1).contiguous(), n      # [N, 8] = n mi_ray

    @staticmethod
    def _torch_points(what, points, radius):
        import torch
        p = points.to(torch.float32)
        if p.ndim != 2 or p.shape[1] != 3 or not p.is_cuda:
            raise ValueError(f"{what}: points must be an [N, 3] tensor on a GPU")
        n = p.shape[0]
        r = torch.as_tensor(radius, dtype=torch.float32, device=p.device).expand(n).reshape(n, 1)
        return torch.cat([p, r], dim=1).contiguous(), n      # [N, 4] = n mi_point

    @staticmethod
    def _torch_records(items, n, entry, *args):
        """What `entry(*args, d_items, d_out, n, ..., stream)` writes as 32-byte records, on torch's current stream: an [N, 8]
        float32 tensor; `_torch_flags`: its one byte per item, as bools."""
        import torch
        raw = torch.empty((n, 8), dtype=torch.float32, device=items.device)
        entry(*args, items.data_ptr(), raw.data_ptr(), n, stream=torch.cuda.current_stream(items.device).cuda_stream)
        return raw

    @staticmethod
    def _torch_flags(items, n, entry, *args):
        import torch
        out = torch.empty(n, dtype=torch.uint8, device=items.device)
        entry(*args, items.data_ptr(), out.data_ptr(), n, stream=torch.cuda.current_stream(items.device).cuda_stream)
        return out.bool()

    @staticmethod
    def _torch_counts(items, n, entry, *args):
        """`_torch_flags` for an entry that writes a uint32 per item: an [N] int32 tensor."""
        import torch
        out = torch.empty(n, dtype=torch.int32, device=items.device)
        entry(*args, items.data_ptr(), out.data_ptr(), n, stream=torch.cuda.current_stream(items.device).cuda_stream)
        return out

    @staticmethod
    def _hit_columns(raw, first, vector):
        """The fields of [N, 8] float32 hit records (mi_query_hit, mi_point_hit) as tensors; `first`, `vector`: what the record's
        first float and its three floats are called."""
        import torch
        words, halves = raw.view(torch.int32), raw.view(torch.int16)
        return {first: raw[:, 0], "prim_id": words[:, 1], "geom_id": halves[:, 4].to(torch.int32), "flags": halves[:, 5],
                vector: raw[:, 3:6], "bary": raw[:, 6:8]}

    # the two list families (crossings of rays, neighbours of points) differ in their entries and their 16-byte record
    def _offsets_host(self, entry, src: np.ndarray) -> np.ndarray:
        offsets = np.zeros(src.size + 1, np.uint64)
        self._check(entry(self._h, src.ctypes.data, offsets.ctypes.data, src.size))
        return offsets

    def _fill_host(self, entry, rec, src: np.ndarray, offsets: np.ndarray, hits: np.ndarray, capacity) -> np.ndarray:
        assert offsets.dtype == np.uint64 and offsets.ndim == 1 and offsets.size == src.size + 1 and offsets.flags["C_CONTIGUOUS"]
        assert hits.dtype == rec and hits.flags["C_CONTIGUOUS"]
        capacity = hits.size if capacity is None else int(capacity)
        assert 0 <= capacity <= hits.size
        self._check(entry(self._h, src.ctypes.data, offsets.ctypes.data, hits.ctypes.data, capacity, src.size))
        return hits

    @staticmethod
    def _all_lists(offsets_of, fill, rec, items: np.ndarray):
        offsets = offsets_of(items)
        total = int(offsets[-1])
        recs = aligned_bytes(max(total, 1) * rec.itemsize).view(rec)      # (the entry refuses a null buffer)
        fill(items, offsets, recs, total)
        return offsets, recs[:total]

    @staticmethod
    def _first_k(fill, rec, items: np.ndarray, k: int) -> np.ndarray:
        n, k = items.size, int(k)
        assert k >= 0
        offsets = (np.arange(n + 1, dtype=np.uint64) * np.uint64(k)).astype(np.uint64)
        recs = aligned_bytes(max(n * k, 1) * rec.itemsize).view(rec)
        fill(items, offsets, recs, n * k)
        return recs[:n * k].reshape(n, k)

    @staticmethod
    def _torch_all_lists(offsets_device, fill_device, items, n, sync_when_empty: bool):
        """(offsets [N + 1] int64, records [total, 4] int32) on torch's current stream: the offsets, one .item() for the total,
        then the fill."""
        import torch
        stream = torch.cuda.current_stream(items.device).cuda_stream
        splits = torch.zeros(n + 1, dtype=torch.int64, device=items.device)
        offsets_device(items.data_ptr(), splits.data_ptr(), n, stream)
        total = int(splits[-1].item()) if (n or sync_when_empty) else 0
        raw = torch.empty((max(total, 1), 4), dtype=torch.int32, device=items.device)
        fill_device(items.data_ptr(), splits.data_ptr(), raw.data_ptr(), total, n, stream)
        return splits, raw[:total]

    @staticmethod
    def _torch_first_k(fill_device, items, n, k: int):
        """(offsets [N + 1] int64 = k i, records [N, k, 4] int32): one launch on torch's current stream, no synchronisation."""
        import torch
        k = int(k)
        offsets = torch.arange(n + 1, dtype=torch.int64, device=items.device) * k
        raw = torch.empty((max(n * k, 1), 4), dtype=torch.int32, device=items.device)
        fill_device(items.data_ptr(), offsets.data_ptr(), raw.data_ptr(), n * k, n, torch.cuda.current_stream(items.device).cuda_stream)
        return offsets, raw[:n * k].reshape(n, k, 4)

    # -- ray queries (mi_query / mi_query_device): CompactBvh::intersect / ::occluded per given ray, no shading --------------
    def _query_host(self, kind: int, rays: np.ndarray, out: np.ndarray) -> np.ndarray:
        src = self._source(rays, RAY)
        self._check(self._lib.mi_query(self._h, kind, src.ctypes.data, out.ctypes.data, src.size))
        return out

    def intersect(self, rays: np.ndarray) -> np.ndarray:
        """Closest hit of every ray (a RAY array, host memory): a QUERY_HIT array. Synchronous; batched by setRayBatch."""
        return self._query_host(QUERY_CLOSEST, rays, aligned_bytes(rays.size * QUERY_HIT.itemsize).view(QUERY_HIT))

    def occluded(self, rays: np.ndarray) -> np.ndarray:
        """Whether anything is hit with tMin < t < tMax, for every ray (a RAY array, host memory): a bool array."""
        return self._query_host(QUERY_ANY, rays, aligned_bytes(rays.size)).view(np.bool_)

    def query_device(self, kind: int, d_rays: int, d_out: int, n: int, stream: int = 0):
        """mi_query_device on device pointers (n RAY records in, n QUERY_HIT records or n bytes out), asynchronous on `stream`."""
        self._check(self._lib.mi_query_device(self._h, int(kind), C.c_void_p(d_rays), C.c_void_p(d_out), int(n), C.c_void_p(stream)))

    def cast(self, origins, directions, t_min=0.0, t_max=float("inf"), any_hit: bool = False) -> dict:
        """Torch convenience over mi_query_device: float32 device tensors of shape [N, 3] (t_min / t_max: numbers or [N]
        tensors), enqueued on torch.cuda.current_stream(). Returns device tensors: closest hit {"t" [N], "prim_id" [N] int32,
        "geom_id" [N] int32 (-1 on a miss, for both), "normal" [N, 3], "bary" [N, 2] (b1, b2)}; any hit {"occluded" [N] bool}."""
        rays, n = self._torch_rays("cast", origins, directions, t_min, t_max)
        if any_hit:
            return {"occluded": self._torch_flags(rays, n, self.query_device, QUERY_ANY)}
        cols = self._hit_columns(self._torch_records(rays, n, self.query_device, QUERY_CLOSEST), "t", "normal")
        return {f: cols[f] for f in ("t", "prim_id", "geom_id", "normal", "bary")}

    # -- point queries (mi_point_query / mi_point_query_device): the nearest primitive within each point's radius -----------------
    def _point_query_host(self, kind: int, points: np.ndarray, out: np.ndarray) -> np.ndarray:
        src = self._source(points, POINT)
        self._check(self._lib.mi_point_query(self._h, kind, src.ctypes.data, out.ctypes.data, src.size))
        return out

    def closest_points(self, points: np.ndarray) -> np.ndarray:
        """The nearest primitive strictly within each point's radius (a POINT array, host memory): a POINT_HIT array - distance,
        ids, the closest point on the primitive, a triangle's barycentrics. Synchronous; batched by setRayBatch."""
        return self._point_query_host(POINT_CLOSEST, points, aligned_bytes(points.size * POINT_HIT.itemsize).view(POINT_HIT))

    def within(self, points: np.ndarray) -> np.ndarray:
        """Whether some primitive lies strictly within each point's radius (a POINT array, host memory): a bool array."""
        return self._point_query_host(POINT_WITHIN, points, aligned_bytes(points.size)).view(np.bool_)

    def point_query_device(self, kind: int, d_points: int, d_out: int, n: int, stream: int = 0):
        """mi_point_query_device on device pointers (n POINT records in, n POINT_HIT records or n bytes out), asynchronous on `stream`."""
        self._check(self._lib.mi_point_query_device(self._h, int(kind), C.c_void_p(d_points), C.c_void_p(d_out), int(n), C.c_void_p(stream)))

    def nearest(self, points, radius=float("inf"), within: bool = False) -> dict:
        """Torch convenience over mi_point_query_device: a float32 device tensor of shape [N, 3] (radius: a number or an [N]
        tensor), enqueued on torch.cuda.current_stream(). Returns device tensors: {"dist" [N], "prim_id" [N] int32, "geom_id" [N]
        int32 (-1 when nothing was found, for both), "point" [N, 3], "bary" [N, 2] (b1, b2)}; within=True: {"within" [N] bool}."""
        pts, n = self._torch_points("nearest", points, radius)
        if within:
            return {"within": self._torch_flags(pts, n, self.point_query_device, POINT_WITHIN)}
        cols = self._hit_columns(self._torch_records(pts, n, self.point_query_device, POINT_CLOSEST), "dist", "point")
        return {f: cols[f] for f in ("dist", "prim_id", "geom_id", "point", "bary")}

    # -- neighbour lists (mi_near_offsets*, mi_near_fill*): every primitive within each point's radius, nearest first ---------------
    def near_offsets(self, points: np.ndarray) -> np.ndarray:
        """mi_near_offsets: a uint64 array of points.size + 1 offsets - 0, then the running total of the number of primitives
        strictly within each point's radius (a POINT array, host memory)."""
        return self._offsets_host(self._lib.mi_near_offsets, self._source(points, POINT))

    def near_fill(self, points: np.ndarray, offsets: np.ndarray, hits: np.ndarray, capacity: int | None = None) -> np.ndarray:
        """mi_near_fill: point i's neighbours, nearest first, into hits[offsets[i]:offsets[i + 1]] (a NEIGHBOUR array at a 16-byte
        aligned address, see aligned_bytes), cut or padded to that length; nothing at or past `capacity` (None: hits.size) is
        written."""
        return self._fill_host(self._lib.mi_near_fill, NEIGHBOUR, self._source(points, POINT), offsets, hits, capacity)

    def neighbours(self, points: np.ndarray):
        """Every primitive strictly within each point's radius (a POINT array, host memory), as (offsets, recs): offsets uint64
        [n + 1], recs a NEIGHBOUR array of offsets[n] records; recs[offsets[i]:offsets[i + 1]] are point i's neighbours in ascending
        order of dist2 (the SQUARED distance; then geomID, primID). Synchronous; batched by setRayBatch."""
        return self._all_lists(self.near_offsets, self.near_fill, NEIGHBOUR, points)

    def k_nearest(self, points: np.ndarray, k: int) -> np.ndarray:
        """The k nearest primitives strictly within each point's radius, in that order: a NEIGHBOUR array [n, k]; points with fewer
        are padded with the empty record (dist2 = +inf, INVALID_PRIM, INVALID_GEOM, FLAG_ESCAPED). One fill, no count pass; the walk
        shrinks its bound to the k-th distance kept, so radius = inf does not walk the whole tree."""
        return self._first_k(self.near_fill, NEIGHBOUR, points, k)

    def near_offsets_device(self, d_points: int, d_offsets: int, n: int, stream: int = 0):
        """mi_near_offsets_device on device pointers (n POINT records in, n + 1 uint64 out), asynchronous on `stream`."""
        self._check(self._lib.mi_near_offsets_device(self._h, C.c_void_p(d_points), C.c_void_p(d_offsets), int(n), C.c_void_p(stream)))

    def near_fill_device(self, d_points: int, d_offsets: int, d_hits: int, capacity: int, n: int, stream: int = 0):
        """mi_near_fill_device on device pointers (n POINT records and n + 1 uint64 in, `capacity` NEIGHBOUR records out),
        asynchronous on `stream`."""
        self._check(self._lib.mi_near_fill_device(self._h, C.c_void_p(d_points), C.c_void_p(d_offsets), C.c_void_p(d_hits), int(capacity),
                                                  int(n), C.c_void_p(stream)))

    @staticmethod
    def _neighbour_columns(raw):
        """The fields of [..., 4] int32 neighbour records as tensors."""
        import torch
        halves = raw.view(torch.int16)
        return {"point_ids": raw[..., 3].to(torch.int64) & 0xFFFFFFFF, "dist2": raw.view(torch.float32)[..., 0], "prim_id": raw[..., 1],
                "geom_id": halves[..., 4].to(torch.int32)}

    def ball_query(self, points, radius) -> dict:
        """Torch convenience over mi_near_offsets_device + mi_near_fill_device (Open3D's search_radius_vector_3d): a float32 device
        tensor of shape [N, 3] (radius: a number or an [N] tensor), enqueued on torch.cuda.current_stream(). It runs the offsets,
        reads the total with one .item() (the one synchronisation), then allocates and fills. Returns device tensors: {"offsets"
        [N + 1] int64, and per neighbour, point by point, nearest first: "point_ids" int64, "dist2" (squared), "prim_id" int32,
        "geom_id" int32}."""
        pts, n = self._torch_points("ball_query", points, radius)
        splits, raw = self._torch_all_lists(self.near_offsets_device, self.near_fill_device, pts, n, sync_when_empty=False)
        return {**self._neighbour_columns(raw), "offsets": splits}

    def knn(self, points, k: int, radius=float("inf")) -> dict:
        """The k nearest primitives of every point strictly within `radius`, as [N, k] columns {"dist2", "prim_id", "geom_id",
        "point_ids"} and "offsets" [N + 1] int64 (= k i): points with fewer are padded with dist2 = +inf and prim_id = geom_id = -1.
        One launch on torch.cuda.current_stream(), no synchronisation."""
        pts, n = self._torch_points("knn", points, radius)
        offsets, raw = self._torch_first_k(self.near_fill_device, pts, n, k)
        return {**self._neighbour_columns(raw), "offsets": offsets}

    # -- the touch families (_TOUCH_FAMILIES): their host and device-pointer methods are bound below the class (_TOUCH_METHODS); here are
    # -- the torch conveniences, whose argument lists differ per family, each over its packer --------------------------------------
    @staticmethod
    def _torch_boxes(what, lo, hi):
        import torch
        a, b = lo.to(torch.float32), hi.to(torch.float32)
        if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape or not a.is_cuda or b.device != a.device:
            raise ValueError(f"{what}: lo and hi must be [N, 3] tensors on one GPU")
        n = a.shape[0]
        pad = torch.zeros((n, 1), dtype=torch.float32, device=a.device)
        return torch.cat([a, pad, b, pad], dim=1).contiguous(), n      # [N, 8] = n mi_box

    def box_any(self, lo, hi):
        """Torch convenience over mi_box_query_device (BOX_ANY): float32 device tensors lo, hi of shape [N, 3], enqueued on
        torch.cuda.current_stream(). Returns an [N] bool device tensor: a primitive touches the box."""
        boxes, n = self._torch_boxes("box_any", lo, hi)
        return self._torch_flags(boxes, n, self.box_query_device, BOX_ANY)

    def box_count(self, lo, hi):
        """The same over mi_box_query_device for BOX_COUNT: an [N] int32 device tensor, the number of primitives touching each box."""
        boxes, n = self._torch_boxes("box_count", lo, hi)
        return self._torch_counts(boxes, n, self.box_query_device, BOX_COUNT)

    def box_list(self, lo, hi):
        """Torch convenience over mi_box_offsets_device + mi_box_fill_device: (offsets [N + 1] int64, recs [total, 4] int32 - the
        words of the OVERLAP records: primID, geomID | flags << 16, box, 0), box by box in ascending (geomID, primID). It runs the
        offsets, reads the total with one .item() (the one synchronisation), then allocates and fills."""
        boxes, n = self._torch_boxes("box_list", lo, hi)
        return self._torch_all_lists(self.box_offsets_device, self.box_fill_device, boxes, n, sync_when_empty=False)

    def voxelize(self, origin, cell, dims, device=None):
        """Surface voxelisation: a bool device tensor [nx, ny, nz], cell (i, j, k) set when a primitive touches the closed box
        lo = origin + (i, j, k) cell, hi = origin + (i + 1, j + 1, k + 1) cell - each one multiply and one add in float32 as written,
        so neighbouring cells share their faces bit for bit and a surface lying in a shared face sets the cells on both sides.
        origin: three floats; cell: a float or three; dims: (nx, ny, nz). One BOX_ANY launch on torch.cuda.current_stream()."""
        import torch
        dev = torch.device("cuda", self.desc.device) if device is None else torch.device(device)
        nx, ny, nz = (int(d) for d in dims)
        o = torch.as_tensor(origin, dtype=torch.float32, device=dev).expand(3)
        c = torch.as_tensor(cell, dtype=torch.float32, device=dev).expand(3)
        axes = [torch.arange(m + 1, dtype=torch.float32, device=dev) * c[a] + o[a] for a, m in enumerate((nx, ny, nz))]      # the grid's planes
        lo = torch.stack(torch.meshgrid(axes[0][:-1], axes[1][:-1], axes[2][:-1], indexing="ij"), dim=-1).reshape(-1, 3)
        hi = torch.stack(torch.meshgrid(axes[0][1:], axes[1][1:], axes[2][1:], indexing="ij"), dim=-1).reshape(-1, 3)
        return self.box_any(lo, hi).reshape(nx, ny, nz)

    @staticmethod
    def _torch_oboxes(what, centre, half, quat):
        import torch
        c, h, q = centre.to(torch.float32), half.to(torch.float32), quat.to(torch.float32)
        if c.ndim != 2 or c.shape[1] != 3 or h.shape != c.shape or q.shape != (c.shape[0], 4) or not c.is_cuda or h.device != c.device or q.device != c.device:
            raise ValueError(f"{what}: centre and half must be [N, 3] tensors and quat an [N, 4] tensor (x, y, z, w) on one GPU")
        n = c.shape[0]
        pad = torch.zeros((n, 1), dtype=torch.float32, device=c.device)
        return torch.cat([c, pad, h, pad, q], dim=1).contiguous(), n      # [N, 12] = n mi_obox

    def obox_any(self, centre, half, quat):
        """Torch convenience over mi_obox_query_device (OBOX_ANY): float32 device tensors centre, half [N, 3] and quat [N, 4] (x, y,
        z, w; need not be unit), packed on the device and enqueued on torch.cuda.current_stream(). Returns an [N] bool device
        tensor: a primitive touches the oriented box."""
        oboxes, n = self._torch_oboxes("obox_any", centre, half, quat)
        return self._torch_flags(oboxes, n, self.obox_query_device, OBOX_ANY)

    def obox_count(self, centre, half, quat):
        """The same over mi_obox_query_device for OBOX_COUNT: an [N] int32 device tensor, the number of primitives touching each oriented box."""
        oboxes, n = self._torch_oboxes("obox_count", centre, half, quat)
        return self._torch_counts(oboxes, n, self.obox_query_device, OBOX_COUNT)

    def obox_list(self, centre, half, quat):
        """Torch convenience over mi_obox_offsets_device + mi_obox_fill_device: (offsets [N + 1] int64, recs [total, 4] int32 - the
        words of the OVERLAP records: primID, geomID | flags << 16, box, 0), box by box in ascending (geomID, primID). It runs the
        offsets, reads the total with one .item() (the one synchronisation), then allocates and fills."""
        oboxes, n = self._torch_oboxes("obox_list", centre, half, quat)
        return self._torch_all_lists(self.obox_offsets_device, self.obox_fill_device, oboxes, n, sync_when_empty=False)

    @staticmethod
    def _torch_capsules(what, a, b, radius):
        import torch
        a, b = a.to(torch.float32), b.to(torch.float32)
        if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape or not a.is_cuda or b.device != a.device:
            raise ValueError(f"{what}: a and b must be [N, 3] tensors on one GPU")
        n = a.shape[0]
        if isinstance(radius, torch.Tensor):
            r = radius.to(torch.float32)
            if r.device != a.device or r.numel() not in (1, n):
                raise ValueError(f"{what}: radius must be a number or an [N] tensor on the same GPU")
            r = r.reshape(-1, 1).expand(n, 1)
        else:
            r = torch.full((n, 1), float(radius), dtype=torch.float32, device=a.device)
        pad = torch.zeros((n, 1), dtype=torch.float32, device=a.device)
        return torch.cat([a, r, b, pad], dim=1).contiguous(), n      # [N, 8] = n mi_capsule

    def capsule_any(self, a, b, radius):
        """Torch convenience over mi_capsule_query_device (CAPSULE_ANY): float32 device tensors a, b [N, 3] and radius (a number or
        an [N] tensor), packed on the device and enqueued on torch.cuda.current_stream(). Returns an [N] bool device tensor: a
        primitive lies within the radius of the segment - a ball of that radius moving from a to b hits something."""
        capsules, n = self._torch_capsules("capsule_any", a, b, radius)
        return self._torch_flags(capsules, n, self.capsule_query_device, CAPSULE_ANY)

    def capsule_count(self, a, b, radius):
        """The same over mi_capsule_query_device for CAPSULE_COUNT: an [N] int32 device tensor, the number of primitives touching each capsule."""
        capsules, n = self._torch_capsules("capsule_count", a, b, radius)
        return self._torch_counts(capsules, n, self.capsule_query_device, CAPSULE_COUNT)

    def capsule_list(self, a, b, radius):
        """Torch convenience over mi_capsule_offsets_device + mi_capsule_fill_device: (offsets [N + 1] int64, recs [total, 4] int32 -
        the words of the OVERLAP records: primID, geomID | flags << 16, capsule, 0), capsule by capsule in ascending (geomID, primID).
        It runs the offsets, reads the total with one .item() (the one synchronisation), then allocates and fills."""
        capsules, n = self._torch_capsules("capsule_list", a, b, radius)
        return self._torch_all_lists(self.capsule_offsets_device, self.capsule_fill_device, capsules, n, sync_when_empty=False)

    @staticmethod
    def _torch_frusta(what, planes):
        import torch
        f = planes.to(torch.float32)
        if f.ndim != 3 or f.shape[1:] != (6, 4) or not f.is_cuda:
            raise ValueError(f"{what}: planes must be an [N, 6, 4] tensor on a GPU")
        return f.contiguous(), f.shape[0]      # [N, 6, 4] = n mi_frustum

    def frustum_any(self, planes):
        """Torch convenience over mi_frustum_query_device (FRUSTUM_ANY): a float32 device tensor planes [N, 6, 4] (nx, ny, nz, d per
        plane, normals inward, a plane of four zeros absent), enqueued on torch.cuda.current_stream(). Returns an [N] bool device
        tensor: a primitive lies inside or touches the region."""
        frusta, n = self._torch_frusta("frustum_any", planes)
        return self._torch_flags(frusta, n, self.frustum_query_device, FRUSTUM_ANY)

    def frustum_count(self, planes):
        """The same over mi_frustum_query_device for FRUSTUM_COUNT: an [N] int32 device tensor, the number of primitives touching each frustum."""
        frusta, n = self._torch_frusta("frustum_count", planes)
        return self._torch_counts(frusta, n, self.frustum_query_device, FRUSTUM_COUNT)

    def frustum_list(self, planes):
        """Torch convenience over mi_frustum_offsets_device + mi_frustum_fill_device: (offsets [N + 1] int64, recs [total, 4] int32 -
        the words of the OVERLAP records: primID, geomID | flags << 16, frustum, 0), frustum by frustum in ascending (geomID, primID).
        It runs the offsets, reads the total with one .item() (the one synchronisation), then allocates and fills."""
        frusta, n = self._torch_frusta("frustum_list", planes)
        return self._torch_all_lists(self.frustum_offsets_device, self.frustum_fill_device, frusta, n, sync_when_empty=False)

    def cull(self, view_proj, depth: str = "zo") -> np.ndarray:
        """What a camera sees, occlusion aside: the list of the one frustum query_batches.make_frusta(view_proj=view_proj, depth=depth)
        makes of a [4, 4] view-projection matrix acting on column vectors ("zo": clip z in [0, w]; "no": in [-w, w]), as int64 rows
        (geomID, primID) [m, 2], ascending. list_frustum_overlaps on one frustum: synchronous, host memory."""
        from . import query_batches as qb
        frusta = qb.make_frusta(view_proj=np.asarray(view_proj, np.float64).reshape(4, 4), depth=depth)
        _, recs = self.list_frustum_overlaps(frusta)
        return np.stack([recs["geomID"].astype(np.int64), recs["primID"].astype(np.int64)], axis=1).reshape(-1, 2)

    @staticmethod
    def _torch_tris(what, tris):
        import torch
        t = tris.to(torch.float32)
        if t.ndim != 3 or t.shape[1:] != (3, 3) or not t.is_cuda:
            raise ValueError(f"{what}: triangles must be an [N, 3, 3] tensor on a GPU")
        return t.contiguous(), t.shape[0]      # [N, 3, 3] = n mi_tri

    @staticmethod
    def _torch_mesh(what, vertices, faces):
        import torch
        if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 or not vertices.is_cuda or faces.device != vertices.device:
            raise ValueError(f"{what}: vertices [V, 3] and faces [F, 3] must be tensors on one GPU")
        return vertices.to(torch.float32)[faces.to(torch.int64)]      # [F, 3, 3]: the gather is the batch

    def tri_any(self, tris):
        """Torch convenience over mi_tri_query_device (TRI_ANY): a float32 device tensor of shape [N, 3, 3] (vertices[faces]),
        enqueued on torch.cuda.current_stream(). Returns an [N] bool device tensor: a primitive touches the triangle."""
        t, n = self._torch_tris("tri_any", tris)
        return self._torch_flags(t, n, self.tri_query_device, TRI_ANY)

    def tri_count(self, tris):
        """The same over mi_tri_query_device for TRI_COUNT: an [N] int32 device tensor, the number of primitives touching each triangle."""
        t, n = self._torch_tris("tri_count", tris)
        return self._torch_counts(t, n, self.tri_query_device, TRI_COUNT)

    def tri_list(self, tris):
        """Torch convenience over mi_tri_offsets_device + mi_tri_fill_device: (offsets [N + 1] int64, recs [total, 4] int32 - the
        words of the CONTACT records: primID, geomID | flags << 16, tri, 0), triangle by triangle in ascending (geomID, primID). It
        runs the offsets, reads the total with one .item() (the one synchronisation), then allocates and fills."""
        t, n = self._torch_tris("tri_list", tris)
        return self._torch_all_lists(self.tri_offsets_device, self.tri_fill_device, t, n, sync_when_empty=False)

    def mesh_contacts(self, vertices, faces):
        """Mesh against scene: every (face of the mesh, primitive of the scene) pair that touches, as an int64 device tensor [m, 3]
        of rows (face, geomID, primID), sorted. vertices: float32 [V, 3], faces: integer [F, 3], device tensors; vertices[faces] is
        gathered on the device and goes through tri_list, on torch.cuda.current_stream(), with no host round trip but the total."""
        import torch
        _, recs = self.tri_list(self._torch_mesh("mesh_contacts", vertices, faces))
        words = recs.to(torch.int64) & 0xFFFFFFFF
        return torch.stack([words[:, 2], words[:, 1] & 0xFFFF, words[:, 0]], dim=1)

    def collides(self, vertices, faces) -> bool:
        """Whether any face of the mesh touches the scene (one TRI_ANY launch over vertices[faces], then any())."""
        return bool(self.tri_any(self._torch_mesh("collides", vertices, faces)).any().item())

    # -- crossing counts, inside tests, signed distance (mi_count_query*, mi_point_sign*) -----------------------------------------------
    def count_crossings(self, rays: np.ndarray) -> np.ndarray:
        """How many surfaces each ray crosses with tMin < t < tMax (a RAY array, host memory): a uint32 array. A sphere counts
        both of its roots. Synchronous; batched by setRayBatch."""
        src = self._source(rays, RAY)
        out = np.zeros(src.size, np.uint32)
        self._check(self._lib.mi_count_query(self._h, src.ctypes.data, out.ctypes.data, src.size))
        return out

    def count_query_device(self, d_rays: int, d_counts: int, n: int, stream: int = 0):
        """mi_count_query_device on device pointers (n RAY records in, n uint32 out), asynchronous on `stream`."""
        self._check(self._lib.mi_count_query_device(self._h, C.c_void_p(d_rays), C.c_void_p(d_counts), int(n), C.c_void_p(stream)))

    @staticmethod
    def _direction(direction):
        """The `dir` argument of mi_point_sign*: None (the library's default) or three floats."""
        return None if direction is None else (C.c_float * 3)(*[float(x) for x in direction])

    def _point_sign_host(self, kind: int, points: np.ndarray, out: np.ndarray, direction) -> np.ndarray:
        src = self._source(points, POINT)
        self._check(self._lib.mi_point_sign(self._h, kind, src.ctypes.data, out.ctypes.data, self._direction(direction), src.size))
        return out

    def inside(self, points: np.ndarray, direction=None) -> np.ndarray:
        """Whether each point (a POINT array, host memory; the radius is ignored) lies inside the scene's closed surfaces: a uint8
        array, 1 = the ray from the point along `direction` (None: DEFAULT_INSIDE_DIR; no component may be zero) crosses an odd
        number of surfaces. Synchronous; batched by setRayBatch."""
        return self._point_sign_host(SIGN_INSIDE, points, aligned_bytes(points.size), direction)

    def signed_distance(self, points: np.ndarray, direction=None) -> np.ndarray:
        """closest_points with a sign: the POINT_HIT array of closest_points(points), and for every point inside (see inside) dist
        negative and FLAG_INSIDE set - also where nothing lies within the radius (dist = -radius)."""
        return self._point_sign_host(SIGN_DISTANCE, points, aligned_bytes(points.size * POINT_HIT.itemsize).view(POINT_HIT), direction)

    def point_sign_device(self, kind: int, d_points: int, d_out: int, n: int, direction=None, stream: int = 0):
        """mi_point_sign_device on device pointers (n POINT records in, n bytes or n POINT_HIT records out), asynchronous on `stream`."""
        self._check(self._lib.mi_point_sign_device(self._h, int(kind), C.c_void_p(d_points), C.c_void_p(d_out), self._direction(direction),
                                                   int(n), C.c_void_p(stream)))

    def sdf(self, points, radius=float("inf"), direction=None) -> dict:
        """Torch convenience over mi_point_sign_device (SIGN_DISTANCE), like nearest: a float32 device tensor of shape [N, 3]
        (radius: a number or an [N] tensor), enqueued on torch.cuda.current_stream(). Returns device tensors: {"dist" [N], signed:
        negative inside, "inside" [N] bool, "prim_id" [N] int32, "geom_id" [N] int32 (-1 when nothing was found, for both),
        "point" [N, 3]}."""
        pts, n = self._torch_points("sdf", points, radius)
        raw = self._torch_records(pts, n, lambda d_pts, d_out, cnt, stream: self.point_sign_device(SIGN_DISTANCE, d_pts, d_out, cnt, direction, stream))
        cols = self._hit_columns(raw, "dist", "point")
        return {"dist": cols["dist"], "inside": (cols["flags"] & FLAG_INSIDE) != 0, "prim_id": cols["prim_id"], "geom_id": cols["geom_id"],
                "point": cols["point"]}

    # -- crossing lists (mi_list_offsets*, mi_list_fill*): every crossing of every ray, sorted along the ray ------------------------------
    def list_offsets(self, rays: np.ndarray) -> np.ndarray:
        """mi_list_offsets: a uint64 array of rays.size + 1 offsets - 0, then the running total of count_crossings(rays)."""
        return self._offsets_host(self._lib.mi_list_offsets, self._source(rays, RAY))

    def list_fill(self, rays: np.ndarray, offsets: np.ndarray, hits: np.ndarray, capacity: int | None = None) -> np.ndarray:
        """mi_list_fill: ray i's crossings, sorted, into hits[offsets[i]:offsets[i + 1]] (a CROSSING array at a 16-byte aligned
        address, see aligned_bytes), cut or padded to that length; nothing at or past `capacity` (None: hits.size) is written."""
        return self._fill_host(self._lib.mi_list_fill, CROSSING, self._source(rays, RAY), offsets, hits, capacity)

    def list_crossings(self, rays: np.ndarray):
        """Every surface each ray crosses with tMin < t < tMax (a RAY array, host memory), as (offsets, hits): offsets uint64
        [n + 1], hits a CROSSING array of offsets[n] records; hits[offsets[i]:offsets[i + 1]] are ray i's crossings in ascending
        order of t (then geomID, primID, a sphere's near root before its far root, which carries CROSS_FAR). The crossings are
        those count_crossings counts. Synchronous; batched by setRayBatch."""
        return self._all_lists(self.list_offsets, self.list_fill, CROSSING, rays)

    def first_crossings(self, rays: np.ndarray, k: int) -> np.ndarray:
        """The first k crossings of every ray in that order: a CROSSING array [n, k]; rays with fewer are padded with the empty
        record (t = +inf, INVALID_PRIM, INVALID_GEOM, FLAG_ESCAPED). One fill, no count pass."""
        return self._first_k(self.list_fill, CROSSING, rays, k)

    def list_offsets_device(self, d_rays: int, d_offsets: int, n: int, stream: int = 0):
        """mi_list_offsets_device on device pointers (n RAY records in, n + 1 uint64 out), asynchronous on `stream`."""
        self._check(self._lib.mi_list_offsets_device(self._h, C.c_void_p(d_rays), C.c_void_p(d_offsets), int(n), C.c_void_p(stream)))

    def list_fill_device(self, d_rays: int, d_offsets: int, d_hits: int, capacity: int, n: int, stream: int = 0):
        """mi_list_fill_device on device pointers (n RAY records and n + 1 uint64 in, `capacity` CROSSING records out), asynchronous
        on `stream`."""
        self._check(self._lib.mi_list_fill_device(self._h, C.c_void_p(d_rays), C.c_void_p(d_offsets), C.c_void_p(d_hits), int(capacity),
                                                  int(n), C.c_void_p(stream)))

    @staticmethod
    def _crossing_columns(raw):
        """The fields of [..., 4] int32 crossing records as tensors."""
        import torch
        halves = raw.view(torch.int16)
        return {"ray_ids": raw[..., 3].to(torch.int64) & 0xFFFFFFFF, "t": raw.view(torch.float32)[..., 0], "prim_id": raw[..., 1],
                "geom_id": halves[..., 4].to(torch.int32), "far": (halves[..., 5] & CROSS_FAR) != 0}

    def cast_all(self, origins, directions, t_min=0.0, t_max=float("inf")) -> dict:
        """Torch convenience over mi_list_offsets_device + mi_list_fill_device (Open3D's list_intersections): float32 device tensors
        of shape [N, 3] (t_min / t_max: numbers or [N] tensors), enqueued on torch.cuda.current_stream(). It runs the offsets,
        reads the total with one .item() (the one synchronisation), then allocates and fills. Returns device tensors: {"ray_splits"
        [N + 1] int64, and per crossing, ray by ray in ascending t: "ray_ids" int64, "t", "prim_id" int32, "geom_id" int32, "far"
        bool (a sphere's far root)}."""
        rays, n = self._torch_rays("cast_all", origins, directions, t_min, t_max)
        splits, raw = self._torch_all_lists(self.list_offsets_device, self.list_fill_device, rays, n, sync_when_empty=True)
        return {**self._crossing_columns(raw), "ray_splits": splits}

    def cast_first(self, origins, directions, k: int, t_min=0.0, t_max=float("inf")) -> dict:
        """The first k crossings of every ray, as cast_all's fields with shape [N, k] (no "ray_splits"): rays with fewer are padded
        with t = +inf and prim_id = geom_id = -1. One launch on torch.cuda.current_stream(), no synchronisation."""
        rays, n = self._torch_rays("cast_first", origins, directions, t_min, t_max)
        return self._crossing_columns(self._torch_first_k(self.list_fill_device, rays, n, k)[1])

    # -- geometry updates (mi_scene_update*): new primitive positions, the BVH refit on the device ------------------------------------
    def update_geometry(self, vertices=None, normals=None, spheres=None, discs=None) -> "IpuScene":
        """New positions for the scene's primitives, HOST arrays: VEC3 / SPHERE / DISC arrays or [n, 3] / [n, 4] / [n, 7] float32
        (None = keep; a given array has exactly the scene's count). Synchronous; work enqueued before sees the old geometry."""
        arrs = [_geometry_array(vertices, VEC3, 3), _geometry_array(normals, VEC3, 3), _geometry_array(spheres, SPHERE, 4),
                _geometry_array(discs, DISC, 7)]
        u = GeometryUpdate()
        for (ptr, cnt), a in zip((("mesh_verts", "num_verts"), ("mesh_normals", "num_normals"), ("spheres", "num_spheres"),
                                  ("discs", "num_discs")), arrs):
            if a is not None:
                setattr(u, ptr, a.ctypes.data)
                setattr(u, cnt, a.size)
        self._check(self._lib.mi_scene_update(self._h, C.byref(u)))
        return self

    def update_geometry_device(self, vertices=None, normals=None, spheres=None, discs=None) -> "IpuScene":
        """The same from contiguous float32 CUDA tensors ([n, 3] / [n, 3] / [n, 4] / [n, 7]), on torch.cuda.current_stream()."""
        import torch
        u = GeometryUpdate()
        keep = []
        dev = None
        for (ptr, cnt, width), t in zip((("mesh_verts", "num_verts", 3), ("mesh_normals", "num_normals", 3), ("spheres", "num_spheres", 4),
                                         ("discs", "num_discs", 7)), (vertices, normals, spheres, discs)):
            if t is None:
                continue
            if not t.is_cuda or t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != width or not t.is_contiguous():
                raise ValueError(f"update_geometry_device: {ptr} must be a contiguous float32 CUDA tensor of shape [n, {width}]")
            dev = t.device
            keep.append(t)
            setattr(u, ptr, t.data_ptr())
            setattr(u, cnt, t.shape[0])
        stream = torch.cuda.current_stream(dev).cuda_stream if dev is not None else 0
        self._check(self._lib.mi_scene_update_device(self._h, C.byref(u), C.c_void_p(stream)))
        return self

    # -- rigid poses (mi_scene_set_poses*): whole geometries moved by one transform each, posed on the device from a rest copy, then the refit --
    def set_poses(self, poses: np.ndarray) -> "IpuScene":
        """One POSE per entry of the scene's geometry list (HOST memory; query_batches.make_poses builds them), applied to the REST
        geometry - the scene's geometry at the first pose call after create, update_geometry*, set_geometry* or bake_poses -, never to
        the previous pose's result. Afterwards the scene is what update_geometry with pose_geometry_host's arrays leaves, bit for
        bit. Synchronous; work enqueued before sees the old geometry."""
        src = self._source(poses, POSE)
        self._check(self._lib.mi_scene_set_poses(self._h, src.ctypes.data if src.size else None, src.size))
        return self

    def set_poses_device(self, d_poses: int, n: int, stream: int = 0) -> "IpuScene":
        """mi_scene_set_poses_device on a device pointer (n POSE records, 16-byte aligned), on `stream`; synchronous."""
        self._check(self._lib.mi_scene_set_poses_device(self._h, C.c_void_p(d_poses), int(n), C.c_void_p(stream)))
        return self

    def poses(self) -> np.ndarray:
        """mi_scene_get_poses: the current pose of every geometry, a POSE array (identities until the first set_poses)."""
        n = C.c_uint32()
        self._check(self._lib.mi_scene_get_poses(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, POSE)
        self._check(self._lib.mi_scene_get_poses(self._h, out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out

    def bake_poses(self) -> "IpuScene":
        """mi_scene_bake_poses: the current geometry becomes the rest geometry, every pose the identity; moves no byte of the scene."""
        self._check(self._lib.mi_scene_bake_poses(self._h))
        return self

    def pose(self, quat, translation, scale=None) -> "IpuScene":
        """Torch convenience over mi_scene_set_poses_device: float32 device tensors quat [G, 4] (x, y, z, w; need not be unit),
        translation [G, 3] and scale [G] (None = 1), packed to [G, 8] on the device and enqueued on torch.cuda.current_stream()."""
        import torch
        q, t = quat, translation
        if not (q.is_cuda and t.is_cuda and q.dtype == torch.float32 and t.dtype == torch.float32 and q.ndim == 2 and t.ndim == 2 and q.shape[1] == 4 and
                t.shape[1] == 3 and q.shape[0] == t.shape[0]):
            raise ValueError("pose: quat [G, 4] and translation [G, 3] must be float32 CUDA tensors of one length")
        g = q.shape[0]
        if scale is None:
            s = torch.ones((g, 1), dtype=torch.float32, device=q.device)
        else:
            if not (scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == g):
                raise ValueError("pose: scale must be a float32 CUDA tensor of G elements")
            s = scale.reshape(g, 1)
        packed = torch.cat([q, t, s], dim=1).contiguous()      # [G, 8] = G mi_pose
        return self.set_poses_device(packed.data_ptr() if g else 0, g, stream=torch.cuda.current_stream(q.device).cuda_stream)

    def pose_timing(self) -> list:
        """mi_get_pose_timing: the last pose call's {pose pass, everything after it} in ms (zeros unless option "refit_timing" is 1)."""
        out = (C.c_double * 2)()
        self._check(self._lib.mi_get_pose_timing(self._h, out))
        return list(out)

    # -- new contents (mi_scene_set_geometry*): another geometry list, other meshes, other counts; the BVH built on the device ------------
    def set_geometry(self, desc: SceneDesc) -> int:
        """Replace the scene's contents by desc's nine arrays (HOST memory; desc's nodes and render parameters are ignored) and
        build their LBVH on the device (build_lbvh is its host twin). Options, counters, the NIF environment and the render
        parameters stay. Synchronous; work enqueued before sees the old contents. Returns the maximal leaf depth (root = 1)."""
        g = SceneGeometry.from_desc(desc)
        depth = C.c_uint32()
        self._check(self._lib.mi_scene_set_geometry(self._h, C.byref(g), C.byref(depth)))
        return depth.value

    def set_geometry_device(self, desc: SceneDesc, tris=None, vertices=None, normals=None, spheres=None, discs=None, stream=None) -> int:
        """The same with the data plane in contiguous CUDA tensors: tris int16 / uint16 [T, 3], vertices and normals float32 [n, 3],
        spheres float32 [n, 4], discs float32 [n, 7] (None = none of that kind). The control plane - geometry, mesh_info, mat_ids,
        materials - is taken from desc (host memory). On `stream` (a raw hipStream_t as an int), default torch.cuda.current_stream()."""
        import torch
        g = SceneGeometry.from_desc(desc)
        keep = []
        dev = None
        for ptr, cnt, width, t in (("mesh_tris", "num_tris", 3, tris), ("mesh_verts", "num_verts", 3, vertices), ("mesh_normals", "num_normals", 3, normals),
                                   ("spheres", "num_spheres", 4, spheres), ("discs", "num_discs", 7, discs)):
            setattr(g, ptr, None)
            setattr(g, cnt, 0)
            if t is None:
                continue
            dtypes = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None) if ptr == "mesh_tris" else (torch.float32,)
            if not t.is_cuda or t.dtype not in dtypes or t.ndim != 2 or t.shape[1] != width or not t.is_contiguous():
                kind = "16-bit integer" if ptr == "mesh_tris" else "float32"
                raise ValueError(f"set_geometry_device: {ptr} must be a contiguous {kind} CUDA tensor of shape [n, {width}]")
            dev = t.device
            keep.append(t)
            if t.shape[0]:
                setattr(g, ptr, t.data_ptr())
            setattr(g, cnt, t.shape[0])
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream if dev is not None else 0
        depth = C.c_uint32()
        self._check(self._lib.mi_scene_set_geometry_device(self._h, C.byref(g), C.c_void_p(stream), C.byref(depth)))
        return depth.value

    def rebuild_bvh(self, stream=None) -> int:
        """mi_scene_rebuild: a new BVH topology from the scene's current geometry, built on the device (an LBVH; build_lbvh is its
        host twin). `stream`: a raw hipStream_t as an int, default torch.cuda.current_stream() when torch is loaded, else the
        null stream. Synchronous. Returns the maximal leaf depth (root = 1)."""
        depth = C.c_uint32()
        self._check(self._lib.mi_scene_rebuild(self._h, C.c_void_p(self._stream(stream)), C.byref(depth)))
        return depth.value

    def rebuild_timing(self) -> list:
        """mi_get_rebuild_timing: the last rebuild's pass times in ms (zeros unless option "rebuild_timing" is 1)."""
        out = (C.c_double * 6)()
        self._check(self._lib.mi_get_rebuild_timing(self._h, out))
        return list(out)

    def _stream(self, stream):
        if stream is None:
            import sys
            torch = sys.modules.get("torch")
            stream = torch.cuda.current_stream().cuda_stream if torch is not None and torch.cuda.is_available() else 0
        return stream

    def bvh_cost(self, stream=None) -> dict:
        """mi_scene_bvh_cost: the surface-area cost of the scene's current BVH, summed on the device (bvh_cost is its host twin,
        bit for bit). `stream` as for rebuild_bvh. Keys as bvh_cost's."""
        out = (C.c_double * 3)()
        self._check(self._lib.mi_scene_bvh_cost(self._h, C.c_void_p(self._stream(stream)), out))
        return _cost_dict(out)

    def live_stats(self) -> dict:
        """mi_get_live_stats: what updates and rebuilds have done to this scene so far."""
        out = (C.c_uint64 * 8)()
        self._check(self._lib.mi_get_live_stats(self._h, out))
        return dict(zip(("updates_applied", "updates_refused", "rebuilds", "auto_rebuilds", "host_derivations", "cost_evaluations",
                         "max_leaf_depth", "geometry_sets"), (int(x) for x in out)))

    def bvh_nodes(self) -> np.ndarray:
        """The scene's current compact BVH nodes (mi_scene_get_bvh): a BVH_NODE array."""
        n = C.c_uint32()
        self._check(self._lib.mi_scene_get_bvh(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=BVH_NODE)
        self._check(self._lib.mi_scene_get_bvh(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out

    def nif_infer_device(self, d_u: int, d_v: int, d_bgr: int, n: int, stream: int = 0):
        self._check(self._lib.mi_nif_infer_device(self._h, C.c_void_p(d_u), C.c_void_p(d_v), C.c_void_p(d_bgr), n, C.c_void_p(stream)))

    def counters(self) -> dict:
        c = (C.c_uint64 * 4)()
        self._check(self._lib.mi_get_counters(self._h, c))
        return {"casts": c[0], "nodes_visited": c[1], "leaf_tests": c[2], "paths": c[3]}

    def phase_stats(self) -> dict:
        c = (C.c_uint64 * 12)()
        self._check(self._lib.mi_get_phase_stats(self._h, c))
        names = ("node", "leaf", "shade", "gen")
        out = {n: {"iters": c[2 * i], "lanes": c[2 * i + 1]} for i, n in enumerate(names)}
        out["cycles"] = {"traverse": c[8], "shade": c[9], "gen": c[10], "total": c[11]}
        return out

    def pool_stats(self) -> dict:
        c = (C.c_uint64 * 8)()
        self._check(self._lib.mi_get_pool_stats(self._h, c))
        return dict(zip(("loops", "refill_turns", "refill_lanes", "idle", "lost_claims", "bursts", "burst_lanes", "refill_cycles"), [int(x) for x in c]))

    def hot_stats(self) -> dict:
        """What the instrumented build (option full_stats) counted of plain renders that walked the private, hot-first copy (option
        hot_nodes): box-test steps that ran from LDS and the lanes in them, the steps of runs that ran from global memory and their
        lanes, and the box tests of nodes inside the staged prefix. All zero while such a render has not run."""
        c = (C.c_uint64 * 5)()
        self._check(self._lib.mi_get_hot_stats(self._h, c))
        return dict(zip(("lds_steps", "lds_lanes", "global_steps", "global_lanes", "hot_visits"), [int(x) for x in c]))

    def launch_progress(self, d_samples: int, n: int, period_ticks: int, stream: int = 0) -> None:
        """mi_debug_launch_progress: one wave samples the work counter of `stream`'s persistent launches n times, period_ticks
        (100-MHz ticks) apart, into 2 n uint64 of device memory at d_samples. Call right before run_device on `stream`."""
        self._check(self._lib.mi_debug_launch_progress(self._h, C.c_void_p(stream), C.c_void_p(d_samples), n, period_ticks))

    def nif_timing(self) -> dict:
        """Milliseconds in MLP launches (and their number) since the last call; needs set_option("nif_timing", 1)."""
        c = (C.c_double * 2)()
        self._check(self._lib.mi_get_nif_timing(self._h, c))
        return {"mlp_ms": float(c[0]), "launches": int(c[1])}

    def nif_clock_ghz(self):
        """The shader clock the last K3a launch ran at (mi_get_nif_clock), None when the network runs nif_mlp_kernel."""
        c = (C.c_uint64 * 2)()
        self._check(self._lib.mi_get_nif_clock(self._h, c))
        return (c[0] / c[1] * 0.1) if c[1] else None

    def reset_counters(self):
        self._check(self._lib.mi_reset_counters(self._h))

    def close(self):
        if self._h:
            self._lib.mi_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The touch families' IpuScene methods: one implementation per kind, bound under each family's names (_TOUCH_FAMILIES).
def _touch_query(fam, self, kind: int, items: np.ndarray, out: np.ndarray) -> np.ndarray:
    src = self._source(items, fam.item)
    self._check(getattr(self._lib, fam.c("query"))(self._h, kind, src.ctypes.data, out.ctypes.data, src.size))
    return out


def _touch_any(fam, self, items: np.ndarray) -> np.ndarray:
    return _touch_query(fam, self, _TOUCH_ANY, items, aligned_bytes(items.size)).view(np.bool_)


def _touch_count(fam, self, items: np.ndarray) -> np.ndarray:
    return _touch_query(fam, self, _TOUCH_COUNT, items, np.zeros(items.size, np.uint32))


def _touch_offsets(fam, self, items: np.ndarray) -> np.ndarray:
    return self._offsets_host(getattr(self._lib, fam.c("offsets")), self._source(items, fam.item))


def _touch_fill(fam, self, items: np.ndarray, offsets: np.ndarray, hits: np.ndarray, capacity: int | None = None) -> np.ndarray:
    return self._fill_host(getattr(self._lib, fam.c("fill")), fam.record, self._source(items, fam.item), offsets, hits, capacity)


def _touch_list(fam, self, items: np.ndarray):
    return self._all_lists(lambda i: _touch_offsets(fam, self, i), lambda *a: _touch_fill(fam, self, *a), fam.record, items)


def _touch_first(fam, self, items: np.ndarray, k: int) -> np.ndarray:
    return self._first_k(lambda *a: _touch_fill(fam, self, *a), fam.record, items, k)


def _touch_query_device(fam, self, kind: int, d_items: int, d_out: int, n: int, stream: int = 0):
    self._check(getattr(self._lib, fam.c("query_device"))(self._h, int(kind), C.c_void_p(d_items), C.c_void_p(d_out), int(n), C.c_void_p(stream)))


def _touch_offsets_device(fam, self, d_items: int, d_offsets: int, n: int, stream: int = 0):
    self._check(getattr(self._lib, fam.c("offsets_device"))(self._h, C.c_void_p(d_items), C.c_void_p(d_offsets), int(n), C.c_void_p(stream)))


def _touch_fill_device(fam, self, d_items: int, d_offsets: int, d_hits: int, capacity: int, n: int, stream: int = 0):
    self._check(getattr(self._lib, fam.c("fill_device"))(self._h, C.c_void_p(d_items), C.c_void_p(d_offsets), C.c_void_p(d_hits), int(capacity), int(n),
                                                         C.c_void_p(stream)))


_TOUCH_METHODS = (      # the public name ({p}: the prefix; a bare word: the row's field), implementation, docstring
    ("any", _touch_any,
     """mi_{p}_query ({ITEM}_ANY): whether some primitive touches each {one} ({a_ITEM} array, host memory; contact counts): a bool
        array. Synchronous; batched by setRayBatch."""),
    ("count", _touch_count,
     """mi_{p}_query ({ITEM}_COUNT): how many primitives touch each {one} ({a_ITEM} array, host memory): a uint32 array."""),
    ("{p}_offsets", _touch_offsets,
     """mi_{p}_offsets: a uint64 array of {arg}.size + 1 offsets - 0, then the running total of {count}({arg})."""),
    ("{p}_fill", _touch_fill,
     """mi_{p}_fill: the primitives touching {one} i, ascending in (geomID, primID), into hits[offsets[i]:offsets[i + 1]] ({a_REC}
        array at a 16-byte aligned address, see aligned_bytes), cut or padded to that length; nothing at or past `capacity`
        (None: hits.size) is written."""),
    ("list", _touch_list,
     """mi_{p}_offsets, then mi_{p}_fill: every primitive that touches each {one} ({a_ITEM} array, host memory), as (offsets, recs):
        offsets uint64 [n + 1], recs {a_REC} array of offsets[n] records; recs[offsets[i]:offsets[i + 1]] are {one} i's primitives in
        ascending order of (geomID, primID){contained}. Synchronous; batched by setRayBatch."""),
    ("first", _touch_first,
     """mi_{p}_fill alone: the k smallest (geomID, primID) of the primitives touching each {one}: {a_REC} array [n, k]; {noun} with
        fewer are padded with the empty record (INVALID_PRIM, INVALID_GEOM, FLAG_ESCAPED). One fill, no count pass."""),
    ("{p}_query_device", _touch_query_device,
     """mi_{p}_query_device on device pointers (n {ITEM} records in, n bytes or n uint32 out), asynchronous on `stream`."""),
    ("{p}_offsets_device", _touch_offsets_device,
     """mi_{p}_offsets_device on device pointers (n {ITEM} records in, n + 1 uint64 out), asynchronous on `stream`."""),
    ("{p}_fill_device", _touch_fill_device,
     """mi_{p}_fill_device on device pointers (n {ITEM} records and n + 1 uint64 in, `capacity` {REC} records out), asynchronous
        on `stream`."""),
)
for _fam in _TOUCH_FAMILIES:
    for _name, _impl, _doc in _TOUCH_METHODS:
        _name = _name.format(p=_fam.prefix) if "{" in _name else getattr(_fam, _name)
        setattr(IpuScene, _name, _bound(_impl, _fam, _name, _doc, "IpuScene."))


class _BorrowedScene(IpuScene):
    """A replica's scene handle inside an IpuGroup (owned by the group: never destroyed from here)."""

    def __init__(self, handle, desc, lib=None):
        self._lib = lib if lib is not None else device_lib()
        self._h = C.c_void_p(handle)
        self.desc = desc

    def close(self):
        self._h = C.c_void_p()


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_COPY = 0, 1, 2


class IpuGroup:
    """An IpuScene with numReplicas > 1 (RuntimeConfig, trace.cpp:297-309) in ONE process: a scene replica per entry
    of `devices` (ordinals may repeat), the host ray stream dealt to them in 8-row bands, one RCCL gather to the first
    replica's device at frame end (mi_group_* in include/mi_raylib.h)."""

    def __init__(self, desc: SceneDesc, devices, transport: int = TRANSPORT_AUTO, variants: bool = False):
        self._lib = device_lib(variants)
        self._h = C.c_void_p()
        self.desc = desc
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        self._check(self._lib.mi_group_create(C.byref(desc), dv.ctypes.data, dv.size, int(transport), C.byref(self._h)))

    _check = IpuScene._check

    def scenes(self):
        return [_BorrowedScene(self._lib.mi_group_scene(self._h, i), self.desc, self._lib) for i in range(self._lib.mi_group_size(self._h))]

    def setRayBatch(self, rays_per_batch: int):
        self._check(self._lib.mi_group_set_ray_batch(self._h, int(rays_per_batch)))

    # The NIF model and its settings go to EVERY replica, as the reference streams the weights to every replica of the
    # replicated graph (src/IpuScene.cpp:535) - what mi::IpuScene::configure does in the C++ host (csrc/host/IpuScene.hpp).
    def setNif(self, kernels, biases, relu, embedding_dimension, max_value, mean, log_tonemap=True):
        for sc in self.scenes():
            sc.setNif(kernels, biases, relu, embedding_dimension, max_value, mean, log_tonemap)

    def loadNifModel(self, asset_path) -> bool:
        return all(sc.loadNifModel(asset_path) for sc in self.scenes())

    def setHdriRotation(self, degrees: float):
        for sc in self.scenes():
            sc.setHdriRotation(degrees)

    def set_option(self, key: str, value) -> "IpuGroup":
        for sc in self.scenes():
            sc.set_option(key, value)
        return self

    def run(self, rays: np.ndarray, mode: int | None = None, callback=None) -> np.ndarray:
        assert rays.dtype == TRACE_RESULT and rays.flags["C_CONTIGUOUS"]
        if mode is None:
            mode = MODE_PATH_TRACE if self.desc.path_trace else MODE_SHADOW_TRACE
        cb = None
        if callback is not None:
            base = rays.ctypes.data
            proto = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t)
            cb = proto(lambda user, idx, ptr, cnt: callback(idx, (ptr - base) // TRACE_RESULT.itemsize, cnt))
        self._check(self._lib.mi_group_render(self._h, mode, rays.ctypes.data, rays.size, cb, None))
        return rays

    def getTraceTimeSecs(self) -> float:
        return float(self._lib.mi_group_trace_time_secs(self._h))

    def counters(self) -> dict:
        c = (C.c_uint64 * 4)()
        self._check(self._lib.mi_group_get_counters(self._h, c))
        return {"casts": c[0], "nodes_visited": c[1], "leaf_tests": c[2], "paths": c[3]}

    def last_transfer(self) -> dict:
        c = (C.c_uint64 * 5)()
        self._check(self._lib.mi_group_last_transfer(self._h, c))
        return {"rccl_messages": c[0], "peer_copies": c[1], "bands": c[2], "upload_copies": c[3], "download_copies": c[4]}

    def last_gather_ms(self) -> float:
        """Milliseconds the last batch's gather took as the first replica's device saw it (HIP events on its stream)."""
        ms = C.c_double()
        self._check(self._lib.mi_group_last_gather_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def devices(self):
        """The distinct device ordinals of the group's communicator, root first (RCCL ranks when the transport is RCCL)."""
        n = C.c_uint32()
        buf = np.zeros(64, np.int32)
        self._check(self._lib.mi_group_devices(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return [int(x) for x in buf[:n.value]]

    # -- the stages one by one: the shares stay resident on the devices between calls --
    def upload(self, rays: np.ndarray):
        assert rays.dtype == TRACE_RESULT and rays.flags["C_CONTIGUOUS"]
        self._check(self._lib.mi_group_upload(self._h, rays.ctypes.data, rays.size))

    def trace(self, mode: int = MODE_PATH_TRACE):
        self._check(self._lib.mi_group_trace(self._h, mode))

    def download(self, rays: np.ndarray) -> np.ndarray:
        assert rays.dtype == TRACE_RESULT and rays.flags["C_CONTIGUOUS"]
        self._check(self._lib.mi_group_download(self._h, rays.ctypes.data, rays.size))
        return rays

    def gathered_device(self):
        """(device pointer of the gathered shares on the first replica's device, first record of every replica's share)"""
        ptr = C.c_void_p()
        n = self._lib.mi_group_size(self._h)
        off = (C.c_uint64 * (n + 1))()
        self._check(self._lib.mi_group_gathered_device(self._h, C.byref(ptr), off, n + 1))
        return ptr.value, [int(x) for x in off]

    def reset_counters(self):
        self._check(self._lib.mi_group_reset_counters(self._h))

    def close(self):
        if self._h:
            self._lib.mi_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
