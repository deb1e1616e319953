// scene_api.cpp — C ABI of the host scene plumbing (include/mi_scene_host.h).
#include <algorithm>
#include <cstring>
#include <vector>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../../include/mi_scene_host.h"
#include "scene_types.hpp"
#include "../scene_blob.hpp"
#include "../ray_shard.hpp"
#include "../bvh_cost_host.hpp"
#include "../canon_prims.hpp"
#include "touch_host.hpp"
#include "../contact_math.hpp"
#include "../obox_math.hpp"
#include "../capsule_math.hpp"
#include "../frustum_math.hpp"

using namespace mi;
using namespace mi::host;

struct mi_host_scene {
  PackedScene packed;
};

namespace {
thread_local std::string g_err;

template <class F>
int guarded(F&& f) {
  try { f(); g_err.clear(); return MI_OK; }
  catch (const std::invalid_argument& e) { g_err = e.what(); return MI_ERR_INVALID_ARG; }
  catch (const std::exception& e) { g_err = e.what(); return MI_ERR_IO; }
}

// The entries of a touch family's twins (touch_host.hpp), one body each; S: the family's shape, fn: the C entry's name.
bool twinArgsBad(const char* fn, const void* desc, const char* kindBad, bool nullBuffer) {
  const char* why = !desc ? "null scene description" : kindBad ? kindBad : nullBuffer ? "null buffer" : nullptr;
  if (why) g_err = std::string(fn) + ": " + why;
  return why != nullptr;
}
template <class S>
int touchQueryTwin(const char* fn, const mi_scene_desc* desc, int kind, const typename S::Item* items, void* out, size_t n, uint64_t* visits) {
  if (twinArgsBad(fn, desc, kind != S::kAny && kind != S::kCount ? S::kKindBad : nullptr, n && (!items || !out))) return MI_ERR_INVALID_ARG;
  return guarded([&] { touchQueryHost<S>(*desc, fn, kind, items, out, n, visits); });
}
template <class S>
int touchOffsetsTwin(const char* fn, const mi_scene_desc* desc, const typename S::Item* items, uint64_t* offsets, size_t n, uint64_t* visits) {
  if (twinArgsBad(fn, desc, nullptr, n && (!items || !offsets))) return MI_ERR_INVALID_ARG;
  return guarded([&] { touchOffsetsHost<S>(*desc, fn, items, offsets, n, visits); });
}
template <class S>
int touchFillTwin(const char* fn, const mi_scene_desc* desc, const typename S::Item* items, const uint64_t* offsets, typename S::Record* hits, size_t capacity, size_t n,
                  uint64_t* visits) {
  if (twinArgsBad(fn, desc, nullptr, n && (!items || !offsets || !hits))) return MI_ERR_INVALID_ARG;
  return guarded([&] { touchFillHost<S>(*desc, fn, items, offsets, hits, capacity, n, visits); });
}
// (no error text: 0 for a null argument, as for an item that is not walked)
template <class S>
int touchMeetsBoundsTwin(const typename S::Item* item, const float mn[3], const float mx[3]) {
  if (!item || !mn || !mx) return 0;
  typename S::Item q;
  memcpy(&q, item, sizeof q);
  return touchMeetsBoundsHost<S>(q, mn, mx) ? 1 : 0;
}
}  // namespace

extern "C" {

const char* mi_host_last_error(void) { return g_err.c_str(); }

int mi_host_scene_builtin(const char* scene_name, const char* mesh_file, mi_host_scene** out) {
  if (!scene_name || !out) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    const std::string name(scene_name);
    SceneDescription desc;
    if (name == "box-simple" || name == "box") desc = makeCornellBoxScene(mesh_file ? mesh_file : "", name == "box-simple");
    else if (name == "spheres") desc = makePrimitiveScene();
    else if (name == "monkey") desc = makeMonkeyScene(mesh_file ? mesh_file : "");
    else throw std::invalid_argument("Invalid scene selection: '" + name + "'");   // src/app_utils.cpp:268-270
    auto* hs = new mi_host_scene;
    hs->packed = packScene(desc);
    *out = hs;
  });
}

int mi_host_scene_import(const char* file, int load_normals, mi_host_scene** out) {
  if (!file || !out) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    const std::string path(file);
    const std::string ext = path.size() >= 4 ? path.substr(path.size() - 4) : "";
    SceneDescription desc;
    if (ext == ".dae" || ext == ".DAE") desc = importColladaScene(path, load_normals != 0);
    else if (ext == ".glb") { loadGlbMeshes(path, false); throw std::runtime_error("No camera found in scene file."); }   // scene_utils.cpp:177-180
    else throw std::runtime_error("Could not load scene file.");
    auto* hs = new mi_host_scene;
    hs->packed = packScene(desc);
    *out = hs;
  });
}

int mi_host_scene_from_arrays(const mi_scene_desc* g, mi_host_scene** out) {
  if (!g || !out) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    // before anything is copied or built (packScene would refuse it too, after the copies)
    if ((uint64_t)g->num_meshes + g->num_spheres + g->num_discs > kMaxGeometries)
      throw std::invalid_argument(std::string("mi_host_scene_from_arrays: ") + kTooManyGeometries);
    SceneDescription d;
    for (uint32_t m = 0; m < g->num_meshes; ++m) {
      const mi_mesh_info& mi_ = g->mesh_info[m];
      TriMesh tm;
      tm.indices.assign(g->mesh_tris + 3 * (size_t)mi_.first_index, g->mesh_tris + 3 * (size_t)(mi_.first_index + mi_.num_triangles));
      for (uint32_t v = 0; v < mi_.num_vertices; ++v) {
        const mi_vec3& p = g->mesh_verts[mi_.first_vertex + v];
        tm.vertices.push_back(mk(p.x, p.y, p.z));
        if (g->num_normals) { const mi_vec3& n = g->mesh_normals[mi_.first_vertex + v]; tm.normals.push_back(mk(n.x, n.y, n.z)); }
      }
      d.meshes.push_back(std::move(tm));
    }
    d.spheres.assign(g->spheres, g->spheres + g->num_spheres);
    d.discs.assign(g->discs, g->discs + g->num_discs);
    d.materials.assign(g->materials, g->materials + g->num_materials);
    d.matIDs.assign(g->mat_ids, g->mat_ids + g->num_mat_ids);
    if (d.matIDs.size() < d.meshes.size() + d.spheres.size() + d.discs.size())
      throw std::invalid_argument("All primitives must be assigned a material.");
    d.horizontalFov = g->fov_radians;
    auto* hs = new mi_host_scene;
    hs->packed = packScene(d);
    *out = hs;
  });
}

int mi_host_scene_fill_desc(const mi_host_scene* scene, mi_scene_desc* desc) {
  if (!scene || !desc) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  const PackedScene& p = scene->packed;
  memset(desc, 0, sizeof *desc);
  desc->geometry = p.geometry.data();       desc->num_geometry = (uint32_t)p.geometry.size();
  desc->mesh_info = p.meshInfo.data();      desc->num_meshes = (uint32_t)p.meshInfo.size();
  desc->mesh_tris = p.meshTris.data();      desc->num_tris = (uint32_t)(p.meshTris.size() / 3);
  desc->mesh_verts = p.meshVerts.data();    desc->num_verts = (uint32_t)p.meshVerts.size();
  desc->mesh_normals = p.meshNormals.data();desc->num_normals = (uint32_t)p.meshNormals.size();
  desc->mat_ids = p.matIDs.data();          desc->num_mat_ids = (uint32_t)p.matIDs.size();
  desc->materials = p.materials.data();     desc->num_materials = (uint32_t)p.materials.size();
  desc->bvh_nodes = p.bvhNodes.data();      desc->num_nodes = (uint32_t)p.bvhNodes.size();
  desc->max_leaf_depth = p.bvhMaxDepth;
  desc->spheres = p.spheres.data();         desc->num_spheres = (uint32_t)p.spheres.size();
  desc->discs = p.discs.data();             desc->num_discs = (uint32_t)p.discs.size();
  // CLI defaults, trace.cpp:343-366
  desc->image_width = 768.f; desc->image_height = 432.f;
  desc->fov_radians = p.horizontalFov;
  desc->anti_alias_scale = .25f;
  desc->max_path_length = 10; desc->roulette_start_depth = 3; desc->samples_per_pixel = 256;
  desc->rng_seed = 1442;
  desc->window_w = 768; desc->window_h = 432; desc->window_c = 0; desc->window_r = 0;
  desc->path_trace = 1;
  desc->device = 0;
  return MI_OK;
}

void mi_host_scene_destroy(mi_host_scene* scene) { delete scene; }

int mi_build_compact_bvh(const float* lower, const float* upper, const uint16_t* geom_ids,
                         const uint32_t* prim_ids, uint32_t n,
                         mi_bvh_node* nodes, uint32_t* num_nodes, uint32_t* max_leaf_depth) {
  if (!lower || !upper || !geom_ids || !prim_ids || !nodes || !num_nodes || !max_leaf_depth) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    std::vector<BuildPrim> prims(n);
    for (uint32_t i = 0; i < n; ++i) {
      prims[i].box.lo = mk(lower[3 * i], lower[3 * i + 1], lower[3 * i + 2]);
      prims[i].box.hi = mk(upper[3 * i], upper[3 * i + 1], upper[3 * i + 2]);
      prims[i].geomID = geom_ids[i]; prims[i].primID = prim_ids[i];
    }
    std::vector<mi_bvh_node> out;
    uint32_t depth = 0;
    buildCompactBvh(prims, out, depth);
    memcpy(nodes, out.data(), out.size() * sizeof(mi_bvh_node));
    *num_nodes = (uint32_t)out.size();
    *max_leaf_depth = depth;
  });
}

int mi_refit_compact_bvh(const mi_scene_desc* desc, mi_bvh_node* out) {
  if (!desc || (!out && desc->num_nodes)) { g_err = "mi_refit_compact_bvh: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { refitCompactBvh(*desc, out); });
}

int mi_build_lbvh_compact(const mi_scene_desc* desc, mi_bvh_node* out, uint32_t* num_nodes, uint32_t* max_leaf_depth) {
  if (!desc || !out || !num_nodes || !max_leaf_depth) { g_err = "mi_build_lbvh_compact: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    std::vector<mi_bvh_node> nodes;
    uint32_t depth = 0;
    buildLbvhCompact(*desc, nodes, depth);
    if (!nodes.empty()) memcpy(out, nodes.data(), nodes.size() * sizeof(mi_bvh_node));
    *num_nodes = (uint32_t)nodes.size();
    *max_leaf_depth = depth;
  });
}

// Point queries: the host twin of mi_point_query / mi_point_query_device (point_query_host.cpp)
int mi_point_query_host(const mi_scene_desc* desc, int kind, const mi_point* points, void* out, size_t n, uint64_t visits[2]) {
  if (!desc) { g_err = "mi_point_query_host: null scene description"; return MI_ERR_INVALID_ARG; }
  if (kind != MI_POINT_CLOSEST && kind != MI_POINT_WITHIN) { g_err = "mi_point_query_host: unknown query kind"; return MI_ERR_INVALID_ARG; }
  if (n && (!points || !out)) { g_err = "mi_point_query_host: null buffer"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { pointQueryHost(*desc, kind, points, out, n, visits); });
}

// Neighbour lists: the host twins of mi_near_offsets* / mi_near_fill* (point_query_host.cpp)
int mi_near_offsets_host(const mi_scene_desc* desc, const mi_point* points, uint64_t* offsets, size_t n, uint64_t visits[2]) {
  if (!desc) { g_err = "mi_near_offsets_host: null scene description"; return MI_ERR_INVALID_ARG; }
  if (n && (!points || !offsets)) { g_err = "mi_near_offsets_host: null buffer"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { nearOffsetsHost(*desc, points, offsets, n, visits); });
}

int mi_near_fill_host(const mi_scene_desc* desc, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits, size_t capacity, size_t n, uint64_t visits[2]) {
  if (!desc) { g_err = "mi_near_fill_host: null scene description"; return MI_ERR_INVALID_ARG; }
  if (n && (!points || !offsets || !hits)) { g_err = "mi_near_fill_host: null buffer"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { nearFillHost(*desc, points, offsets, hits, capacity, n, visits); });
}

// Touch queries: the host twins of mi_X_query* / mi_X_offsets* / mi_X_fill* and, where the family has one, the node test alone.
// The bodies are the templates above; a family is its shape.
#define MI_TOUCH_TWINS(X, S)                                                                                                                            \
  int mi_##X##_query_host(const mi_scene_desc* desc, int kind, const S::Item* items, void* out, size_t n, uint64_t visits[2]) {                         \
    return touchQueryTwin<S>("mi_" #X "_query_host", desc, kind, items, out, n, visits);                                                                \
  }                                                                                                                                                     \
  int mi_##X##_offsets_host(const mi_scene_desc* desc, const S::Item* items, uint64_t* offsets, size_t n, uint64_t visits[2]) {                         \
    return touchOffsetsTwin<S>("mi_" #X "_offsets_host", desc, items, offsets, n, visits);                                                              \
  }                                                                                                                                                     \
  int mi_##X##_fill_host(const mi_scene_desc* desc, const S::Item* items, const uint64_t* offsets, S::Record* hits, size_t capacity, size_t n,          \
                         uint64_t visits[2]) {                                                                                                          \
    return touchFillTwin<S>("mi_" #X "_fill_host", desc, items, offsets, hits, capacity, n, visits);                                                    \
  }
MI_TOUCH_TWINS(box, BoxShape)
MI_TOUCH_TWINS(tri, TriShape)
MI_TOUCH_TWINS(obox, OBoxShape)
MI_TOUCH_TWINS(capsule, CapsuleShape)
MI_TOUCH_TWINS(frustum, FrustumShape)
#undef MI_TOUCH_TWINS
int mi_obox_meets_bounds_host(const mi_obox* obox, const float mn[3], const float mx[3]) { return touchMeetsBoundsTwin<OBoxShape>(obox, mn, mx); }
int mi_capsule_meets_bounds_host(const mi_capsule* capsule, const float mn[3], const float mx[3]) { return touchMeetsBoundsTwin<CapsuleShape>(capsule, mn, mx); }
int mi_frustum_meets_bounds_host(const mi_frustum* frustum, const float mn[3], const float mx[3]) { return touchMeetsBoundsTwin<FrustumShape>(frustum, mn, mx); }

// Rigid poses: the host twin of the pose pass of mi_scene_set_poses* (pose_host.cpp)
int mi_pose_geometry_host(const mi_scene_desc* rest, const mi_pose* poses, uint32_t num_geometry, mi_vec3* verts_out, mi_vec3* normals_out,
                          mi_sphere* spheres_out, mi_disc* discs_out) {
  if (!rest) { g_err = "mi_pose_geometry_host: null scene description"; return MI_ERR_INVALID_ARG; }
  if (num_geometry && !poses) { g_err = "mi_pose_geometry_host: null poses"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { poseGeometryHost(*rest, poses, num_geometry, verts_out, normals_out, spheres_out, discs_out); });
}

// The canonical primitive table of desc's arrays: the host twin of canon_prim_kernel (canon_kernels.hpp, mi_scene_set_geometry*) -
// the same prefix, the same search and record per canonical index (canon_prims.hpp), the same checks with mi_scene_create's words
int mi_canonical_prims(const mi_scene_desc* desc, void* out, uint32_t capacity, uint32_t* count) {
  if (!desc || !count) { g_err = "mi_canonical_prims: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    auto need = [](bool ok, const char* what) { if (!ok) throw std::invalid_argument(std::string("mi_canonical_prims: ") + what); };
    const mi_scene_geometry g = canon_geometry_of(*desc);
    canon_check_control(g, 1u << 26, need);
    std::vector<uint32_t> primStart((size_t)g.num_geometry + 1);
    const uint32_t P = canon_prim_starts(g, primStart.data());
    *count = P;
    if (!out && !capacity) return;                       // only the count
    need(out && capacity >= P, "capacity is smaller than the scene's primitive count");
    RebuildPrim* prims = (RebuildPrim*)out;
    for (uint32_t p = 0; p < P; ++p) {
      RebuildPrim q;
      need(canon_prim(p, primStart.data(), g.num_geometry, g.geometry, g.mesh_info, g.mat_ids, g.mesh_tris, q), "triangle vertex index out of range");
      memcpy(&prims[p], &q, sizeof q);                   // (the caller's buffer need not be 16-byte aligned)
    }
  });
}

// The surface-area cost of a tree of compact nodes: the host twin of mi_scene_bvh_cost (bvh_cost_host.hpp)
int mi_bvh_cost_compact_block(const mi_bvh_node* nodes, uint32_t n, uint32_t block, double out[3]) {
  if (!out || (!nodes && n)) { g_err = "mi_bvh_cost_compact: null argument"; return MI_ERR_INVALID_ARG; }
  if (block < 2 || (block & (block - 1))) { g_err = "mi_bvh_cost_compact_block: the block width is a power of two, at least 2"; return MI_ERR_INVALID_ARG; }
  return guarded([&] { bvh_cost_host(nodes, n, block, out); });
}
int mi_bvh_cost_compact(const mi_bvh_node* nodes, uint32_t n, double out[3]) { return mi_bvh_cost_compact_block(nodes, n, kCostBlock, out); }
double mi_bvh_cost_estimate(const double cost[3]) { return cost ? bvh_cost_estimate(cost) : 0.0; }

// initPerspectiveRayStream with gen == nullptr, then zeroRgb (src/app_utils.cpp:19-53)
int mi_init_ray_stream(const mi_scene_desc* d, mi_trace_result* rays, size_t capacity) {
  if (!d || !rays) { g_err = "null argument"; return MI_ERR_INVALID_ARG; }
  if (d->window_w < 0 || d->window_h < 0 || capacity < (size_t)d->window_w * (size_t)d->window_h) { g_err = "ray buffer smaller than the render window"; return MI_ERR_INVALID_ARG; }
  float s, c;
  sincos_deg_table(d->fov_radians / 2.f, sinTable(), s, c);
  const float tanTheta = s / c;
  size_t i = 0;
  for (uint32_t r = (uint32_t)d->window_r; r < (uint32_t)(d->window_r + d->window_h); ++r)
    for (uint32_t col = (uint32_t)d->window_c; col < (uint32_t)(d->window_c + d->window_w); ++col) {
      const f3 dir = pixel_to_ray_dir((float)col, (float)r, d->image_width, d->image_height, tanTheta);
      mi_trace_result& t = rays[i++];
      memset(&t, 0, sizeof t);
      t.u = (float)r; t.v = (float)col;
      t.h.r.t_min = 0.f; t.h.r.t_max = std::numeric_limits<float>::infinity();
      t.h.r.direction = {dir.x, dir.y, dir.z};
      t.h.prim_id = MI_INVALID_PRIM;
      t.h.normal = {0.f, 0.f, 1.f};
      t.h.geom_id = MI_INVALID_GEOM;
      t.h.flags = 0;
    }
  return MI_OK;
}

void mi_scale_rgb(mi_trace_result* rays, size_t n, float scale) {
  for (size_t i = 0; i < n; ++i) { rays[i].rgb.x *= scale; rays[i].rgb.y *= scale; rays[i].rgb.z *= scale; }
}

size_t mi_scene_blob_size(const mi_scene_desc* d) {
  if (!d) return 0;
  mi::blob::Writer w(16);
  mi::blob::serialiseScene(w, *d);
  return w.bytes.size();
}

int mi_scene_serialise(const mi_scene_desc* d, uint8_t* out, size_t capacity, size_t* written) {
  return guarded([&] {
    if (!d || !out) throw std::runtime_error("null argument");
    mi::blob::Writer w(16, 600 * 1024);                            // the reference reserves 600 KiB (src/IpuScene.cpp:31)
    mi::blob::serialiseScene(w, *d);
    if (w.bytes.size() > capacity) throw std::runtime_error("serialised scene needs " + std::to_string(w.bytes.size()) + " bytes");
    std::memcpy(out, w.bytes.data(), w.bytes.size());
    if (written) *written = w.bytes.size();
  });
}

int mi_scene_deserialise(const uint8_t* blob, size_t size, mi_scene_desc* d, size_t* consumed) {
  return guarded([&] {
    if (!blob || !d) throw std::runtime_error("null argument");
    if ((uintptr_t)blob % 16) throw std::runtime_error("serialised scene must be 16-byte aligned to be aliased in place");
    const size_t used = mi::blob::deserialiseScene(blob, size, *d, 16);
    if (consumed) *consumed = used;
  });
}

size_t mi_shard_band_rays(size_t n, uint32_t window_w) { return mi::shard::band_rays(n, window_w); }

size_t mi_shard_count(size_t n, size_t band, uint32_t replicas, uint32_t r) { return mi::shard::replica_count(n, band, replicas, r); }

int mi_shard_stream_index(size_t n, size_t band, uint32_t replicas, uint32_t r, uint64_t* out, size_t capacity) {
  if (!out || band == 0 || replicas == 0 || r >= replicas) { g_err = "mi_shard_stream_index: bad argument"; return MI_ERR_INVALID_ARG; }
  if (capacity < mi::shard::replica_count(n, band, replicas, r)) { g_err = "mi_shard_stream_index: output too small"; return MI_ERR_INVALID_ARG; }
  size_t k = 0;
  for (size_t b = r; b * band < n; b += replicas)
    for (size_t i = b * band; i < std::min(n, (b + 1) * band); ++i) out[k++] = i;
  return MI_OK;
}

int mi_shard_frame_index(size_t n, size_t band, uint32_t replicas, uint64_t* out) {
  if (!out || band == 0 || replicas == 0) { g_err = "mi_shard_frame_index: bad argument"; return MI_ERR_INVALID_ARG; }
  std::vector<size_t> offset(replicas + 1, 0);
  for (uint32_t r = 0; r < replicas; ++r) offset[r + 1] = offset[r] + mi::shard::replica_count(n, band, replicas, r);
  for (size_t i = 0; i < n; ++i) {
    uint32_t r; size_t pos;
    mi::shard::locate(band, replicas, i, r, pos);
    out[i] = offset[r] + pos;
  }
  return MI_OK;
}

uint32_t mi_blob_padding(uint32_t base_align, size_t offset, uint32_t align) {
  return align ? mi::blob::padding(base_align, offset, align) : 0u;
}

}  // extern "C"
