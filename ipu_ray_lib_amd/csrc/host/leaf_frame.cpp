// leaf_frame.cpp — mi_leaf_frames / mi_diffuse_frame (include/mi_scene_host.h): the per-leaf tangent-frame records of a scene without
// vertex normals (csrc/leaf_frame.hpp: fill_leaf_frames, the function the device library's upload runs), compiled for the host so that
// the records and their permutation into K1w's private copies can be checked without a GPU.
#include "../leaf_frame.hpp"
#include "../../../include/mi_scene_host.h"

#include <cstring>
#include <vector>

extern "C" void mi_diffuse_frame(const float normal[3], float xb[3], float yb[3]) {
  mi::f3 x, y;
  mi::diffuse_frame(mi::mk(normal[0], normal[1], normal[2]), x, y);
  xb[0] = x.x; xb[1] = x.y; xb[2] = x.z;
  yb[0] = y.x; yb[1] = y.y; yb[2] = y.z;
}

// Per node of desc's BVH the normal SHADE reads for a hit on it, as the upload stores it - a triangle's face normal
// normalise(cross(p1 - p0, p2 - p0)) (GLeaf::n), a disc's plane normal - and the record of the node at each of `count` places.
extern "C" int mi_leaf_frames(const mi_scene_desc* d, const uint32_t* at, uint32_t count, float* frames, float* normals) {
  if (!d || (count && !frames) || (d->num_nodes && !d->bvh_nodes)) return MI_ERR_INVALID_ARG;
  const uint32_t N = d->num_nodes;
  std::vector<uint8_t> framed(N, 0);
  std::vector<float> normal(3 * (size_t)N, 0.f);
  for (uint32_t i = 0; i < N; ++i) {
    const mi_bvh_node& n = d->bvh_nodes[i];
    if (n.geom_id == MI_INVALID_GEOM) continue;
    if (n.geom_id >= d->num_geometry) return MI_ERR_INVALID_ARG;
    const mi_geom_ref& r = d->geometry[n.geom_id];
    if (r.type == 0) {
      if (r.index >= d->num_meshes) return MI_ERR_INVALID_ARG;
      const mi_mesh_info& m = d->mesh_info[r.index];
      if (n.prim_or_second_child >= m.num_triangles) return MI_ERR_INVALID_ARG;
      const size_t base = 3 * ((size_t)m.first_index + n.prim_or_second_child);
      mi::f3 p[3];
      for (int k = 0; k < 3; ++k) {
        const size_t v = (size_t)m.first_vertex + d->mesh_tris[base + k];
        if (v >= d->num_verts) return MI_ERR_INVALID_ARG;
        p[k] = mi::mk(d->mesh_verts[v].x, d->mesh_verts[v].y, d->mesh_verts[v].z);
      }
      const mi::f3 fn = mi::normalized(mi::cross(p[1] - p[0], p[2] - p[0]));                        // Mesh.hpp:112-114
      normal[3 * (size_t)i] = fn.x; normal[3 * (size_t)i + 1] = fn.y; normal[3 * (size_t)i + 2] = fn.z;
      framed[i] = 1;
    } else if (r.type == 2) {
      if (r.index >= d->num_discs) return MI_ERR_INVALID_ARG;
      const mi_disc& c = d->discs[r.index];
      normal[3 * (size_t)i] = c.nx; normal[3 * (size_t)i + 1] = c.ny; normal[3 * (size_t)i + 2] = c.nz;
      framed[i] = 1;
    }
  }
  for (uint32_t k = 0; k < count; ++k) if (at && at[k] >= N) return MI_ERR_INVALID_ARG;
  if (!at && count > N) return MI_ERR_INVALID_ARG;
  static_assert(sizeof(mi::GLeafFrame) == 8 * sizeof(float), "a record is eight floats");
  std::vector<mi::GLeafFrame> out(count);
  mi::fill_leaf_frames(framed.data(), normal.data(), at, count, out.data());
  if (count) std::memcpy(frames, out.data(), (size_t)count * sizeof(mi::GLeafFrame));
  if (normals && N) std::memcpy(normals, normal.data(), normal.size() * sizeof(float));
  return MI_OK;
}
