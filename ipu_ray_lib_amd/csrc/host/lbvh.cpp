// lbvh.cpp — mi_build_lbvh_compact (include/mi_scene_host.h): the host twin of the device rebuild (rebuild_kernels.hpp,
// mi_scene_rebuild). A linear BVH over the scene's primitives taken in canonical order (geometry 0 .. G - 1, inside a mesh
// triangle 0 .. T - 1): Morton keys of the box centroids inside the scene box, a sort by (key, canonical index), Karras' 2012
// hierarchy, boxes bottom-up, the builder's child-order rule, preorder layout. Key, hierarchy, box and encoding code is the
// MI_HD code of ray_math.h that the kernels run, and every step is a compare / select, an integer operation or one rounded
// floating-point operation, so the nodes equal the device's byte for byte.
#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "scene_types.hpp"

namespace mi::host {

namespace {
struct CanonPrim { Box3 box; uint16_t geomID; uint32_t primID; };
}

void buildLbvhCompact(const mi_scene_desc& d, std::vector<mi_bvh_node>& out, uint32_t& maxDepth) {
  auto need = [](bool ok, const char* what) { if (!ok) throw std::invalid_argument(std::string("mi_build_lbvh_compact: ") + what); };
  need(d.num_geometry == 0 || d.geometry, "geometry is null");
  need(d.num_geometry <= kMaxGeometries, kTooManyGeometries);
  need(d.num_meshes == 0 || (d.mesh_info && d.mesh_tris && d.mesh_verts), "mesh arrays are null");
  need(d.num_spheres == 0 || d.spheres, "spheres is null");
  need(d.num_discs == 0 || d.discs, "discs is null");
  out.clear();
  maxDepth = 0;

  // canonical primitives and their boxes
  std::vector<CanonPrim> prims;
  for (uint32_t g = 0; g < d.num_geometry; ++g) {
    const mi_geom_ref& r = d.geometry[g];
    need(r.type <= 2 && r.index < (r.type == 0 ? d.num_meshes : r.type == 1 ? d.num_spheres : d.num_discs), "geometry index out of range");
    if (r.type == 0) {
      const mi_mesh_info& m = d.mesh_info[r.index];
      need((uint64_t)m.first_index + m.num_triangles <= d.num_tris, "leaf primID out of range");
      for (uint32_t t = 0; t < m.num_triangles; ++t) {
        f3 p[3];
        for (int k = 0; k < 3; ++k) {
          const uint32_t v = d.mesh_tris[3 * ((size_t)m.first_index + t) + k];
          need(v < m.num_vertices && (uint64_t)m.first_vertex + v < d.num_verts, "triangle vertex index out of range");
          const mi_vec3& q = d.mesh_verts[m.first_vertex + v];
          p[k] = mk(q.x, q.y, q.z);
        }
        prims.push_back({triangle_box(p[0], p[1], p[2]), (uint16_t)g, t});
      }
    } else if (r.type == 1) {
      const mi_sphere& s = d.spheres[r.index];
      prims.push_back({ball_box(s.x, s.y, s.z, s.radius), (uint16_t)g, 0u});
    } else {
      const mi_disc& c = d.discs[r.index];
      prims.push_back({ball_box(c.cx, c.cy, c.cz, c.r), (uint16_t)g, 0u});
    }
  }
  const uint32_t P = (uint32_t)prims.size();
  if (P == 0) return;
  need(P < (1u << 25), "more than 2^25 - 1 primitives");
  const uint32_t I = P - 1;          // interior nodes 0 .. I - 1, leaf j (sorted position) = node I + j

  // scene box, keys, sort
  Box3 scene = box_empty();
  for (const CanonPrim& p : prims) scene = box_merge(scene, p.box);
  scene = lbvh_scene_box(scene);
  std::vector<uint64_t> key(P);
  for (uint32_t p = 0; p < P; ++p) key[p] = lbvh_key(prims[p].box, scene);
  std::vector<uint32_t> sorted(P);
  std::iota(sorted.begin(), sorted.end(), 0u);
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<uint64_t> keys(P);
  for (uint32_t j = 0; j < P; ++j) keys[j] = key[sorted[j]];

  // hierarchy
  const uint32_t M = 2 * P - 1;
  std::vector<uint32_t> left(I), right(I), first(I), last(I), parent(M, 0);
  for (uint32_t i = 0; i < I; ++i) {
    uint32_t split;
    lbvh_node(keys.data(), P, i, first[i], last[i], split);
    left[i] = first[i] == split ? I + split : split;
    right[i] = last[i] == split + 1 ? I + split + 1 : split + 1;
    parent[left[i]] = i; parent[right[i]] = i;
  }
  // depth of the interior nodes (root 0), then the nodes deepest first
  std::vector<uint32_t> depth(I, 0), order(I);
  for (uint32_t i = 0; i < I; ++i)
    for (uint32_t c = i; c != 0; c = parent[c]) ++depth[i];
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return depth[a] > depth[b]; });
  // boxes bottom-up and the child order: the child whose box centre is nearer the origin first, the lower-key child on a tie
  std::vector<Box3> box(M);
  for (uint32_t j = 0; j < P; ++j) box[I + j] = prims[sorted[j]].box;
  std::vector<uint8_t> swapped(I, 0);
  for (uint32_t i : order) {
    swapped[i] = box_centre_dist2(box[right[i]]) < box_centre_dist2(box[left[i]]);
    box[i] = swapped[i] ? box_union(box[right[i]], box[left[i]]) : box_union(box[left[i]], box[right[i]]);
  }
  uint32_t err = 0;
  for (uint32_t n = 0; n < M; ++n) {
    mi_bvh_node c;
    const uint32_t code = box_encode(box[n], c.min_x, c.min_y, c.min_z, c.dx, c.dy, c.dz);
    if (code != kBoxOk) err |= 1u << code;
  }
  if (err & (1u << kBoxNotFinite)) throw std::invalid_argument("mi_build_lbvh_compact: a node box is not finite");
  if (err) throw std::runtime_error("Cannot compress BVH bounds into fp16 (half)");

  // preorder layout (an explicit stack: depth is bounded by key bits + index bits, but there is no need to recurse)
  auto size = [&](uint32_t n) { return n >= I ? 1u : 2u * (last[n] - first[n] + 1u) - 1u; };
  out.resize(M);
  struct Item { uint32_t node, at, depth; };
  std::vector<Item> stack;
  stack.push_back({P == 1 ? I : 0u, 0u, 1u});
  while (!stack.empty()) {
    const Item it = stack.back(); stack.pop_back();
    mi_bvh_node c;
    box_encode(box[it.node], c.min_x, c.min_y, c.min_z, c.dx, c.dy, c.dz);
    if (it.node >= I) {
      const CanonPrim& p = prims[sorted[it.node - I]];
      c.geom_id = p.geomID; c.prim_or_second_child = p.primID;
      if (it.depth > maxDepth) maxDepth = it.depth;
    } else {
      const uint32_t a = swapped[it.node] ? right[it.node] : left[it.node], b = swapped[it.node] ? left[it.node] : right[it.node];
      c.geom_id = MI_INVALID_GEOM; c.prim_or_second_child = it.at + 1 + size(a);
      stack.push_back({b, it.at + 1 + size(a), it.depth + 1});
      stack.push_back({a, it.at + 1, it.depth + 1});
    }
    out[it.at] = c;
  }
}

}  // namespace mi::host
