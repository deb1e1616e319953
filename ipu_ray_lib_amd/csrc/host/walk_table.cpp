// walk_table.cpp — walkTable (scene_types.hpp): the table the host twins of the point queries, the neighbour lists, the box queries
// and the triangle queries walk (walkHost, walk_host.hpp). A node's box is min and min + (float)extent (one rounded add, as the
// device record carries it), a leaf's primitive is resolved from the scene's arrays as mi_scene_create resolves it - the first 40
// bytes of the device's leaf record -, and a description mi_scene_create would refuse is refused here in the same words.
#include <stdexcept>
#include <string>
#include <vector>

#include "scene_types.hpp"

namespace mi::host {

// The walk's table of desc's nodes; fn: the entry's name, for the message of what is refused.
std::vector<WalkNode> walkTable(const mi_scene_desc& d, const char* fn) {
  auto need = [fn](bool ok, const char* what) { if (!ok) throw std::invalid_argument(std::string(fn) + ": " + what); };
  const uint32_t N = d.num_nodes;
  need(N == 0 || d.bvh_nodes, "bvh_nodes is null");
  need(d.num_geometry == 0 || d.geometry, "geometry is null");
  need(d.num_geometry <= kMaxGeometries, kTooManyGeometries);
  need(d.num_meshes == 0 || (d.mesh_info && d.mesh_tris && d.mesh_verts), "mesh arrays are null");
  need(d.num_spheres == 0 || d.spheres, "spheres is null");
  need(d.num_discs == 0 || d.discs, "discs is null");

  // the walk's table: skip links from the back (mi_scene_create's checks of the depth-first layout), boxes, leaf records
  std::vector<WalkNode> nodes(N);
  for (uint32_t i = N; i-- > 0;) {
    const mi_bvh_node& c = d.bvh_nodes[i];
    WalkNode& w = nodes[i];
    w.minx = c.min_x; w.miny = c.min_y; w.minz = c.min_z;
    w.maxx = c.min_x + half_bits_to_float(c.dx);
    w.maxy = c.min_y + half_bits_to_float(c.dy);
    w.maxz = c.min_z + half_bits_to_float(c.dz);
    for (float& x : w.f) x = 0.f;
    w.primID = c.prim_or_second_child; w.geomID = c.geom_id;
    if (c.geom_id == MI_INVALID_GEOM) {
      const uint32_t second = c.prim_or_second_child;
      need(i + 1 < N && second > i + 1 && second < N, "BVH is not a depth-first BVH2 (bad second child index)");
      need(nodes[i + 1].skip == second, "BVH is not in depth-first order (first child's subtree must end at the second child)");
      w.skip = nodes[second].skip;
      w.kind = kInterior;
      continue;
    }
    w.skip = i + 1;
    need(c.geom_id < d.num_geometry, "leaf geomID out of range");
    const mi_geom_ref& r = d.geometry[c.geom_id];
    need(r.type <= 2 && r.index < (r.type == 0 ? d.num_meshes : r.type == 1 ? d.num_spheres : d.num_discs), "geometry index out of range");
    w.kind = r.type;
    if (r.type == 0) {
      const mi_mesh_info& m = d.mesh_info[r.index];
      need(c.prim_or_second_child < m.num_triangles && (uint64_t)m.first_index + c.prim_or_second_child < d.num_tris, "leaf primID out of range");
      const size_t base = 3 * ((size_t)m.first_index + c.prim_or_second_child);
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = d.mesh_tris[base + k];
        need((uint64_t)m.first_vertex + v < d.num_verts, "triangle vertex index out of range");
        const mi_vec3& p = d.mesh_verts[m.first_vertex + v];
        w.f[3 * k] = p.x; w.f[3 * k + 1] = p.y; w.f[3 * k + 2] = p.z;
      }
    } else if (r.type == 1) {
      const mi_sphere& s = d.spheres[r.index];
      w.f[0] = s.x; w.f[1] = s.y; w.f[2] = s.z; w.f[3] = s.radius; w.f[4] = s.radius * s.radius;
      w.primID = 0;
    } else {
      const mi_disc& c2 = d.discs[r.index];
      w.f[0] = c2.nx; w.f[1] = c2.ny; w.f[2] = c2.nz; w.f[3] = c2.cx; w.f[4] = c2.cy; w.f[5] = c2.cz; w.f[6] = c2.r * c2.r;
      w.primID = 0;
    }
  }
  need(N == 0 || nodes[0].skip == N, "BVH root does not span the node array");
  return nodes;
}

}  // namespace mi::host
