// canon_prims.hpp — the canonical primitive table of a scene: its primitives in canonical order (geometry 0 .. G - 1, inside a mesh
// triangle 0 .. T - 1), 32 bytes each. It is what the device LBVH build (rebuild_kernels.hpp) sorts and scatters, so it fixes the
// tree. One definition of the record, of the search from a canonical index to its geometry and of the argument checks serves the
// device kernel (canon_kernels.hpp, mi_scene_set_geometry*), the host loop of a scene's first mi_scene_rebuild (raylib.hip,
// rebuildTables) and the host twin mi_canonical_prims (host/scene_api.cpp). Plain C++: no HIP needed.
#pragma once

#include <stdint.h>

#include "ray_math.h"
#include "../../include/mi_raylib.h"

namespace mi {

// A canonical primitive: what its box is computed from, as the refit's RefitPrim states it (kind 0 = triangle: a, b, c = absolute
// vertex indices; 1 = sphere, 2 = disc: a = the index - the kinds are the geometry types, refit_kernels.hpp REFIT_*), and what its
// leaf record carries.
struct __attribute__((aligned(16))) RebuildPrim { uint32_t a, b, c, kind, geomID, primID, triBase, matIndex; };
static_assert(sizeof(RebuildPrim) == 32, "RebuildPrim: 32 B");

// bit of the passes' error word (beside 1 << kBoxTooLarge and 1 << kBoxNotFinite, ray_math.h): a triangle's vertex index is not
// below its mesh's num_vertices
constexpr uint32_t kTriIndexOutOfRange = 3;

// primStart[0 .. G]: the exclusive prefix of the geometries' primitive counts (a mesh's num_triangles, 1 for a sphere or disc).
// The geometry of canonical primitive p < primStart[G]: g = max { g : primStart[g] <= p }. Geometries without primitives make
// consecutive entries equal; the maximum steps over them wherever they sit.
MI_HD uint32_t canon_find_geometry(const uint32_t* primStart, uint32_t G, uint32_t p) {
  uint32_t lo = 0, hi = G;                  // primStart[lo] <= p < primStart[hi] throughout
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (primStart[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// Canonical primitive p's record. The arrays are the scene's (checked: canon_check_control). Returns false where a triangle's
// vertex index is not below its mesh's num_vertices; the record then names the mesh's vertex 0 in its place, so that nothing
// computed from it reads outside the vertex array (a mesh with triangles has a vertex: canon_check_control).
MI_HD bool canon_prim(uint32_t p, const uint32_t* primStart, uint32_t G, const mi_geom_ref* geometry, const mi_mesh_info* meshInfo,
                      const uint32_t* matIds, const uint16_t* tris, RebuildPrim& out) {
  const uint32_t g = canon_find_geometry(primStart, G, p), t = p - primStart[g];
  const mi_geom_ref r = geometry[g];
  bool ok = true;
  if (r.type == 0) {
    const mi_mesh_info m = meshInfo[r.index];
    const size_t base = 3 * ((size_t)m.first_index + t);
    uint32_t v[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = tris[base + k];
      if (v[k] >= m.num_vertices) { v[k] = 0u; ok = false; }
    }
    out.a = m.first_vertex + v[0]; out.b = m.first_vertex + v[1]; out.c = m.first_vertex + v[2];
    out.kind = 0u; out.geomID = g; out.primID = t; out.triBase = (uint32_t)base; out.matIndex = matIds[g];
  } else {
    out.a = r.index; out.b = 0u; out.c = 0u;
    out.kind = r.type; out.geomID = g; out.primID = 0u; out.triBase = 0u; out.matIndex = matIds[g];
  }
  return ok;
}

// The checks mi_scene_create makes of the arrays a scene's geometry comes in, in its order and with its words, for everything that
// can be told without reading the triangle list, the vertices or the primitives (they may be device memory): need(ok, what) is
// called for each. maxNodes: the node count 2 P - 1 must stay below it.
template <class Need>
inline void canon_check_control(const mi_scene_geometry& d, uint32_t maxNodes, Need&& need) {
  need(d.num_geometry == 0 || d.geometry, "geometry is null");
  need(d.num_geometry <= 0xFFFF, "more than 65535 geometries (geomID is 16 bit)");
  need(d.num_mat_ids >= d.num_geometry, "All primitives must be assigned a material.");
  need(d.num_mat_ids == 0 || d.mat_ids, "mat_ids is null");
  need(d.num_materials == 0 || d.materials, "materials is null");
  need(d.num_meshes == 0 || (d.mesh_info && d.mesh_tris && d.mesh_verts), "mesh arrays are null");
  need(d.num_normals == 0 || (d.num_normals == d.num_verts && d.mesh_normals), "normals must be absent or one per vertex");
  need(d.num_spheres == 0 || d.spheres, "spheres is null");
  need(d.num_discs == 0 || d.discs, "discs is null");
  for (uint32_t g = 0; g < d.num_geometry; ++g) {
    const mi_geom_ref& r = d.geometry[g];
    need(r.type <= 2, "unknown geometry type");
    need(r.index < (r.type == 0 ? d.num_meshes : r.type == 1 ? d.num_spheres : d.num_discs), "geometry index out of range");
    need(d.mat_ids[g] < d.num_materials, "material index out of range");
  }
  for (uint32_t m = 0; m < d.num_meshes; ++m) {
    const mi_mesh_info& mi_ = d.mesh_info[m];
    need((uint64_t)mi_.first_index + mi_.num_triangles <= d.num_tris, "mesh triangle range out of bounds");
    need((uint64_t)mi_.first_vertex + mi_.num_vertices <= d.num_verts, "mesh vertex range out of bounds");
    // (no vertex: every index of every triangle is out of range, whatever the list holds)
    need(mi_.num_triangles == 0 || mi_.num_vertices > 0, "triangle vertex index out of range");
  }
  uint64_t prims = 0;
  for (uint32_t g = 0; g < d.num_geometry; ++g) prims += d.geometry[g].type == 0 ? d.mesh_info[d.geometry[g].index].num_triangles : 1u;
  need(prims == 0 || 2 * prims - 1 < maxNodes, "more than 2^26 - 1 BVH nodes");
}

// primStart[0 .. G] of the checked arrays (room for G + 1 entries); returns P
inline uint32_t canon_prim_starts(const mi_scene_geometry& d, uint32_t* primStart) {
  uint32_t at = 0;
  for (uint32_t g = 0; g < d.num_geometry; ++g) {
    primStart[g] = at;
    at += d.geometry[g].type == 0 ? d.mesh_info[d.geometry[g].index].num_triangles : 1u;
  }
  primStart[d.num_geometry] = at;
  return at;
}

// the nine arrays of a desc
inline mi_scene_geometry canon_geometry_of(const mi_scene_desc& d) {
  mi_scene_geometry g{};
  g.geometry = d.geometry; g.num_geometry = d.num_geometry; g.mesh_info = d.mesh_info; g.num_meshes = d.num_meshes;
  g.mat_ids = d.mat_ids; g.num_mat_ids = d.num_mat_ids; g.materials = d.materials; g.num_materials = d.num_materials;
  g.mesh_tris = d.mesh_tris; g.num_tris = d.num_tris; g.mesh_verts = d.mesh_verts; g.num_verts = d.num_verts;
  g.mesh_normals = d.mesh_normals; g.num_normals = d.num_normals; g.spheres = d.spheres; g.num_spheres = d.num_spheres;
  g.discs = d.discs; g.num_discs = d.num_discs;
  return g;
}

}  // namespace mi
