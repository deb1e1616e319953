// canon_kernels.hpp — gfx950 kernels of mi_scene_set_geometry*: the canonical primitive table of NEW scene contents, written on the
// device. A scene's first mi_scene_rebuild builds the table with a host loop over the host copies of its arrays (raylib.hip,
// rebuildTables); replaced contents have no host copies - the triangle list of mi_scene_set_geometry_device is device memory - and
// a loop over a million triangles would be the call's only O(P) host work. The record and the search are canon_prims.hpp's, which
// the host loop and the host twin mi_canonical_prims run too. The driver is setGeometry in raylib.hip; DESIGN.md §19.
//
// The host uploads the control plane: primStart[0 .. G] (the exclusive prefix of the geometries' primitive counts), the geometry
// refs, the mesh infos and the material ids, all checked there (canon_check_control): every index a thread forms from them is in
// range. What the host cannot check without reading device memory - a triangle's vertex index against its mesh's num_vertices -
// is checked here and raises a bit of the passes' error word; the record then names a vertex that exists, so the passes behind it
// read nothing out of bounds before the host has read the word and refused.
// No workgroup reads what another wrote; the only atomic is the atomicOr on the error word, as in the passes that follow.
#pragma once

#include <hip/hip_runtime.h>

#include "canon_prims.hpp"

namespace mi {

// one thread per canonical primitive
__global__ void __launch_bounds__(256) canon_prim_kernel(uint32_t P, const uint32_t* primStart, uint32_t G, const mi_geom_ref* geometry,
                                                         const mi_mesh_info* meshInfo, const uint32_t* matIds, const uint16_t* tris,
                                                         RebuildPrim* canon, uint32_t* err) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  RebuildPrim q;
  if (!canon_prim(p, primStart, G, geometry, meshInfo, matIds, tris, q)) atomicOr(err, 1u << kTriIndexOutOfRange);
  canon[p] = q;
}

// one thread per geometry: DeviceScene::geomFirstVertex, as buildDeviceScene fills it (a mesh's first vertex, 0 for the others)
__global__ void __launch_bounds__(256) canon_first_vertex_kernel(uint32_t G, const mi_geom_ref* geometry, const mi_mesh_info* meshInfo,
                                                                 uint32_t* geomFirstVertex) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const mi_geom_ref r = geometry[g];
  geomFirstVertex[g] = r.type == 0 ? meshInfo[r.index].first_vertex : 0u;
}

}  // namespace mi
