// refit_kernels.hpp — gfx950 kernels of mi_scene_update / mi_scene_update_device: new primitive positions in a live scene,
// the BVH's topology kept and every box recomputed (Embree's refit commit, OptiX's update build), then the scene's device
// records rewritten in place. The driver is refitScene in raylib.hip; DESIGN.md §14 has the passes and the numbers.
//
// Exactness. A node's compact box is a pure function of the primitives below it: a leaf's is its primitive's box, an
// interior node's the union of its children's float boxes, encoded as min + extent rounded up to binary16. Every step is a
// compare / select or one rounded binary32 operation (ray_math.h box_*, the same code the host builder and the host refit
// run), and min / max are exact, so the result does not depend on the order the threads run in: the device nodes equal
// mi_refit_compact_bvh's byte for byte, and every record rewritten from them equals what mi_scene_create derives from the
// moved arrays and those nodes.
//
// Passes, all on the caller's stream, kernel boundaries giving visibility between them:
//   1 refit_leaf_kernel    one thread per leaf: the primitive's box -> float box + compact node (scratch only)
//   2 refit_level_kernel   one launch per height (leaf 0, interior 1 + the higher child), one thread per node of that height:
//                          union of the two children's float boxes -> float box + compact node (scratch only);
//     refit_top_kernel     the small top levels in ONE workgroup, __syncthreads() between levels
//   3 (host) read back the error word and the root node; on an error the scene is untouched
//   4 refit_write_kernel   one thread per node: GNode min / max, GLeaf, GLeafRot and the vertex normals of the leaf record
#pragma once

#include <hip/hip_runtime.h>

#include "ray_math.h"
#include "trace_kernels.hpp"
#include "../../include/mi_raylib.h"

namespace mi {

// What a node's box is computed from (16 B per node, built on the host at the first update). kind REFIT_TRI: a, b, c = the
// triangle's absolute vertex indices; REFIT_SPHERE / REFIT_DISC: a = the sphere's / disc's index; REFIT_INTERIOR: a = the
// second child (the first is the node's successor).
enum : uint32_t { REFIT_TRI = 0, REFIT_SPHERE = 1, REFIT_DISC = 2, REFIT_INTERIOR = 3 };
struct __attribute__((aligned(16))) RefitPrim { uint32_t a, b, c, kind; };
static_assert(sizeof(RefitPrim) == 16, "RefitPrim: 16 B");

// The geometry a refit reads: the caller's new arrays where given, the scene's current copies otherwise. normals: only
// when new vertex normals were given (NULL otherwise: the records' normals stay).
struct RefitGeom {
  const mi_vec3* verts;
  const mi_sphere* spheres;
  const mi_disc* discs;
  const mi_vec3* normals;
};

struct __attribute__((aligned(8))) RefitBox { float lx, ly, lz, hx, hy, hz; };   // a node's float box, 24 B
static_assert(sizeof(RefitBox) == 24, "RefitBox: 24 B");

__device__ __forceinline__ f3 refit_vertex(const mi_vec3* v, uint32_t i) { const mi_vec3 p = v[i]; return mk(p.x, p.y, p.z); }

__device__ __forceinline__ Box3 refit_prim_box(const RefitPrim& p, const RefitGeom& g) {
  if (p.kind == REFIT_TRI) return triangle_box(refit_vertex(g.verts, p.a), refit_vertex(g.verts, p.b), refit_vertex(g.verts, p.c));
  if (p.kind == REFIT_SPHERE) { const mi_sphere s = g.spheres[p.a]; return ball_box(s.x, s.y, s.z, s.radius); }
  const mi_disc c = g.discs[p.a];
  return ball_box(c.cx, c.cy, c.cz, c.r);
}

__device__ __forceinline__ Box3 refit_load_box(const RefitBox* boxes, uint32_t i) {
  const RefitBox r = boxes[i];
  Box3 b; b.lo = mk(r.lx, r.ly, r.lz); b.hi = mk(r.hx, r.hy, r.hz);
  return b;
}

// Stores node i's float box and compact node (its link and geomID word kept); a box the scene could not hold raises *err.
__device__ __forceinline__ void refit_store(uint32_t i, const Box3& b, RefitBox* boxes, mi_bvh_node* cnodes, uint32_t* err) {
  RefitBox r; r.lx = b.lo.x; r.ly = b.lo.y; r.lz = b.lo.z; r.hx = b.hi.x; r.hy = b.hi.y; r.hz = b.hi.z;
  boxes[i] = r;
  mi_bvh_node c = cnodes[i];
  const uint32_t code = box_encode(b, c.min_x, c.min_y, c.min_z, c.dx, c.dy, c.dz);
  cnodes[i] = c;
  if (code != kBoxOk) atomicOr(err, 1u << code);
}

// pass 1: order[0 .. count) = the leaves
__global__ void __launch_bounds__(256) refit_leaf_kernel(const uint32_t* order, uint32_t count, const RefitPrim* prims, RefitGeom g,
                                                         RefitBox* boxes, mi_bvh_node* cnodes, uint32_t* err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t i = order[k];
  refit_store(i, refit_prim_box(prims[i], g), boxes, cnodes, err);
}

__device__ __forceinline__ void refit_interior(uint32_t i, const RefitPrim* prims, RefitBox* boxes, mi_bvh_node* cnodes, uint32_t* err) {
  refit_store(i, box_union(refit_load_box(boxes, i + 1), refit_load_box(boxes, prims[i].a)), boxes, cnodes, err);
}

// pass 2: order[begin .. begin + count) = the interior nodes of one height
__global__ void __launch_bounds__(256) refit_level_kernel(const uint32_t* order, uint32_t begin, uint32_t count, const RefitPrim* prims,
                                                          RefitBox* boxes, mi_bvh_node* cnodes, uint32_t* err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  refit_interior(order[begin + k], prims, boxes, cnodes, err);
}

// pass 2, the top: heights first .. last in one workgroup; levelStart[h] = first entry of height h in order[]. The barrier
// orders every level's box stores before the next level's loads (workgroup scope: all waves of the workgroup share one
// compute unit and its L1).
constexpr uint32_t kRefitTopThreads = 1024;
__global__ void __launch_bounds__(kRefitTopThreads) refit_top_kernel(const uint32_t* order, const uint32_t* levelStart, uint32_t first, uint32_t last,
                                                                     const RefitPrim* prims, RefitBox* boxes, mi_bvh_node* cnodes, uint32_t* err) {
  for (uint32_t h = first; h <= last; ++h) {
    const uint32_t b = levelStart[h], e = levelStart[h + 1];
    for (uint32_t k = b + threadIdx.x; k < e; k += blockDim.x) refit_interior(order[k], prims, boxes, cnodes, err);
    __syncthreads();
  }
}

// pass 4: node i's device records from its new compact node and its primitive, as buildDeviceScene (raylib.hip) derives them
// at create. Links, types, primIDs, triBase and material indices do not change.
__global__ void __launch_bounds__(256) refit_write_kernel(uint32_t n, const RefitPrim* prims, const mi_bvh_node* cnodes, RefitGeom g,
                                                          GNode* nodes, GLeaf* leaves, GLeafRot* rot, float* leafNormals, GLeafFrame* leafFrames) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const mi_bvh_node c = cnodes[i];
  GNode nd = nodes[i];
  nd.minx = c.min_x; nd.maxx = c.min_x + half_bits_to_float(c.dx);          // CompactBVH2Node.cpp:8-10, one rounded add each
  nd.miny = c.min_y; nd.maxy = c.min_y + half_bits_to_float(c.dy);
  nd.minz = c.min_z; nd.maxz = c.min_z + half_bits_to_float(c.dz);
  nodes[i] = nd;
  const RefitPrim p = prims[i];
  if (p.kind == REFIT_INTERIOR) return;
  GLeaf L = leaves[i];
  if (p.kind == REFIT_TRI) {
    const f3 p0 = refit_vertex(g.verts, p.a), p1 = refit_vertex(g.verts, p.b), p2 = refit_vertex(g.verts, p.c);
    L.f[0] = p0.x; L.f[1] = p0.y; L.f[2] = p0.z; L.f[3] = p1.x; L.f[4] = p1.y; L.f[5] = p1.z; L.f[6] = p2.x; L.f[7] = p2.y; L.f[8] = p2.z;
    const f3 fn = normalized(cross(p1 - p0, p2 - p0));                        // Mesh.hpp:112-114
    L.n[0] = fn.x; L.n[1] = fn.y; L.n[2] = fn.z;
    if (g.normals && leafNormals) {
      const uint32_t v[3] = {p.a, p.b, p.c};
      for (int k = 0; k < 3; ++k) {
        const mi_vec3 q = g.normals[v[k]];
        leafNormals[9 * (size_t)i + 3 * k] = q.x; leafNormals[9 * (size_t)i + 3 * k + 1] = q.y; leafNormals[9 * (size_t)i + 3 * k + 2] = q.z;
      }
    }
  } else if (p.kind == REFIT_SPHERE) {
    const mi_sphere s = g.spheres[p.a];
    L.f[0] = s.x; L.f[1] = s.y; L.f[2] = s.z; L.f[3] = s.radius; L.f[4] = s.radius * s.radius;   // Primitives.hpp:44
  } else {
    const mi_disc d = g.discs[p.a];
    L.f[0] = d.nx; L.f[1] = d.ny; L.f[2] = d.nz; L.f[3] = d.cx; L.f[4] = d.cy; L.f[5] = d.cz; L.f[6] = d.r * d.r;
  }
  leaves[i] = L;
  // (scenes without vertex normals: the tangent frame about the normal just stored, leaf_frame.hpp; a sphere's stays zero)
  if (leafFrames && p.kind != REFIT_SPHERE) leafFrames[i] = leaf_frame_of(p.kind == REFIT_TRI ? mk(L.n[0], L.n[1], L.n[2]) : mk(L.f[0], L.f[1], L.f[2]));
  // GLeafRot: block kz = the record's floats, a triangle's vertex components rotated so that component kz comes last
  for (uint32_t kz = 0; kz < 3; ++kz) {
    GLeafBlock B;
    B.type = L.type;
    for (int q = 0; q < 9; ++q) B.f[q] = L.f[q];
    if (p.kind == REFIT_TRI) {
      const uint32_t kx = (kz + 1) % 3, ky = (kz + 2) % 3;
      for (int v = 0; v < 3; ++v) { B.f[3 * v] = L.f[3 * v + kx]; B.f[3 * v + 1] = L.f[3 * v + ky]; B.f[3 * v + 2] = L.f[3 * v + kz]; }
    }
    rot[i].b[kz] = B;
  }
}

}  // namespace mi
