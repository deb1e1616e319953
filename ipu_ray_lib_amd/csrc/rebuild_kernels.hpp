// rebuild_kernels.hpp — gfx950 kernels of mi_scene_rebuild: a new BVH topology for a live scene from its CURRENT geometry, built on
// the device (Embree's RTC_BUILD_QUALITY_LOW rebuild next to its refit, OptiX's BUILD next to UPDATE). The tree is a linear BVH:
// Morton keys of the primitive centroids, a radix sort, Karras' 2012 hierarchy. The driver is rebuildScene in raylib.hip, the host
// twin mi_build_lbvh_compact (host/lbvh.cpp); DESIGN.md §17 has the passes, the exactness argument and the numbers.
//
// Exactness. The primitives are taken in canonical order (geometry 0 .. G - 1, inside a mesh triangle 0 .. T - 1), which the scene
// fixes and the current node order does not touch. Boxes, keys, delta, the child-order rule and the node encoding are the MI_HD
// code of ray_math.h the twin runs; the sort is stable over the canonical index; every other step is integer work. min / max are
// compare / select and the scene box is cleared of signed zeros, so no result depends on the order the threads run in: the
// nodes equal the twin's byte for byte, whatever tree the scene had before.
//
// Passes, all on the caller's stream. Kernel boundaries are the only thing that makes one pass's stores visible to the next; no
// workgroup reads what another workgroup of the same launch wrote (inside rebuild_top_kernel and the two reductions one workgroup
// reads its own stores across __syncthreads()).
//   1 rebuild_prim_kernel       one thread per canonical primitive: its box, and the workgroup's part of the scene box
//     rebuild_scene_kernel      one workgroup: the scene box from the parts
//   2 rebuild_key_kernel        one thread per primitive: the 63-bit Morton key, and the iota the sort carries
//   3 (rocPRIM radix sort)      (key, canonical index) pairs, stable
//   4 rebuild_hierarchy_kernel  one thread per sorted position: the leaf's box; interior node i: children, range, parents
//   5 rebuild_depth_kernel      one thread per interior node: its depth, walking up the parents pass 4 wrote
//     (rocPRIM radix sort)      interior nodes by depth, stable; rebuild_levels_kernel: where each depth starts
//   6 rebuild_level_kernel      one launch per depth, deepest first: the child order and the union of the children's boxes;
//     rebuild_top_kernel        the small top levels in ONE workgroup, __syncthreads() between levels
//   7 rebuild_preorder_kernel   one thread per node: its preorder index, walking up once more
//   8 rebuild_heightkey_kernel one thread per node: (height, preorder index) at its preorder index - the heights come from pass 6
//     (rocPRIM radix sort)      nodes by height, stable: leaves first, inside a height by preorder index;
//     rebuild_heights_kernel    where each height starts - the refit's d_order / levelStart of the new topology (refit_kernels.hpp)
//   9 (host) read back the error word, the root box and the height starts; on an error the scene is untouched (all of the above
//     wrote scratch)
//  10 rebuild_scatter_kernel    one thread per node: the compact node, GNode, GLeaf, GLeafRot, vertex normals and the refit's
//                               RefitPrim at its new index
#pragma once

#include <hip/hip_runtime.h>

#include "ray_math.h"
#include "trace_kernels.hpp"
#include "refit_kernels.hpp"
#include "canon_prims.hpp"
#include "../../include/mi_raylib.h"

namespace mi {

// A canonical primitive is a RebuildPrim (canon_prims.hpp; 32 B, built on the host at the first rebuild and kept, or on the device
// by mi_scene_set_geometry*): what its box is computed from, as RefitPrim (kind REFIT_TRI: a, b, c = absolute vertex indices;
// REFIT_SPHERE / REFIT_DISC: a = the index), and what its leaf record carries.
static_assert(REFIT_TRI == 0 && REFIT_SPHERE == 1 && REFIT_DISC == 2, "a RebuildPrim's kind is its geometry's type");

// Node numbering until the scatter: interior nodes 0 .. P - 2 (Karras' indices, the root is 0), the leaf at sorted position j is
// node P - 1 + j. One primitive: node 0 is its leaf.
struct RebuildTree {
  uint32_t numPrims;
  const uint32_t* sorted;       // [P] canonical index at each sorted position
  uint2* child;                 // [P - 1] (lower-key child, higher-key child)
  uint2* range;                 // [P - 1] (first, last) sorted position below the node
  uint32_t* parent;             // [2 P - 1] (the root's entry is never read)
  uint8_t* swapped;             // [P - 1] 1 = the higher-key child goes first
  RefitBox* boxes;              // [2 P - 1] float boxes
  uint32_t* index;              // [2 P - 1] preorder index
  uint32_t* height;             // [2 P - 1] leaf 0, interior 1 + the higher child (what the refit buckets its passes by)
};

constexpr uint32_t kRebuildParts = 1024;       // workgroups of pass 1 = parts of the scene box, reduced by one workgroup of as many threads
constexpr uint32_t kRebuildMaxDepth = 128;     // interior depths are below 63 key bits + 32 index bits
// heights 0 .. H with H <= kRebuildMaxDepth (the root's height is the deepest interior depth + 1): heightStart[0 .. H + 1], and H
// itself in the last slot
constexpr uint32_t kRebuildHeightSlots = kRebuildMaxDepth + 3;

__device__ __forceinline__ void rebuild_store_box(RefitBox* boxes, uint32_t i, const Box3& b) {
  RefitBox r; r.lx = b.lo.x; r.ly = b.lo.y; r.lz = b.lo.z; r.hx = b.hi.x; r.hy = b.hi.y; r.hz = b.hi.z;
  boxes[i] = r;
}
// raises *err as the refit raises it when the scene could not hold the box
__device__ __forceinline__ void rebuild_check_box(const Box3& b, uint32_t* err) {
  mi_bvh_node c;
  const uint32_t code = box_encode(b, c.min_x, c.min_y, c.min_z, c.dx, c.dy, c.dz);
  if (code != kBoxOk) atomicOr(err, 1u << code);
}

// The workgroup's threads' boxes merged into sh[0] (blockDim.x a power of two, at most 1024). Empty boxes are neutral.
__device__ __forceinline__ void rebuild_block_merge(Box3* sh, const Box3& mine) {
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = box_merge(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
}

// pass 1: at most kRebuildParts workgroups, grid-stride
__global__ void __launch_bounds__(256) rebuild_prim_kernel(uint32_t P, const RebuildPrim* canon, RefitGeom g, RefitBox* primBoxes, RefitBox* parts, uint32_t* err) {
  __shared__ Box3 sh[256];
  Box3 acc = box_empty();
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    const RebuildPrim q = canon[p];
    RefitPrim rp; rp.a = q.a; rp.b = q.b; rp.c = q.c; rp.kind = q.kind;
    const Box3 b = refit_prim_box(rp, g);
    rebuild_store_box(primBoxes, p, b);
    rebuild_check_box(b, err);
    acc = box_merge(acc, b);
  }
  rebuild_block_merge(sh, acc);
  if (threadIdx.x == 0) rebuild_store_box(parts, blockIdx.x, sh[0]);
}

__global__ void __launch_bounds__(kRebuildParts) rebuild_scene_kernel(const RefitBox* parts, uint32_t count, RefitBox* scene) {
  __shared__ Box3 sh[kRebuildParts];
  rebuild_block_merge(sh, threadIdx.x < count ? refit_load_box(parts, threadIdx.x) : box_empty());
  if (threadIdx.x == 0) rebuild_store_box(scene, 0, lbvh_scene_box(sh[0]));
}

// pass 2
__global__ void __launch_bounds__(256) rebuild_key_kernel(uint32_t P, const RefitBox* primBoxes, const RefitBox* scene, uint64_t* keys, uint32_t* iota) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  keys[p] = lbvh_key(refit_load_box(primBoxes, p), refit_load_box(scene, 0));
  iota[p] = p;
}

// pass 4: keys[] sorted
__global__ void __launch_bounds__(256) rebuild_hierarchy_kernel(const uint64_t* keys, const RefitBox* primBoxes, RebuildTree t) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t P = t.numPrims, I = P - 1;
  if (j >= P) return;
  t.boxes[I + j] = primBoxes[t.sorted[j]];
  t.height[I + j] = 0u;
  if (j >= I) return;
  uint32_t first, last, split;
  lbvh_node(keys, P, j, first, last, split);
  const uint32_t l = first == split ? I + split : split, r = last == split + 1 ? I + split + 1 : split + 1;
  t.child[j] = make_uint2(l, r);
  t.range[j] = make_uint2(first, last);
  t.parent[l] = j; t.parent[r] = j;
}

// pass 5
__global__ void __launch_bounds__(256) rebuild_depth_kernel(uint32_t I, const uint32_t* parent, uint32_t* depth, uint32_t* iota) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  uint32_t d = 0;
  for (uint32_t c = i; c != 0; c = parent[c]) ++d;
  depth[i] = d;
  iota[i] = i;
}
// depth[] sorted: levelStart[d] = the first position of depth d, levelStart[D + 1] = I for the largest depth D, which goes to
// levelStart[kRebuildMaxDepth + 1] (every depth 0 .. D has a node; the array was cleared before)
__global__ void __launch_bounds__(256) rebuild_levels_kernel(uint32_t I, const uint32_t* depth, uint32_t* levelStart) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= I) return;
  const uint32_t d = depth[k];
  if (d >= kRebuildMaxDepth) { if (k == I - 1) levelStart[kRebuildMaxDepth + 1] = d; return; }   // (cannot happen; the driver refuses it)
  if (k == 0 || depth[k - 1] != d) levelStart[d] = k;
  if (k == I - 1) { levelStart[d + 1] = I; levelStart[kRebuildMaxDepth + 1] = d; }
}

// pass 6: interior node i from its children's boxes - the child whose box centre is nearer the origin first (the builder's rule,
// host/bvh_sah.cpp), the lower-key child on a tie; the union in that order, as the refit forms it
__device__ __forceinline__ void rebuild_interior(uint32_t i, const RebuildTree& t, uint32_t* err) {
  const uint2 c = t.child[i];
  const Box3 l = refit_load_box(t.boxes, c.x), r = refit_load_box(t.boxes, c.y);
  const bool sw = box_centre_dist2(r) < box_centre_dist2(l);
  const Box3 u = sw ? box_union(r, l) : box_union(l, r);
  t.swapped[i] = sw ? 1 : 0;
  const uint32_t hl = t.height[c.x], hr = t.height[c.y];
  t.height[i] = 1u + (hl > hr ? hl : hr);
  rebuild_store_box(t.boxes, i, u);
  rebuild_check_box(u, err);
}
__global__ void __launch_bounds__(256) rebuild_level_kernel(const uint32_t* order, uint32_t begin, uint32_t count, RebuildTree t, uint32_t* err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  rebuild_interior(order[begin + k], t, err);
}
// depths first, first - 1, .. 0 in one workgroup. The barrier orders every level's box stores before the next level's loads
// (workgroup scope, as in refit_top_kernel).
__global__ void __launch_bounds__(kRefitTopThreads) rebuild_top_kernel(const uint32_t* order, const uint32_t* levelStart, uint32_t first, RebuildTree t, uint32_t* err) {
  for (uint32_t d = first + 1; d-- > 0;) {
    const uint32_t b = levelStart[d], e = levelStart[d + 1];
    for (uint32_t k = b + threadIdx.x; k < e; k += blockDim.x) rebuild_interior(order[k], t, err);
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t rebuild_size(const RebuildTree& t, uint32_t n) {
  if (n >= t.numPrims - 1) return 1u;
  const uint2 r = t.range[n];
  return 2u * (r.y - r.x + 1u) - 1u;
}

// pass 7: the sum over the ancestors of 1 where the node lies in their first child, 1 + size(first child) where in their second
__global__ void __launch_bounds__(256) rebuild_preorder_kernel(RebuildTree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= 2 * t.numPrims - 1) return;
  uint32_t at = 0;
  for (uint32_t c = n; c != 0;) {
    const uint32_t a = t.parent[c];
    const uint2 ch = t.child[a];
    const uint32_t firstChild = t.swapped[a] ? ch.y : ch.x;
    at += c == firstChild ? 1u : 1u + rebuild_size(t, firstChild);
    c = a;
  }
  t.index[n] = at;
}

// pass 8: the refit's order of the new topology. Slot i (a preorder index) gets (height, i), so that the stable sort by height
// leaves every height's nodes in preorder - the order the host derivation of a scene's first update gives them.
__global__ void __launch_bounds__(256) rebuild_heightkey_kernel(RebuildTree t, uint32_t* keys, uint32_t* vals) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= 2 * t.numPrims - 1) return;
  const uint32_t i = t.index[n];
  keys[i] = t.height[n];
  vals[i] = i;
}
// height[] sorted, N entries: heightStart[h] = the first position of height h, heightStart[H + 1] = N for the largest height H,
// which goes to the last slot (every height 0 .. H has a node; the array was cleared before)
__global__ void __launch_bounds__(256) rebuild_heights_kernel(uint32_t N, const uint32_t* height, uint32_t* heightStart) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const uint32_t h = height[k];
  if (h > kRebuildMaxDepth) { if (k == N - 1) heightStart[kRebuildHeightSlots - 1] = h; return; }   // (cannot happen; the driver refuses it)
  if (k == 0 || height[k - 1] != h) heightStart[h] = k;
  if (k == N - 1) { heightStart[h + 1] = N; heightStart[kRebuildHeightSlots - 1] = h; }
}

// pass 10: node n's records at its preorder index, as buildDeviceScene (raylib.hip) derives them at create from the compact nodes
// and the geometry; interior nodes leave zero records behind, as at create. prims[i]: what a later refit computes node i's box from.
__global__ void __launch_bounds__(256) rebuild_scatter_kernel(RebuildTree t, const RebuildPrim* canon, RefitGeom g, mi_bvh_node* cnodes,
                                                              GNode* nodes, GLeaf* leaves, GLeafRot* rot, float* leafNormals, GLeafFrame* leafFrames, RefitPrim* prims) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t P = t.numPrims, I = P - 1;
  if (n >= 2 * P - 1) return;
  const uint32_t i = t.index[n];
  const uint32_t end = i + rebuild_size(t, n);
  mi_bvh_node c;
  box_encode(refit_load_box(t.boxes, n), c.min_x, c.min_y, c.min_z, c.dx, c.dy, c.dz);
  GNode nd;
  nd.minx = c.min_x; nd.maxx = c.min_x + half_bits_to_float(c.dx);          // CompactBVH2Node.cpp:8-10, one rounded add each
  nd.miny = c.min_y; nd.maxy = c.min_y + half_bits_to_float(c.dy);
  nd.minz = c.min_z; nd.maxz = c.min_z + half_bits_to_float(c.dz);
  nd.link = end << 5;
  GLeaf L;
  GLeafRot R;
  __builtin_memset(&L, 0, sizeof L);
  __builtin_memset(&R, 0, sizeof R);
  float vn[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  GLeafFrame F = leaf_frame_zero();      // (scenes without vertex normals: the tangent frame about a triangle's or disc's normal, leaf_frame.hpp)
  RefitPrim rp;
  if (n < I) {
    const uint2 ch = t.child[n];
    c.geom_id = MI_INVALID_GEOM;
    c.prim_or_second_child = i + 1u + rebuild_size(t, t.swapped[n] ? ch.y : ch.x);
    nd.hit = (i + 1u) << 5;
    rp.a = c.prim_or_second_child; rp.b = 0u; rp.c = 0u; rp.kind = REFIT_INTERIOR;
  } else {
    const RebuildPrim p = canon[t.sorted[n - I]];
    rp.a = p.a; rp.b = p.b; rp.c = p.c; rp.kind = p.kind;
    c.geom_id = (uint16_t)p.geomID;
    c.prim_or_second_child = p.primID;
    nd.hit = (end << 5) | kLeafFlag;
    L.primID = p.primID; L.matIndex = p.matIndex;
    if (p.kind == REFIT_TRI) {
      const f3 p0 = refit_vertex(g.verts, p.a), p1 = refit_vertex(g.verts, p.b), p2 = refit_vertex(g.verts, p.c);
      L.f[0] = p0.x; L.f[1] = p0.y; L.f[2] = p0.z; L.f[3] = p1.x; L.f[4] = p1.y; L.f[5] = p1.z; L.f[6] = p2.x; L.f[7] = p2.y; L.f[8] = p2.z;
      L.type = LEAF_TRI | (p.geomID << 16); L.triBase = p.triBase;
      const f3 fn = normalized(cross(p1 - p0, p2 - p0));                        // Mesh.hpp:112-114
      L.n[0] = fn.x; L.n[1] = fn.y; L.n[2] = fn.z;
      if (g.normals) {
        const uint32_t v[3] = {p.a, p.b, p.c};
        for (int k = 0; k < 3; ++k) { const mi_vec3 q = g.normals[v[k]]; vn[3 * k] = q.x; vn[3 * k + 1] = q.y; vn[3 * k + 2] = q.z; }
      }
      if (leafFrames) F = leaf_frame_of(fn);
    } else if (p.kind == REFIT_SPHERE) {
      const mi_sphere s = g.spheres[p.a];
      L.f[0] = s.x; L.f[1] = s.y; L.f[2] = s.z; L.f[3] = s.radius; L.f[4] = s.radius * s.radius;   // Primitives.hpp:44
      L.type = LEAF_SPHERE | (p.geomID << 16);
    } else {
      const mi_disc d = g.discs[p.a];
      L.f[0] = d.nx; L.f[1] = d.ny; L.f[2] = d.nz; L.f[3] = d.cx; L.f[4] = d.cy; L.f[5] = d.cz; L.f[6] = d.r * d.r;
      L.type = LEAF_DISC | (p.geomID << 16);
      if (leafFrames) F = leaf_frame_of(mk(L.f[0], L.f[1], L.f[2]));
    }
    // GLeafRot: block kz = the record's floats, a triangle's vertex components rotated so that component kz comes last
    for (uint32_t kz = 0; kz < 3; ++kz) {
      GLeafBlock& B = R.b[kz];
      B.type = L.type;
      for (int q = 0; q < 9; ++q) B.f[q] = L.f[q];
      if (p.kind == REFIT_TRI) {
        const uint32_t kx = (kz + 1) % 3, ky = (kz + 2) % 3;
        for (int v = 0; v < 3; ++v) { B.f[3 * v] = L.f[3 * v + kx]; B.f[3 * v + 1] = L.f[3 * v + ky]; B.f[3 * v + 2] = L.f[3 * v + kz]; }
      }
    }
  }
  cnodes[i] = c;
  prims[i] = rp;
  nodes[i] = nd;
  leaves[i] = L;
  rot[i] = R;
  if (leafNormals) for (int k = 0; k < 9; ++k) leafNormals[9 * (size_t)i + k] = vn[k];
  if (leafFrames) leafFrames[i] = F;
}

}  // namespace mi
