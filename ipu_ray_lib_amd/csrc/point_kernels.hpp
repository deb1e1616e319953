// point_kernels.hpp — point queries on caller-supplied point batches (mi_point_query / mi_point_query_device, include/mi_raylib.h):
//   for each point, the primitive of the live BVH nearest to it within the point's radius, the distance and the closest point on
//   that primitive (MI_POINT_CLOSEST, Embree's rtcPointQuery), or whether any primitive lies within the radius (MI_POINT_WITHIN).
//
//   point_query_kernel   one thread per point, the form of query_plain_kernel (DESIGN.md §6 measured it faster than the persistent
//                        form for ray queries). The walk is walk_preorder (bvh_walk.hpp) with a distance test at the nodes: the
//                        squared distance of the point from the node's box is compared with the best squared distance so far
//                        (radius^2 at the start), a box strictly nearer is entered, any other is passed. At a leaf so reached the
//                        primitive's closest point is evaluated (point_math.hpp) and accepted when strictly nearer: of equal
//                        distances the first leaf in preorder wins, and a NaN distance is never accepted.
// No LDS, no stack, no scratch: a lane carries the point, the best squared distance, the winning leaf's index, its closest point
// and barycentrics. The host twin (host/point_query_host.cpp) walks the compact nodes through the same point_math.hpp and returns
// the same bytes.
#pragma once

#include "bvh_walk.hpp"
#include "point_math.hpp"

namespace mi {

static_assert(sizeof(mi_point) == 16, "mi_point must stay 16 bytes (one 16-byte load)");
static_assert(sizeof(mi_point_hit) == 32, "mi_point_hit must stay 32 bytes (two 16-byte stores)");

constexpr uint32_t kNoPointLeaf = 0xFFFFFFFFu;

template <bool WITHIN, bool STATS>
__global__ void __launch_bounds__(256) point_query_kernel(DeviceScene sc, const mi_point* points, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const float4 pt = reinterpret_cast<const float4*>(points)[idx];      // mi_point: x, y, z, radius
    const f3 p = mk(pt.x, pt.y, pt.z);
    float best = pt.w * pt.w;
    uint32_t leaf = kNoPointLeaf;
    ClosestPoint win;
    win.q = mk(0.f, 0.f, 0.f); win.v = win.w = 0.f;
    walk_preorder<STATS>(sc, point_query_valid(p, pt.w), cs,
      [&](const GNode& nd) { return point_box_dist2(nd.minx, nd.maxx, nd.miny, nd.maxy, nd.minz, nd.maxz, p) < best; },
      [&](uint32_t at, uint32_t type, const float (&f)[9]) {
        const ClosestPoint c = closest_on_prim(type & 0xFFFFu, f, p);
        const float d2 = point_dist2(p, c.q);
        if (d2 < best) {
          leaf = at;
          if constexpr (WITHIN) return true;
          best = d2; win = c;
        }
        return false;
      });
    if constexpr (WITHIN) {
      static_cast<uint8_t*>(out)[idx] = leaf != kNoPointLeaf ? 1u : 0u;
    } else {
      // two 16-byte stores: {dist, primID, geomID | flags << 16, q.x} {q.y, q.z, b1, b2}; nothing found: the radius as given,
      // invalid ids, MI_FLAG_ESCAPED, zeros
      float4 w0, w1;
      if (leaf != kNoPointLeaf) {
        const GLeaf& L = sc.leaves[leaf];
        w0 = make_float4(sqrtf(best), __uint_as_float(L.primID), __uint_as_float(leaf_geom(L)), win.q.x);
        w1 = make_float4(win.q.y, win.q.z, win.v, win.w);
      } else {
        w0 = make_float4(pt.w, __uint_as_float(MI_INVALID_PRIM), __uint_as_float((uint32_t)MI_INVALID_GEOM | ((uint32_t)MI_FLAG_ESCAPED << 16)), 0.f);
        w1 = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float4* q = reinterpret_cast<float4*>(static_cast<mi_point_hit*>(out) + idx);
      q[0] = w0; q[1] = w1;
    }
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);      // box tests -> "nodes visited", primitive evaluations -> "leaf tests"; no casts, no paths
}

}  // namespace mi
