// count_kernels.hpp — crossing counts of a live scene (mi_count_query / mi_count_query_device, mi_point_sign / mi_point_sign_device,
// include/mi_raylib.h): how many surfaces a ray crosses inside its interval, and from the parity of that count whether a point
// lies inside (Open3D's count_intersections / compute_occupancy / compute_signed_distance).
//
//   count_crossings      walk_preorder (bvh_walk.hpp) with the literal box test of traverse<> over the FIXED interval [tMin, tMax]
//                        (ray_meets_node) - a closest-hit cast shrinks its interval and prunes what lies behind the hit, a count
//                        must not -, so the leaves visited are a function of the ray and the nodes alone and the count, a sum
//                        over them, does not depend on the visit order. A triangle or a disc adds 1 when prim_hit accepts it
//                        against tMax, a sphere adds sphere_crossings (cross_math.hpp: both roots, which the reference's one-t
//                        sphere test cannot give).
//   count_query_kernel   one thread per ray, the form of query_plain_kernel: one uint32 per ray.
//   point_sign_kernel    one thread per point: the ray from the point along the launch's direction over (0, +inf); an odd count is
//                        "inside". MI_SIGN_INSIDE writes a byte; MI_SIGN_DISTANCE finds the record point_query_kernel wrote for
//                        the point and sets the sign bit of dist and MI_FLAG_INSIDE in place.
// No LDS, no stack, no scratch: a lane carries the ray (origin, direction, reciprocal, shear), the interval, the node offset and
// one counter.
#pragma once

#include "bvh_walk.hpp"
#include "query_kernels.hpp"      // load_query_ray
#include "point_math.hpp"         // point_query_valid
#include "cross_math.hpp"

namespace mi {

// The literal box test of traverse<> over the FIXED interval [tMin, tMax] (never narrowed by a hit: nothing is pruned): what the
// walks of count_crossings and list_crossings (list_kernels.hpp) enter a node by.
__device__ __forceinline__ bool ray_meets_node(const GNode& nd, f3 o, f3 inv, float tMin, float tMax) {
  float t0 = tMin, t1 = tMax;
  box_hit_literal_axis((nd.minx - o.x) * inv.x, (nd.maxx - o.x) * inv.x, t0, t1);
  box_hit_literal_axis((nd.miny - o.y) * inv.y, (nd.maxy - o.y) * inv.y, t0, t1);
  box_hit_literal_axis((nd.minz - o.z) * inv.z, (nd.maxz - o.z) * inv.z, t0, t1);
  return !(t0 > t1);
}

template <bool STATS, bool DF>
__device__ __forceinline__ uint32_t count_crossings(const DeviceScene& sc, f3 o, f3 d, float tMin, float tMax, CastStats& cs) {
  const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
  const Shear sh = make_shear(d, inv);
  uint32_t count = 0;
  walk_preorder<STATS>(sc, true, cs,
    [&](const GNode& nd) { return ray_meets_node(nd, o, inv, tMin, tMax); },
    [&](uint32_t, uint32_t type, const float (&f)[9]) {
      const GLeafBlock B = {type, {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]}};
      if (leaf_kind(B) == LEAF_SPHERE) {
        count += sphere_crossings(mk(B.f[0], B.f[1], B.f[2]), B.f[4], o, d, tMin, tMax);
      } else {
        float t, b0, b1, b2;
        count += prim_hit<DF>(B, o, d, sh, tMin, tMax, t, b0, b1, b2) ? 1u : 0u;
      }
      return false;
    });
  return count;
}

template <bool STATS, bool DF>
__global__ void __launch_bounds__(256) count_query_kernel(DeviceScene sc, const mi_ray* rays, uint32_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const QueryRay r = load_query_ray(rays, idx);
    counts[idx] = count_crossings<STATS, DF>(sc, r.o, r.d, r.tMin, r.tMax, cs);
  }
  flush_stats(sc, idx < n ? 1u : 0u, cs, 0u);
}

// DISTANCE: `out` holds the n mi_point_hit records point_query_kernel<false, ...> wrote for these points on the same stream
template <bool DISTANCE, bool STATS, bool DF>
__global__ void __launch_bounds__(256) point_sign_kernel(DeviceScene sc, const mi_point* points, void* out, f3 dir, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  uint32_t walked = 0;
  if (idx < n) {
    const float4 pt = reinterpret_cast<const float4*>(points)[idx];      // mi_point: x, y, z, radius
    const f3 p = mk(pt.x, pt.y, pt.z);
    // INSIDE ignores the radius: every point with finite coordinates is walked; DISTANCE walks what the point query walked
    const bool valid = DISTANCE ? point_query_valid(p, pt.w) : point_query_valid(p, 0.f);
    bool inside = false;
    if (valid) {
      walked = 1;
      inside = (count_crossings<STATS, DF>(sc, p, dir, 0.f, kInf, cs) & 1u) != 0u;
    }
    if constexpr (DISTANCE) {
      if (inside) {
        // the record's words 0 and 2: dist gets its sign bit, flags (the high half of word 2) MI_FLAG_INSIDE
        uint32_t* rec = reinterpret_cast<uint32_t*>(static_cast<mi_point_hit*>(out) + idx);
        rec[0] |= 0x80000000u;
        rec[2] |= (uint32_t)MI_FLAG_INSIDE << 16;
      }
    } else {
      static_cast<uint8_t*>(out)[idx] = inside ? 1u : 0u;
    }
  }
  flush_stats(sc, walked, cs, 0u);
}

}  // namespace mi
