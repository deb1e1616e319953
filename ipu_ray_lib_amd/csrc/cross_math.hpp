// cross_math.hpp — the arithmetic of crossing counts that has no reference counterpart (mi_count_query / mi_point_sign,
// include/mi_raylib.h): how often a ray crosses a sphere's shell inside its interval. One definition, compiled by hipcc for
// count_crossings (count_kernels.hpp) and list_crossings (list_kernels.hpp) and by g++ for mi_sphere_crossings_host and
// mi_sphere_roots_host (host/cross_host.cpp): a sequence of single
// binary32 operations in the order written (no contraction, correctly rounded divide and sqrt on both sides), so the two return
// the same bits. A dot product is (x x' + y y') + z z' (ray_math.h dot).
#pragma once

#include "ray_math.h"

namespace mi {

// Crossings of the shell of the sphere (centre c, squared radius radius2) by the ray o + t d with tMin < t < tMax: 0, 1 or 2.
// The reference's sphere test (Primitives.cpp:24-47, intersect_sphere in trace_kernels.hpp) answers ONE t, gives up when the
// centre lies behind the origin (tca < 0) even for an origin inside the sphere, and scales td by 1 / d.d where sqrt(1 / d.d)
// is meant; a parity needs both roots, so this is a test of its own:
//   - no tca < 0 early-out: an origin inside the sphere with the centre behind it counts the one crossing ahead;
//   - t is in units of d for any length of d: tca = (f.d) / d.d and td = sqrt((radius2 - l2) / d.d);
//   - a tangent ray (td == 0) has t0 == t1, so it adds 0 or 2 and a parity survives it;
//   - a NaN never counts: !(l2 <= radius2) is true for a NaN l2, and a NaN root fails both ordered compares.
MI_HD uint32_t sphere_crossings(f3 c, float radius2, f3 o, f3 d, float tMin, float tMax) {
  const f3 f = c - o;
  const float dd = dot(d, d);
  const float tca = dot(f, d) / dd;
  const f3 l = f - d * tca;
  const float l2 = dot(l, l);
  if (!(l2 <= radius2)) return 0u;
  const float td = sqrtf((radius2 - l2) / dd);
  const float t0 = tca - td, t1 = tca + td;
  return (uint32_t)(t0 > tMin && t0 < tMax) + (uint32_t)(t1 > tMin && t1 < tMax);
}

// The same crossings with their t, for the crossing lists (mi_list_fill, list_kernels.hpp): the operations of sphere_crossings in
// the same order, so popcount(sphere_roots(...)) == sphere_crossings(...) bit for bit of every input. Returns a mask of the
// accepted roots - bit 0: the near root t0, written to t[0]; bit 1: the far root t1, written to t[1] (the one a list marks
// MI_CROSS_FAR). When the line misses the sphere (or l2 is NaN) t[] is left as it was and the mask is 0.
MI_HD uint32_t sphere_roots(f3 c, float radius2, f3 o, f3 d, float tMin, float tMax, float t[2]) {
  const f3 f = c - o;
  const float dd = dot(d, d);
  const float tca = dot(f, d) / dd;
  const f3 l = f - d * tca;
  const float l2 = dot(l, l);
  if (!(l2 <= radius2)) return 0u;
  const float td = sqrtf((radius2 - l2) / dd);
  const float t0 = tca - td, t1 = tca + td;
  t[0] = t0; t[1] = t1;
  return (uint32_t)(t0 > tMin && t0 < tMax) | ((uint32_t)(t1 > tMin && t1 < tMax) << 1);
}

}  // namespace mi
