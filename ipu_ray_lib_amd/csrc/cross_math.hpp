// cross_math.hpp — the arithmetic of crossing counts that has no reference counterpart (mi_count_query / mi_point_sign,
// include/mi_raylib.h): how often a ray crosses a sphere's shell inside its interval. One definition, compiled by hipcc for
// count_crossings (count_kernels.hpp) and by g++ for mi_sphere_crossings_host (host/cross_host.cpp): a sequence of single
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

}  // namespace mi
