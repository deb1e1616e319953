// capsule_kernels.hpp — capsule queries of a live scene (mi_capsule_query* / mi_capsule_offsets* / mi_capsule_fill*,
// include/mi_raylib.h): every primitive within a radius of a caller's segment - a robot link, a limb, a character's body, the
// volume a ball sweeps on a straight move. The form is that of the box queries (box_kernels.hpp): any / count, or
// count -> prefix sum -> fill. The kernels are the touch family's (touch_kernels.hpp: touch_query_kernel, touch_count_kernel,
// touch_fill_kernel over CapsuleTouch); what is the capsules' own is here:
//
//   CapsuleShape         (capsule_math.hpp) what touch_walk runs: capsule_meets_bounds at the nodes - the six compares against the
//                        query's world bounds, then the three lateral axes and the axis d, the six subtractions shared by the
//                        four - and capsule_touches_prim at a reached leaf: the same bounds test on the primitive's own bounds,
//                        then the test of its kind; a record's flags are MI_OVERLAP_CONTAINED or 0.
//   load_capsule         a capsule's two 16-byte loads.
//   CapsuleTouch         the shape, the loads and the entries' names, as the touch kernels take them.
// A lane carries the struct Capsule across the walk - the ends and d (9 floats), radius, r2 and dd (3), the world bounds (6), the
// four widths (4) -, all in named registers: nothing is indexed, no per-lane array, no LDS, no scratch. The node test is written
// with & and |, not && and ||: its result selects between nd.hit and nd.link, and a short-circuit would have the compiler branch
// around that select (DESIGN.md §32 records the trap for near_walk). The host twin (host/touch_host.hpp over the same
// CapsuleShape) returns the same bytes and the same visit totals.
#pragma once

#include "touch_kernels.hpp"
#include "capsule_math.hpp"

namespace mi {

static_assert(sizeof(mi_capsule) == 32, "mi_capsule must stay 32 bytes (two 16-byte loads)");

// mi_capsule: a[3], radius, b[3], reserved - two 16-byte loads
__device__ __forceinline__ void load_capsule(const mi_capsule* capsules, uint32_t idx, f3& a, f3& b, float& radius) {
  const float4* p = reinterpret_cast<const float4*>(capsules) + 2 * (size_t)idx;
  const float4 lo = p[0], hi = p[1];
  a = mk(lo.x, lo.y, lo.z);
  radius = lo.w;
  b = mk(hi.x, hi.y, hi.z);
}

struct CapsuleTouch : SharedWalk<CapsuleShape> {
  static constexpr const char *kQuery = "mi_capsule_query", *kOffsets = "mi_capsule_offsets", *kFill = "mi_capsule_fill";
  static __device__ __forceinline__ Fields load(const mi_capsule* capsules, uint32_t idx) {
    Fields c;
    load_capsule(capsules, idx, c.a, c.b, c.radius);
    return c;
  }
};

}  // namespace mi
