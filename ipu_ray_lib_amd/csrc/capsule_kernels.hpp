// capsule_kernels.hpp — capsule queries of a live scene (mi_capsule_query* / mi_capsule_offsets* / mi_capsule_fill*,
// include/mi_raylib.h): every primitive within a radius of a caller's segment - a robot link, a limb, a character's body, the
// volume a ball sweeps on a straight move. The form is that of the box queries (box_kernels.hpp): any / count, or
// count -> prefix sum -> fill. The kernels are the touch family's (touch_kernels.hpp: touch_query_kernel, touch_count_kernel,
// touch_fill_kernel over CapsuleTouch); what is the capsules' own is here:
//
//   capsule_walk         walk_preorder (bvh_walk.hpp) with capsule_meets_bounds (capsule_math.hpp) at the nodes - the six compares
//                        against the query's world bounds, then the three lateral axes and the axis d, the six subtractions
//                        shared by the four - and capsule_touches_prim at a reached leaf: the same bounds test on the primitive's
//                        own bounds, then the test of its kind. accept(leaf index, geomID, contained) is called for each touching
//                        primitive; returning true ends the walk.
//   load_capsule         a capsule's two 16-byte loads.
//   CapsuleTouch         the two as the touch family takes them; a record's flags are MI_OVERLAP_CONTAINED or 0.
// A lane carries the struct Capsule across the walk - the ends and d (9 floats), radius, r2 and dd (3), the world bounds (6), the
// four widths (4) -, all in named registers: nothing is indexed, no per-lane array, no LDS, no scratch. The node test is written
// with & and |, not && and ||: its result selects between nd.hit and nd.link, and a short-circuit would have the compiler branch
// around that select (DESIGN.md §32 records the trap for near_walk). The host twin (host/capsule_query_host.cpp) returns the same
// bytes and the same visit totals.
#pragma once

#include "touch_kernels.hpp"
#include "capsule_math.hpp"

namespace mi {

static_assert(sizeof(mi_capsule) == 32, "mi_capsule must stay 32 bytes (two 16-byte loads)");

template <bool STATS, class Accept>
__device__ __forceinline__ void capsule_walk(const DeviceScene& sc, f3 a, f3 b, float radius, CastStats& cs, const Accept& accept) {
  const Capsule q = capsule_make(a, b, radius);
  walk_preorder<STATS>(sc, capsule_query_valid(a, b, radius), cs,
    [&](const GNode& nd) { return capsule_meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), q); },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      bool contained;
      return capsule_touches_prim(type & 0xFFFFu, f, q, &contained) && accept(at, type >> 16, contained);
    });
}

// mi_capsule: a[3], radius, b[3], reserved - two 16-byte loads
__device__ __forceinline__ void load_capsule(const mi_capsule* capsules, uint32_t idx, f3& a, f3& b, float& radius) {
  const float4* p = reinterpret_cast<const float4*>(capsules) + 2 * (size_t)idx;
  const float4 lo = p[0], hi = p[1];
  a = mk(lo.x, lo.y, lo.z);
  radius = lo.w;
  b = mk(hi.x, hi.y, hi.z);
}

struct CapsuleTouch {
  using Item = mi_capsule;
  using Record = mi_overlap;
  struct Loaded { f3 a, b; float radius; };
  static constexpr const char *kQuery = "mi_capsule_query", *kOffsets = "mi_capsule_offsets", *kFill = "mi_capsule_fill", *kNoun = "capsules";
  static __device__ __forceinline__ Loaded load(const mi_capsule* capsules, uint32_t idx) {
    Loaded c;
    load_capsule(capsules, idx, c.a, c.b, c.radius);
    return c;
  }
  template <bool STATS, class Accept>
  static __device__ __forceinline__ void walk(const DeviceScene& sc, const Loaded& c, CastStats& cs, const Accept& accept) {
    capsule_walk<STATS>(sc, c.a, c.b, c.radius, cs, [&](uint32_t at, uint32_t geomID, bool contained) { return accept(at, geomID, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u); });
  }
};

}  // namespace mi
