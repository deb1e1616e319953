// frustum_kernels.hpp — frustum queries of a live scene (mi_frustum_query* / mi_frustum_offsets* / mi_frustum_fill*,
// include/mi_raylib.h): every primitive inside or touching the region that six caller-supplied planes leave - a camera's view
// volume, a screen tile's sub-frustum, a marquee selection, a shadow cascade, a half-space, a slab. The form is that of the box
// queries (box_kernels.hpp): any / count, or count -> prefix sum -> fill. The kernels are the touch family's
// (touch_kernels.hpp: touch_query_kernel, touch_count_kernel, touch_fill_kernel over FrustumTouch); what is the frusta's own is
// here:
//
//   FrustumShape         (frustum_math.hpp) what touch_walk runs: frustum_meets_bounds at the nodes - per plane the corner of the
//                        box farthest along the normal, nothing else: the region has no finite world bounds - and
//                        frustum_touches_prim at a reached leaf: the same bounds test on the primitive's own bounds, then the
//                        test of its kind; a record's flags are MI_OVERLAP_CONTAINED or 0.
//   load_frustum         a frustum's six 16-byte loads.
//   FrustumTouch         the shape, the loads and the entries' names, as the touch kernels take them.
// A lane carries the struct Frustum across the walk - six planes, 24 floats -, all in named registers: nothing is indexed, no
// per-lane array, no LDS, no scratch. The node test is written with |, not ||: its result selects between nd.hit and nd.link, and
// a short-circuit would have the compiler branch around that select (DESIGN.md §32 records the trap for near_walk). The host twin
// (host/touch_host.hpp over the same FrustumShape) returns the same bytes and the same visit totals.
#pragma once

#include "touch_kernels.hpp"
#include "frustum_math.hpp"

namespace mi {

static_assert(sizeof(mi_frustum) == 96, "mi_frustum must stay 96 bytes (six 16-byte loads)");

// mi_frustum: six planes nx, ny, nz, d - six 16-byte loads
__device__ __forceinline__ FPlane frustum_plane_of(float4 v) {
  FPlane p;
  p.x = v.x;
  p.y = v.y;
  p.z = v.z;
  p.d = v.w;
  return p;
}
__device__ __forceinline__ void load_frustum(const mi_frustum* frusta, uint32_t idx, Frustum& q) {
  const float4* p = reinterpret_cast<const float4*>(frusta) + 6 * (size_t)idx;
  const float4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3], v4 = p[4], v5 = p[5];
  q.p0 = frustum_plane_of(v0);
  q.p1 = frustum_plane_of(v1);
  q.p2 = frustum_plane_of(v2);
  q.p3 = frustum_plane_of(v3);
  q.p4 = frustum_plane_of(v4);
  q.p5 = frustum_plane_of(v5);
}

struct FrustumTouch : SharedWalk<FrustumShape> {
  static constexpr const char *kQuery = "mi_frustum_query", *kOffsets = "mi_frustum_offsets", *kFill = "mi_frustum_fill";
  static __device__ __forceinline__ Fields load(const mi_frustum* frusta, uint32_t idx) {
    Fields q;
    load_frustum(frusta, idx, q);
    return q;
  }
};

}  // namespace mi
