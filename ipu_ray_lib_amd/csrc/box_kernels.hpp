// box_kernels.hpp — box queries of a live scene (mi_box_query* / mi_box_offsets* / mi_box_fill*, include/mi_raylib.h): every
// primitive that TOUCHES a caller's axis-aligned box - a voxel, a culling cell, a broad-phase cell (Open3D's
// VoxelGrid.create_from_triangle_mesh, PCL's boxSearch, a physics engine's overlap-box). The form is that of the neighbour
// lists (near_kernels.hpp): any / count, or count -> prefix sum -> fill. The kernels are the touch family's
// (touch_kernels.hpp: touch_query_kernel, touch_count_kernel, touch_fill_kernel over BoxTouch); what is the boxes' own is here:
//
//   BoxShape             (box_math.hpp) what touch_walk runs: a box-box compare at the nodes (box_meets_bounds: closed, no
//                        arithmetic) and box_touches_prim (the primitive's own bounds, then for a triangle the separating-axis
//                        test) at a reached leaf; a record's flags are MI_OVERLAP_CONTAINED or 0.
//   load_box             a box's two 16-byte loads.
//   BoxTouch             the shape, the loads and the entries' names, as the touch kernels take them.
// The host twin (host/touch_host.hpp over the same BoxShape) returns the same bytes and the same visit totals.
#pragma once

#include "touch_kernels.hpp"

namespace mi {

static_assert(sizeof(mi_box) == 32, "mi_box must stay 32 bytes (two 16-byte loads)");
static_assert(sizeof(mi_overlap) == 16, "mi_overlap must stay 16 bytes (one 16-byte load or store)");

// mi_box: lo[3], reserved0, hi[3], reserved1 - two 16-byte loads
__device__ __forceinline__ void load_box(const mi_box* boxes, uint32_t idx, f3& lo, f3& hi) {
  const float4 a = reinterpret_cast<const float4*>(boxes)[2 * (size_t)idx], b = reinterpret_cast<const float4*>(boxes)[2 * (size_t)idx + 1];
  lo = mk(a.x, a.y, a.z);
  hi = mk(b.x, b.y, b.z);
}

struct BoxTouch : SharedWalk<BoxShape> {
  static constexpr const char *kQuery = "mi_box_query", *kOffsets = "mi_box_offsets", *kFill = "mi_box_fill";
  static __device__ __forceinline__ Fields load(const mi_box* boxes, uint32_t idx) {
    Fields b;
    load_box(boxes, idx, b.lo, b.hi);
    return b;
  }
};

}  // namespace mi
