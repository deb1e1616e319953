// obox_kernels.hpp — oriented-box queries of a live scene (mi_obox_query* / mi_obox_offsets* / mi_obox_fill*, include/mi_raylib.h):
// every primitive that TOUCHES a caller's rotated box - a rigid body's bounding box, a robot link, a beam, a selection volume, a
// voxel of a rotated grid. The form is that of the box queries (box_kernels.hpp): any / count, or count -> prefix
// sum -> fill. The kernels are the touch family's (touch_kernels.hpp: touch_query_kernel, touch_count_kernel, touch_fill_kernel
// over OBoxTouch); what is the oriented boxes' own is here:
//
//   obox_walk            walk_preorder (bvh_walk.hpp) with obox_meets_bounds (obox_math.hpp) at the nodes - the six compares against
//                        the query's world bounds, then the three slabs of the box's own frame, the six subtractions shared by
//                        the three axes - and obox_touches_prim at a reached leaf: the same bounds test on the primitive's own
//                        bounds, then the box family's test in the box's frame. accept(leaf index, geomID, contained) is called
//                        for each touching primitive; returning true ends the walk.
//   load_obox            an oriented box's three 16-byte loads.
//   OBoxTouch            the two as the touch kernels take them, on top of the family's shape (OBoxShape, obox_math.hpp: item, record
//                        and the argument rules' words); a record's flags are MI_OVERLAP_CONTAINED or 0. The walk stays written out
//                        here: through touch_walk over OBoxShape the same arithmetic compiles to other code - operands of
//                        commutative instructions change places - and the device code is held fixed.
// A lane carries the frame (9 floats), the centre and half extents (6) and the world bounds (6) across the walk, all in named
// registers: nothing is indexed, no per-lane array, no LDS, no scratch. The node test is written with & and |, not && and ||: its
// result selects between nd.hit and nd.link, and a short-circuit would have the compiler branch around that select (DESIGN.md
// §32 records the trap for near_walk). The host twin (host/touch_host.hpp over OBoxShape) returns the same bytes and the same visit
// totals.
#pragma once

#include "touch_kernels.hpp"
#include "obox_math.hpp"

namespace mi {

static_assert(sizeof(mi_obox) == 48, "mi_obox must stay 48 bytes (three 16-byte loads)");

template <bool STATS, class Accept>
__device__ __forceinline__ void obox_walk(const DeviceScene& sc, f3 c, f3 h, float4 quat, CastStats& cs, const Accept& accept) {
  const OBox q = obox_make(c, h, quat.x, quat.y, quat.z, quat.w);
  walk_preorder<STATS>(sc, obox_query_valid(c, h, quat.x, quat.y, quat.z, quat.w), cs,
    [&](const GNode& nd) { return obox_meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), q); },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      bool contained;
      return obox_touches_prim(type & 0xFFFFu, f, q, &contained) && accept(at, type >> 16, contained);
    });
}

// mi_obox: centre[3], reserved0, half[3], reserved1, quat[4] - three 16-byte loads
__device__ __forceinline__ void load_obox(const mi_obox* oboxes, uint32_t idx, f3& c, f3& h, float4& quat) {
  const float4* p = reinterpret_cast<const float4*>(oboxes) + 3 * (size_t)idx;
  const float4 a = p[0], b = p[1];
  c = mk(a.x, a.y, a.z);
  h = mk(b.x, b.y, b.z);
  quat = p[2];
}

struct OBoxTouch : OBoxShape {
  struct Loaded { f3 c, h; float4 quat; };
  static constexpr const char *kQuery = "mi_obox_query", *kOffsets = "mi_obox_offsets", *kFill = "mi_obox_fill";
  static __device__ __forceinline__ Loaded load(const mi_obox* oboxes, uint32_t idx) {
    Loaded b;
    load_obox(oboxes, idx, b.c, b.h, b.quat);
    return b;
  }
  template <bool STATS, class Accept>
  static __device__ __forceinline__ void walk(const DeviceScene& sc, const Loaded& b, CastStats& cs, const Accept& accept) {
    obox_walk<STATS>(sc, b.c, b.h, b.quat, cs, [&](uint32_t at, uint32_t geomID, bool contained) { return accept(at, geomID, flags(contained)); });
  }
};

}  // namespace mi
