// contact_kernels.hpp — triangle queries of a live scene (mi_tri_query* / mi_tri_offsets* / mi_tri_fill*, include/mi_raylib.h):
// every primitive that TOUCHES a caller's triangle - one face of another mesh (Embree's rtcCollide, FCL's collision manager), a
// cutting plane's facet, a sweep's cap. The form is that of the box queries (box_kernels.hpp): any / count, or
// count -> prefix sum -> fill. The kernels are the touch family's (touch_kernels.hpp: touch_query_kernel, touch_count_kernel,
// touch_fill_kernel over TriTouch); what is the triangles' own is here:
//
//   tri_walk             walk_preorder (bvh_walk.hpp) with the query's bounds [qmn, qmx] for the box at the nodes
//                        (box_meets_bounds: closed, no arithmetic; no plane test there) and tri_touches_prim (contact_math.hpp:
//                        the primitive's own bounds, then for a triangle the 17-axis separating-axis test relative to q0) at a
//                        reached leaf. accept(leaf index, geomID) is called for each touching primitive; returning true ends the
//                        walk. A primitive's bounds are computed from the whole record (nine floats of a triangle, seven of a
//                        disc), so there is no word whose load the bounds compare could spare.
//   load_tri             a triangle's nine 4-byte loads.
//   TriTouch             the two as the touch kernels take them, on top of the family's shape (TriShape, contact_math.hpp: item,
//                        record and the argument rules' words); a record's flags are 0. The walk stays written out here: through
//                        touch_walk over TriShape the same arithmetic compiles to other code - operands of additions change
//                        places - and the device code is held fixed.
// A lane carries the query's nine floats and its bounds; the axes of the separating-axis test are spelled out one by one
// (contact_math.hpp). The host twin (host/touch_host.hpp over TriShape) returns the same bytes and the same visit totals.
#pragma once

#include "touch_kernels.hpp"
#include "contact_math.hpp"

namespace mi {

static_assert(sizeof(mi_tri) == 36, "mi_tri must stay 36 bytes: a float32 [n, 3, 3] array is a batch");
static_assert(sizeof(mi_contact) == 16, "mi_contact must stay 16 bytes (one 16-byte load or store)");

template <bool STATS, class Accept>
__device__ __forceinline__ void tri_walk(const DeviceScene& sc, f3 q0, f3 q1, f3 q2, CastStats& cs, const Accept& accept) {
  f3 qmn, qmx;
  tri_query_bounds(q0, q1, q2, qmn, qmx);
  walk_preorder<STATS>(sc, tri_query_valid(q0, q1, q2), cs,
    [&](const GNode& nd) { return box_meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), qmn, qmx); },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      return tri_touches_prim(type & 0xFFFFu, f, q0, q1, q2, qmn, qmx) && accept(at, type >> 16);
    });
}

// mi_tri: a[3], b[3], c[3] - nine floats at a 4-byte aligned address (36 is no multiple of 8: no wider load is aligned)
__device__ __forceinline__ void load_tri(const mi_tri* tris, uint32_t idx, f3& q0, f3& q1, f3& q2) {
  const float* p = reinterpret_cast<const float*>(tris) + 9 * (size_t)idx;
  q0 = mk(p[0], p[1], p[2]);
  q1 = mk(p[3], p[4], p[5]);
  q2 = mk(p[6], p[7], p[8]);
}

struct TriTouch : TriShape {
  struct Loaded { f3 q0, q1, q2; };
  static constexpr const char *kQuery = "mi_tri_query", *kOffsets = "mi_tri_offsets", *kFill = "mi_tri_fill";
  static __device__ __forceinline__ Loaded load(const mi_tri* tris, uint32_t idx) {
    Loaded t;
    load_tri(tris, idx, t.q0, t.q1, t.q2);
    return t;
  }
  template <bool STATS, class Accept>
  static __device__ __forceinline__ void walk(const DeviceScene& sc, const Loaded& t, CastStats& cs, const Accept& accept) {
    tri_walk<STATS>(sc, t.q0, t.q1, t.q2, cs, [&](uint32_t at, uint32_t geomID) { return accept(at, geomID, 0u); });
  }
};

}  // namespace mi
