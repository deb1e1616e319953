// near_kernels.hpp — neighbour lists of a live scene (mi_near_offsets* / mi_near_fill*, include/mi_raylib.h): EVERY primitive
// strictly within a point's radius, nearest first, not only the nearest one (point_kernels.hpp); PCL's radiusSearch /
// nearestKSearch, Open3D's search_radius_vector_3d / search_knn_vector_3d. The form is that of the crossing lists
// (list_kernels.hpp): count -> prefix sum -> fill.
//
//   near_walk            walk_preorder (bvh_walk.hpp) with point_query_kernel's box distance, closest_on_prim and point_dist2
//                        (point_math.hpp). A node is entered when its box distance db satisfies
//                        db < r2 && db <= bound: `bound` is +inf for the count - the FIXED radius alone decides, so the set of
//                        neighbours is a function of the point and the geometry - and may be lowered by the fill's accept.
//                        accept(d2, leaf index, geomID) is called for each primitive of a reached leaf with d2 < r2 (strictly; a NaN never).
//   near_count_kernel    one thread per point: the number of neighbours, stored as 64 bits (scan_*_kernel of list_kernels.hpp then
//                        runs in place on them).
//   near_fill_kernel     one thread per point: list_fill_kernel's insertion into the point's OWN segment [offsets[i],
//                        offsets[i + 1]) cut at `capacity`, the order by a key of the neighbour itself - dist2 as a float, then
//                        geomID, then primID. Once the segment is full the walk's bound is the last record's dist2: a box farther
//                        than it holds nothing that would be kept, a box at exactly that distance may (an equal-distance primitive
//                        with smaller ids displaces the last record), hence `<=`. The bound lives in a register and is updated
//                        when the last record changes; it is never read back from memory. A point whose segment is empty is not
//                        walked.
// No LDS, no stack, no per-lane array, no scratch: a lane carries the point, r2, the bound, the segment's base and length, the
// number of records held and the record being placed. The host twin (host/point_query_host.cpp) passes the same two lambdas to
// walkHost over the compact nodes and returns the same bytes and the same visit totals.
#pragma once

#include "list_kernels.hpp"
#include "point_kernels.hpp"

namespace mi {

static_assert(sizeof(mi_neighbour) == 16, "mi_neighbour must stay 16 bytes (one 16-byte load or store)");

// A record as the four words it is stored as: {dist2, primID, geomID | flags << 16, point}
__device__ __forceinline__ uint4 neighbour_words(float d2, uint32_t primID, uint32_t geomID, uint32_t flags, uint32_t point) {
  return make_uint4(__float_as_uint(d2), primID, geomID | (flags << 16), point);
}

// a sorts before b: dist2 as a float, then geomID, then primID. An accepted dist2 is never NaN (a NaN fails d2 < r2).
__device__ __forceinline__ bool neighbour_before(const uint4& a, const uint4& b) {
  const float da = __uint_as_float(a.x), db = __uint_as_float(b.x);
  const uint64_t ra = ((uint64_t)(a.z & 0xFFFFu) << 32) | a.y, rb = ((uint64_t)(b.z & 0xFFFFu) << 32) | b.y;
  return da < db || (da == db && ra < rb);
}

// walk_preorder with the point queries' arithmetic, a fixed radius and a bound the caller may lower inside `accept`.
template <bool STATS, class Accept>
__device__ __forceinline__ void near_walk(const DeviceScene& sc, f3 p, float radius, float r2, float& bound, CastStats& cs, const Accept& accept) {
  walk_preorder<STATS>(sc, point_query_valid(p, radius), cs,
    [&](const GNode& nd) {
      const float db = point_box_dist2(nd.minx, nd.maxx, nd.miny, nd.maxy, nd.minz, nd.maxz, p);
      // (bound = +inf: db < r2 alone; db is never NaN, point_math.hpp. `&`, not `&&`: two compares and no branch, so that the
      // walk's choice between GNode.hit and GNode.link stays a select behind one 16-byte load of the node's second half)
      return (db < r2) & (db <= bound);
    },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      const ClosestPoint c = closest_on_prim(type & 0xFFFFu, f, p);
      const float d2 = point_dist2(p, c.q);
      if (d2 < r2) accept(d2, at, type >> 16);
      return false;
    });
}

// counts[i] = the number of primitives strictly within point i's radius, as 64 bits (the scan runs in place on them)
template <bool STATS>
__global__ void __launch_bounds__(256) near_count_kernel(DeviceScene sc, const mi_point* points, uint64_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const float4 pt = reinterpret_cast<const float4*>(points)[idx];      // mi_point: x, y, z, radius
    float bound = kInf;                                                   // (never lowered: the fixed radius alone decides)
    uint64_t count = 0;
    near_walk<STATS>(sc, mk(pt.x, pt.y, pt.z), pt.w, pt.w * pt.w, bound, cs, [&](float, uint32_t, uint32_t) { ++count; });
    counts[idx] = count;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);      // box tests -> "nodes visited", primitive evaluations -> "leaf tests"; no casts
}

// pointBase: what is added to the thread's index for the record's `point` field (the host entry's batches; 0 for the device entry).
template <bool STATS>
__global__ void __launch_bounds__(256) near_fill_kernel(DeviceScene sc, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits,
                                                        uint64_t capacity, uint32_t pointBase, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const uint64_t lo = offsets[idx], len = segment_len(lo, offsets[idx + 1], capacity);      // (list_segment.hpp)
    if (len) {                                                            // (an empty segment: nothing to write, no walk)
      const float4 pt = reinterpret_cast<const float4*>(points)[idx];    // mi_point: x, y, z, radius
      uint4* seg = reinterpret_cast<uint4*>(hits) + lo;                   // every access below is seg[j] with j < len
      const uint32_t point = pointBase + idx;
      uint64_t held = 0;                                                  // seg[0 .. held) is sorted, held <= len
      uint4 tail = make_uint4(0u, 0u, 0u, 0u);                            // seg[len - 1] once held == len: a copy in registers
      float bound = kInf;                                                 // its dist2; +inf while held < len
      near_walk<STATS>(sc, mk(pt.x, pt.y, pt.z), pt.w, pt.w * pt.w, bound, cs, [&](float d2, uint32_t at, uint32_t geomID) {
        const uint4 rec = neighbour_words(d2, sc.leaves[at].primID, geomID, 0u, point);
        uint64_t j;                                                       // the place that is free: records at j' < j may still move up
        if (held < len) {
          j = held++;
        } else {
          if (!neighbour_before(rec, tail)) return;                       // full, and this one sorts behind everything kept
          j = len - 1;                                                    // the last record is dropped
        }
        const bool last = j == len - 1;                                   // seg[len - 1] is written by this insertion: with rec, or with
        uint4 end = rec;                                                  // the record in front of it when rec sorts before that
        while (j > 0) {
          const uint4 prev = seg[j - 1];
          if (!neighbour_before(rec, prev)) break;
          seg[j] = prev;
          if (j == len - 1) end = prev;
          --j;
        }
        seg[j] = rec;
        if (last) { tail = end; bound = __uint_as_float(end.x); }
      });
      const uint4 pad = neighbour_words(kInf, MI_INVALID_PRIM, (uint32_t)MI_INVALID_GEOM, (uint32_t)MI_FLAG_ESCAPED, point);
      for (uint64_t j = held; j < len; ++j) seg[j] = pad;
    }
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

}  // namespace mi
