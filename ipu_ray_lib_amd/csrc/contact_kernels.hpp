// contact_kernels.hpp — triangle queries of a live scene (mi_tri_query* / mi_tri_offsets* / mi_tri_fill*, include/mi_raylib.h):
// every primitive that TOUCHES a caller's triangle - one face of another mesh (Embree's rtcCollide, FCL's collision manager), a
// cutting plane's facet, a sweep's cap. The form is that of the box queries (box_kernels.hpp): any / count, or
// count -> prefix sum -> fill.
//
//   tri_walk             box_walk's loads - the 32-byte node, the first 40 bytes of the leaf record - with the query's bounds [qmn,
//                        qmx] for the box at the nodes (box_meets_bounds: closed, no arithmetic; no plane test there) and
//                        tri_touches_prim (contact_math.hpp: the primitive's own bounds, then for a triangle the 17-axis
//                        separating-axis test relative to q0) at a reached leaf. accept(leaf index, geomID) is called for each
//                        touching primitive; returning true ends the walk. A primitive's bounds are computed from the whole record
//                        (nine floats of a triangle, seven of a disc), so there is no word whose load the bounds compare could spare.
//   tri_query_kernel     one thread per triangle: a byte (MI_TRI_ANY: the walk stops at the first accept) or a uint32 count.
//   tri_count_kernel     one thread per triangle: the count as 64 bits (scan_*_kernel of list_kernels.hpp then runs in place).
//   tri_fill_kernel      one thread per triangle: key_heap_fill of box_kernels.hpp over tri_walk - the len smallest keys (geomID,
//                        primID) as a max-heap inside the segment, heap-sorted and padded behind the walk.
// No LDS, no stack, no per-lane array, no scratch: a lane carries the query's nine floats and its bounds; the axes of the
// separating-axis test are spelled out one by one (contact_math.hpp). The host twin (host/tri_query_host.cpp) returns the same
// bytes and the same visit totals.
#pragma once

#include "box_kernels.hpp"
#include "contact_math.hpp"

namespace mi {

static_assert(sizeof(mi_tri) == 36, "mi_tri must stay 36 bytes: a float32 [n, 3, 3] array is a batch");
static_assert(sizeof(mi_contact) == 16, "mi_contact must stay 16 bytes (one 16-byte load or store)");

// The stackless preorder walk of the box queries with the triangle's bounds for the box and the triangle itself at the leaves.
template <bool STATS, class Accept>
__device__ __forceinline__ void tri_walk(const DeviceScene& sc, f3 q0, f3 q1, f3 q2, CastStats& cs, const Accept& accept) {
  f3 qmn, qmx;
  tri_query_bounds(q0, q1, q2, qmn, qmx);
  // node positions are BYTE offsets into the node array (GNode); a query that is not walked ends before its first node
  const uint32_t end = tri_query_valid(q0, q1, q2) ? sc.numNodes << 5 : 0u;
  uint32_t node = 0;
  while (node < end) {
    const GNode nd = *reinterpret_cast<const GNode*>(reinterpret_cast<const char*>(sc.nodes) + node);
    if (STATS) cs.nodes++;
    const bool enter = box_meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), qmn, qmx);
    uint32_t next = enter ? nd.hit : nd.link;
    if (next & kLeafFlag) {
      // a leaf's hit successor is its link with kLeafFlag: the primitive of THIS node is tested, the walk goes on behind it
      next &= ~kLeafFlag;
      if (STATS) cs.leaves++;
      const uint32_t at = node >> 5;
      const float4* rec = reinterpret_cast<const float4*>(sc.leaves + at);      // the first 40 bytes: type, nine floats
      const float4 r0 = rec[0], r1 = rec[1];
      const float2 r2w = *reinterpret_cast<const float2*>(rec + 2);
      const float f[9] = {r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2w.x, r2w.y};
      if (tri_touches_prim(__float_as_uint(r0.x) & 0xFFFFu, f, q0, q1, q2, qmn, qmx) && accept(at, __float_as_uint(r0.x) >> 16)) break;
    }
    node = next;
  }
}

// mi_tri: a[3], b[3], c[3] - nine floats at a 4-byte aligned address (36 is no multiple of 8: no wider load is aligned)
__device__ __forceinline__ void load_tri(const mi_tri* tris, uint32_t idx, f3& q0, f3& q1, f3& q2) {
  const float* p = reinterpret_cast<const float*>(tris) + 9 * (size_t)idx;
  q0 = mk(p[0], p[1], p[2]);
  q1 = mk(p[3], p[4], p[5]);
  q2 = mk(p[6], p[7], p[8]);
}

// COUNT: out = n uint32_t, the number of touching primitives; otherwise n bytes, 1 when there is one.
template <bool COUNT, bool STATS>
__global__ void __launch_bounds__(256) tri_query_kernel(DeviceScene sc, const mi_tri* tris, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    f3 q0, q1, q2;
    load_tri(tris, idx, q0, q1, q2);
    uint32_t count = 0;
    tri_walk<STATS>(sc, q0, q1, q2, cs, [&](uint32_t, uint32_t) { ++count; return !COUNT; });
    if constexpr (COUNT) static_cast<uint32_t*>(out)[idx] = count;
    else static_cast<uint8_t*>(out)[idx] = count ? 1u : 0u;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);      // box tests -> "nodes visited", primitive tests -> "leaf tests"; no casts
}

// counts[i] = the number of primitives touching triangle i, as 64 bits (the scan runs in place on them)
template <bool STATS>
__global__ void __launch_bounds__(256) tri_count_kernel(DeviceScene sc, const mi_tri* tris, uint64_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    f3 q0, q1, q2;
    load_tri(tris, idx, q0, q1, q2);
    uint64_t count = 0;
    tri_walk<STATS>(sc, q0, q1, q2, cs, [&](uint32_t, uint32_t) { ++count; return false; });
    counts[idx] = count;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

// triBase: what is added to the thread's index for the record's `tri` field (the host entry's batches; 0 for the device entry).
template <bool STATS>
__global__ void __launch_bounds__(256) tri_fill_kernel(DeviceScene sc, const mi_tri* tris, const uint64_t* offsets, mi_contact* hits,
                                                       uint64_t capacity, uint32_t triBase, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    key_heap_fill(sc, offsets, hits, capacity, idx, triBase + idx, [&](const auto& accept) {
      f3 q0, q1, q2;
      load_tri(tris, idx, q0, q1, q2);
      tri_walk<STATS>(sc, q0, q1, q2, cs, [&](uint32_t at, uint32_t geomID) { return accept(at, geomID, 0u); });
    });
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

}  // namespace mi
