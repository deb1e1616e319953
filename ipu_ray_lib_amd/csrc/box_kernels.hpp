// box_kernels.hpp — box queries of a live scene (mi_box_query* / mi_box_offsets* / mi_box_fill*, include/mi_raylib.h): every
// primitive that TOUCHES a caller's axis-aligned box - a voxel, a culling cell, a broad-phase cell (Open3D's
// VoxelGrid.create_from_triangle_mesh, PCL's boxSearch, a physics engine's overlap-box). The form is that of the neighbour
// lists (near_kernels.hpp): any / count, or count -> prefix sum -> fill.
//
//   box_walk             near_walk's loads - the 32-byte node, the first 40 bytes of the leaf record - with a box-box compare in
//                        place of the box distance (box_meets_bounds: closed, no arithmetic) and box_touches_prim (box_math.hpp:
//                        the primitive's own bounds, then for a triangle the separating-axis test) at a reached leaf.
//                        accept(leaf index, geomID, contained) is called for each touching primitive; returning true ends the walk.
//   box_query_kernel     one thread per box: a byte (MI_BOX_ANY: the walk stops at the first accept) or a uint32 count.
//   box_count_kernel     one thread per box: the count as 64 bits (scan_*_kernel of list_kernels.hpp then runs in place on them).
//   box_fill_kernel      (key_heap_fill, which the triangle queries' fill shares) one thread per box, into the box's OWN segment [offsets[i], offsets[i + 1]) cut at `capacity`. The key
//                        (geomID, primID) has no spatial bound, so the fill cannot prune: it walks what the count walk walks. The
//                        segment holds the `len` smallest keys seen so far as a binary MAX-heap (a box routinely holds hundreds of
//                        primitives, and list_fill_kernel's insertion moves O(len^2) records): appended and sifted up while
//                        held < len, after that a smaller key replaces the root - whose key lives in a register - and is sifted
//                        down. Behind the walk the segment is heap-sorted in place and padded. Keys are unique within a box, so
//                        the bytes do not depend on the visit order. A box whose segment is empty is not walked.
// No LDS, no stack, no per-lane array, no scratch: a lane carries the box, the segment's base and length, the number of records
// held, the root's key and the record being placed. The host twin (host/box_query_host.cpp) returns the same bytes and the same
// visit totals.
#pragma once

#include "box_math.hpp"
#include "near_kernels.hpp"

namespace mi {

static_assert(sizeof(mi_box) == 32, "mi_box must stay 32 bytes (two 16-byte loads)");
static_assert(sizeof(mi_overlap) == 16, "mi_overlap must stay 16 bytes (one 16-byte load or store)");

// A record as the four words it is stored as: {primID, geomID | flags << 16, box, 0}
__device__ __forceinline__ uint4 overlap_words(uint32_t primID, uint32_t geomID, uint32_t flags, uint32_t box) {
  return make_uint4(primID, geomID | (flags << 16), box, 0u);
}
__device__ __forceinline__ uint64_t overlap_key_of(const uint4& r) { return overlap_key(r.y & 0xFFFFu, r.x); }

// The stackless preorder walk of the point queries with a box for a point.
template <bool STATS, class Accept>
__device__ __forceinline__ void box_walk(const DeviceScene& sc, f3 lo, f3 hi, CastStats& cs, const Accept& accept) {
  // node positions are BYTE offsets into the node array (GNode); a query that is not walked ends before its first node
  const uint32_t end = box_query_valid(lo, hi) ? sc.numNodes << 5 : 0u;
  uint32_t node = 0;
  while (node < end) {
    const GNode nd = *reinterpret_cast<const GNode*>(reinterpret_cast<const char*>(sc.nodes) + node);
    if (STATS) cs.nodes++;
    const bool enter = box_meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), lo, hi);
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
      bool contained;
      if (box_touches_prim(__float_as_uint(r0.x) & 0xFFFFu, f, lo, hi, &contained) && accept(at, __float_as_uint(r0.x) >> 16, contained)) break;
    }
    node = next;
  }
}

// mi_box: lo[3], reserved0, hi[3], reserved1 - two 16-byte loads
__device__ __forceinline__ void load_box(const mi_box* boxes, uint32_t idx, f3& lo, f3& hi) {
  const float4 a = reinterpret_cast<const float4*>(boxes)[2 * (size_t)idx], b = reinterpret_cast<const float4*>(boxes)[2 * (size_t)idx + 1];
  lo = mk(a.x, a.y, a.z);
  hi = mk(b.x, b.y, b.z);
}

// COUNT: out = n uint32_t, the number of touching primitives; otherwise n bytes, 1 when there is one.
template <bool COUNT, bool STATS>
__global__ void __launch_bounds__(256) box_query_kernel(DeviceScene sc, const mi_box* boxes, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    f3 lo, hi;
    load_box(boxes, idx, lo, hi);
    uint32_t count = 0;
    box_walk<STATS>(sc, lo, hi, cs, [&](uint32_t, uint32_t, bool) { ++count; return !COUNT; });
    if constexpr (COUNT) static_cast<uint32_t*>(out)[idx] = count;
    else static_cast<uint8_t*>(out)[idx] = count ? 1u : 0u;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);      // box tests -> "nodes visited", primitive tests -> "leaf tests"; no casts
}

// counts[i] = the number of primitives touching box i, as 64 bits (the scan runs in place on them)
template <bool STATS>
__global__ void __launch_bounds__(256) box_count_kernel(DeviceScene sc, const mi_box* boxes, uint64_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    f3 lo, hi;
    load_box(boxes, idx, lo, hi);
    uint64_t count = 0;
    box_walk<STATS>(sc, lo, hi, cs, [&](uint32_t, uint32_t, bool) { ++count; return false; });
    counts[idx] = count;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

// seg[0 .. m) is a max-heap but for its root, which is free: rec goes where it belongs below it. Every access is seg[j], j < m.
__device__ __forceinline__ void overlap_sift_down(uint4* seg, uint64_t m, const uint4& rec) {
  const uint64_t key = overlap_key_of(rec);
  uint64_t j = 0;
  for (;;) {
    uint64_t c = 2 * j + 1;
    if (c >= m) break;
    uint4 child = seg[c];
    if (c + 1 < m) {
      const uint4 other = seg[c + 1];
      if (overlap_key_of(other) > overlap_key_of(child)) { child = other; ++c; }
    }
    if (!(overlap_key_of(child) > key)) break;
    seg[j] = child;
    j = c;
  }
  seg[j] = rec;
}

// The fill of the lists whose key is (geomID, primID) - the box lists here, the triangle queries' contact lists
// (contact_kernels.hpp): item idx's segment [offsets[idx], offsets[idx + 1]) cut at `capacity` receives the `len` smallest keys,
// ascending, then the empty record. walk(accept) runs the item's walk - it is not called for an empty segment, so it is also what
// loads the query - and calls accept(leaf index, geomID, flags) for each touching primitive; `item` is the record's third word.
template <class Walk>
__device__ __forceinline__ void key_heap_fill(const DeviceScene& sc, const uint64_t* offsets, void* hits, uint64_t capacity, uint32_t idx, uint32_t item,
                                              const Walk& walk) {
  // the segment: [lo, hi) cut at capacity; a decreasing pair, or a start at or past capacity, is an empty one
  const uint64_t first = offsets[idx], last = offsets[idx + 1];
  uint64_t len = 0;
  if (last > first && first < capacity) len = (last < capacity ? last : capacity) - first;
  if (!len) return;                                                     // (an empty segment: nothing to write, no walk)
  uint4* seg = reinterpret_cast<uint4*>(hits) + first;                  // every access below is seg[j] with j < len
  uint64_t held = 0;                                                    // seg[0 .. held) is a max-heap by key, held <= len
  uint64_t rootKey = 0;                                                 // the key of seg[0] once held > 0: a copy in registers
  walk([&](uint32_t at, uint32_t geomID, uint32_t flags) {
    const uint4 rec = overlap_words(sc.leaves[at].primID, geomID, flags, item);
    const uint64_t key = overlap_key_of(rec);
    if (held < len) {
      uint64_t j = held++;                                              // appended, then sifted up: parents smaller than it move down
      while (j > 0) {
        const uint64_t p = (j - 1) >> 1;
        const uint4 parent = seg[p];
        if (!(key > overlap_key_of(parent))) break;
        seg[j] = parent;
        j = p;
      }
      seg[j] = rec;
      if (j == 0) rootKey = key;
    } else if (key < rootKey) {                                         // full: the largest key kept makes room for a smaller one
      overlap_sift_down(seg, len, rec);
      rootKey = overlap_key_of(seg[0]);
    }
    return false;
  });
  // heap sort in place: the largest key of seg[0 .. m) goes to seg[m - 1], the record that was there is sifted down from the root
  for (uint64_t m = held; m > 1; --m) {
    const uint4 top = seg[0], moved = seg[m - 1];
    seg[m - 1] = top;
    overlap_sift_down(seg, m - 1, moved);
  }
  const uint4 pad = overlap_words(MI_INVALID_PRIM, (uint32_t)MI_INVALID_GEOM, (uint32_t)MI_FLAG_ESCAPED, item);
  for (uint64_t j = held; j < len; ++j) seg[j] = pad;
}

// boxBase: what is added to the thread's index for the record's `box` field (the host entry's batches; 0 for the device entry).
template <bool STATS>
__global__ void __launch_bounds__(256) box_fill_kernel(DeviceScene sc, const mi_box* boxes, const uint64_t* offsets, mi_overlap* hits,
                                                       uint64_t capacity, uint32_t boxBase, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    key_heap_fill(sc, offsets, hits, capacity, idx, boxBase + idx, [&](const auto& accept) {
      f3 lo, hi;
      load_box(boxes, idx, lo, hi);
      box_walk<STATS>(sc, lo, hi, cs, [&](uint32_t at, uint32_t geomID, bool contained) { return accept(at, geomID, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u); });
    });
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

}  // namespace mi
