// touch_kernels.hpp — the kernels of a "touch query": every primitive that TOUCHES a caller-supplied item, with no distance and
// no order among the touching primitives but their key (geomID, primID). The families are the ones query_drivers.hpp lists in
// TouchFamilies; a family describes itself once, by a shape S next to its arithmetic (BoxShape in box_math.hpp is the plainest),
// which the kernels here and their host twins (host/touch_host.hpp) both walk with:
//
//   S::Item, S::Record                      what a batch holds and what a list holds (16 bytes: {primID, geomID | flags << 16, item, 0})
//   S::Fields, S::fields(item)              the item's fields as the arithmetic takes them, from the C struct
//   S::valid(fields)                        whether the item is walked at all
//   S::Carried, S::carry(fields)            what a lane carries across the walk
//   S::meets_bounds(mn, mx, carried)        whether a node's box is entered; a primitive's own bounds precede its test
//   S::touches_prim(kind, f, carried, &contained)
//   S::flags(contained)                     what a record of a touching primitive carries
//   S::kAny, kCount, kNoun, kKindBad, kAlign, kAlignBad
//                                           the kinds, and the words and the item alignment of the entries' argument rules
//
// and for the device by Q = the shape plus (box_kernels.hpp is the plainest)
//
//   Q::load(items, idx)                     item idx as the walk takes it: the width of the loads is the family's choice
//   Q::walk<STATS>(sc, item, cs, accept)    the item's walk over walk_preorder (bvh_walk.hpp): accept(leaf index, geomID, flags) is
//                                           called for each touching primitive; returning true ends the walk. SharedWalk<S> below
//                                           supplies it from the shape; a family whose kernels would come out as other code
//                                           through it keeps a walk of its own (DESIGN.md §38 names them)
//   Q::kQuery, kOffsets, kFill              the entries' names, for query_drivers.hpp's launchers
//
//   touch_walk           walk_preorder with S::meets_bounds at the nodes and S::touches_prim at a reached leaf.
//   touch_query_kernel   one thread per item: a byte (ANY: the walk stops at the first accept) or a uint32 count.
//   touch_count_kernel   one thread per item: the count as 64 bits (scan_*_kernel of list_kernels.hpp then runs in place on them).
//   touch_fill_kernel    (key_heap_fill) one thread per item, into the item's OWN segment [offsets[i], offsets[i + 1]) cut at
//                        `capacity` (list_segment.hpp). The key (geomID, primID) has no spatial bound, so the fill cannot prune: it
//                        walks what the count walk walks. The segment holds the `len` smallest keys seen so far as a binary
//                        MAX-heap (an item routinely touches hundreds of primitives, and list_fill_kernel's insertion moves
//                        O(len^2) records): appended and sifted up while held < len, after that a smaller key replaces the root -
//                        whose key lives in a register - and is sifted down. Behind the walk the segment is heap-sorted in place
//                        and padded. Keys are unique within an item, so the bytes do not depend on the visit order. An item whose
//                        segment is empty is not walked.
// No LDS, no stack, no per-lane array, no scratch: a lane carries the item, the segment's base and length, the number of records
// held, the root's key and the record being placed.
#pragma once

#include "bvh_walk.hpp"
#include "box_math.hpp"      // overlap_key
#include "list_segment.hpp"

namespace mi {

// A record as the four words it is stored as: {primID, geomID | flags << 16, item, 0}
__device__ __forceinline__ uint4 overlap_words(uint32_t primID, uint32_t geomID, uint32_t flags, uint32_t item) {
  return make_uint4(primID, geomID | (flags << 16), item, 0u);
}
__device__ __forceinline__ uint64_t overlap_key_of(const uint4& r) { return overlap_key(r.y & 0xFFFFu, r.x); }

// The walk of one item. The node test's result selects between nd.hit and nd.link: a family writes it with & and |, never && and ||,
// where a short-circuit would have the compiler branch around that select.
template <class S, bool STATS, class Accept>
__device__ __forceinline__ void touch_walk(const DeviceScene& sc, const typename S::Fields& item, CastStats& cs, const Accept& accept) {
  const auto& q = S::carry(item);
  walk_preorder<STATS>(sc, S::valid(item), cs,
    [&](const GNode& nd) { return S::meets_bounds(mk(nd.minx, nd.miny, nd.minz), mk(nd.maxx, nd.maxy, nd.maxz), q); },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      bool contained;
      return S::touches_prim(type & 0xFFFFu, f, q, &contained) && accept(at, type >> 16, S::flags(contained));
    });
}

// The device side of a family that walks through touch_walk: its Q is this plus load and the entries' names.
template <class S>
struct SharedWalk : S {
  template <bool STATS, class Accept>
  static __device__ __forceinline__ void walk(const DeviceScene& sc, const typename S::Fields& item, CastStats& cs, const Accept& accept) {
    touch_walk<S, STATS>(sc, item, cs, accept);
  }
};

// COUNT: out = n uint32_t, the number of touching primitives; otherwise n bytes, 1 when there is one.
template <class Q, bool COUNT, bool STATS>
__global__ void __launch_bounds__(256) touch_query_kernel(DeviceScene sc, const typename Q::Item* items, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    uint32_t count = 0;
    Q::template walk<STATS>(sc, Q::load(items, idx), cs, [&](uint32_t, uint32_t, uint32_t) { ++count; return !COUNT; });
    if constexpr (COUNT) static_cast<uint32_t*>(out)[idx] = count;
    else static_cast<uint8_t*>(out)[idx] = count ? 1u : 0u;
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);      // box tests -> "nodes visited", primitive tests -> "leaf tests"; no casts
}

// counts[i] = the number of primitives touching item i, as 64 bits (the scan runs in place on them)
template <class Q, bool STATS>
__global__ void __launch_bounds__(256) touch_count_kernel(DeviceScene sc, const typename Q::Item* items, uint64_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    uint64_t count = 0;
    Q::template walk<STATS>(sc, Q::load(items, idx), cs, [&](uint32_t, uint32_t, uint32_t) { ++count; return false; });
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

// The fill of the lists whose key is (geomID, primID): item idx's segment receives the `len` smallest keys, ascending, then the
// empty record. walk(accept) runs the item's walk - it is not called for an empty segment, so it is also what loads the item - and
// calls accept(leaf index, geomID, flags) for each touching primitive; `item` is the record's third word.
template <class Walk>
__device__ __forceinline__ void key_heap_fill(const DeviceScene& sc, const uint64_t* offsets, void* hits, uint64_t capacity, uint32_t idx, uint32_t item,
                                              const Walk& walk) {
  const uint64_t first = offsets[idx], len = segment_len(first, offsets[idx + 1], capacity);
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

// itemBase: what is added to the thread's index for the record's item field (the host entry's batches; 0 for the device entry).
template <class Q, bool STATS>
__global__ void __launch_bounds__(256) touch_fill_kernel(DeviceScene sc, const typename Q::Item* items, const uint64_t* offsets, typename Q::Record* hits,
                                                         uint64_t capacity, uint32_t itemBase, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    key_heap_fill(sc, offsets, hits, capacity, idx, itemBase + idx, [&](const auto& accept) {
      Q::template walk<STATS>(sc, Q::load(items, idx), cs, accept);
    });
  }
  if constexpr (STATS) flush_stats(sc, 0u, cs, 0u);
}

}  // namespace mi
