// list_kernels.hpp — crossing lists of a live scene (mi_list_offsets* / mi_list_fill*, include/mi_raylib.h): every crossing of a
// ray inside its interval, not their number (count_kernels.hpp) and not the first one (query_kernels.hpp); Open3D's
// list_intersections. The form is count -> prefix sum -> fill:
//
//   list_count_kernel    one thread per ray: count_crossings (count_kernels.hpp, the function itself), the count stored as 64 bits
//   scan_*_kernel        an inclusive prefix sum of those counts in place, in 64 bits: tile sums, a scan of the tile sums by one
//                        workgroup, the scan of every tile with its tile's base added. The sums are integers: the result does not
//                        depend on the order they are added in.
//   list_crossings       count_crossings' two lambdas over walk_preorder (bvh_walk.hpp) - the same box test (ray_meets_node),
//                        prim_hit and sphere arithmetic (sphere_roots: the operations of sphere_crossings with their t kept) -
//                        calling `emit` where count_crossings adds to its counter. The interval is FIXED, so the set of crossings
//                        is a function of the ray and the geometry alone; sorted by a key of the crossing itself the list is the
//                        same bytes on any tree.
//   list_fill_kernel     one thread per ray: each accepted crossing is inserted at its sorted place into the ray's OWN segment of
//                        the output, [offsets[i], offsets[i + 1]) cut at `capacity`: records behind it move up by one, the last one
//                        is dropped when the segment is full, and what the walk leaves unused is padded with the empty record.
//                        Each record moves as one 16-byte load and one 16-byte store.
// Cost of the fill: O(crossings x len) record moves per ray, in global memory (a segment a lane has just written sits in its
// compute unit's cache). Lists are short where rays are plentiful (tools/bench_list_query.py records their lengths); a caller with
// thousands of layers per ray pays the square. A lane only reads back records it wrote itself (segments of distinct rays are
// disjoint when the offsets ascend; offsets that make them overlap give unspecified records, never a write outside the segment).
// No LDS in the walks, no per-lane array, no stack, no scratch: a lane carries count_crossings' state, the segment's base and
// length, the number of records held and the record being placed.
#pragma once

#include "count_kernels.hpp"
#include "list_segment.hpp"

namespace mi {

static_assert(sizeof(mi_crossing) == 16, "mi_crossing must stay 16 bytes (one 16-byte load or store)");

// A record as the four words it is stored as: {t, primID, geomID | flags << 16, ray}
__device__ __forceinline__ uint4 crossing_words(float t, uint32_t primID, uint32_t geomID, uint32_t flags, uint32_t ray) {
  return make_uint4(__float_as_uint(t), primID, geomID | (flags << 16), ray);
}

// The part of the key behind t: geomID, then primID, then near before far. (MI_CROSS_FAR is bit 3 of flags = bit 19 of word 2.)
__device__ __forceinline__ uint64_t crossing_rank(const uint4& r) {
  return ((uint64_t)(r.z & 0xFFFFu) << 33) | ((uint64_t)r.y << 1) | (uint64_t)((r.z >> 19) & 1u);
}

// a sorts before b. An accepted t is never NaN (a NaN fails prim_hit's and sphere_roots' ordered compares).
__device__ __forceinline__ bool crossing_before(const uint4& a, const uint4& b) {
  const float ta = __uint_as_float(a.x), tb = __uint_as_float(b.x);
  return ta < tb || (ta == tb && crossing_rank(a) < crossing_rank(b));
}

// The walk of count_crossings (count_kernels.hpp); emit(t, primID, geomID, flags) is called for each crossing count_crossings
// counts.
template <bool STATS, bool DF, class Emit>
__device__ __forceinline__ void list_crossings(const DeviceScene& sc, f3 o, f3 d, float tMin, float tMax, CastStats& cs, const Emit& emit) {
  const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
  const Shear sh = make_shear(d, inv);
  walk_preorder<STATS>(sc, true, cs,
    [&](const GNode& nd) { return ray_meets_node(nd, o, inv, tMin, tMax); },
    [&](uint32_t at, uint32_t type, const float (&f)[9]) {
      const GLeafBlock B = {type, {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]}};
      const GLeaf* leaf = sc.leaves + at;
      const uint32_t geomID = B.type >> 16;
      if (leaf_kind(B) == LEAF_SPHERE) {
        float t[2];
        const uint32_t roots = sphere_roots(mk(B.f[0], B.f[1], B.f[2]), B.f[4], o, d, tMin, tMax, t);
        if (roots & 1u) emit(t[0], leaf->primID, geomID, 0u);
        if (roots & 2u) emit(t[1], leaf->primID, geomID, (uint32_t)MI_CROSS_FAR);
      } else {
        float t, b0, b1, b2;
        if (prim_hit<DF>(B, o, d, sh, tMin, tMax, t, b0, b1, b2)) emit(t, leaf->primID, geomID, 0u);
      }
      return false;
    });
}

// counts[i] = ray i's crossing count, as 64 bits (the scan below runs in place on them)
template <bool STATS, bool DF>
__global__ void __launch_bounds__(256) list_count_kernel(DeviceScene sc, const mi_ray* rays, uint64_t* counts, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const QueryRay r = load_query_ray(rays, idx);
    counts[idx] = count_crossings<STATS, DF>(sc, r.o, r.d, r.tMin, r.tMax, cs);
  }
  flush_stats(sc, idx < n ? 1u : 0u, cs, 0u);
}

// ---- the prefix sum: 256 threads x 8 consecutive values = one tile of 2048 --------------------------------------------
constexpr uint32_t kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;

// Exclusive prefix of `v` over the workgroup's kScanThreads threads in thread order; `total` = the sum over all of them.
// part: kScanThreads / 64 words of LDS. Safe to call again at once (it ends with a barrier).
__device__ __forceinline__ uint64_t scan_block_exclusive(uint64_t v, uint64_t* part, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t up = __shfl_up(incl, off);
    if (lane >= (uint32_t)off) incl += up;
  }
  if (lane == 63u) part[wave] = incl;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
  for (uint32_t w = 0; w < kScanThreads / 64; ++w) { const uint64_t p = part[w]; if (w < wave) before += p; total += p; }
  __syncthreads();
  return before + incl - v;
}

// sums[b] = the sum of tile b of a[0 .. n)
__global__ void __launch_bounds__(kScanThreads) scan_tile_sums_kernel(const uint64_t* a, uint64_t* sums, uint32_t n) {
  __shared__ uint64_t part[kScanThreads / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint64_t v = 0;
  for (uint32_t k = 0; k < kScanItems; ++k) if (first + k < n) v += a[first + k];
  uint64_t total;
  (void)scan_block_exclusive(v, part, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. m) becomes its own exclusive prefix: ONE workgroup, kScanThreads values per turn with a running carry
__global__ void __launch_bounds__(kScanThreads) scan_sums_kernel(uint64_t* sums, uint32_t m) {
  __shared__ uint64_t part[kScanThreads / 64];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < m; base += kScanThreads) {      // (m and base are the same for every thread: the barriers inside are uniform)
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < m ? sums[i] : 0;
    uint64_t total;
    const uint64_t ex = scan_block_exclusive(v, part, total);
    if (i < m) sums[i] = carry + ex;
    carry += total;
  }
}

// a[0 .. n) becomes its own inclusive prefix, tile by tile; base[b] = what precedes tile b (nullptr: a single tile)
__global__ void __launch_bounds__(kScanThreads) scan_apply_kernel(uint64_t* a, const uint64_t* base, uint32_t n) {
  __shared__ uint64_t part[kScanThreads / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint64_t v[kScanItems];
  uint64_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; ++k) { v[k] = first + k < n ? a[first + k] : 0; sum += v[k]; }
  uint64_t total;
  uint64_t run = scan_block_exclusive(sum, part, total) + (base ? base[blockIdx.x] : 0);
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; ++k) { run += v[k]; if (first + k < n) a[first + k] = run; }
}

// ---- the fill ----------------------------------------------------------------------------------------------------------
// rayBase: what is added to the thread's index for the record's `ray` field (the host entry's batches; 0 for the device entry).
template <bool STATS, bool DF>
__global__ void __launch_bounds__(256) list_fill_kernel(DeviceScene sc, const mi_ray* rays, const uint64_t* offsets, mi_crossing* hits,
                                                        uint64_t capacity, uint32_t rayBase, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const QueryRay r = load_query_ray(rays, idx);
    const uint64_t lo = offsets[idx], len = segment_len(lo, offsets[idx + 1], capacity);      // (list_segment.hpp)
    uint4* seg = reinterpret_cast<uint4*>(hits) + (len ? lo : 0);      // every access below is seg[j] with j < len
    const uint32_t ray = rayBase + idx;
    uint64_t held = 0;                                                  // seg[0 .. held) is sorted, held <= len
    list_crossings<STATS, DF>(sc, r.o, r.d, r.tMin, r.tMax, cs, [&](float t, uint32_t primID, uint32_t geomID, uint32_t flags) {
      const uint4 rec = crossing_words(t, primID, geomID, flags, ray);
      uint64_t j;                                                       // the place that is free: records at j' < j may still move up
      if (held < len) {
        j = held++;
      } else {
        if (len == 0 || !crossing_before(rec, seg[len - 1])) return;    // full, and this one sorts behind everything kept
        j = len - 1;                                                    // the last record is dropped
      }
      while (j > 0) {
        const uint4 prev = seg[j - 1];
        if (!crossing_before(rec, prev)) break;
        seg[j] = prev;
        --j;
      }
      seg[j] = rec;
    });
    const uint4 pad = crossing_words(kInf, MI_INVALID_PRIM, (uint32_t)MI_INVALID_GEOM, (uint32_t)MI_FLAG_ESCAPED, ray);
    for (uint64_t j = held; j < len; ++j) seg[j] = pad;
  }
  flush_stats(sc, idx < n ? 1u : 0u, cs, 0u);
}

}  // namespace mi
