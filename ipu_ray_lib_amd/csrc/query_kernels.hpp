// query_kernels.hpp — ray queries on caller-supplied ray batches (mi_query / mi_query_device, include/mi_raylib.h):
//   CompactBvh::intersect (closest hit, CompactBvh.hpp:80-139) and ::occluded (any hit, :33-78) for each given ray, with its
//   own tMin / tMax. No shading: a query is traversal alone.
//
//   query_plain_kernel  scene option query_kernel = 0, the default: one thread per ray over traverse<> - the readable statement
//                       of the contract, and measured faster than K4 on every batch of tools/bench_query.py ("K4")
//   query_wave_kernel   K4, query_kernel = 1: persistent and phase-scheduled ("K4"). Every lane is in one of the
//                       phases NODE (one box test of the stackless walk), LEAF (one primitive test), WRITE (its cast is over:
//                       the result is stored) or FETCH (it takes the next ray from the launch's work counter); the wave votes
//                       between NODE and LEAF, runs several box tests per vote, and lanes whose cast ended are refilled
//                       between bursts, so waves stay full until the batch drains.
// Both kernels perform, per ray, exactly the reference's sequence of box tests, primitive tests and closest-hit updates with the
// same arithmetic, so they write the same bytes (and, in the exact tiers, the oracle's).
#pragma once

#include "trace_wavefront.hpp"     // fast_box_setup, lane_rank, PH_*

namespace mi {

static_assert(sizeof(mi_query_hit) == 32, "mi_query_hit must stay 32 bytes (two 16-byte stores)");

// K4's scheduling weights (runtime arguments: scene option "query_tune"):
//   leafAt    a LEAF turn runs when cL * leafAt > cN * 4 (as K1w's leafAt)
//   dbl, maxExtra   a NODE turn runs 1 + min(cN / dbl, maxExtra) box tests before the wave votes again
//   burst     at most this many NODE / LEAF turns between two refills
//   keep8     ... or fewer, once fewer than keep8 / 8 of the lanes that started the burst still walk: the finished ones are
//             written out and refilled then (8 = refill as soon as one lane is done)
struct QueryTune { uint32_t leafAt, dbl, maxExtra, burst, keep8; };
constexpr QueryTune kDefaultQueryTune = {8, 2, 8, 48, 7};      // best of the five sets tools/bench_query.py timed ("K4")

constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;

struct QueryRay { f3 o, d; float tMin, tMax; };

// mi_ray (32 B) as two 16-byte loads (the entry points require 16-byte aligned buffers)
__device__ __forceinline__ QueryRay load_query_ray(const mi_ray* rays, uint32_t i) {
  const float4* p = reinterpret_cast<const float4*>(rays + i);
  const float4 a = p[0], b = p[1];
  QueryRay r;
  r.o = mk(a.x, a.y, a.z); r.tMin = a.w;
  r.d = mk(b.x, b.y, b.z); r.tMax = b.w;
  return r;
}

// The result of a closest-hit cast as two 16-byte stores: {t, primID, geomID | flags << 16, n.x} {n.y, n.z, b1, b2}.
// A miss: t = tMax, invalid ids, MI_FLAG_ESCAPED, zeros. The normal is Primitive::normal at o + t d (Render.hpp:21-22,
// hit_normal), the barycentrics those of the hit triangle's test (0 for spheres and discs).
__device__ __forceinline__ void store_query_hit(const DeviceScene& sc, mi_query_hit* out, uint32_t i, f3 o, f3 d, const Hit& hit) {
  float4 w0, w1;
  if (hit.leaf != kNoLeaf) {
    const GLeaf& L = sc.leaves[hit.leaf];
    const f3 nrm = hit_normal(sc, hit, o + d * hit.t);
    const bool tri = leaf_kind(L) == LEAF_TRI;
    w0 = make_float4(hit.t, __uint_as_float(L.primID), __uint_as_float(leaf_geom(L)), nrm.x);
    w1 = make_float4(nrm.y, nrm.z, tri ? hit.b1 : 0.f, tri ? hit.b2 : 0.f);
  } else {
    w0 = make_float4(hit.t, __uint_as_float(MI_INVALID_PRIM), __uint_as_float((uint32_t)MI_INVALID_GEOM | ((uint32_t)MI_FLAG_ESCAPED << 16)), 0.f);
    w1 = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4* q = reinterpret_cast<float4*>(out + i);
  q[0] = w0; q[1] = w1;
}

// FAST tier box test (trace_wavefront.hpp, nodeBodyT with FAST): three pairs of FMAs on (plane, 1/d, -o/d), the far side widened
// by slabPad; tMin instead of the path tracer's 0. Shared by both query kernels so that they agree bit for bit in this tier too.
__device__ __forceinline__ bool box_hit_fast(const GNode& nd, f3 inv, f3 oi, float slabPad, float tMin, float tCur) {
  const float ax = __builtin_fmaf(nd.minx, inv.x, oi.x), bx = __builtin_fmaf(nd.maxx, inv.x, oi.x);
  const float ay = __builtin_fmaf(nd.miny, inv.y, oi.y), by = __builtin_fmaf(nd.maxy, inv.y, oi.y);
  const float az = __builtin_fmaf(nd.minz, inv.z, oi.z), bz = __builtin_fmaf(nd.maxz, inv.z, oi.z);
  const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tMin));
  const float t1 = fminf(__builtin_fmaf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), kSlabScale, slabPad), tCur);
  return !(t0 > t1);
}

// Exact box test (CompactBVH2Node.cpp:5-22, intersectRaySlab CompactBVH2Node.hpp:14-50) in the min / max form of K1w: with no NaN
// among the slab products, tMin and tCur, the reference's ordered compare / selects ARE min / max and the far side may be scaled
// once (trace_wavefront.hpp). `literal` lanes - a non-finite origin, direction or reciprocal, or a NaN tMin / tMax: NaN can
// then arise - redo the test with the reference's literal sequence, as traverse<> evaluates it.
__device__ __forceinline__ bool box_hit_exact(const GNode& nd, f3 o, f3 inv, float tMin, float tCur, bool literal) {
  const float ax = (nd.minx - o.x) * inv.x, bx = (nd.maxx - o.x) * inv.x;
  const float ay = (nd.miny - o.y) * inv.y, by = (nd.maxy - o.y) * inv.y;
  const float az = (nd.minz - o.z) * inv.z, bz = (nd.maxz - o.z) * inv.z;
  float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tMin));
  float t1 = fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * kSlabScale, tCur);
  if (literal) {
    t0 = tMin; t1 = tCur;
    { float tmin = ax, tmax = bx; if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; } tmax *= kSlabScale; t0 = tmin > t0 ? tmin : t0; t1 = tmax < t1 ? tmax : t1; }
    { float tmin = ay, tmax = by; if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; } tmax *= kSlabScale; t0 = tmin > t0 ? tmin : t0; t1 = tmax < t1 ? tmax : t1; }
    { float tmin = az, tmax = bz; if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; } tmax *= kSlabScale; t0 = tmin > t0 ? tmin : t0; t1 = tmax < t1 ? tmax : t1; }
  }
  return !(t0 > t1);
}

// Whether a cast needs the literal box test (box_hit_exact): the min / max form is only valid when nothing can be NaN. With a
// finite origin and finite direction components, 1/d is never 0, so (plane - o) * (1/d) is never inf * 0.
__device__ __forceinline__ bool needs_literal_box(f3 o, f3 d, f3 inv, float tMin, float tMax) {
  return !(fabsf(inv.x) < kInf && fabsf(inv.y) < kInf && fabsf(inv.z) < kInf && fabsf(o.x) < kInf && fabsf(o.y) < kInf && fabsf(o.z) < kInf &&
           fabsf(d.x) < kInf && fabsf(d.y) < kInf && fabsf(d.z) < kInf) | (tMin != tMin) | (tMax != tMax);
}

// One primitive test at leaf node `leaf` (Mesh.cpp:6-104, Primitives.cpp:24-67) and the reference's acceptance
// t > tMin && t < closest (CompactBvh.hpp:124 / :60). ROT: the record of the cast's shear axis from GLeafRot (the vertices arrive
// rotated; exact, trace_kernels.hpp intersect_triangle PRE). Returns whether the hit is accepted; t and the barycentrics in t, b.
template <bool DF, bool FAST, bool ROT>
__device__ __forceinline__ bool leaf_test(const DeviceScene& sc, uint32_t leaf, f3 o, f3 d, const Shear& sh, float tMin, float tCur, float& tOut, float& b0, float& b1, float& b2) {
  GLeaf L;
  if constexpr (ROT) {
    const GLeafBlock B = *reinterpret_cast<const GLeafBlock*>(reinterpret_cast<const char*>(sc.leavesRot) + (size_t)leaf * sizeof(GLeafRot) + sh.kz * sizeof(GLeafBlock));
    L.type = B.type;
#pragma unroll
    for (int q = 0; q < 9; ++q) L.f[q] = B.f[q];
  } else {
    const GLeaf& G = sc.leaves[leaf];
    L.type = G.type;
#pragma unroll
    for (int q = 0; q < 9; ++q) L.f[q] = G.f[q];
  }
  float t;
  bool cand;
  b0 = b1 = b2 = 0.f;
  const uint32_t kind = leaf_kind(L);
  if (kind == LEAF_TRI) {
    const f3 p0 = mk(L.f[0], L.f[1], L.f[2]), p1 = mk(L.f[3], L.f[4], L.f[5]), p2 = mk(L.f[6], L.f[7], L.f[8]);
    if constexpr (FAST) t = intersect_triangle_fast(p0, p1, p2, o, sh, b0, b1, b2);
    else if constexpr (ROT) t = intersect_triangle<DF, true>(p0, p1, p2, permute_kz(o, sh.kz), sh, b0, b1, b2);
    else t = intersect_triangle<DF>(p0, p1, p2, o, sh, b0, b1, b2);
    cand = t > 0.f && t < kInf;                 // Mesh.hpp:93
  } else if (kind == LEAF_SPHERE) {
    t = intersect_sphere(L, o, d, tMin);
    cand = true;                                // Failed() carries t = 0, rejected by t > tMin
  } else {
    t = intersect_disc(L, o, d);
    cand = true;
  }
  tOut = t;
  return cand & (t > tMin) & (t < tCur);
}

// The FAST tier's walk for the one-thread-per-ray kernel: traverse<> with the tier's cast set-up, box test and triangle test.
template <bool ANY_HIT, bool STATS>
__device__ __forceinline__ bool traverse_fast(const DeviceScene& sc, f3 o, f3 d, float tMin, float tMax, Hit& hit, CastStats& cs) {
  f3 inv = fast_inverse(d), oi;
  const Shear sh = make_shear_fast(d, inv);
  float slabPad;
  fast_box_setup(o, inv, oi, slabPad);
  hit.t = tMax; hit.leaf = kNoLeaf; hit.geomID = 0xFFFFu; hit.b0 = hit.b1 = hit.b2 = 0.f;
  uint32_t i = 0;
  while (i < sc.numNodes) {
    const GNode nd = sc.nodes[i];
    if (STATS) cs.nodes++;
    const bool boxHit = box_hit_fast(nd, inv, oi, slabPad, tMin, hit.t);
    const bool isLeaf = node_is_leaf(nd);
    if (boxHit && isLeaf) {
      if (STATS) cs.leaves++;
      float t, b0, b1, b2;
      if (leaf_test<false, true, false>(sc, i, o, d, sh, tMin, hit.t, t, b0, b1, b2)) {
        if (ANY_HIT) return true;
        hit.t = t; hit.leaf = i; hit.b0 = b0; hit.b1 = b1; hit.b2 = b2;
      }
    }
    i = (boxHit && !isLeaf) ? i + 1 : (nd.link >> 5);
  }
  return hit.leaf != kNoLeaf;
}

// ---- query_kernel = 0: one thread per ray --------------------------------------------------------------------------
template <bool ANY_HIT, bool STATS, bool DF, bool FAST>
__global__ void __launch_bounds__(256) query_plain_kernel(DeviceScene sc, const mi_ray* rays, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const QueryRay r = load_query_ray(rays, idx);
    Hit hit;
    bool found;
    if constexpr (FAST) found = traverse_fast<ANY_HIT, STATS>(sc, r.o, r.d, r.tMin, r.tMax, hit, cs);
    else found = traverse<ANY_HIT, STATS, DF>(sc, r.o, r.d, r.tMin, r.tMax, hit, cs);
    if constexpr (ANY_HIT) static_cast<uint8_t*>(out)[idx] = found ? 1u : 0u;
    else store_query_hit(sc, static_cast<mi_query_hit*>(out), idx, r.o, r.d, hit);
  }
  flush_stats(sc, idx < n ? 1u : 0u, cs, 0u);
}

// ---- K4, query_kernel = 1: persistent, phase-scheduled --------------------------------------------------------------
// Lane phases: PH_NODE, PH_LEAF, PH_SHADE (here: the cast is over, its result is to be written), PH_FETCH, PH_DONE.
template <bool ANY_HIT, bool STATS, bool DF, bool FAST>
__global__ void __launch_bounds__(256) query_wave_kernel(DeviceScene sc, const mi_ray* rays, void* out, uint32_t n, uint32_t* workCounter, QueryTune tune) {
  constexpr bool ROT = !FAST;                    // pre-rotated primitive records for the exact tiers (the FAST triangle test has no PRE form)
  constexpr uint32_t kChunk = 64;                // work indices per global atomic
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t numNodes = sc.numNodes << 5;    // node positions are BYTE offsets into the node array (GNode)
  uint32_t chunkNext = 0, chunkEnd = 0;          // wave-uniform: the local range of work indices not handed out yet

  uint32_t ph = PH_FETCH, node = 0, ray = 0;
  f3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0), oi = mk(0, 0, 0);
  float tMin = 0.f, slabPad = 0.f;
  bool literal = false;
  Shear sh; sh.kz = 2; sh.sx = sh.sy = 0.f; sh.sz = 1.f;
  Hit hit; hit.t = 0.f; hit.leaf = kNoLeaf; hit.geomID = 0xFFFFu; hit.b0 = hit.b1 = hit.b2 = 0.f;
  CastStats cs = {0, 0};
  uint32_t casts = 0;

  auto nodeStep = [&]() {
    const GNode nd = *reinterpret_cast<const GNode*>(reinterpret_cast<const char*>(sc.nodes) + node);
    if (STATS) cs.nodes++;
    const bool boxHit = FAST ? box_hit_fast(nd, inv, oi, slabPad, tMin, hit.t) : box_hit_exact(nd, o, inv, tMin, hit.t, literal);
    // one select (GNode: a leaf's hit successor is its link with kLeafFlag: "stop, test the primitive of the node before it")
    node = boxHit ? nd.hit : nd.link;
    if (node & kLeafFlag) { node &= ~kLeafFlag; ph = PH_LEAF; }
    else if (node >= numNodes) ph = PH_SHADE;
  };

  for (;;) {
    // ---------------- WRITE + FETCH: finished casts leave, their lanes take the next rays ----------------
    if (ph == PH_SHADE) {
      if constexpr (ANY_HIT) static_cast<uint8_t*>(out)[ray] = hit.leaf != kNoLeaf ? 1u : 0u;
      else store_query_hit(sc, static_cast<mi_query_hit*>(out), ray, o, d, hit);
      ph = PH_FETCH;
    }
    for (;;) {
      const unsigned long long mF = __ballot(ph == PH_FETCH);
      if (!mF) break;
      if (chunkNext >= chunkEnd) {
        const uint32_t firstF = (uint32_t)__ffsll((long long)mF) - 1u;
        uint32_t base = 0;
        if (lane == firstF) base = atomicAdd(workCounter, kChunk);
        chunkNext = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(base, firstF));
        chunkEnd = chunkNext + kChunk;
      }
      const uint32_t avail = chunkEnd - chunkNext, rankF = lane_rank(mF), chunkBase = chunkNext;
      chunkNext += min((uint32_t)__popcll(mF), avail);
      if (ph == PH_FETCH && rankF < avail) {
        const uint32_t idx = chunkBase + rankF;
        if (idx < n) {
          // the cast set-up, once per ray: as traverse<> (exact reciprocal, shear) or as the FAST tier's
          const QueryRay r = load_query_ray(rays, idx);
          ray = idx; o = r.o; d = r.d; tMin = r.tMin;
          if constexpr (FAST) { inv = fast_inverse(d); sh = make_shear_fast(d, inv); fast_box_setup(o, inv, oi, slabPad); }
          else { inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z); sh = make_shear(d, inv); literal = needs_literal_box(o, d, inv, r.tMin, r.tMax); }
          hit.t = r.tMax; hit.leaf = kNoLeaf; hit.b0 = hit.b1 = hit.b2 = 0.f;
          node = 0;
          ++casts;
          ph = numNodes ? PH_NODE : PH_SHADE;
        } else {
          ph = PH_DONE;
        }
      }
    }
    // lanes of an empty scene finish in their set-up turn
    if (__ballot(ph == PH_SHADE)) continue;

    uint32_t cN = (uint32_t)__popcll(__ballot(ph == PH_NODE)), cL = (uint32_t)__popcll(__ballot(ph == PH_LEAF));
    if ((cN | cL) == 0) break;                   // every lane DONE: the batch has drained

    // ---------------- TRAVERSE: NODE and LEAF turns under a two-way vote ----------------
    __builtin_amdgcn_s_setprio(1);
    const uint32_t startT = cN + cL;
    for (uint32_t steps = 0;;) {
      if (cN * 4u >= cL * tune.leafAt && cN > 0) {
        // NODE: 1 + min(cN / dbl, maxExtra) box tests per lane before the next vote; lanes that reach a leaf or the end sit the rest out
        const uint32_t extra = min(cN / tune.dbl, tune.maxExtra);
        if (ph == PH_NODE) nodeStep();
        for (uint32_t e = 0; e < extra; ++e)
          if (ph == PH_NODE) nodeStep();
      } else {
        // LEAF: one primitive test per lane; the walk continues behind the leaf (node = leaf + 1), any-hit lanes leave on a hit
        if (ph == PH_LEAF) {
          if (STATS) cs.leaves++;
          const uint32_t atLeaf = (node >> 5) - 1u;
          float t, b0, b1, b2;
          const bool accept = leaf_test<DF, FAST, ROT>(sc, atLeaf, o, d, sh, tMin, hit.t, t, b0, b1, b2);
          if (ANY_HIT) {
            hit.leaf = accept ? atLeaf : hit.leaf;
            ph = (accept || node >= numNodes) ? PH_SHADE : PH_NODE;
          } else {
            hit.t = accept ? t : hit.t; hit.leaf = accept ? atLeaf : hit.leaf;
            hit.b0 = accept ? b0 : hit.b0; hit.b1 = accept ? b1 : hit.b1; hit.b2 = accept ? b2 : hit.b2;
            ph = (node >= numNodes) ? PH_SHADE : PH_NODE;
          }
          // every lane that waited for its primitive is walking again: its next box test follows at once
          if (ph == PH_NODE) nodeStep();
        }
      }
      cN = (uint32_t)__popcll(__ballot(ph == PH_NODE));
      cL = (uint32_t)__popcll(__ballot(ph == PH_LEAF));
      if (++steps >= tune.burst || (cN + cL) * 8u < startT * tune.keep8 || (cN + cL) == 0) break;
    }
    __builtin_amdgcn_s_setprio(0);
  }
  flush_stats(sc, casts, cs, 0u);
}

}  // namespace mi
