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

#include "trace_wavefront.hpp"     // lane_rank, PH_*

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

// Whether a query cast needs the literal box test (box_hit_span in trace_kernels.hpp): the path tracer's condition, and besides
// a non-finite direction (its reciprocal is then 0, and (plane - o) * 0 is NaN for an infinite plane distance) or a NaN tMin / tMax.
__device__ __forceinline__ bool query_needs_literal_box(f3 o, f3 d, f3 inv, float tMin, float tMax) {
  const bool pathTracer = needs_literal_box(o, inv);
  return pathTracer | !(fabsf(d.x) < kInf && fabsf(d.y) < kInf && fabsf(d.z) < kInf) | (tMin != tMin) | (tMax != tMax);
}

// ---- query_kernel = 0: one thread per ray --------------------------------------------------------------------------
template <bool ANY_HIT, bool STATS, bool DF, bool FAST>
__global__ void __launch_bounds__(256) query_plain_kernel(DeviceScene sc, const mi_ray* rays, void* out, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  CastStats cs = {0, 0};
  if (idx < n) {
    const QueryRay r = load_query_ray(rays, idx);
    Hit hit;
    const bool found = traverse<ANY_HIT, STATS, DF, FAST>(sc, r.o, r.d, r.tMin, r.tMax, hit, cs);
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
    const bool boxHit = FAST ? box_hit_fast(nd, inv, oi, slabPad, tMin, hit.t) : box_hit_exact(nd, o, inv, tMin, hit.t, literal);    // box test: see box_hit_* in trace_kernels.hpp
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
          else { inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z); sh = make_shear(d, inv); literal = query_needs_literal_box(o, d, inv, r.tMin, r.tMax); }
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
          bool accept;
          if constexpr (ROT) accept = prim_hit<DF, false, true>(sc.leavesRot[atLeaf].b[sh.kz], o, d, sh, tMin, hit.t, t, b0, b1, b2);
          else accept = prim_hit<DF, FAST>(sc.leaves[atLeaf], o, d, sh, tMin, hit.t, t, b0, b1, b2);
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
