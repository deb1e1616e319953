// bvh_walk.hpp — the stackless preorder walk of the one-thread-per-item query kernels (point queries, neighbour lists, box
// queries, triangle queries, crossing counts, crossing lists), written once. A family supplies what is its own - when a node is
// entered, what happens at a reached leaf - as two lambdas; the loads, the successor rule and the counters are here. The host
// twins' loop is walkHost (host/walk_host.hpp), with the same signature over the compact nodes.
// Not walked through here: traverse<> (trace_kernels.hpp), K4 (query_kernels.hpp), K1w and the pool - those narrow an interval
// as they go and are scheduled in phases.
#pragma once

#include "trace_kernels.hpp"

namespace mi {

// Every node of sc in preorder, first child first, from the root; `valid` false: nothing is walked (an item the family refuses,
// e.g. a NaN coordinate).
//   enter(const GNode&) -> bool           a node whose box is entered goes on at GNode.hit, any other at GNode.link, the node behind
//                                         its subtree.
//   leaf(at, type, f) -> bool             called for the primitive of an entered leaf: `at` the leaf's node index (sc.leaves[at] is
//                                         its record), `type` the record's first word (LEAF_* in bits 0..15, geomID in bits
//                                         16..31), f the record's nine floats. Returning true ends the walk.
// STATS: cs.nodes counts the nodes loaded (one box test each), cs.leaves the calls of `leaf`.
// No LDS, no stack, no scratch: the walk's own state is the node offset.
template <bool STATS, class Enter, class Leaf>
__device__ __forceinline__ void walk_preorder(const DeviceScene& sc, bool valid, CastStats& cs, const Enter& enter, const Leaf& leaf) {
  // node positions are BYTE offsets into the node array (GNode); an item that is not walked ends before its first node
  const uint32_t end = valid ? sc.numNodes << 5 : 0u;
  uint32_t node = 0;
  while (node < end) {
    const GNode nd = *reinterpret_cast<const GNode*>(reinterpret_cast<const char*>(sc.nodes) + node);
    if (STATS) cs.nodes++;
    uint32_t next = enter(nd) ? nd.hit : nd.link;
    if (next & kLeafFlag) {
      // a leaf's hit successor is its link with kLeafFlag: the primitive of THIS node is handed to `leaf`, the walk goes on behind it
      next &= ~kLeafFlag;
      if (STATS) cs.leaves++;
      const uint32_t at = node >> 5;
      const float4* rec = reinterpret_cast<const float4*>(sc.leaves + at);      // the first 40 bytes: type, nine floats
      const float4 r0 = rec[0], r1 = rec[1];
      const float2 r2 = *reinterpret_cast<const float2*>(rec + 2);
      const float f[9] = {r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};
      if (leaf(at, __float_as_uint(r0.x), f)) break;
    }
    node = next;
  }
}

}  // namespace mi
